"""Inputs of the concat-conditioning / ancestral-sampler fixtures, regenerated from seeds (shared by
tests/golden/make_golden_concat_ancestral.py and the tests): N(0, 1) fp32 from numpy's PCG64 (vq_util.randn), so
the fixtures hold the reference's outputs only."""
import numpy as np

import vq_util as vu

# ---- schedules whose seven posterior buffers are compared bit for bit (kwargs of DDPM.register_schedule)
SCHEDULES = {"linear": dict(beta_schedule="linear", timesteps=1000, linear_start=0.00085, linear_end=0.012),
             "cosine": dict(beta_schedule="cosine", timesteps=200)}
V_POSTERIORS = (0.0, 0.5)
NEW_BUFFERS = ("log_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod",
               "posterior_variance", "posterior_log_variance_clipped", "posterior_mean_coef1",
               "posterior_mean_coef2")
OLD_BUFFERS = ("betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod",
               "sqrt_one_minus_alphas_cumprod")


def sched_tag(name, v):
    return f"{name}_v{int(v * 10)}"


# ---- single posterior steps: (shape, per-sample t) on the linear 1000-step schedule
STEP_SCHEDULE = SCHEDULES["linear"]
STEP_CASES = [((2, 4, 8, 8), [417, 417]), ((1, 3, 5, 5), [3]), ((3, 4, 2, 2), [0, 1, 999])]
STEP_PARAMS = ("eps", "x0")
STEP_TEMPS = (1.0, 0.7)


def step_tag(shape, param, clip, temp):
    return "s{}_{}_clip{}_T{}".format("x".join(map(str, shape)), param, int(clip), int(temp * 10))


def step_inputs(shape):
    """(x, model_out, noise): unit-variance, so both parameterisations put values on both sides of the
    clamp's ±1 (the generator asserts that the clamp changes some and not all of them)."""
    s = 7001 + 13 * int(np.prod(shape))
    return vu.randn(s, *shape), vu.randn(s + 1, *shape), vu.randn(s + 2, *shape)


# ---- known-region blend: q_sample + blend of p_sample_loop at every step of the 6-step schedule
LOOP_SCHEDULE = dict(beta_schedule="linear", timesteps=6, linear_start=0.02, linear_end=0.4)
LOOP_T = 6
BLEND_SHAPE = (2, 3, 5, 5)
BLEND_MASKS = ("b1hw", "11hw", "bchw")


def blend_mask(kind, binary, shape=BLEND_SHAPE, seed=7100):
    b, c, h, w = shape
    ms = {"b1hw": (b, 1, h, w), "11hw": (1, 1, h, w), "bchw": (b, c, h, w)}[kind]
    u = np.random.Generator(np.random.PCG64(seed + len(kind) + 17 * sum(ms))).random(ms, dtype=np.float32)
    return (u > 0.5).astype(np.float32) if binary else u


def blend_inputs():
    """(x0, q-noise [T, ...], img per step [T, ...]) indexed by timestep."""
    return (vu.randn(7200, *BLEND_SHAPE), vu.randn(7201, LOOP_T, *BLEND_SHAPE),
            vu.randn(7202, LOOP_T, *BLEND_SHAPE))


# ---- whole loops with a stub model that returns recorded tensors
LOOP_SHAPE = (2, 4, 8, 8)
LOOP_VQ_CASE = (256, 4, 2, 8, 8)          # the codebook of vq_util's case
LOOP_MODES = ("plain", "mask", "clip", "quantize")


def loop_inputs():
    """x_T, model outputs, step noise and q_sample noise by TIMESTEP [T, ...], x0 and a [B,1,H,W] mask.
    The model outputs are scaled down so six steps of recorded (not learnt) eps keep |x| of order one."""
    e = vu.randn(7301, LOOP_T, *LOOP_SHAPE) * np.float32(0.5)
    return dict(xT=vu.randn(7300, *LOOP_SHAPE), es=e, nz=vu.randn(7302, LOOP_T, *LOOP_SHAPE),
                qn=vu.randn(7303, LOOP_T, *LOOP_SHAPE), x0=vu.randn(7304, *LOOP_SHAPE),
                mask=blend_mask("b1hw", True, LOOP_SHAPE, seed=7305))


# ---- tiny 9-channel UNet (inpainting layout: 4 latent + 1 mask + 4 masked-image latent channels)
TINY_UNET_CONCAT = dict(image_size=16, in_channels=9, out_channels=4, model_channels=32, attention_resolutions=[1, 2],
                        num_res_blocks=1, channel_mult=[1, 2], num_heads=4, use_spatial_transformer=True,
                        transformer_depth=1, context_dim=48, use_checkpoint=False, legacy=False)
UNET_SEED = 71


def unet_inputs():
    s = 7400
    return dict(x=vu.randn(s, 2, 4, 16, 16), m=(vu.randn(s + 1, 2, 1, 16, 16) > 0).astype(np.float32),
                zi=vu.randn(s + 2, 2, 4, 16, 16), ctx=vu.randn(s + 3, 2, 7, 48),
                t=np.asarray([981, 1], dtype=np.int64))


# ---- limits of the model-level parity test: (rel-L2, max |got - ref| / max |ref|), each at <= 3.5x the error
# measured on MI355X (profiles/concat_ancestral_parity_errors.txt); fp16 activations vs the fp32 reference
PARITY_LIMITS = {
    "tiny 9-channel hybrid UNet vs reference": (5e-3, 4.5e-3),   # measured 1.451e-3 / 1.366e-3
}
