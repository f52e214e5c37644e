"""Inputs and limits of the sampler-option fixtures (DDIM mask / x0, original steps, noise dropout, score
correctors, progressive_denoising, shorten_cond_schedule), regenerated from seeds and shared by
tests/golden/make_golden_sampler_options.py and the tests: N(0, 1) fp32 from numpy's PCG64 (vq_util.randn), so the
fixtures hold only what the reference produced (its outputs and the dropout keep masks it drew)."""
import itertools

import numpy as np

import ca_util as cu
import vq_util as vu

# ---- kernel forms: one p_sample_ddim call (and the blend that opens the next iteration) of a 3-step DDIM
# schedule over the 6-step model schedule: ddim_timesteps [1, 3, 5], the call at index 2 (t = 5), the blend at t = 3
SCHEDULE = cu.LOOP_SCHEDULE
T = cu.LOOP_T
S = 3
KERNEL_SHAPES = [(2, 3, 5, 5), (1, 3, 5, 5), (2, 4, 8, 8)]     # n = 150 (a tail of 2), 75 (a tail of 3), 512 (aligned)
ETAS = (0.0, 1.0)
TEMPS = (1.0, 0.7)
DROPS = (0.0, 0.3, 0.75)
GUIDANCE = 2.5
MASK_KINDS = cu.BLEND_MASKS
# the blend fixtures: every mask shape, binary and fractional, at both etas on the fullest step form
BLEND_STEP = dict(temp=0.7, guided=True, p=0.3)


def shape_tag(shape):
    return "x".join(map(str, shape))


def step_combos():
    """(eta, temperature, guided, dropout p) of the kernel-form fixtures."""
    return list(itertools.product(ETAS, TEMPS, (False, True), DROPS))


def step_tag(shape, eta, temp, guided, p):
    return "k{}_eta{}_T{}_g{}_p{}".format(shape_tag(shape), int(eta), int(temp * 10), int(guided), int(p * 100))


def blend_tag(shape, eta, kind, binary):
    return "b{}_eta{}_{}_{}".format(shape_tag(shape), int(eta), kind, "bin" if binary else "frac")


def keep_tag(shape, p):
    return "keep{}_p{}".format(shape_tag(shape), int(p * 100))


def kernel_inputs(shape):
    """x_T, the conditional and unconditional model outputs, step noise, x0, and the q-noise of the first and of
    the next blend."""
    s = 9001 + 17 * int(np.prod(shape))
    names = ("xT", "e", "eu", "nz", "x0", "qn0", "qn1")
    return {k: vu.randn(s + i, *shape) * np.float32(0.5 if k in ("e", "eu") else 1.0) for i, k in enumerate(names)}


def mask_of(kind, binary, shape):
    return cu.blend_mask(kind, binary, shape, seed=9100)


def drop_seed(shape, p):
    """torch.manual_seed before the reference's F.dropout draws, one per (shape, p): every step form of one shape
    and p sees the same keep mask."""
    return 9200 + int(np.prod(shape)) + int(p * 100)


# ---- posterior step with dropout: ca_util.STEP_CASES on the 1000-step schedule, temperature 0.7
POST_DROPS = (0.3, 0.75)
POST_TEMP = 0.7


def post_tag(shape, param, clip, p):
    return "s{}_{}_clip{}_p{}".format(shape_tag(shape), param, int(clip), int(p * 100))


# ---- loops: stub model, (2, 4, 8, 8), the 6-step schedule, S = 3, log_every_t = 1
LOOP_SHAPE = cu.LOOP_SHAPE
LOOP_DROP = 0.3
DDIM_CASES = ("mask_b1hw", "mask_11hw", "mask_bchw", "mask_eta1", "mask_quantize", "mask_cfg", "orig_eta0",
              "orig_eta", "orig_timesteps", "orig_decode", "dropout_eta1", "corrector", "corrector_cfg")
ORIG_ETAS = (1.0, 0.5, 0.25)        # the generator takes the first with 1 - a_prev - sigma^2 >= 0 at every index
ORIG_TIMESTEPS = 4                  # timesteps= / t_start= of the two shortened original-steps cases
COND_SCHEDULES = ((6, 3), (1000, 4))          # (timesteps, num_timesteps_cond) of the cond_ids fixtures
NUM_TIMESTEPS_COND = 3
TEMP_LIST = (1.0, 0.7, 0.9, 1.0, 0.8, 0.6)    # progressive_denoising's per-timestep temperature


def loop_inputs():
    """Everything by TIMESTEP [T, ...]: conditional / unconditional model outputs, step noise, q-noise, the
    corrector's addend and the conditioning's q-noise; x_T, x0, the conditioning and a mask per shape."""
    d = dict(cu.loop_inputs())
    sh = (T,) + LOOP_SHAPE
    d.update(eu=vu.randn(9301, *sh) * np.float32(0.5), add=vu.randn(9302, *sh) * np.float32(0.25),
             cn=vu.randn(9303, *sh), cond=vu.randn(9304, *LOOP_SHAPE))
    for kind in MASK_KINDS:
        d["mask_" + kind] = cu.blend_mask(kind, kind != "bchw", LOOP_SHAPE, seed=9305)    # bchw: fractional
    return d


# ---- model level: the tiny 9-channel hybrid UNet of ca_util through 4 masked DDIM steps, eta = 0
MODEL_STEPS = 4


def model_inputs():
    d = dict(cu.unet_inputs())
    d["qn"] = vu.randn(9400, MODEL_STEPS, *d["x"].shape)          # q-noise by loop counter
    return d


# ---- limits of the model-level parity test: (rel-L2, max |got - ref| / max |ref|), each at <= 3.5x the error
# measured on MI355X (profiles/sampler_options_parity_errors.txt); fp16 activations vs the fp32 reference
PARITY_LIMITS = {
    "masked DDIM x4, tiny 9-channel hybrid UNet vs reference": (1.7e-3, 1.6e-3),   # measured 5.128e-4 / 4.724e-4
}
