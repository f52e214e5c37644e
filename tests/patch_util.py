"""Configurations, inputs and limits of the patch-wise UNet / tiled encode fixtures (``split_input_params``),
shared by tests/golden/make_golden_patch.py and the tests.  Inputs are regenerated from seeds (N(0, 1) fp32 from
numpy's PCG64, vq_util.randn), so the fixtures hold the reference's outputs only."""
import numpy as np

import adm_util as au
import vq_util as vu

# ---- patch_grid: (h, w, ks, stride) -> (ks', stride', Ly, Lx); the last three clip ks / stride to the tensor
GRID_CASES = [((12, 20, (8, 8), (4, 4)), ((8, 8), (4, 4), 2, 4)),
              ((12, 20, (8, 4), (4, 8)), ((8, 4), (4, 8), 2, 3)),
              ((12, 12, (8, 8), (4, 4)), ((8, 8), (4, 4), 2, 2)),
              ((24, 24, (16, 16), (8, 8)), ((16, 16), (8, 8), 2, 2)),
              ((128, 128, (64, 64), (32, 32)), ((64, 64), (32, 32), 3, 3)),
              ((12, 20, (12, 20), (4, 4)), ((12, 20), (4, 4), 1, 1)),
              ((8, 8, (64, 64), (32, 32)), ((8, 8), (8, 8), 1, 1)),
              ((8, 40, (16, 16), (64, 8)), ((8, 16), (8, 8), 1, 4)),
              ((13, 12, (8, 8), (4, 4)), ((8, 8), (4, 4), 2, 2))]          # ragged in h: row 12 is uncovered


def split_params(ks, stride, tie=True, **extra):
    sp = {"ks": tuple(ks), "stride": tuple(stride), "clip_min_weight": 0.01, "clip_max_weight": 0.5,
          "tie_braker": bool(tie), "clip_min_tie_weight": 0.01, "clip_max_tie_weight": 0.5}
    sp.update(extra)
    return sp


# ---- patch-wise UNet: x (2, C, 12, 12), patches of 8x8 every 4 -> a 2x2 grid, 8 UNet samples
X_SHAPE = (2, 4, 12, 12)
KS, STRIDE = (8, 8), (4, 4)
T_STEPS = np.asarray([881, 1], dtype=np.int64)
LABELS = np.asarray([3, 9], dtype=np.int64)

# the AttentionBlock UNet of unet_tiny_uncond.npz with 4 + 5 input channels: DiffusionWrapper 'concat' passes no
# context, so the concat model carries no cross-attention
UNET_CONCAT = dict(image_size=16, in_channels=9, out_channels=4, model_channels=32, attention_resolutions=[2],
                   num_res_blocks=1, channel_mult=[1, 2], num_heads=2, use_spatial_transformer=False,
                   use_checkpoint=False, legacy=False)
# the cross-attention UNet of unet_tiny.npz
UNET_CROSS = dict(image_size=16, in_channels=4, out_channels=4, model_channels=32, attention_resolutions=[1, 2],
                  num_res_blocks=1, channel_mult=[1, 2], num_heads=4, use_spatial_transformer=True,
                  transformer_depth=1, context_dim=48, use_checkpoint=False, legacy=False)
# both: the 9-channel cross-attention UNet of unet_tiny_concat.npz (no reference fixture: the reference asserts one key)
UNET_HYBRID = dict(UNET_CROSS, in_channels=9)
UNET_ADM = au.ADM_WRAP
MODELS = {"concat": (UNET_CONCAT, 91), "crossattn": (UNET_CROSS, 93), "adm": (UNET_ADM, 95), "hybrid": (UNET_HYBRID, 97)}
DDIM_STEPS = 3
CFG_SCALE = 7.5
# 900 steps: the reference's uniform DDIM timesteps range(0, T, T // S) + 1 stay below T only where S divides T
SCHEDULE = dict(beta_schedule="linear", timesteps=900, linear_start=0.00085, linear_end=0.012)


def unet_inputs(seed=9100):
    """x, the 5-channel concat tensor (a 0 / 1 mask and a 4-channel latent), its two parts, context, the
    unconditional context, x_T of the DDIM loops, timesteps and labels."""
    m = (vu.randn(seed + 1, 2, 1, 12, 12) > 0).astype(np.float32)
    zi = vu.randn(seed + 2, 2, 4, 12, 12)
    return dict(x=vu.randn(seed, *X_SHAPE), m=m, zi=zi, cc=np.concatenate([m, zi], 1),
                ctx=vu.randn(seed + 3, 2, 7, 48), uc=vu.randn(seed + 4, 2, 7, 48) * np.float32(0.1),
                xT=vu.randn(seed + 5, *X_SHAPE), t=T_STEPS.copy(), y=LABELS.copy())


# ---- tiled encode: x (2, 3, 24, 24), patches of 16x16 every 8 at vqf 2 -> a 2x2 grid of 8x8 latent patches
ENC_SHAPE = (2, 3, 24, 24)
ENC_KS, ENC_STRIDE, ENC_VQF = (16, 16), (8, 8), 2
TINY_VAE = dict(double_z=True, z_channels=4, resolution=32, in_channels=3, out_ch=3, ch=32, ch_mult=[1, 2],
                num_res_blocks=1, attn_resolutions=[], dropout=0.0)
TINY_VQ = dict(TINY_VAE, double_z=False)
TINY_VQ_EMBED, TINY_VQ_CODES = 3, 64
ENC_SEEDS = {"kl": 101, "vq": 103}


def encode_input(seed=9200):
    return np.random.Generator(np.random.PCG64(seed)).random(ENC_SHAPE, dtype=np.float32) * 2 - 1


# ---- weighting tables: (h, w, ks, stride, df) of the fold; uf = df = 1 is apply_model's, df = 2 the encode's
TABLE_CASES = {"unet": (12, 12, KS, STRIDE, 1), "unet_wide": (12, 20, (8, 4), (4, 2), 1),
               "encode": (24, 24, ENC_KS, ENC_STRIDE, 2)}


def overlap_add(pix, lw, h, w, stride, Ly, Lx):
    """NumPy normalisation table: the sum over the patches of pix (x) lw, as torch.nn.Fold(weighting) gives it."""
    kh, kw = pix.shape
    norm = np.zeros((h, w), dtype=np.float32)
    for ly in range(Ly):
        for lx in range(Lx):
            f = np.float32(1.0) if lw is None else lw[ly * Lx + lx]
            norm[ly * stride[0]:ly * stride[0] + kh, lx * stride[1]:lx * stride[1] + kw] += pix * f
    return norm


# ---- limits of the comparisons with the reference's fixtures: (rel-L2, max |got - ref| / max |ref|), each at
# <= 3.5x the error measured on MI355X (profiles/patch_unet_parity_errors.txt).  A normalised weighted average is
# no further from the reference than its worst patch, so no single-call limit exceeds the tiny-UNet entries of
# gpu_util.GOLDEN_LIMITS (5e-3 / 6e-3), no loop limit 'tiny DDIM CFG vs reference' (1e-2), no encode limit
# 'tiny VAE encode moments vs reference' (3e-3).
PARITY_LIMITS = {
    "patch-wise concat UNet vs reference": (5e-3, 6e-3),   # measured 1.669e-3 / 1.844e-3 (tie-breaker on and off)
    "patch-wise crossattn UNet vs reference": (5e-3, 5.5e-3),   # measured 1.496e-3 / 1.680e-3 (on and off)
    "patch-wise adm UNet vs reference": (5e-3, 6e-3),   # measured 3.000e-3 / 2.941e-3
    "patch-wise concat DDIM loop vs reference": (1.9e-3, 2.8e-3),   # measured 5.668e-4 / 8.008e-4
    "patch-wise crossattn DDIM loop vs reference": (1e-2, 1e-2),   # measured 3.079e-3 / 3.498e-3
    "tiled kl encode vs reference": (3e-3, 2.8e-3),   # measured 9.574e-4 / 8.266e-4 (max_batch 16 and 3)
    "tiled vq encode vs reference": (3e-3, 3e-3),   # measured 1.028e-3 / 1.409e-3 (max_batch 16 and 3)
}
