"""Configurations and inputs of the ADM-option UNet fixtures (use_scale_shift_norm, resblock_updown,
conv_resample=False, num_classes), regenerated from seeds (shared by tests/golden/make_golden_adm.py and the
tests): N(0, 1) fp32 from numpy's PCG64 (vq_util.randn), so the fixtures hold the reference's outputs only."""
import numpy as np

import vq_util as vu

# the reference's __main__ configuration (openai_model/model.py:604-622) scaled down: spatial transformer,
# resampling ResBlocks, FiLM, a class head.  model_channels = 32: GroupNorm32 has 1-channel groups and every
# level's channel count is a multiple of 8.
ADM_FULL = dict(image_size=16, in_channels=4, out_channels=4, model_channels=32, attention_resolutions=[1, 2],
                num_res_blocks=1, channel_mult=[1, 2, 2], num_heads=4, use_spatial_transformer=True,
                transformer_depth=1, context_dim=48, use_checkpoint=False, legacy=False, resblock_updown=True,
                use_scale_shift_norm=True, num_classes=10)
# the unconditional AttentionBlock UNet of unet_tiny_uncond.npz with the avg-pool Downsample and the conv-less
# Upsample (each followed by a GroupNorm over a tensor that carries no producer statistics)
ADM_POOL = dict(image_size=16, in_channels=4, out_channels=4, model_channels=32, attention_resolutions=[2],
                num_res_blocks=1, channel_mult=[1, 2], num_heads=2, use_spatial_transformer=False,
                use_checkpoint=False, legacy=False, conv_resample=False)
# FiLM alone (conv resampling, no classes): a fault in the fold is not masked by the resample path
ADM_FILM_ONLY = dict(image_size=16, in_channels=4, out_channels=4, model_channels=32, attention_resolutions=[1, 2],
                     num_res_blocks=1, channel_mult=[1, 2], num_heads=4, use_spatial_transformer=True,
                     transformer_depth=1, context_dim=48, use_checkpoint=False, legacy=False,
                     use_scale_shift_norm=True)
# ADM_FULL without the spatial transformer, for DiffusionWrapper.forward('adm') (which passes no context)
ADM_WRAP = dict(image_size=16, in_channels=4, out_channels=4, model_channels=32, attention_resolutions=[1, 2],
                num_res_blocks=1, channel_mult=[1, 2, 2], num_heads=-1, num_head_channels=16,
                use_spatial_transformer=False, use_checkpoint=False, legacy=False, resblock_updown=True,
                use_scale_shift_norm=True, num_classes=10)

# fixture name -> (configuration, weight seed)
FIXTURES = {"unet_tiny_adm_full": (ADM_FULL, 81), "unet_tiny_adm_pool": (ADM_POOL, 83),
            "unet_tiny_adm_film": (ADM_FILM_ONLY, 85), "unet_tiny_adm_wrap": (ADM_WRAP, 87)}

T_STEPS = np.asarray([981, 1], dtype=np.int64)
LABELS = np.asarray([3, 9], dtype=np.int64)


def inputs(shape=(2, 4, 16, 16), seed=8100):
    """x, t, context (2, 7, 48) and labels of one forward; ``shape`` (2, 4, 8, 24) is the H != W input."""
    s = seed + 7 * shape[2] + shape[3]
    return dict(x=vu.randn(s, *shape), ctx=vu.randn(s + 1, shape[0], 7, 48), t=T_STEPS.copy(), y=LABELS.copy())


WIDE = (2, 4, 8, 24)     # H != W: a transposed resample cannot pass

# ---- limits of the model-level parity tests: (rel-L2, max |got - ref| / max |ref|), each at <= 3.5x the error
# measured on MI355X (profiles/adm_unet_parity_errors.txt); fp16 activations vs the reference's fp32 outputs
PARITY_LIMITS = {
    "ADM_FULL vs reference": (6e-3, 6e-3),   # measured 2.035e-3 / 2.079e-3
    "ADM_FULL 8x24 vs reference": (6e-3, 6e-3),   # measured 2.020e-3 / 2.050e-3
    "ADM_POOL vs reference": (7e-3, 7.5e-3),   # measured 2.378e-3 / 2.541e-3
    "ADM_FILM_ONLY vs reference": (5e-3, 5.5e-3),   # measured 1.690e-3 / 1.804e-3
    "adm wrapper vs reference": (8e-3, 7e-3),   # measured 2.672e-3 / 2.324e-3
}
