"""``use_linear_in_transformer`` on the MI355X (run with -m gpu): the SD-2 UNet's Linear proj_in / proj_out run the
kernels of the 1x1-conv form bit for bit, 4-D tensors do not load into the linear build, and a shrunken copy of
configs/sd-v2-inference-v.yaml runs from token ids to an image on the HIP path."""
import copy
import os

import pytest
import torch

import openclip_util as ou
from golden_util import cfg_of, load, weights_of
from gpu_util import check_golden
from synth import keys_shapes_of, synth_weights

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _is_proj(k):
    return k.endswith(("proj_in.weight", "proj_out.weight")) and "transformer_blocks" not in k


def _squeezed(sd):
    return {k: (v[:, :, 0, 0] if _is_proj(k) else v) for k, v in sd.items()}


def test_linear_projections_are_bit_equal_to_the_conv_form(sdk):
    from sd_amd.openai_model.model import UNetModel
    z = load("unet_tiny")
    cfg, sd = cfg_of(z), weights_of(z)
    n_proj = sum(_is_proj(k) for k in sd)
    assert n_proj >= 2 and all(float(sd[k].abs().max()) > 0 for k in sd if _is_proj(k))    # proj_out is not trivial
    x, t, ctx = (torch.from_numpy(z[k]).to(DEV) for k in ("x", "t", "ctx"))
    conv = UNetModel(**cfg)
    conv.load_state_dict(sd)
    y_conv = conv(x, t, ctx)
    lin = UNetModel(**cfg, use_linear_in_transformer=True)
    lin.load_state_dict(_squeezed(sd), strict=True)
    assert all(v.dim() == 2 for k, v in lin.state_dict().items() if _is_proj(k))
    y_lin = lin(x, t, ctx)
    assert y_lin.dtype == torch.float32 and torch.equal(y_lin, y_conv)
    check_golden("tiny UNet unet_tiny vs reference", y_lin, torch.from_numpy(z["y"]))


def test_conv_shaped_weights_do_not_load_into_the_linear_build(sdk):
    from sd_amd.openai_model.model import UNetModel
    z = load("unet_tiny")
    lin = UNetModel(**cfg_of(z), use_linear_in_transformer=True)
    with pytest.raises(RuntimeError, match="size mismatch for .*proj_in.weight"):
        lin.load_state_dict(weights_of(z))


def _tiny_sd2(sdk):
    """LatentDiffusion from configs/sd-v2-inference-v.yaml shrunk to the tiny fixtures' sizes."""
    import yaml
    from sd_amd.Diffusion.utils import instantiate_from_config
    cfg = copy.deepcopy(yaml.safe_load(open(os.path.join(ROOT, "configs", "sd-v2-inference-v.yaml")))["model"])
    p = cfg["params"]
    p.update(image_size=8, channels=4)
    p["unet_config"]["params"].update(image_size=8, model_channels=32, attention_resolutions=[1, 2], num_res_blocks=1,
                                      channel_mult=[1, 2], num_head_channels=16, context_dim=ou.TINY["width"],
                                      use_checkpoint=False)
    p["first_stage_config"]["params"]["ddconfig"] = cfg_of(load("vae_tiny"))
    p["cond_stage_config"]["params"].update(arch="tiny", config=ou.TINY)
    assert p["parameterization"] == "v" and p["unet_config"]["params"]["use_linear_in_transformer"] is True
    assert p["cond_stage_config"]["params"]["layer"] == "penultimate"
    ld = instantiate_from_config(cfg)
    for mod, seed in ((ld.model.diffusion_model, 9901), (ld.first_stage_model, 9902)):
        w = synth_weights(keys_shapes_of(mod.state_dict()), seed)
        mod.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    ld.cond_stage_model.load_state_dict(ou.openclip_weights(ou.TINY, 9903), strict=True)
    return ld.to(DEV)


# four DDIM steps: S = 3 does not divide the YAML's 1000 training steps (the uniform discretisation lands on timestep
# 1000 and DDIMSampler refuses it, as the reference does)
DDIM_STEPS = 4


def test_tiny_sd2_from_token_ids_to_image(sdk):
    from sd_amd.clip_encoder.modules import FrozenOpenCLIPEmbedder, openclip_pad
    from sd_amd.DDIM.ddim import DDIMSampler
    ld = _tiny_sd2(sdk)
    assert type(ld.cond_stage_model) is FrozenOpenCLIPEmbedder and ld.parameterization == "v"
    unet = ld.model.diffusion_model
    assert all(v.dim() == 2 for k, v in unet.state_dict().items() if _is_proj(k))
    ids = ou.seeded_ids(ou.TINY, 9904).to(DEV)
    empty = openclip_pad([[], []], 77, ou.SOT, ou.EOT).to(DEV)
    g = torch.Generator().manual_seed(9905)
    xT = torch.randn(2, 4, 8, 8, generator=g).to(DEV)

    def run(prompt_ids):
        c = ld.get_learned_conditioning(prompt_ids)
        uc = ld.get_learned_conditioning(empty)
        assert c.dtype == torch.float16 and tuple(c.shape) == (2, 77, ou.TINY["width"])
        z, _ = DDIMSampler(ld).sample(S=DDIM_STEPS, batch_size=2, shape=(4, 8, 8), conditioning=c, eta=0.0,
                                      verbose=False, unconditional_guidance_scale=3.0,
                                      unconditional_conditioning=uc, x_T=xT.clone())
        return ld.decode_first_stage(z)

    img = run(ids)
    assert tuple(img.shape) == (2, 3, 16, 16) and bool(torch.isfinite(img).all()) and float(img.abs().max()) > 0
    assert torch.equal(run(ids), img)                                  # bitwise reproducible
    other = ids.clone()
    other[:, 1:9] = (other[:, 1:9] + 101) % 900 + 1                    # another prompt of the same length
    assert not torch.equal(run(other), img)
