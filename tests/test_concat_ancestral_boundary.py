"""CPU tests of the concat / hybrid conditioning and the ancestral sampler's boundary: the posterior
schedule buffers against the reference's (tests/golden/make_golden_concat_ancestral.py, bit for bit), the
new C ABI symbols in the header / binding / INTEGRATION.md, and argument validation."""
import os
import re

import numpy as np
import pytest
import torch

import ca_util as cu
from golden_util import cfg_of, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sdk_concat_nchw_to_nhwc", "sdk_posterior_step", "sdk_masked_q_sample")


@pytest.mark.parametrize("name", list(cu.SCHEDULES))
@pytest.mark.parametrize("v", cu.V_POSTERIORS)
def test_posterior_schedule_buffers_equal_the_reference(sdk, name, v):
    from sd_amd.DDIM.diffusion_modules import register_schedule
    kw = cu.SCHEDULES[name]
    sch = register_schedule(kw["timesteps"], kw.get("linear_start", 1e-4), kw.get("linear_end", 2e-2),
                            kw["beta_schedule"], v_posterior=v)
    fx = load("ca_schedule")
    assert sch["num_timesteps"] == kw["timesteps"]
    for k in cu.OLD_BUFFERS + cu.NEW_BUFFERS:
        got, ref = sch[k].numpy(), fx[f"{cu.sched_tag(name, v)}_{k}"]
        assert got.dtype == np.float32 and got.shape == ref.shape
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), k
    assert register_schedule(10).keys() == sch.keys()         # v_posterior defaults to 0


def test_new_symbols_in_header_binding_and_integration_table(sdk):
    from sd_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "sdk_amd.h")).read()
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % sym, header), sym
        assert sym in _lib.EXPORTS, sym
        assert re.search(r"^\| `%s` \|" % sym, table, re.M), sym
    for fn in ("concat_nchw_to_nhwc", "posterior_step", "masked_q_sample"):
        assert callable(getattr(ops, fn))
    for struct in ("PosteriorArgs", "MaskedQArgs", "ConcatArgs"):
        assert hasattr(_lib, struct)


def _tiny_ld(sdk, **kw):
    from sd_amd.Diffusion.ddpm import LatentDiffusion
    u, v = load("unet_tiny"), load("vae_tiny")
    return LatentDiffusion(
        first_stage_config={"target": "VAE.autoencoder.AutoEncoderKL",
                            "params": {"ddconfig": cfg_of(v), "embed_dim": 4,
                                       "lossconfig": {"target": "torch.nn.Identity"}}},
        cond_stage_config="__is_unconditional__",
        unet_config={"target": "openai_model.model.UNetModel", "params": cfg_of(u)}, timesteps=6, **kw)


def test_channel_sum_mismatch_raises_value_error(sdk):
    from sd_amd.openai_model.model import UNetModel
    m = UNetModel(**cu.TINY_UNET_CONCAT)
    x, t = torch.zeros(1, 4, 16, 16), torch.zeros(1, dtype=torch.long)
    with pytest.raises(ValueError, match="in_channels"):
        m(x, t, context=torch.zeros(1, 7, 48), concat=[torch.zeros(1, 1, 16, 16), torch.zeros(1, 3, 16, 16)])
    with pytest.raises(ValueError, match="spatial"):
        m(x, t, context=torch.zeros(1, 7, 48), concat=[torch.zeros(1, 1, 16, 16), torch.zeros(1, 4, 8, 8)])
    with pytest.raises(ValueError, match="at most 3"):
        m(x, t, context=torch.zeros(1, 7, 48), concat=[torch.zeros(1, 1, 16, 16)] * 5)


def test_x0_parameterization_constructs_and_ddim_refuses_it(sdk):
    from sd_amd.DDIM.ddim import DDIMSampler
    ld = _tiny_ld(sdk, parameterization="x0", clip_denoised=False, v_posterior=0.5)
    assert ld.parameterization == "x0" and ld.clip_denoised is False and ld.v_posterior == 0.5
    names = {k for k, _ in ld.named_buffers(recurse=False)}
    assert set(cu.OLD_BUFFERS + cu.NEW_BUFFERS) <= names
    assert set(cu.NEW_BUFFERS) <= set(ld.state_dict().keys())
    assert _tiny_ld(sdk).clip_denoised is True                  # the reference's default
    s = DDIMSampler(ld)
    s.make_schedule(2, verbose=False)
    with pytest.raises(NotImplementedError, match="x0"):
        s.p_sample_ddim(torch.zeros(1, 4, 8, 8), None, torch.zeros(1, dtype=torch.long), index=0)


def test_ancestral_sampler_argument_validation(sdk):
    ld = _tiny_ld(sdk)
    shape = (1, 4, 8, 8)
    x, t = torch.zeros(shape), torch.zeros(1, dtype=torch.long)
    with pytest.raises(ValueError, match="x0"):
        ld.p_sample_loop(None, shape, mask=torch.ones(1, 1, 8, 8))
    with pytest.raises(ValueError, match="spatial"):
        ld.p_sample_loop(None, shape, mask=torch.ones(1, 1, 4, 4), x0=torch.zeros(shape))
    for kw in (dict(score_corrector=object()), dict(noise_dropout=0.1), dict(return_codebook_ids=True)):
        with pytest.raises(NotImplementedError):
            ld.p_sample(x, None, t, **kw)
        with pytest.raises(NotImplementedError):
            ld.sample(None, batch_size=1, shape=shape, **kw)
    with pytest.raises(NotImplementedError):
        ld.p_mean_variance(x, None, t, clip_denoised=False, score_corrector=object())
    with pytest.raises(NotImplementedError):
        ld.progressive_denoising(None, shape)
    ld.shorten_cond_schedule = True
    with pytest.raises(NotImplementedError, match="shorten_cond_schedule"):
        ld.p_sample_loop(None, shape)
    ld.shorten_cond_schedule = False
    with pytest.raises(AttributeError, match="VQ first stage"):
        ld.p_sample_loop(None, shape, quantize_denoised=True)
    with pytest.raises(ValueError, match="timesteps"):
        ld.q_sample(x, torch.tensor([6]))                       # t outside the 6-step schedule


def test_adm_still_raises_and_concat_needs_its_conditioning(sdk):
    from sd_amd.Diffusion.ddpm import DiffusionWrapper
    dw = DiffusionWrapper.__new__(DiffusionWrapper)
    torch.nn.Module.__init__(dw)
    dw.diffusion_model, dw._graphed, dw._graphs_on = None, None, False
    x, t = torch.zeros(1, 4, 8, 8), torch.zeros(1, dtype=torch.long)
    dw.conditioning_key = "adm"
    with pytest.raises(NotImplementedError):
        dw(x, t, c_crossattn=[torch.zeros(1, 10)])
    dw.conditioning_key = "concat"
    with pytest.raises(ValueError, match="c_concat"):
        dw(x, t)
    dw.conditioning_key = "hybrid"
    with pytest.raises(ValueError, match="c_crossattn"):
        dw(x, t, c_concat=[x])
