"""CPU tests of the sampler options' boundary: the new C ABI symbols in the header / binding / INTEGRATION.md, the
public signatures against the reference's argument names, ``cond_ids`` and the original-steps scalars against the
reference's (tests/golden/make_golden_sampler_options.py, bit for bit), and the two refusals that remain."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import sampler_opt_util as su
from golden_util import cfg_of, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sdk_cfg_combine", "sdk_ddim_step_ex", "sdk_posterior_step_ex")


def test_new_symbols_in_header_binding_and_integration_table(sdk):
    from sd_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "sdk_amd.h")).read()
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % sym, header), sym
        assert sym in _lib.EXPORTS, sym
        assert re.search(r"^\| `%s` \|" % sym, table, re.M), sym
    assert callable(ops.cfg_combine)
    for struct in ("sdk_ddim_ex_args", "sdk_posterior_ex_args"):
        assert re.search(r"\} %s;" % struct, header) and struct in table, struct
    # the new structs embed the old ones unchanged, in front
    assert _lib.DdimExArgs._fields_[0] == ("step", _lib.DdimArgs) and _lib.DdimExArgs.step.offset == 0
    assert _lib.DdimExArgs._fields_[-1] == ("blend", _lib.MaskedQArgs)
    assert _lib.PosteriorExArgs._fields_[0] == ("step", _lib.PosteriorArgs) and _lib.PosteriorExArgs.step.offset == 0
    assert C.sizeof(_lib.DdimArgs) == 96 and C.sizeof(_lib.PosteriorArgs) == 96 and C.sizeof(_lib.MaskedQArgs) == 72
    assert C.sizeof(_lib.DdimExArgs) == 96 + 16 + 72 and C.sizeof(_lib.PosteriorExArgs) == 96 + 16


def _params(fn):
    return set(inspect.signature(fn).parameters)


def test_public_signatures_accept_the_reference_argument_names(sdk):
    from sd_amd import ops
    from sd_amd.DDIM.ddim import DDIMSampler
    from sd_amd.Diffusion.ddpm import LatentDiffusion
    loop = {"mask", "x0", "noise_dropout", "score_corrector", "corrector_kwargs", "temperature", "quantize_denoised"}
    assert loop | {"ddim_use_original_steps", "timesteps", "q_noise_fn", "dropout_fn", "noise_fn"} \
        <= _params(DDIMSampler.ddim_sampling)
    assert (loop - {"quantize_denoised"}) | {"quantize_x0", "eta", "q_noise_fn", "dropout_fn"} <= _params(DDIMSampler.sample)
    assert {"use_original_steps", "noise_dropout", "score_corrector", "corrector_kwargs", "repeat_noise", "keep"} \
        <= _params(DDIMSampler.p_sample_ddim)
    assert "use_original_steps" in _params(DDIMSampler.step_scalars) and "use_original_steps" in _params(DDIMSampler.decode)
    ref_prog = {"cond", "shape", "verbose", "callback", "quantize_denoised", "img_callback", "mask", "x0", "temperture",
                "noise_dropout", "score_corrector", "corrector_kwargs", "batch_size", "x_T", "start_T", "log_every_t"}
    assert ref_prog | {"noise_fn", "q_noise_fn", "dropout_fn", "cond_noise_fn"} <= _params(LatentDiffusion.progressive_denoising)
    assert {"dropout_fn", "cond_noise_fn", "noise_dropout", "score_corrector"} <= _params(LatentDiffusion.p_sample_loop)
    assert {"noise_dropout", "score_corrector", "corrector_kwargs", "temperture", "keep"} <= _params(LatentDiffusion.p_sample)
    assert list(inspect.signature(LatentDiffusion.sample_log).parameters)[:5] == ["self", "cond", "batch_size", "ddim",
                                                                                "ddim_steps"]
    assert callable(LatentDiffusion.make_cond_schedule)
    for fn in (ops.ddim_step, ops.ddim_xprev):
        assert {"keep", "drop_p", "blend_x0", "blend_noise", "blend_mask", "blend_sqrt_acp", "blend_sqrt_1m_acp"} <= _params(fn)
    assert {"keep", "drop_p"} <= _params(ops.posterior_step)
    assert list(inspect.signature(ops.cfg_combine).parameters)[:3] == ["e_uncond", "e_cond", "guidance"]


def _tiny_ld(sdk, **kw):
    from sd_amd.Diffusion.ddpm import LatentDiffusion
    u, v = load("unet_tiny"), load("vae_tiny")
    kw.setdefault("timesteps", su.T)
    return LatentDiffusion(
        first_stage_config={"target": "VAE.autoencoder.AutoEncoderKL",
                            "params": {"ddconfig": cfg_of(v), "embed_dim": 4,
                                       "lossconfig": {"target": "torch.nn.Identity"}}},
        cond_stage_config="__is_unconditional__",
        unet_config={"target": "openai_model.model.UNetModel", "params": cfg_of(u)}, **kw)


@pytest.mark.parametrize("timesteps,ncond", su.COND_SCHEDULES)
def test_cond_ids_equal_the_reference(sdk, timesteps, ncond):
    sch = dict(su.SCHEDULE, timesteps=timesteps) if timesteps == su.T else dict(timesteps=timesteps)
    ld = _tiny_ld(sdk, num_timesteps_cond=ncond, **sch)
    assert ld.shorten_cond_schedule and ld.cond_ids.dtype == torch.long
    assert np.array_equal(ld.cond_ids.numpy(), load("so_ancestral")[f"cond_ids_{timesteps}_{ncond}"])
    assert not hasattr(_tiny_ld(sdk), "cond_ids")                # num_timesteps_cond = 1: no schedule, as the reference


def test_original_steps_scalars_equal_the_reference(sdk):
    from sd_amd.DDIM.ddim import DDIMSampler
    fx = load("so_ddim_loops")
    s = DDIMSampler(_tiny_ld(sdk, **su.SCHEDULE))
    s.make_schedule(su.S, ddim_eta=float(fx["orig_eta"]), verbose=False)
    sig = s.ddim_sigmas_for_original_num_steps
    assert sig.dtype == torch.float32 and np.array_equal(sig.numpy().view(np.uint32), fx["orig_sigmas"].view(np.uint32))
    assert float(fx["orig_eta"]) > 0 and float(sig.max()) > 0
    keys = ("sqrt_one_minus_at", "sqrt_at", "dir_coef", "sqrt_a_prev", "sigma")
    for i in range(su.T):
        sc = s.step_scalars(i, use_original_steps=True)
        got = np.asarray([sc[k] for k in keys], dtype=np.float32)
        assert np.array_equal(got.view(np.uint32), fx["orig_scalars"][i].view(np.uint32)), (i, got, fx["orig_scalars"][i])
        assert set(sc) == set(s.step_scalars(0))                 # the same eight scalars as the DDIM tables give
    assert s.step_scalars(1) == s.step_scalars(1, use_original_steps=False)


def test_off_the_gpu_the_options_stay_not_implemented_before_any_model_call(sdk):
    """The options are HIP kernels only: on a CPU model they raise what they raised before they existed, and
    argument errors still come first."""
    from sd_amd.DDIM.ddim import DDIMSampler
    shape = (1, 4, 8, 8)
    x, t = torch.zeros(shape), torch.zeros(1, dtype=torch.long)
    ld = _tiny_ld(sdk, **su.SCHEDULE)
    ld.apply_model = None                                        # any model call would be a TypeError
    s = DDIMSampler(ld)
    s.make_schedule(su.S, verbose=False)
    for kw in (dict(use_original_steps=True), dict(noise_dropout=0.5), dict(score_corrector=object())):
        with pytest.raises(NotImplementedError, match="GPU only"):
            s.p_sample_ddim(x, None, t, index=0, **kw)
    with pytest.raises(NotImplementedError, match="original-steps"):
        s.decode(x, None, 2, use_original_steps=True)
    with pytest.raises(NotImplementedError, match="mask / x0"):
        s.sample(su.S, 1, shape[1:], mask=torch.ones(1, 1, 8, 8), x0=x, verbose=False)
    with pytest.raises(NotImplementedError, match="progressive_denoising"):
        ld.progressive_denoising(None, shape[1:], batch_size=1)
    with pytest.raises(NotImplementedError, match="noise_dropout"):
        ld.sample_log(None, 1, ddim=False, ddim_steps=su.S, shape=shape, noise_dropout=0.5)
    with pytest.raises(ValueError, match="noise_dropout"):
        ld.p_sample(x, None, t, noise_dropout=1.5)
    with pytest.raises(ValueError, match="x0"):
        s.ddim_sampling(None, shape, mask=torch.ones(1, 1, 8, 8))


def test_the_two_remaining_refusals_still_raise(sdk):
    from sd_amd.DDIM.ddim import DDIMSampler
    shape = (1, 4, 8, 8)
    x, t = torch.zeros(shape), torch.zeros(1, dtype=torch.long)
    ld = _tiny_ld(sdk)
    for call in (lambda: ld.p_sample(x, None, t, return_codebook_ids=True),
                 lambda: ld.p_mean_variance(x, None, t, clip_denoised=False, return_codebook_ids=True),
                 lambda: ld.sample(None, batch_size=1, shape=shape, return_codebook_ids=True)):
        with pytest.raises(NotImplementedError, match="return_codebook_ids"):
            call()
    s = DDIMSampler(_tiny_ld(sdk, parameterization="x0"))
    s.make_schedule(2, verbose=False)
    with pytest.raises(NotImplementedError, match="x0"):
        s.p_sample_ddim(x, None, t, index=0)
    with pytest.raises(NotImplementedError, match="x0"):
        s.p_sample_ddim(x, None, t, index=0, use_original_steps=True, noise_dropout=0.5)
