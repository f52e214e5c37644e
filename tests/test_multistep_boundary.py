"""CPU tests of the multistep samplers' boundary: the new C ABI symbol in the header / binding / INTEGRATION.md, the
public signatures (CompVis' names for PLMS), the refusals, the DPM-Solver++ coefficients against the test's own
float64 values, and the float64 restatement (tests/multistep_util.py) against the accuracy scenario's numbers, so
that the GPU accuracy test cannot hide behind a restatement that is itself off."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import multistep_util as mu
from golden_util import cfg_of, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SD_SCHEDULE = dict(timesteps=1000, linear_start=0.00085, linear_end=0.012, beta_schedule="linear")


def test_new_symbol_in_header_binding_and_integration_table(sdk):
    from sd_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "sdk_amd.h")).read()
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sym = "sdk_multistep_step"
    assert re.search(r"\bint %s\(const sdk_multistep_args\*" % sym, header)
    assert sym in _lib.EXPORTS
    assert re.search(r"^\| `%s` \|" % sym, table, re.M)
    assert re.search(r"\} sdk_multistep_args;", header) and "sdk_multistep_args" in table
    assert callable(ops.multistep_step)
    # the new struct embeds sdk_ddim_args unchanged in front and ends with the blend, as sdk_ddim_ex_args
    M = _lib.MultistepArgs
    assert M._fields_[0] == ("step", _lib.DdimArgs) and M.step.offset == 0
    assert M._fields_[-1] == ("blend", _lib.MaskedQArgs)
    assert M.blend.offset + C.sizeof(_lib.MaskedQArgs) == C.sizeof(M) and M.blend.offset % 8 == 0
    assert M.hist.offset == 96 and M.hist.size == 24
    # the old structs keep their sizes
    assert C.sizeof(_lib.DdimArgs) == 96 and C.sizeof(_lib.PosteriorArgs) == 96 and C.sizeof(_lib.MaskedQArgs) == 72
    assert C.sizeof(_lib.DdimExArgs) == 184 and C.sizeof(_lib.PosteriorExArgs) == 112
    # the header's struct, field by field, is the binding's
    body = re.search(r"typedef struct \{([^}]*)\} sdk_multistep_args;", header).group(1)
    names = re.findall(r"(\w+)(?:\[\d+\])?\s*[;,]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [f[0] for f in M._fields_], names
    forms = re.search(r"enum \{ SDK_MULTISTEP_PLMS = 0, SDK_MULTISTEP_PLMS_WARMUP = 1, SDK_MULTISTEP_DPM = 2 \};", header)
    assert forms and (_lib.MULTISTEP_PLMS, _lib.MULTISTEP_PLMS_WARMUP, _lib.MULTISTEP_DPM) == (0, 1, 2)


def _params(fn):
    return list(inspect.signature(fn).parameters)


def test_public_signatures(sdk):
    from sd_amd import ops
    from sd_amd.DDIM.ddim import DDIMSampler
    from sd_amd.DDIM.dpm_solver import DPMSolverSampler
    from sd_amd.DDIM.plms import PLMSSampler
    assert issubclass(PLMSSampler, DDIMSampler) and issubclass(DPMSolverSampler, DDIMSampler)
    for name in ("make_schedule", "sample", "plms_sampling", "p_sample_plms"):
        assert callable(getattr(PLMSSampler, name)), name
    # CompVis' argument names, in its order
    assert _params(PLMSSampler.make_schedule) == ["self", "ddim_num_steps", "ddim_discretize", "ddim_eta", "verbose"]
    compvis_sample = ["self", "S", "batch_size", "shape", "conditioning", "callback", "normals_sequence", "img_callback",
                      "quantize_x0", "eta", "mask", "x0", "temperature", "noise_dropout", "score_corrector",
                      "corrector_kwargs", "verbose", "x_T", "log_every_t", "unconditional_guidance_scale",
                      "unconditional_conditioning"]
    assert _params(PLMSSampler.sample)[:len(compvis_sample)] == compvis_sample
    assert {"q_noise_fn", "kwargs"} <= set(_params(PLMSSampler.sample))
    compvis_loop = ["self", "cond", "shape", "x_T", "ddim_use_original_steps", "callback", "timesteps",
                    "quantize_denoised", "mask", "x0", "img_callback", "log_every_t", "temperature", "noise_dropout",
                    "score_corrector", "corrector_kwargs", "unconditional_guidance_scale", "unconditional_conditioning"]
    assert _params(PLMSSampler.plms_sampling)[:len(compvis_loop)] == compvis_loop
    compvis_step = ["self", "x", "c", "t", "index", "repeat_noise", "use_original_steps", "quantize_denoised",
                    "temperature", "noise_dropout", "score_corrector", "corrector_kwargs",
                    "unconditional_guidance_scale", "unconditional_conditioning", "old_eps", "t_next"]
    assert _params(PLMSSampler.p_sample_plms)[:len(compvis_step)] == compvis_step
    sig = inspect.signature(PLMSSampler.p_sample_plms).parameters
    assert sig["old_eps"].default is None and sig["t_next"].default is None
    dpm = inspect.signature(DPMSolverSampler.sample).parameters
    assert list(dpm) == ["self", "S", "batch_size", "shape", "conditioning", "x_T", "unconditional_guidance_scale",
                         "unconditional_conditioning", "mask", "x0", "callback", "img_callback", "log_every_t",
                         "lower_order_final", "verbose", "kwargs"]
    assert dpm["lower_order_final"].default is True and dpm["log_every_t"].default == 100
    assert dpm["unconditional_guidance_scale"].default == 1. and dpm["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    assert "continuous-time" in DPMSolverSampler.sample.__doc__ and "DDIM grid" in DPMSolverSampler.sample.__doc__
    assert _params(DPMSolverSampler.step_coefficients) == ["self", "index", "prev_index"]
    assert inspect.signature(DPMSolverSampler.step_coefficients).parameters["prev_index"].default is None
    assert {"blend_x0", "blend_noise", "blend_mask", "blend_sqrt_acp", "blend_sqrt_1m_acp", "x_next", "x_prev", "pred_x0",
            "hist_out", "e_uncond", "guidance", "v_param"} <= set(_params(ops.multistep_step))


def _tiny_ld(sdk, **kw):
    from sd_amd.Diffusion.ddpm import LatentDiffusion
    u, v = load("unet_tiny"), load("vae_tiny")
    return LatentDiffusion(
        first_stage_config={"target": "VAE.autoencoder.AutoEncoderKL",
                            "params": {"ddconfig": cfg_of(v), "embed_dim": 4,
                                       "lossconfig": {"target": "torch.nn.Identity"}}},
        cond_stage_config="__is_unconditional__",
        unet_config={"target": "openai_model.model.UNetModel", "params": cfg_of(u)}, **dict(SD_SCHEDULE, **kw))


def _samplers(sdk):
    from sd_amd.DDIM.dpm_solver import DPMSolverSampler
    from sd_amd.DDIM.plms import PLMSSampler
    return PLMSSampler, DPMSolverSampler


def test_eta_must_be_zero(sdk):
    ld = _tiny_ld(sdk)
    ld.apply_model = None
    for cls in _samplers(sdk):
        with pytest.raises(ValueError, match="ddim_eta must be 0"):
            cls(ld).make_schedule(4, ddim_eta=0.5, verbose=False)
        with pytest.raises(ValueError, match="ddim_eta must be 0"):
            cls(ld).sample(4, 1, (4, 8, 8), eta=1.0, verbose=False)
        cls(ld).make_schedule(4, ddim_eta=0.0, verbose=False)


def test_the_four_refusals_name_the_option(sdk):
    shape = (1, 4, 8, 8)
    x, t = torch.zeros(shape), torch.zeros(1, dtype=torch.long)
    ld = _tiny_ld(sdk)
    ld.apply_model = None                                        # any model call would be a TypeError
    ldx0 = _tiny_ld(sdk, parameterization="x0")
    ldx0.apply_model = None
    options = (("quantize_x0", dict(quantize_x0=True)), ("noise_dropout", dict(noise_dropout=0.5)),
               ("score_corrector", dict(score_corrector=object())))
    for cls in _samplers(sdk):
        for name, kw in options:
            with pytest.raises(NotImplementedError, match=name):
                cls(ld).sample(4, 1, shape[1:], verbose=False, **kw)
        with pytest.raises(NotImplementedError, match="x0"):
            cls(ldx0).sample(4, 1, shape[1:], verbose=False)
    PLMS, DPM = _samplers(sdk)
    s = PLMS(ld)
    s.make_schedule(4, verbose=False)
    for name, kw in (("quantize_x0", dict(quantize_denoised=True)),) + options[1:]:
        with pytest.raises(NotImplementedError, match=name):
            s.plms_sampling(None, shape, **kw)
        with pytest.raises(NotImplementedError, match=name):
            s.p_sample_plms(x, None, t, index=0, **kw)
    sx = PLMS(ldx0)
    sx.make_schedule(4, verbose=False)
    with pytest.raises(NotImplementedError, match="x0"):
        sx.p_sample_plms(x, None, t, index=0)
    dx = DPM(ldx0)
    dx.make_schedule(4, verbose=False)
    with pytest.raises(NotImplementedError, match="x0"):
        dx.p_sample_dpm(x, None, t, index=3)


def test_off_the_gpu_not_implemented_before_any_model_call(sdk):
    shape = (1, 4, 8, 8)
    x, t = torch.zeros(shape), torch.zeros(1, dtype=torch.long)
    ld = _tiny_ld(sdk)
    ld.apply_model = None                                        # any model call would be a TypeError
    PLMS, DPM = _samplers(sdk)
    for cls in (PLMS, DPM):
        with pytest.raises(NotImplementedError, match="GPU only"):
            cls(ld).sample(4, 1, shape[1:], verbose=False)
        with pytest.raises(NotImplementedError, match="GPU only"):
            cls(ld).sample(4, 1, shape[1:], verbose=False, x_T=x, mask=torch.ones(1, 1, 8, 8), x0=x)
        with pytest.raises(ValueError, match="x0"):                  # argument errors still come first
            cls(ld).sample(4, 1, shape[1:], verbose=False, mask=torch.ones(1, 1, 8, 8))
    s = PLMS(ld)
    s.make_schedule(4, verbose=False)
    with pytest.raises(NotImplementedError, match="GPU only"):
        s.p_sample_plms(x, None, t, index=3, t_next=t)
    with pytest.raises(NotImplementedError, match="GPU only"):
        s.plms_sampling(None, shape)
    d = DPM(ld)
    d.make_schedule(4, verbose=False)
    with pytest.raises(NotImplementedError, match="GPU only"):
        d.p_sample_dpm(x, None, t, index=3)


def _ulp_apart(a, b):
    """Distance in fp32 ulps between two finite fp32 values of one sign (or zeros)."""
    ia, ib = (int(np.float32(v).view(np.int32)) & 0x7fffffff for v in (a, b))
    assert (a == 0 and b == 0) or np.sign(a) == np.sign(b), (a, b)
    return abs(ia - ib)


@pytest.mark.parametrize("S", mu.COEF_STEPS)
def test_dpm_coefficients_and_order_switch(sdk, S):
    _, DPM = _samplers(sdk)
    s = DPM(_tiny_ld(sdk))
    s.make_schedule(S, ddim_discretize=mu.discretize(S), verbose=False)
    tab = mu.tables(S)
    assert np.array_equal(s.ddim_timesteps, tab["ddim_timesteps"]) and len(s.ddim_timesteps) == S
    for index in range(S):
        for prev in (None, index + 1 if index + 1 < S else None):
            got = s.step_coefficients(index, prev)
            assert all(isinstance(c, float) and np.float32(c) == c for c in got), got     # fp32 values
            ref = mu.dpm_coefficients64(tab, index, prev)
            for name, g, r in zip(("c_x", "c_0", "c_1"), got, ref):
                assert _ulp_apart(np.float32(g), np.float32(r)) <= 1, (S, index, prev, name, g, float(r))
            if prev is None:
                assert got[2] == 0.0
            else:
                assert got[1] > 0 and got[2] < 0 and got[0] > 0            # φ < 0: c_0 = −α'φ(...) > 0, c_1 < 0
        first = index == S - 1 or (index == 0 and S < 15)
        assert s.step_order(index) == (1 if first else 2) == mu.dpm_order(S, index)
        assert s.step_order(index, lower_order_final=False) == (1 if index == S - 1 else 2)
    if S == 14:
        # the uniform discretisation gives 15 timesteps for S = 14: the switch goes by the steps the loop takes
        s.make_schedule(14, verbose=False)
        assert len(s.ddim_timesteps) == 15 and s.step_order(0) == 2 and s.step_order(14) == 1
    # first order is the eta = 0 DDIM step: c_x x + c_0 D = sqrt(a') D + sqrt(1 - a') e with e = (x - sqrt(a) D)/sqrt(1 - a)
    for index in range(S):
        a, ap = np.float64(tab["ddim_alphas"][index]), np.float64(tab["ddim_alphas_prev"][index])
        c_x, c_0, _ = mu.dpm_coefficients64(tab, index)
        assert abs(c_x - np.sqrt((1 - ap) / (1 - a))) < 1e-12
        assert abs(c_0 - (np.sqrt(ap) - np.sqrt(a) * np.sqrt((1 - ap) / (1 - a)))) < 1e-12


@pytest.mark.parametrize("S", sorted(mu.SCENARIO_ERRORS))
def test_float64_restatement_reproduces_the_scenario_numbers(S):
    """Data N(0, 2²), the ideal model, exact x_T·sqrt(v(acp[0]) / v(acp[t_S])): the restatement's max-abs errors over
    x_T = (1.3, −0.7, 0.2, 2.1) are those of DESIGN.md §3.2's float64 table to its four digits."""
    got = mu.scenario_errors64(S)
    for name, g, want in zip(("DDIM", "PLMS", "DPM++ 2M"), got, mu.SCENARIO_ERRORS[S]):
        print(f"S = {S} {name}: {g:.4e} (table {want:.3e})")
        assert abs(g / want - 1.0) < 5e-4, (S, name, g, want)
    ddim, plms, dpm = got
    assert plms < ddim / 10 and dpm < ddim / 2


def test_restatement_orders(sdk):
    """The fp32 restatement itself: PLMS with a constant model output is DDIM (every combination of equal ε is ε up
    to rounding), and DPM first order is the DDIM step up to rounding."""
    xT = mu.randn(1, *mu.LOOP_SHAPE)
    b, _ = mu.stub_bias()
    const = lambda x, t: (b[0], None)                                 # noqa: E731
    for S in (3, 5):
        ref = mu.run_loop("ddim", const, xT, S)
        for kind in ("plms", "dpm"):
            out = mu.run_loop(kind, const, xT, S)
            assert len(out["calls"]) == S + (kind == "plms")
            assert np.abs(out["x"] - ref["x"]).max() < 2e-5, (S, kind)
