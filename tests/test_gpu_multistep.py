"""Multistep samplers on the GPU (run with -m gpu): the fused ``sdk_multistep_step`` forms, the PLMS and
DPM-Solver++(2M) loops, their accuracy on a model whose exact answer is known, and a tiny real UNet + VAE.

Kernel and loop tests compare with the numpy fp32 restatement of tests/multistep_util.py bit for bit: the kernel
evaluates the same expressions operation by operation without contraction, so no tolerance applies.  The accuracy
test is the check that the coefficients are the right ones and not merely self-consistent: with the ideal model
of Gaussian data both samplers must beat DDIM at the same number of steps by the margins the float64 restatement
shows (tests/test_multistep_boundary.py pins that restatement to the float64 numbers of the scenario).  The model-level
test compares the fp16-activation UNet with the fp32 CPU loop of the restatement driving oracle/unet_ref.py under
multistep_util.PARITY_LIMITS (at most 3.5x the errors measured on MI355X, profiles/multistep_parity_errors.txt)."""
import os

import numpy as np
import pytest
import torch

import multistep_util as mu
from ca_util import BLEND_MASKS
from golden_util import cfg_of, load, weights_of
from gpu_util import rel_l2

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SENTINEL = -12345.5
NAN = float("nan")


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    a = t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return a.view(np.uint32)


def _same(got, ref, what=""):
    assert np.array_equal(_bits(got), _bits(np.asarray(ref, dtype=F32))), what


class Boxed:
    """Tensors as views ``off`` elements into filled buffers (``off`` 1: not 16-byte aligned, the scalar path):
    operands sit in NaN, outputs in a sentinel; ``intact()`` checks that nothing outside the views was written."""
    PAD = 8

    def __init__(self, off):
        self.off, self.bufs = off, []

    def new(self, shape, src=None):
        n = int(np.prod(shape))
        fill = NAN if src is not None else SENTINEL
        buf = torch.full((n + 2 * self.PAD,), fill, dtype=torch.float32, device=DEV)
        v = buf[self.PAD + self.off:self.PAD + self.off + n].view(shape)
        if src is not None:
            v.copy_(torch.from_numpy(np.ascontiguousarray(src)))
        assert v.data_ptr() % 16 == 4 * self.off
        self.bufs.append((buf, n, fill))
        return v

    def intact(self):
        for buf, n, fill in self.bufs:
            lo, hi = self.PAD + self.off, self.PAD + self.off + n
            edge = torch.cat([buf[:lo], buf[hi:]])
            same = torch.isnan(edge) if fill != fill else edge == fill
            assert bool(same.all()), "written outside the view"


# ------------------------------------------------------------------ stand-in models
class StubLD:
    """What the samplers need of a model: the SD schedule's tables, a device, and ``apply_model``, which evaluates
    ``fn(x, t, uncond)`` with torch ops on the GPU and records every call's (x, t).  A doubled batch is
    classifier-free guidance: the first half is the unconditional one."""
    num_timesteps = mu.NUM_TIMESTEPS

    def __init__(self, sdk, fn, batch, parameterization="eps"):
        from sd_amd.DDIM.diffusion_modules import register_schedule
        tab = register_schedule(1000, 0.00085, 0.012)
        self.alphas_cumprod, self.alphas_cumprod_prev = tab["alphas_cumprod"], tab["alphas_cumprod_prev"]
        self.sqrt_alphas_cumprod = tab["sqrt_alphas_cumprod"]
        self.sqrt_one_minus_alphas_cumprod = tab["sqrt_one_minus_alphas_cumprod"]
        self.device, self.parameterization, self.fn, self.batch, self.calls = DEV, parameterization, fn, batch, []

    def apply_model(self, x, t, c):
        assert x.is_cuda and x.dtype == torch.float32 and bool((t == t[0]).all()) and t.shape[0] == x.shape[0]
        step, b = int(t[0]), self.batch
        if x.shape[0] == 2 * b:
            assert torch.equal(x[:b], x[b:]) and c.shape[0] == 2 * b
            self.calls.append((x[b:].clone(), step))
            return torch.cat([self.fn(x[:b], step, True), self.fn(x[b:], step, False)])
        assert x.shape[0] == b
        self.calls.append((x.clone(), step))
        return self.fn(x, step, False)


def _bias_model(b, bu):
    gb, gbu = _gpu(b), _gpu(bu)
    return lambda x, t, uncond: 0.25 * x + (gbu if uncond else gb)[t % 8]


def _sampler(kind, ld):
    from sd_amd.DDIM.ddim import DDIMSampler
    from sd_amd.DDIM.dpm_solver import DPMSolverSampler
    from sd_amd.DDIM.plms import PLMSSampler
    return {"ddim": DDIMSampler, "plms": PLMSSampler, "dpm": DPMSolverSampler}[kind](ld)


def _run(kind, ld, S, xT, cond=None, **kw):
    """Through ``sample`` where the uniform grid has S timesteps, else ``make_schedule`` (quad) + the loop method."""
    s = _sampler(kind, ld)
    shape = tuple(xT.shape)
    if mu.discretize(S) == "uniform":
        if kind == "ddim":
            kw["eta"] = 0.0
        return s.sample(S, shape[0], shape[1:], conditioning=cond, x_T=xT, verbose=False, log_every_t=1, **kw)
    s.make_schedule(S, ddim_discretize=mu.discretize(S), verbose=False)
    assert len(s.ddim_timesteps) == S
    loop = {"ddim": "ddim_sampling", "plms": "plms_sampling", "dpm": "dpm_sampling"}[kind]
    return getattr(s, loop)(cond, shape, x_T=xT, log_every_t=1, **kw)


# ------------------------------------------------------------------ kernel forms
FORMS = [("plms", 0), ("plms", 1), ("plms", 2), ("plms", 3), ("plms_warmup", 0), ("dpm", 0), ("dpm", 1)]
KERNEL_CASES = [(s, 0) for s in mu.KERNEL_SHAPES] + [(mu.KERNEL_SHAPES[0], 1)]
KERNEL_S, KERNEL_INDEX, BLEND_T = 4, 2, 251


def _kernel_inputs(shape):
    s = 8001 + 17 * int(np.prod(shape))
    names = ("x", "e", "eu", "h1", "h2", "h3", "en", "x0", "qn")
    return {k: mu.randn(s + i, *shape) * F32(0.5 if k in ("e", "eu", "h1", "h2", "h3", "en") else 1.0)
            for i, k in enumerate(names)}


def _expected(form, nhist, k, sc, coefs, guided, v):
    """(x_prev, pred_x0, history entry) of one form by the restatement."""
    e = mu.guided_eps(k["x"], k["e"], k["eu"] if guided else None, mu.GUIDANCE,
                      (sc["v_sqrt_a"], sc["v_sqrt_1ma"]) if v else None)
    hist = [k["h1"], k["h2"], k["h3"]][:nhist]
    if form == "dpm":
        xp, d = mu.dpm_step(k["x"], e, sc, [F32(c) for c in coefs], hist[0] if nhist else None)
        return xp, d, d
    ep = mu.plms_eprime(e, hist, k["en"] if form == "plms_warmup" else None)
    xp, p0 = mu.ddim0(k["x"], ep, sc)
    return xp, p0, e


@pytest.mark.parametrize("shape,off", KERNEL_CASES, ids=["x".join(map(str, s)) + ("_offset1" if o else "") for s, o in KERNEL_CASES])
def test_kernel_forms_bitexact_vs_restatement(sdk, shape, off):
    from sd_amd import ops
    k = _kernel_inputs(shape)
    tab = mu.tables(KERNEL_S)
    sc = mu.scalars(tab, KERNEL_INDEX)
    dpm = _sampler("dpm", StubLD(sdk, None, shape[0]))
    dpm.make_schedule(KERNEL_S, verbose=False)
    masks = [(kind, binary, mu.blend_mask(kind, binary, shape)) for kind in BLEND_MASKS for binary in (True, False)]
    for form, nhist in FORMS:
        coefs = dpm.step_coefficients(KERNEL_INDEX, KERNEL_INDEX + 1 if nhist else None) if form == "dpm" else None
        for guided in (False, True):
            for v in (False, True):
                tag = f"{form} nhist {nhist} guided {guided} v {v}"
                want_xp, want_p0, want_h = _expected(form, nhist, k, sc, coefs, guided, v)
                for blend in [None] + (masks if guided and v else []):
                    box = Boxed(off)
                    x, e = box.new(shape, k["x"]), box.new(shape, k["e"])
                    hist = [box.new(shape, k[n]) for n in ("h1", "h2", "h3")[:nhist]]
                    kw = dict(history=hist, x_prev=box.new(shape), pred_x0=box.new(shape))
                    # the history entry goes over the oldest one where there is one (read and written by one launch)
                    kw["hist_out"] = hist[-1] if hist else box.new(shape)
                    if guided:
                        kw.update(e_uncond=box.new(shape, k["eu"]), guidance=mu.GUIDANCE)
                    if v:
                        kw.update(v_param=(float(sc["v_sqrt_a"]), float(sc["v_sqrt_1ma"])))
                    if form == "plms_warmup":
                        kw.update(e_next=box.new(shape, k["en"]))
                    if form == "dpm":
                        kw.update(coefs=coefs)
                    if blend is not None:
                        sa = tab["schedule"]["sqrt_alphas_cumprod"][BLEND_T]
                        s1m = tab["schedule"]["sqrt_one_minus_alphas_cumprod"][BLEND_T]
                        # the blended next input goes over x (read and written by one launch)
                        kw.update(blend_x0=box.new(shape, k["x0"]), blend_noise=box.new(shape, k["qn"]),
                                  blend_mask=_gpu(blend[2]), blend_sqrt_acp=float(sa), blend_sqrt_1m_acp=float(s1m),
                                  x_next=x)
                    outs = ops.multistep_step(x, e, sc, form, **kw)
                    assert outs[0].data_ptr() == kw["x_prev"].data_ptr() and outs[1].data_ptr() == kw["pred_x0"].data_ptr()
                    _same(outs[0], want_xp, tag + " x_prev")
                    _same(outs[1], want_p0, tag + " pred_x0")
                    _same(kw["hist_out"], want_h, tag + " hist_out")
                    for h, n in zip(hist[:-1], ("h1", "h2")):
                        _same(h, k[n], tag + " history written")
                    if blend is not None:
                        assert outs[2].data_ptr() == x.data_ptr()
                        _same(x, mu.blend(k["x0"], k["qn"], blend[2], want_xp, tab, BLEND_T),
                              f"{tag} blend {blend[0]} binary {blend[1]}")
                    else:
                        _same(x, k["x"], tag + " x written")
                    box.intact()


def test_grid_stride_and_argument_errors(sdk):
    """More work than one pass of the capped grid (2048 blocks x 256 threads x 4 elements) plus a tail, and the
    argument checks of the op."""
    from sd_amd import ops
    n = 2048 * 256 * 4 + 23
    shape = (1, 1, 1, n)
    k = {name: mu.randn(8500 + i, *shape) for i, name in enumerate(("x", "e", "eu", "h1", "h2", "h3"))}
    sc = mu.scalars(mu.tables(KERNEL_S), KERNEL_INDEX)
    e = mu.guided_eps(k["x"], k["e"], k["eu"], mu.GUIDANCE, None)
    want_xp, want_p0 = mu.ddim0(k["x"], mu.plms_eprime(e, [k["h1"], k["h2"], k["h3"]]), sc)
    g = {name: _gpu(a) for name, a in k.items()}
    hist = [g["h1"], g["h2"], g["h3"]]
    xp, p0 = ops.multistep_step(g["x"], g["e"], sc, "plms", history=hist, e_uncond=g["eu"], guidance=mu.GUIDANCE,
                                hist_out=g["h3"])
    _same(xp, want_xp), _same(p0, want_p0), _same(g["h3"], e)
    x, ee = g["x"][..., :16].contiguous(), g["e"][..., :16].contiguous()
    with pytest.raises(ValueError, match="form"):
        ops.multistep_step(x, ee, sc, "heun")
    with pytest.raises(ValueError, match="history"):
        ops.multistep_step(x, ee, sc, "dpm", history=[x, x], coefs=(1., 1., 1.))
    with pytest.raises(ValueError, match="e_next"):
        ops.multistep_step(x, ee, sc, "plms_warmup")
    with pytest.raises(ValueError, match="coefs"):
        ops.multistep_step(x, ee, sc, "dpm")
    with pytest.raises(ValueError, match="eta = 0"):
        ops.multistep_step(x, ee, dict(sc, sigma=0.5), "plms")
    with pytest.raises(ValueError, match="hist_out"):
        ops.multistep_step(x, ee, sc, "plms", hist_out=g["x"])
    with pytest.raises(ValueError, match=r"history\[0\]"):
        ops.multistep_step(x, ee, sc, "plms", history=[g["x"]])
    with pytest.raises(ValueError, match="blend_mask"):
        ops.multistep_step(x, ee, sc, "plms", blend_x0=x)
    with pytest.raises(TypeError):
        ops.multistep_step(x.cpu(), ee, sc, "plms")


# ------------------------------------------------------------------ loops
LOOP_CASES = [("plms", S, True) for S in mu.PLMS_STEPS] + [("dpm", S, True) for S in mu.DPM_STEPS] + [("dpm", 14, False)]


def _check_loop(sdk, kind, S, lower_order_final=True, guided=False, v=False, mask_kind=None):
    b, bu = mu.stub_bias()
    d = mu.loop_inputs()
    B = mu.LOOP_SHAPE[0]
    ld = StubLD(sdk, _bias_model(b, bu), B, "v" if v else "eps")
    kw, rkw = {}, {}
    cond = None
    if guided:
        cond = torch.zeros(B, 1, device=DEV)
        kw.update(unconditional_guidance_scale=mu.GUIDANCE, unconditional_conditioning=torch.ones(B, 1, device=DEV))
        rkw.update(g=mu.GUIDANCE)
    if mask_kind is not None:
        m = mu.blend_mask(mask_kind, mask_kind != "bchw", mu.LOOP_SHAPE)          # bchw: fractional
        qn = _gpu(d["qn"])
        kw.update(mask=_gpu(m), x0=_gpu(d["x0"]), q_noise_fn=lambda i, shape: qn[i])
        rkw.update(mask=m, x0=d["x0"], qn=d["qn"])
    if kind == "dpm":
        kw.update(lower_order_final=lower_order_final)
        rkw.update(lower_order_final=lower_order_final)
    xT = _gpu(d["xT"])
    x, inter = _run(kind, ld, S, xT, cond, **kw)
    ref = mu.run_loop(kind, mu.stub_model(b, bu), d["xT"], S, v=v, **rkw)
    tag = f"{kind} S {S}"
    assert len(ld.calls) == len(ref["calls"]) == S + (kind == "plms"), tag
    for n, ((gx, gt), (rx, rt)) in enumerate(zip(ld.calls, ref["calls"])):
        assert gt == rt, f"{tag}: model call {n} at t = {gt}, restatement {rt}"
        _same(gx, rx, f"{tag}: x of model call {n}")
    _same(x, ref["x"], tag + " result")
    assert len(inter["x_inter"]) == S + 1 == len(inter["pred_x0"])
    for i in range(S):
        _same(inter["x_inter"][i + 1], ref["x_inter"][i], f"{tag}: x_inter of step {i}")
        _same(inter["pred_x0"][i + 1], ref["pred_x0"][i], f"{tag}: pred_x0 of step {i}")
    _same(xT, d["xT"], "x_T was written")
    return ld


@pytest.mark.parametrize("kind,S,lof", LOOP_CASES, ids=[f"{k}_S{S}" + ("" if lof else "_no_lower_order_final")
                                                      for k, S, lof in LOOP_CASES])
def test_loops_bitexact_vs_restatement(sdk, kind, S, lof):
    _check_loop(sdk, kind, S, lof)


@pytest.mark.parametrize("variant", ["cfg", "v", "cfg_v"] + ["mask_" + m for m in BLEND_MASKS])
@pytest.mark.parametrize("kind,S", [("plms", 5), ("dpm", 4)])
def test_loop_variants_bitexact_vs_restatement(sdk, kind, S, variant):
    _check_loop(sdk, kind, S, guided="cfg" in variant, v=variant.endswith("v"),
                mask_kind=variant[5:] if variant.startswith("mask_") else None)


def test_loop_callbacks_and_draws(sdk):
    """callback / img_callback / log_every_t as in DDIMSampler, and the loops draw x_T and the q-noise themselves."""
    b, bu = mu.stub_bias()
    d = mu.loop_inputs()
    B = mu.LOOP_SHAPE[0]
    for kind in ("plms", "dpm"):
        ld = StubLD(sdk, _bias_model(b, bu), B)
        seen, imgs = [], []
        s = _sampler(kind, ld)
        x, inter = s.sample(8, B, mu.LOOP_SHAPE[1:], verbose=False, log_every_t=3, callback=seen.append,
                            img_callback=lambda p0, i: imgs.append(i), mask=_gpu(mu.blend_mask("b1hw", True, mu.LOOP_SHAPE)),
                            x0=_gpu(d["x0"]))
        assert seen == list(range(8)) == imgs and tuple(x.shape) == mu.LOOP_SHAPE and bool(torch.isfinite(x).all())
        assert len(inter["x_inter"]) == 1 + len([i for i in range(8) if i % 3 == 0 or i == 7])


# ------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("S", sorted(mu.SCENARIO_ERRORS))
def test_accuracy_against_ddim_on_the_ideal_gaussian_model(sdk, S):
    """Data N(0, 2²): ε*(x, t) = σ_t x / (a_t s² + 1 − a_t) and the exact result is known.  All three samplers in
    one test, fp32 on the GPU; the float64 ratios are 62 / 170 (PLMS) and 2.3 / 3.8 (DPM++) at S = 10 / 20."""
    tab = mu.tables(S)
    ac = tab["schedule"]["alphas_cumprod"].astype(np.float64)
    coef = np.sqrt(1.0 - ac) / mu.scenario_variance(ac)
    xT = _gpu(np.asarray(mu.SCENARIO_XT, dtype=F32).reshape(1, 1, 2, 2))
    exact = mu.scenario_exact(S)
    err = {}
    for kind in ("ddim", "plms", "dpm"):
        ld = StubLD(sdk, lambda x, t, uncond: x * float(F32(coef[t])), 1)
        x, _ = _run(kind, ld, S, xT)
        err[kind] = float(np.abs(x.cpu().numpy().astype(np.float64).reshape(-1) - exact).max())
        assert len(ld.calls) == S + (kind == "plms")
    want = dict(zip(("ddim", "plms", "dpm"), mu.SCENARIO_ERRORS[S]))
    print(f"S = {S}: " + ", ".join(f"{k} {err[k]:.4e} (float64 {want[k]:.3e})" for k in err), flush=True)
    assert err["plms"] < err["ddim"] / 10, err
    assert err["dpm"] < err["ddim"] / 2, err


# ------------------------------------------------------------------ tiny real model
def _tiny_ld(graphs):
    import yaml
    from sd_amd.Diffusion.utils import instantiate_from_config
    u, v = load("unet_tiny"), load("vae_tiny")
    y = yaml.safe_load(open(os.path.join(ROOT, "configs", "sd-v1-txt2img.yaml")))["model"]
    y["params"]["unet_config"]["params"] = cfg_of(u)
    y["params"]["first_stage_config"]["params"]["ddconfig"] = cfg_of(v)
    y["params"]["cond_stage_config"] = None
    ld = instantiate_from_config(y)
    ld.model.diffusion_model.load_state_dict(weights_of(u))
    ld.first_stage_model.load_state_dict(weights_of(v))
    ld = ld.to(DEV)
    ld.use_graphs(graphs)
    return ld


def make_tiny_inputs():
    u = load("unet_tiny")
    g = torch.Generator().manual_seed(23)
    return dict(xT=torch.randn(2, 4, 16, 16, generator=g), c=torch.from_numpy(u["ctx"]).float(),
                uc=torch.randn(*u["ctx"].shape, generator=g))


@pytest.fixture(scope="module")
def tiny_inputs():
    return make_tiny_inputs()


def tiny_reference(kind, inp, scale_factor):
    """The fp32 CPU chain: the restatement's loop on oracle/unet_ref.py, then oracle/vae_ref.py's decode."""
    from oracle import unet_ref, vae_ref
    u, v = load("unet_tiny"), load("vae_tiny")
    usd, ucfg = weights_of(u), cfg_of(u)

    def model(x, t):
        xt, tt = torch.from_numpy(x), torch.full((x.shape[0],), t, dtype=torch.long)
        return tuple(unet_ref.unet_forward(usd, ucfg, xt, tt, c).contiguous().numpy() for c in (inp["c"], inp["uc"]))

    z = mu.run_loop(kind, model, inp["xT"].numpy(), mu.MODEL_STEPS, g=mu.MODEL_SCALE)["x"]
    return torch.from_numpy(z), vae_ref.decode_first_stage(weights_of(v), cfg_of(v), torch.from_numpy(z), scale_factor)


def tiny_sample(kind, ld, inp):
    kw = dict(eta=0.0) if kind == "ddim" else {}
    z, _ = _sampler(kind, ld).sample(mu.MODEL_STEPS, 2, (4, 16, 16), conditioning=inp["c"].to(DEV), verbose=False,
                                     x_T=inp["xT"].to(DEV), unconditional_guidance_scale=mu.MODEL_SCALE,
                                     unconditional_conditioning=inp["uc"].to(DEV), **kw)
    return z, ld.decode_first_stage(z)


@pytest.mark.parametrize("kind", ["plms", "dpm"])
def test_tiny_model_graphs_equal_eager_and_vs_fp32_reference(sdk, kind, tiny_inputs):
    """4 steps with CFG on unet_tiny, then decode_first_stage on vae_tiny: graph replay gives the eager bits, and
    the image is within multistep_util.PARITY_LIMITS (3.5x the rel-L2 measured on MI355X) of the fp32 CPU chain."""
    ld = _tiny_ld(False)
    z, img = (t.clone() for t in tiny_sample(kind, ld, tiny_inputs))
    ld.use_graphs(True)
    for rnd in range(2):
        zg, ig = tiny_sample(kind, ld, tiny_inputs)
        assert np.array_equal(_bits(zg), _bits(z)) and np.array_equal(_bits(ig), _bits(img)), f"round {rnd}"
    zr, ir = tiny_reference(kind, tiny_inputs, ld.scale_factor)
    rz, ri = rel_l2(z, zr), rel_l2(img, ir)
    limit = mu.PARITY_LIMITS[kind]
    print(f"[parity] tiny {kind} x{mu.MODEL_STEPS} CFG vs fp32 reference: latent rel-L2 {rz:.3e}, image rel-L2 {ri:.3e} "
          f"(<= {limit})", flush=True)
    assert limit is not None and rz <= limit[0] and ri <= limit[1], (rz, ri, limit)
