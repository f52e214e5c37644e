"""Sampler options on the GPU (run with -m gpu): DDIM mask / x0, original steps, noise dropout, score correctors,
progressive_denoising, shorten_cond_schedule, sample_log.

Kernel and loop tests compare with fixtures written by the reference's own functions
(tests/golden/make_golden_sampler_options.py) bit for bit: the kernels evaluate the reference's fp32 expressions
operation by operation without contraction, so no tolerance applies.  The reference has no v-prediction, so the
v forms are compared with the same torch expressions evaluated on the CPU inside the test, as is the grid-stride
case.  The step fixtures cover eta x temperature x guidance x dropout per shape; the blend fixtures cover every
mask shape, binary and fractional, at both etas on the fullest step form, and for EVERY step form the fused blend
must equal ``masked_q_sample(ddim_step(...))`` bit for bit.  The model-level test compares the fp16-activation
UNet with the reference's fp32 run under sampler_opt_util.PARITY_LIMITS (at most 3.5x the errors measured on
MI355X, profiles/sampler_options_parity_errors.txt)."""
import types

import numpy as np
import pytest
import torch

import ca_util as cu
import sampler_opt_util as su
import vq_util as vu
from golden_util import cfg_of, load, weights_of
from gpu_util import check_parity

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32
SENTINEL = -12345.5


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(got, ref, what=""):
    """fp32 equality as np.array_equal sees it (the reference fixture as the yardstick)."""
    assert np.array_equal(got.detach().cpu().numpy(), np.asarray(ref)), what


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


# ------------------------------------------------------------------ stand-in model
def _stub_ld(sdk, schedule=su.SCHEDULE, parameterization="eps", outputs=None, uncond=None, codebook=None,
             conditioning_key=None, num_timesteps_cond=1):
    """A LatentDiffusion whose apply_model returns recorded tensors by timestep (``uncond[t]`` in front for a
    doubled batch) and records the conditioning it received; no UNet / first stage."""
    from sd_amd.Diffusion.ddpm import LatentDiffusion

    class StubLD(LatentDiffusion):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.parameterization, self.clip_denoised, self.v_posterior = parameterization, False, 0.
            self.log_every_t = 1
            self.channels, self.image_size = su.LOOP_SHAPE[1], su.LOOP_SHAPE[2]
            self.model = types.SimpleNamespace(conditioning_key=conditioning_key)
            kw = dict(schedule)
            self.register_schedule(beta_schedule=kw.pop("beta_schedule"), **kw)
            self.num_timesteps_cond = num_timesteps_cond
            self.shorten_cond_schedule = num_timesteps_cond > 1
            if self.shorten_cond_schedule:
                self.make_cond_schedule()
            self.cur, self.conds = None, []

        @property
        def device(self):
            return self.betas.device

        def apply_model(self, x_noisy, t, cond, return_ids=False):
            self.cur = int(t[0])
            if torch.is_tensor(cond):
                self.conds.append(cond.clone())
            e = outputs[self.cur]
            return torch.cat([uncond[self.cur], e]) if x_noisy.shape[0] == 2 * e.shape[0] else e

    ld = StubLD()
    if codebook is not None:
        from sd_amd.vqvae.quantize import VectorQuantize2
        q = VectorQuantize2(codebook.shape[0], codebook.shape[1], 0.25)
        q.load_state_dict({"embedding.weight": torch.from_numpy(codebook)}, strict=False)
        ld.first_stage_model = torch.nn.Module()
        ld.first_stage_model.quantize = q
    return ld.to(DEV)


class Corrector:
    """Adds a recorded tensor (by timestep) to the score, as the fixture generator's."""
    def __init__(self, add):
        self.add, self.models = add, []

    def modify_score(self, model, e_t, x, t, c, scale=1.0):
        self.models.append(model)
        return e_t + scale * self.add[int(t[0])]


def _sampler(ld, eta, steps=su.S):
    from sd_amd.DDIM.ddim import DDIMSampler
    s = DDIMSampler(ld)
    s.make_schedule(steps, ddim_eta=eta, verbose=False)
    return s


# ------------------------------------------------------------------ kernel forms
class Boxed:
    """Tensors as views ``off`` elements into sentinel-filled buffers (``off`` 1: not 16-byte aligned, the scalar
    path); ``intact()`` checks that nothing outside the views was written."""
    PAD = 8

    def __init__(self, off):
        self.off, self.bufs = off, []

    def new(self, shape, src=None, dtype=torch.float32, fill=SENTINEL):
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * self.PAD,), fill, dtype=dtype, device=DEV)
        v = buf[self.PAD + self.off:self.PAD + self.off + n].view(shape)
        if src is not None:
            v.copy_(src if torch.is_tensor(src) else torch.from_numpy(np.ascontiguousarray(src)))
        assert dtype != torch.float32 or v.data_ptr() % 16 == 4 * self.off
        self.bufs.append((buf, n, fill))
        return v

    def intact(self):
        for buf, n, fill in self.bufs:
            lo, hi = self.PAD + self.off, self.PAD + self.off + n
            edge = torch.cat([buf[:lo], buf[hi:]])
            same = torch.isnan(edge) if fill != fill else edge == fill
            assert bool(same.all()), "written outside the output"


def _ref_step(x, e, sc, nz, temp, keep=None, p=0.0, eu=None, g=1.0, v=None, pred_in=None):
    """The reference's expressions (ddim.py:171-204; v: e = sqrt(a) v + sqrt(1 - a) x) with torch on the CPU."""
    S = lambda val: torch.full((x.shape[0], 1, 1, 1), float(val))        # noqa: E731
    if eu is not None:
        e = eu + g * (e - eu)
    if v is not None:
        e = S(v[0]) * e + S(v[1]) * x
    pred = (x - S(sc["sqrt_one_minus_at"]) * e) / S(sc["sqrt_at"]) if pred_in is None else pred_in
    noise = S(sc["sigma"]) * nz * temp
    if keep is not None:
        noise = noise * (keep.float() * (0.0 if p == 1.0 else float(F32(1.0 / (1.0 - p)))))
    return S(sc["sqrt_a_prev"]) * pred + S(sc["dir_coef"]) * e + noise, pred


def _ref_blend(x0, qn, mask, img, sa, s1m):
    return (float(sa) * x0 + float(s1m) * qn) * mask + (1. - mask) * img


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("shape", su.KERNEL_SHAPES, ids=su.shape_tag)
def test_step_forms_bitexact_vs_reference(sdk, shape, off):
    from sd_amd import ops
    fx = load("so_kernel")
    k = su.kernel_inputs(shape)
    ld = _stub_ld(sdk)
    tab = ld._host_tables()
    masks = [(kind, binary, su.mask_of(kind, binary, shape)) for kind in su.MASK_KINDS for binary in (True, False)]
    for eta, temp, guided, p in su.step_combos():
        sc = _sampler(ld, eta).step_scalars(2)
        box = Boxed(off)
        x, e, eu, nz = (box.new(shape, k[n]) for n in ("xT", "e", "eu", "nz"))
        kw = dict(temperature=temp)
        if guided:
            kw.update(e_uncond=eu, guidance=su.GUIDANCE)
        if eta > 0:
            kw.update(noise=nz)
            if p > 0:
                kw.update(keep=box.new(shape, fx[su.keep_tag(shape, p)], dtype=torch.uint8, fill=7), drop_p=p)
        xp, p0 = ops.ddim_step(x, e, sc, x_prev=box.new(shape), pred_x0=box.new(shape), **kw)
        tag = su.step_tag(shape, eta, temp, guided, p)
        _same(xp, fx[tag + "_xprev"], tag)
        _same(p0, fx[f"k{su.shape_tag(shape)}_g{int(guided)}_pred_x0"], tag + " pred_x0")
        # the second half, fed the first half's pred_x0 (and a NaN x it must not read), gives the same x_prev
        nan_x = box.new(shape, fill=float("nan"))
        xp2 = ops.ddim_xprev(p0, e, sc, x=nan_x, x_prev=box.new(shape), **kw)
        assert np.array_equal(_bits(xp2), _bits(xp)), tag + " xprev half"
        # cfg_combine followed by an unguided step is the guided step
        if guided:
            ec = ops.cfg_combine(eu, e, su.GUIDANCE, out=box.new(shape))
            kw1 = {a: b for a, b in kw.items() if a not in ("e_uncond", "guidance")}
            xp3, p03 = ops.ddim_step(x, ec, sc, **kw1)
            assert np.array_equal(_bits(xp3), _bits(xp)) and np.array_equal(_bits(p03), _bits(p0)), tag + " combine"
        # v-prediction (no reference path): the torch expressions on the CPU
        vp = (sc["v_sqrt_a"], sc["v_sqrt_1ma"])
        cpu = {n: torch.from_numpy(k[n]) for n in ("xT", "e", "eu", "nz")}
        keep_c = torch.from_numpy(fx[su.keep_tag(shape, p)]) if "keep" in kw else None
        rx, rp = _ref_step(cpu["xT"], cpu["e"], sc, cpu["nz"], temp, keep_c, p, cpu["eu"] if guided else None,
                           su.GUIDANCE, v=vp)
        xv, pv = ops.ddim_step(x, e, sc, v_param=vp, x_prev=box.new(shape), pred_x0=box.new(shape), **kw)
        assert torch.equal(xv.cpu(), rx) and torch.equal(pv.cpu(), rp), tag + " v"
        xv2 = ops.ddim_xprev(pv, e, sc, x=x, v_param=vp, **kw)
        assert np.array_equal(_bits(xv2), _bits(xv)), tag + " v xprev half"
        # the same reference expressions reproduce the fixture (the yardstick of the v comparison)
        rx0, _ = _ref_step(cpu["xT"], cpu["e"], sc, cpu["nz"], temp, keep_c, p, cpu["eu"] if guided else None, su.GUIDANCE)
        _same(rx0, fx[tag + "_xprev"], tag + " torch expressions")
        # dropout p = 1 multiplies the noise term by zero
        if eta > 0 and p == 0:
            z = torch.zeros(shape, dtype=torch.uint8, device=DEV)
            xz, _ = ops.ddim_step(x, e, sc, **dict(kw, keep=z, drop_p=1.0))
            x0n, _ = ops.ddim_step(x, e, sc, **dict(kw, noise=torch.zeros_like(x)))
            assert torch.equal(xz, x0n), tag + " p = 1"
        # the fused blend of the next iteration equals the two launches, for every mask form
        x0, qn = box.new(shape, k["x0"]), box.new(shape, k["qn1"])
        for kind, binary, m in masks:
            mk = _gpu(m)
            xpf, p0f, xn = ops.ddim_step(x, e, sc, x_prev=box.new(shape), pred_x0=box.new(shape), blend_x0=x0,
                                         blend_noise=qn, blend_mask=mk, blend_sqrt_acp=float(tab["sqrt_acp"][3]),
                                         blend_sqrt_1m_acp=float(tab["sqrt_1m_acp"][3]), x_next=box.new(shape), **kw)
            two = ops.masked_q_sample(x0.contiguous(), qn.contiguous(), mk, xp.contiguous(), 3, tab["sqrt_acp"],
                                      tab["sqrt_1m_acp"])
            assert np.array_equal(_bits(xpf), _bits(xp)) and np.array_equal(_bits(p0f), _bits(p0))
            assert np.array_equal(_bits(xn), _bits(two)), f"{tag} {kind} {binary}: fused blend != two launches"
            _, xn2 = ops.ddim_xprev(p0, e, sc, blend_x0=x0, blend_noise=qn, blend_mask=mk,
                                    blend_sqrt_acp=float(tab["sqrt_acp"][3]),
                                    blend_sqrt_1m_acp=float(tab["sqrt_1m_acp"][3]), **kw)
            assert np.array_equal(_bits(xn2), _bits(two))
        box.intact()


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("shape", su.KERNEL_SHAPES, ids=su.shape_tag)
def test_fused_blend_bitexact_vs_reference(sdk, shape, off):
    """The reference's own loop: blend of x_T (t = 5), the step on it, the blend that opens the next iteration
    (t = 3) — the last two in one launch."""
    from sd_amd import ops
    fx = load("so_kernel")
    k = su.kernel_inputs(shape)
    ld = _stub_ld(sdk)
    tab = ld._host_tables()
    temp, p = su.BLEND_STEP["temp"], su.BLEND_STEP["p"]
    for eta in su.ETAS:
        sc = _sampler(ld, eta).step_scalars(2)
        for kind in su.MASK_KINDS:
            for binary in (True, False):
                tag = su.blend_tag(shape, eta, kind, binary)
                box = Boxed(off)
                xT, e, eu, nz, x0, qn0, qn1 = (box.new(shape, k[n]) for n in ("xT", "e", "eu", "nz", "x0", "qn0", "qn1"))
                mk = _gpu(su.mask_of(kind, binary, shape))
                first = ops.masked_q_sample(x0.contiguous(), qn0.contiguous(), mk, xT.contiguous(), 5, tab["sqrt_acp"],
                                            tab["sqrt_1m_acp"])
                _same(first, fx[tag + "_first"], tag + " first blend")
                kw = dict(temperature=temp, e_uncond=eu, guidance=su.GUIDANCE)
                if eta > 0:
                    kw.update(noise=nz, keep=box.new(shape, fx[su.keep_tag(shape, p)], dtype=torch.uint8, fill=7), drop_p=p)
                xin = box.new(shape, first)
                xp, _, xn = ops.ddim_step(xin, e, sc, x_prev=box.new(shape), pred_x0=box.new(shape), blend_x0=x0,
                                          blend_noise=qn1, blend_mask=mk, blend_sqrt_acp=float(tab["sqrt_acp"][3]),
                                          blend_sqrt_1m_acp=float(tab["sqrt_1m_acp"][3]), x_next=box.new(shape), **kw)
                _same(xp, fx[tag + "_xprev"], tag + " x_prev (unblended)")
                _same(xn, fx[tag + "_next"], tag + " next blend")
                # in place over the step's input
                _, _, xn2 = ops.ddim_step(xin, e, sc, blend_x0=x0, blend_noise=qn1, blend_mask=mk,
                                          blend_sqrt_acp=float(tab["sqrt_acp"][3]),
                                          blend_sqrt_1m_acp=float(tab["sqrt_1m_acp"][3]), x_next=xin, **kw)
                assert xn2.data_ptr() == xin.data_ptr()
                _same(xin, fx[tag + "_next"], tag + " in place")
                box.intact()


POST_IDS = ["x".join(map(str, s)) for s, _ in cu.STEP_CASES]


@pytest.mark.parametrize("p", su.POST_DROPS, ids=lambda v: f"p{v}")
@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("param", cu.STEP_PARAMS)
@pytest.mark.parametrize("case", cu.STEP_CASES, ids=POST_IDS)
def test_posterior_step_with_dropout_bitexact_vs_reference(sdk, case, param, clip, p):
    from sd_amd import ops
    shape, t = case
    fx = load("so_posterior")
    x, mo, nz = (_gpu(a) for a in cu.step_inputs(shape))
    keep = _gpu(fx[su.keep_tag(shape, p)])
    ld = _stub_ld(sdk, cu.STEP_SCHEDULE, param, outputs={tt: mo for tt in t})
    tt = torch.tensor(t, device=DEV)
    xp = ld.p_sample(x, None, tt, clip_denoised=clip, temperture=su.POST_TEMP, noise_dropout=p, noise=nz, keep=keep)
    _same(xp, fx[su.post_tag(shape, param, clip, p) + "_xprev"])
    # a bool keep mask, an unaligned in-place update and the two halves give the same bits
    tab = ld._host_tables()
    kw = dict(noise=nz, temperature=su.POST_TEMP, keep=keep.bool(), drop_p=p)
    box = Boxed(1)
    xs = box.new(shape, x)
    out, _ = ops.posterior_step(xs, mo, t, tab, clip=clip, x0_param=param == "x0", x_prev=xs, **kw)
    assert out.data_ptr() == xs.data_ptr() and np.array_equal(_bits(xs), _bits(xp))
    box.intact()
    _, xr = ops.posterior_step(x, mo, t, tab, stage=1, clip=clip, x0_param=param == "x0")
    xp2, _ = ops.posterior_step(x, None, t, tab, stage=2, x_recon_in=xr, **kw)
    assert np.array_equal(_bits(xp2), _bits(xp))
    # p = 1: zeros, as torch returns
    zero, _ = ops.posterior_step(x, mo, t, tab, clip=clip, x0_param=param == "x0", noise=nz,
                                 keep=torch.zeros_like(keep), drop_p=1.0)
    mean, _ = ops.posterior_step(x, mo, t, tab, clip=clip, x0_param=param == "x0", noise=torch.zeros_like(nz))
    assert torch.equal(zero, mean)


def test_grid_stride_and_tail(sdk):
    """More work than one pass of the capped grid (2048 blocks x 256 threads x 4 elements), plus a tail."""
    from sd_amd import ops
    n = 2048 * 256 * 4 + 23
    shape = (1, 1, 1, n)
    g = torch.Generator().manual_seed(11)
    x, e, eu, nz, x0, qn = (torch.randn(shape, generator=g) for _ in range(6))
    mask = torch.rand(shape, generator=g)
    keep = torch.rand(shape, generator=g) > 0.3
    a_t, a_prev, sigma = F32(0.5), F32(0.6), F32(0.3)
    sc = {"sqrt_one_minus_at": float(np.sqrt(F32(1) - a_t)), "sqrt_at": float(np.sqrt(a_t)),
          "dir_coef": float(np.sqrt(F32(F32(1) - a_prev) - sigma * sigma)), "sqrt_a_prev": float(np.sqrt(a_prev)),
          "sigma": float(sigma)}
    sa, s1m = float(F32(0.8)), float(F32(0.6))
    rx, rp = _ref_step(x, e, sc, nz, 0.7, keep, 0.3, eu, 2.5)
    X, E, EU, NZ, X0, QN, M, K = (t.to(DEV) for t in (x, e, eu, nz, x0, qn, mask, keep))
    xp, p0, xn = ops.ddim_step(X, E, sc, noise=NZ, e_uncond=EU, guidance=2.5, temperature=0.7, keep=K, drop_p=0.3,
                               blend_x0=X0, blend_noise=QN, blend_mask=M, blend_sqrt_acp=sa, blend_sqrt_1m_acp=s1m)
    assert torch.equal(xp.cpu(), rx) and torch.equal(p0.cpu(), rp)
    assert torch.equal(xn.cpu(), _ref_blend(x0, qn, mask, rx, sa, s1m))
    assert torch.equal(ops.cfg_combine(EU, E, 2.5).cpu(), eu + 2.5 * (e - eu))
    tab = {k: np.asarray([v], dtype=F32) for k, v in dict(c_recip=1.3, c_recipm1=0.8, coef1=0.4, coef2=0.6,
                                                           sigma=0.5).items()}
    tab = {k: np.concatenate([v, v]) for k, v in tab.items()}        # t = 1: nonzero
    got, _ = ops.posterior_step(X.view(1, n), E.view(1, n), 1, tab, noise=NZ.view(1, n), temperature=0.7,
                                keep=K.view(1, n), drop_p=0.3)
    x1, e1, n1, k1 = (t.view(1, n) for t in (x, e, nz, keep))
    xr = float(tab["c_recip"][1]) * x1 - float(tab["c_recipm1"][1]) * e1
    mean = float(tab["coef1"][1]) * xr + float(tab["coef2"][1]) * x1
    noise = (n1 * 0.7) * (k1.float() * float(F32(1.0 / 0.7)))
    assert torch.equal(got.cpu(), mean + (1.0 * float(tab["sigma"][1])) * noise)


# ------------------------------------------------------------------ DDIM loops
def _loop_data():
    return {k: _gpu(v) for k, v in su.loop_inputs().items()}


@pytest.mark.parametrize("case", su.DDIM_CASES)
def test_ddim_loops_bitexact_vs_reference(sdk, case, monkeypatch):
    from sd_amd.DDIM import ddim as ddim_mod
    fx = load("so_ddim_loops")
    d = _loop_data()
    orig = case.startswith("orig")
    eta = 1.0 if case.endswith("eta1") else float(fx["orig_eta"]) if case in ("orig_eta", "orig_timesteps", "orig_decode") \
        else 0.0
    cb = vu.case_data(cu.LOOP_VQ_CASE)[0] if case == "mask_quantize" else None
    ld = _stub_ld(sdk, outputs=d["es"], uncond=d["eu"], codebook=cb)
    s = _sampler(ld, eta)
    steps = su.ORIG_TIMESTEPS if case in ("orig_timesteps", "orig_decode") else su.T if orig else su.S
    tr = list(range(steps - 1, -1, -1)) if orig else [5, 3, 1]                 # timestep of loop counter i
    b = su.LOOP_SHAPE[0]
    c, uc = torch.zeros(b, 1, device=DEV), torch.ones(b, 1, device=DEV)
    kw = dict(log_every_t=1, noise_fn=lambda i, shape: d["nz"][tr[i]], q_noise_fn=lambda i, shape: d["qn"][tr[i]])
    corr = None
    if case.startswith("mask"):
        kind = case[5:] if case[5:] in su.MASK_KINDS else "b1hw"
        kw.update(mask=d["mask_" + kind], x0=d["x0"])
    if case.endswith("cfg"):
        kw.update(unconditional_guidance_scale=su.GUIDANCE, unconditional_conditioning=uc)
    if case.startswith("corrector"):
        corr = Corrector(d["add"])
        kw.update(score_corrector=corr, corrector_kwargs={"scale": 0.5})
    if case == "dropout_eta1":
        keep = _gpu(fx[case + "_keep"])
        kw.update(noise_dropout=su.LOOP_DROP, dropout_fn=lambda i, shape: keep[i])
    if orig:
        kw.update(ddim_use_original_steps=True)
    if case == "orig_timesteps":
        kw.update(timesteps=su.ORIG_TIMESTEPS)
    xT = d["xT"].clone()
    if case == "orig_decode":
        # decode has no noise hook: the step noise comes from the module's noise_like, as in the reference
        monkeypatch.setattr(ddim_mod, "noise_like", lambda shape, device, repeat=False: d["nz"][ld.cur])
        calls, step = [], s.p_sample_ddim
        s.p_sample_ddim = lambda *a, **k: calls.append(step(*a, **k)) or calls[-1]
        x = s.decode(xT, c, su.ORIG_TIMESTEPS, use_original_steps=True)
        inter = {"x_inter": [None] + [o[0] for o in calls], "pred_x0": [None] + [o[1] for o in calls]}
    else:
        x, inter = s.ddim_sampling(c, su.LOOP_SHAPE, x_T=xT, quantize_denoised=case == "mask_quantize", **kw)
    assert len(inter["x_inter"]) == steps + 1 == len(inter["pred_x0"])
    for i in range(steps):
        _same(inter["x_inter"][i + 1], fx[case + "_x_inter"][i], f"{case}: x_inter after t = {tr[i]}")
        _same(inter["pred_x0"][i + 1], fx[case + "_pred_x0"][i], f"{case}: pred_x0 at t = {tr[i]}")
    assert torch.equal(x, inter["x_inter"][-1])
    _same(xT, su.loop_inputs()["xT"], "x_T was written")
    if corr is not None:
        assert len(corr.models) == steps and all(m is ld for m in corr.models)


# ------------------------------------------------------------------ ancestral loops
def _hooks(d, keep=None):
    h = dict(noise_fn=lambda i, shape: d["nz"][i], q_noise_fn=lambda i, shape: d["qn"][i],
             cond_noise_fn=lambda i, shape: d["cn"][i])
    if keep is not None:
        h["dropout_fn"] = lambda i, shape: keep[su.T - 1 - i]        # recorded in loop order, t = T-1 .. 0
    return h


def test_p_sample_loop_with_dropout_corrector_and_mask(sdk):
    fx = load("so_ancestral")
    d = _loop_data()
    ld = _stub_ld(sdk, outputs=d["es"])
    corr = Corrector(d["add"])
    img, inter = ld.p_sample_loop(None, su.LOOP_SHAPE, return_intermediates=True, x_T=d["xT"], verbose=False,
                                  log_every_t=1, mask=d["mask_b1hw"], x0=d["x0"], noise_dropout=su.LOOP_DROP,
                                  score_corrector=corr, **_hooks(d, _gpu(fx["loop_options_keep"])))
    assert len(inter) == su.T + 1 and len(corr.models) == su.T
    for k in range(su.T):
        _same(inter[k + 1], fx["loop_options"][k], f"after timestep {su.T - 1 - k}")
    # sample() passes the options on
    out = ld.sample(None, batch_size=su.LOOP_SHAPE[0], x_T=d["xT"], mask=d["mask_b1hw"], x0=d["x0"],
                    noise_dropout=su.LOOP_DROP, score_corrector=Corrector(d["add"]), corrector_kwargs=None,
                    **_hooks(d, _gpu(fx["loop_options_keep"])))
    assert np.array_equal(_bits(out), _bits(img))


def test_progressive_denoising_bitexact_vs_reference(sdk):
    fx = load("so_ancestral")
    d = _loop_data()
    ld = _stub_ld(sdk, outputs=d["es"])
    seen = []
    img, inter = ld.progressive_denoising(None, su.LOOP_SHAPE[1:], verbose=False, temperture=list(su.TEMP_LIST),
                                          batch_size=su.LOOP_SHAPE[0], x_T=d["xT"], log_every_t=1,
                                          mask=d["mask_b1hw"], x0=d["x0"], noise_dropout=su.LOOP_DROP,
                                          score_corrector=Corrector(d["add"]), corrector_kwargs=None,
                                          img_callback=lambda im, i: seen.append(i),
                                          **_hooks(d, _gpu(fx["prog_options_keep"])))
    assert len(inter) == su.T and seen == list(range(su.T - 1, -1, -1))
    _same(img, fx["prog_options_img"], "img")
    for k in range(su.T):
        _same(inter[k], fx["prog_options_x0"][k], f"x0_partial at timestep {su.T - 1 - k}")
    _same(d["xT"], su.loop_inputs()["xT"], "x_T was written")
    # a float temperature, start_T and log_every_t from the model
    img2, inter2 = ld.progressive_denoising(None, su.LOOP_SHAPE, verbose=False, temperture=1., x_T=d["xT"], start_T=2,
                                            **_hooks(d))
    assert len(inter2) == 2 and tuple(img2.shape) == su.LOOP_SHAPE


@pytest.mark.parametrize("name", ["loop", "prog"])
def test_shorten_cond_schedule_bitexact_vs_reference(sdk, name):
    fx = load("so_ancestral")
    d = _loop_data()
    ld = _stub_ld(sdk, outputs=d["es"], conditioning_key="concat", num_timesteps_cond=su.NUM_TIMESTEPS_COND)
    cond = d["cond"].clone()
    if name == "loop":
        img = ld.p_sample_loop(cond, su.LOOP_SHAPE, x_T=d["xT"], verbose=False, **_hooks(d))
    else:
        img, _ = ld.progressive_denoising(cond, su.LOOP_SHAPE, verbose=False, x_T=d["xT"], **_hooks(d))
    assert len(ld.conds) == su.T
    for k in range(su.T):
        _same(ld.conds[k], fx[f"shorten_{name}_conds"][k], f"cond at timestep {su.T - 1 - k}")
    _same(img, fx[f"shorten_{name}_img"], "img")
    _same(cond, su.loop_inputs()["cond"], "the caller's cond was written")


def test_sample_log_both_branches(sdk):
    fx = load("so_ancestral")
    d = _loop_data()
    ld = _stub_ld(sdk, outputs=d["es"])
    tr = [5, 3, 1]
    x, inter = ld.sample_log(None, su.LOOP_SHAPE[0], True, su.S, x_T=d["xT"], eta=1.0, log_every_t=1,
                             noise_fn=lambda i, shape: d["nz"][tr[i]])
    assert len(inter["x_inter"]) == su.S + 1 and torch.equal(x, inter["x_inter"][-1])
    for i in range(su.S):
        _same(inter["x_inter"][i + 1], fx["sample_log_ddim"][i], f"ddim: after t = {tr[i]}")
    x, inter = ld.sample_log(None, su.LOOP_SHAPE[0], False, su.S, x_T=d["xT"], noise_fn=lambda i, shape: d["nz"][i])
    assert len(inter) == su.T + 1 and torch.equal(x, inter[-1])
    for k in range(su.T):
        _same(inter[k + 1], fx["sample_log_ancestral"][k], f"ancestral: after timestep {su.T - 1 - k}")


def test_default_draws_without_hooks(sdk):
    """Without the hooks the samplers draw for themselves: the keep mask of noise_dropout on the device (every element
    is the kept or the dropped value, both occur; p = 1 drops everything), the q-noise and the conditioning noise."""
    from sd_amd import ops
    d = _loop_data()
    ld = _stub_ld(sdk, outputs=d["es"])
    t = torch.full((2,), 3, device=DEV, dtype=torch.long)
    tab = ld._host_tables()
    scale = torch.ones(su.LOOP_SHAPE, dtype=torch.uint8, device=DEV)
    got = ld.p_sample(d["xT"], None, t, noise_dropout=0.5, noise=d["nz"][3])
    kept, _ = ops.posterior_step(d["xT"], d["es"][3], 3, tab, noise=d["nz"][3], keep=scale, drop_p=0.5)
    dropped, _ = ops.posterior_step(d["xT"], d["es"][3], 3, tab, noise=d["nz"][3], keep=scale * 0, drop_p=0.5)
    is_kept, is_dropped = got == kept, got == dropped
    assert bool((is_kept | is_dropped).all()) and 0.25 < float(is_kept.float().mean()) < 0.75
    s = _sampler(ld, 1.0)
    sc = s.step_scalars(2)
    got, _ = s.p_sample_ddim(d["xT"], None, t + 2, index=2, noise_dropout=0.5, noise=d["nz"][5])
    kept, _ = ops.ddim_step(d["xT"], d["es"][5], sc, noise=d["nz"][5], keep=scale, drop_p=0.5)
    dropped, _ = ops.ddim_step(d["xT"], d["es"][5], sc, noise=d["nz"][5], keep=scale * 0, drop_p=0.5)
    is_kept, is_dropped = got == kept, got == dropped
    assert bool((is_kept | is_dropped).all()) and 0.25 < float(is_kept.float().mean()) < 0.75
    all_dropped, _ = s.p_sample_ddim(d["xT"], None, t + 2, index=2, noise_dropout=1.0, noise=d["nz"][5])
    assert torch.equal(all_dropped, ops.ddim_step(d["xT"], d["es"][5], sc, noise=torch.zeros_like(d["xT"]))[0])
    x, _ = s.ddim_sampling(None, su.LOOP_SHAPE, x_T=d["xT"], mask=d["mask_b1hw"], x0=d["x0"], noise_dropout=0.5)
    assert tuple(x.shape) == su.LOOP_SHAPE and bool(torch.isfinite(x).all())
    cc = _stub_ld(sdk, outputs=d["es"], conditioning_key="concat", num_timesteps_cond=su.NUM_TIMESTEPS_COND)
    x = cc.p_sample_loop(d["cond"], su.LOOP_SHAPE, x_T=d["xT"], mask=d["mask_b1hw"], x0=d["x0"], noise_dropout=0.5)
    assert bool(torch.isfinite(x).all()) and len(cc.conds) == su.T and not torch.equal(cc.conds[0], d["cond"])


# ------------------------------------------------------------------ model level
MODEL_TAG = "masked DDIM x4, tiny 9-channel hybrid UNet vs reference"


def _model_ld(sdk):
    from sd_amd.Diffusion.ddpm import DiffusionWrapper, LatentDiffusion
    from sd_amd.openai_model.model import UNetModel
    z = load("unet_tiny_concat")
    assert cfg_of(z) == cu.TINY_UNET_CONCAT and int(load("so_model")["seed"]) == int(z["seed"])
    m = UNetModel(**cfg_of(z))
    m.load_state_dict(weights_of(z))
    dw = DiffusionWrapper.__new__(DiffusionWrapper)
    torch.nn.Module.__init__(dw)
    dw.diffusion_model, dw.conditioning_key, dw._graphed, dw._graphs_on = m, "hybrid", None, False

    class LD(LatentDiffusion):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.parameterization, self.v_posterior = "eps", 0.
            self.model = dw
            kw = dict(cu.STEP_SCHEDULE)
            self.register_schedule(beta_schedule=kw.pop("beta_schedule"), **kw)

    return LD().to(DEV)


def _model_inputs():
    return {k: _gpu(v) for k, v in su.model_inputs().items()}


def _model_run(ld, d):
    cond = {"c_concat": [d["m"], d["zi"]], "c_crossattn": [d["ctx"]]}
    s = _sampler(ld, 0.0, su.MODEL_STEPS)
    x, inter = s.ddim_sampling(cond, tuple(d["x"].shape), x_T=d["x"], mask=d["m"], x0=d["zi"], log_every_t=1,
                               q_noise_fn=lambda i, shape: d["qn"][i])
    assert len(inter["x_inter"]) == su.MODEL_STEPS + 1
    return x, inter["pred_x0"][-1]


def test_masked_ddim_on_the_concat_unet_vs_reference(sdk):
    """fp16 activations against the reference's fp32 UNet and sampler, so not bit-equal: the limits are at most
    3.5x the errors measured on MI355X (sampler_opt_util.PARITY_LIMITS)."""
    fx = load("so_model")
    x, p0 = _model_run(_model_ld(sdk), _model_inputs())
    check_parity(MODEL_TAG + " (pred_x0)", p0, torch.from_numpy(fx["pred_x0_last"]), *su.PARITY_LIMITS[MODEL_TAG])
    check_parity(MODEL_TAG, x, torch.from_numpy(fx["samples"]), *su.PARITY_LIMITS[MODEL_TAG])


def test_masked_ddim_graph_replay_equals_eager(sdk):
    ld, d = _model_ld(sdk), _model_inputs()
    eager = [t.clone() for t in _model_run(ld, d)]
    ld.use_graphs(True)
    for rnd in range(2):
        for got, ref in zip(_model_run(ld, d), eager):
            assert np.array_equal(_bits(got), _bits(ref)), f"round {rnd}"
    assert len(ld.model._graphed.graphs) >= 1


# ------------------------------------------------------------------ errors
def test_argument_errors(sdk):
    from sd_amd import ops
    d = _loop_data()
    ld = _stub_ld(sdk, outputs=d["es"])
    s = _sampler(ld, 1.0)
    run = lambda **kw: s.ddim_sampling(None, su.LOOP_SHAPE, x_T=d["xT"], **kw)          # noqa: E731
    with pytest.raises(ValueError, match="x0"):
        run(mask=d["mask_b1hw"])
    with pytest.raises(ValueError, match="spatial"):
        run(mask=d["mask_b1hw"][:, :, :4, :4], x0=d["x0"])
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="noise_dropout"):
            run(noise_dropout=bad)
        with pytest.raises(ValueError, match="noise_dropout"):
            ld.p_sample(d["xT"], None, torch.zeros(2, dtype=torch.long, device=DEV), noise_dropout=bad)
        with pytest.raises(ValueError, match="drop_p"):
            ops.ddim_step(d["xT"], d["es"][0], s.step_scalars(0), noise=d["nz"][0], drop_p=bad,
                          keep=torch.ones(su.LOOP_SHAPE, dtype=torch.uint8, device=DEV))

    class CpuCorrector:
        def modify_score(self, model, e_t, x, t, c):
            return e_t.cpu()

    with pytest.raises(ValueError, match="score_corrector"):
        run(score_corrector=CpuCorrector())
    with pytest.raises(ValueError, match="score_corrector"):
        ld.p_sample_loop(None, su.LOOP_SHAPE, x_T=d["xT"], score_corrector=CpuCorrector())
    vs = _sampler(_stub_ld(sdk, parameterization="v", outputs=d["es"]), 0.0)
    with pytest.raises(AssertionError, match="eps"):
        vs.ddim_sampling(None, su.LOOP_SHAPE, x_T=d["xT"], score_corrector=Corrector(d["add"]))
    hy = _stub_ld(sdk, outputs=d["es"], conditioning_key="hybrid", num_timesteps_cond=su.NUM_TIMESTEPS_COND)
    with pytest.raises(AssertionError, match="hybrid"):
        hy.p_sample_loop(d["cond"], su.LOOP_SHAPE, x_T=d["xT"])
    cc = _stub_ld(sdk, outputs=d["es"], conditioning_key="concat", num_timesteps_cond=su.NUM_TIMESTEPS_COND)
    with pytest.raises(ValueError, match="one tensor"):
        cc.progressive_denoising({"c_concat": [d["cond"]]}, su.LOOP_SHAPE, x_T=d["xT"])
    # ops-level shape / dtype / device errors
    sc = s.step_scalars(0)
    with pytest.raises(ValueError):
        ops.ddim_step(d["xT"], d["es"][0], sc, noise=d["nz"][0], keep=torch.ones(2, 4, 8, 4, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        ops.ddim_step(d["xT"], d["es"][0], sc, noise=d["nz"][0], keep=torch.ones(su.LOOP_SHAPE, device=DEV))
    with pytest.raises(ValueError):
        ops.ddim_step(d["xT"], d["es"][0], sc, blend_mask=d["mask_b1hw"], blend_x0=d["x0"])
    with pytest.raises(ValueError):
        ops.ddim_step(d["xT"], d["es"][0], sc, blend_mask=d["mask_b1hw"][:1, :, :4], blend_x0=d["x0"], blend_noise=d["x0"],
                      blend_sqrt_acp=1.0, blend_sqrt_1m_acp=0.0)
    with pytest.raises(ValueError):
        ops.cfg_combine(d["xT"].cpu(), d["xT"], 2.0)
    with pytest.raises(ValueError):
        ops.cfg_combine(d["xT"][:1], d["xT"], 2.0)
