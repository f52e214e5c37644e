"""Generate the sampler-option fixtures by running the REFERENCE itself (build container only, CPU).

Run from the repo root:  python tests/golden/make_golden_sampler_options.py
Needs what make_golden_concat_ancestral.py needs; reuses its shims, its ``ref_schedule`` and its stand-in ``self``
(class ``Stand``).  The arithmetic is executed by the reference's own functions: ``DDIMSampler.make_schedule`` /
``ddim_sampling`` / ``p_sample_ddim`` / ``decode`` of ``DDIM/ddim.py``; ``LatentDiffusion.p_sample`` /
``p_mean_variance`` / ``p_sample_loop`` / ``progressive_denoising`` / ``sample`` / ``sample_log`` /
``make_cond_schedule`` and ``DDPM.q_sample`` of ``ldm/diffusion/ddpm.py``; ``DiffusionWrapper.forward`` and
``UNetModel`` for the model-level case.  What the stand-in supplies (each a documented quirk):

* recorded model outputs (``apply_model``), recorded step noise (the modules' ``noise_like``), recorded GAUSSIAN
  q-noise (``q_sample`` is the reference's ``DDPM.q_sample`` called with it: its own default and the progressive
  loop's ``rand_like`` are uniform) — for the mask blend and for the shortened conditioning schedule;
* ``model.ddim_sigmas_for_original_num_steps``: the sampler registers that table on itself and reads it from the
  model (``ddim.py:54,187``); the stand-in aliases the sampler's own table onto the model;
* ``torch.nn.functional.dropout`` is wrapped: the reference's own call runs, and the keep mask it drew is
  recorded next to its output (the fixtures hold those masks);
* ``p_sample_loop`` gets ``noise_dropout`` / ``score_corrector`` by binding them into the reference's ``p_sample``
  (the reference's loop does not pass them on); ``progressive_denoising``'s ``p_sample(return_x0=True)`` is the
  reference's ``p_sample(return_x0=False)`` plus the x_recon of its ``p_mean_variance`` (``:1633`` multiplies
  where CompVis adds);
* the score corrector adds a recorded tensor to the model output.

Inputs are regenerated from seeds (tests/sampler_opt_util.py); the fixtures hold the reference's outputs:

* so_kernel.npz — x_prev / pred_x0 of one ``p_sample_ddim`` call per shape x eta x temperature x guidance x
  dropout, the blended image that opens the next iteration per mask shape, binary / fractional, and the keep masks;
* so_posterior.npz — ``p_sample`` with dropout per case of ca_util.STEP_CASES x eps / x0 x clip x p;
* so_ddim_loops.npz — every x_inter / pred_x0 of the DDIM loops of sampler_opt_util.DDIM_CASES, the original-steps
  sigma table and step scalars, and the eta chosen for them;
* so_ancestral.npz — ``p_sample_loop`` / ``progressive_denoising`` with dropout, corrector, mask and a temperature
  list, the shortened conditioning schedule (every ``cond`` the model received), ``cond_ids``, ``sample_log``;
* so_model.npz — the tiny 9-channel hybrid UNet through 4 masked DDIM steps.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg                                    # noqa: E402
import make_golden_concat_ancestral as mca                  # noqa: E402
import make_golden_vq as mgv                                # noqa: E402
import ca_util as cu                                        # noqa: E402
import sampler_opt_util as su                               # noqa: E402
import vq_util as vu                                        # noqa: E402

OUT = HERE
T = torch.from_numpy
DROPPED = []            # (input, output, p) of every F.dropout call of the reference


def wrap_dropout():
    real = torch.nn.functional.dropout

    def dropout(x, p=0.5, training=True, inplace=False):
        y = real(x.clone(), p=p, training=training, inplace=False)
        DROPPED.append((x.clone(), y.clone(), p))
        return y

    torch.nn.functional.dropout = dropout


def keep_of(x, y, p):
    """The keep mask of one recorded F.dropout call, checked: every kept element equals input * fp32(1/(1-p))."""
    scale = np.float32(1.0 / (1.0 - p))
    assert np.float32(1.0) / np.float32(1.0 - p) == scale, f"fp32(1)/fp32(1-p) != fp32(1/(1-p)) for p = {p}"
    keep = (y != 0) | (x == 0)                     # a zero input is zero either way (and keeps its sign)
    assert torch.equal(torch.where(keep, x * float(scale), torch.zeros_like(x)), y), f"dropout p = {p}: not x * scale"
    return keep.numpy().astype(np.uint8)


def save(name, out):
    for k, v in out.items():
        if np.issubdtype(np.asarray(v).dtype, np.floating):
            assert not np.isnan(v).any(), f"{name}: NaN in {k}"
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 250_000, f"{name}: {os.path.getsize(path)} bytes"
    print(name, os.path.getsize(path))


class Corrector:
    def __init__(self, add):
        self.add, self.seen = add, []

    def modify_score(self, model, e_t, x, t, c, scale=1.0):
        self.seen.append(int(t[0]))
        return e_t + scale * T(self.add[int(t[0])])


def ddim_model(ldm, sched, d, b, quantizer=None):
    """Stand-in model of the reference DDIMSampler: ``apply_model`` returns d['e'][t] (and d['eu'][t] in front of it
    for a doubled batch), ``q_sample`` draws d['qn'][t]."""
    st = mca.make_stand(ldm, sched, quantizer=quantizer)
    st.cur = None

    def apply_model(x, t, c, return_ids=False):
        st.cur = int(t[0])
        e = T(d["e"][st.cur]).clone()
        return torch.cat([T(d["eu"][st.cur]).clone(), e]) if x.shape[0] == 2 * b else e

    st.apply_model = apply_model
    st.q_sample = lambda x_start, t, noise=None: ldm.DDPM.q_sample(st, x_start, t, noise=T(d["qn"][int(t[0])]).clone())
    return st


def ddim_sampler(ddim_mod, st, d, steps, eta):
    ddim_mod.noise_like = lambda shape, device, repeat=False: T(d["nz"][st.cur]).clone()
    s = ddim_mod.DDIMSampler(st)
    with mg.quiet():
        s.make_schedule(steps, ddim_eta=eta, verbose=False)
    st.ddim_sigmas_for_original_num_steps = s.ddim_sigmas_for_original_num_steps     # ddim.py:187 reads the model
    return s


def record_calls(s):
    """Every input image and output pair of the sampler's p_sample_ddim calls."""
    calls, orig = [], s.p_sample_ddim

    def p_sample_ddim(x, *a, **kw):
        out = orig(x, *a, **kw)
        calls.append((x.clone(), out[0].clone(), out[1].clone()))
        return out

    s.p_sample_ddim = p_sample_ddim
    return calls


def gen_kernel(ldm, top, ddim_mod):
    sched = mca.ref_schedule(top, **su.SCHEDULE)
    out = {}
    ts = [1, 3, 5]
    for shape in su.KERNEL_SHAPES:
        k = su.kernel_inputs(shape)
        b = shape[0]
        d = dict(e={t: k["e"] for t in ts}, eu={t: k["eu"] for t in ts}, nz={t: k["nz"] for t in ts},
                 qn={5: k["qn0"], 3: k["qn1"], 1: k["qn1"]})
        c, uc = torch.zeros(b, 1), torch.ones(b, 1)

        def run(eta, temp, guided, p, mask=None):
            st = ddim_model(ldm, sched, d, b)
            s = ddim_sampler(ddim_mod, st, d, su.S, eta)
            assert list(s.ddim_timesteps) == ts
            calls = record_calls(s)
            del DROPPED[:]
            torch.manual_seed(su.drop_seed(shape, p))
            kw = dict(mask=T(mask), x0=T(k["x0"])) if mask is not None else {}
            with mg.quiet(), torch.no_grad():
                s.ddim_sampling(c, shape, x_T=T(k["xT"]).clone(), temperature=temp, noise_dropout=p,
                                unconditional_guidance_scale=su.GUIDANCE if guided else 1.,
                                unconditional_conditioning=uc if guided else None, log_every_t=1, **kw)
            if p > 0:
                key, keep = su.keep_tag(shape, p), keep_of(*DROPPED[0])
                if eta > 0:
                    assert key not in out or np.array_equal(out[key], keep)
                    out[key] = keep
            return calls

        for eta, temp, guided, p in su.step_combos():
            calls = run(eta, temp, guided, p)
            tag = su.step_tag(shape, eta, temp, guided, p)
            out[tag + "_xprev"] = calls[0][1].numpy()
            ptag = f"k{su.shape_tag(shape)}_g{int(guided)}_pred_x0"
            assert ptag not in out or np.array_equal(out[ptag], calls[0][2].numpy())
            out[ptag] = calls[0][2].numpy()
        for eta in su.ETAS:
            for kind in su.MASK_KINDS:
                for binary in (True, False):
                    calls = run(eta, su.BLEND_STEP["temp"], su.BLEND_STEP["guided"], su.BLEND_STEP["p"],
                                mask=su.mask_of(kind, binary, shape))
                    btag = su.blend_tag(shape, eta, kind, binary)
                    out[btag + "_first"] = calls[0][0].numpy()        # the blend of x_T that opens iteration 0
                    out[btag + "_xprev"] = calls[0][1].numpy()        # the step on it (unblended)
                    out[btag + "_next"] = calls[1][0].numpy()         # its blend that opens iteration 1
    save("so_kernel.npz", out)


def gen_posterior(ldm, top):
    sched = mca.ref_schedule(top, **cu.STEP_SCHEDULE)
    out = {}
    for shape, t in cu.STEP_CASES:
        x, mo, nz = cu.step_inputs(shape)
        tt = torch.tensor(t, dtype=torch.long)
        for param in cu.STEP_PARAMS:
            for clip in (False, True):
                for p in su.POST_DROPS:
                    st = mca.make_stand(ldm, sched, param)
                    st.apply_model = lambda x_, t_, c_, return_ids=False: T(mo).clone()
                    ldm.noise_like = lambda shape_, device, repeat=False: T(nz).clone()
                    del DROPPED[:]
                    torch.manual_seed(su.drop_seed(shape, p))
                    with torch.no_grad():
                        xp = st.p_sample(T(x).clone(), None, tt, clip_denoised=clip, temperture=su.POST_TEMP,
                                         noise_dropout=p)
                    tag = su.post_tag(shape, param, clip, p)
                    out[tag + "_xprev"] = xp.numpy()
                    key, keep = su.keep_tag(shape, p), keep_of(*DROPPED[0])
                    assert key not in out or np.array_equal(out[key], keep)
                    out[key] = keep
    save("so_posterior.npz", out)


def gen_ddim_loops(ldm, top, ddim_mod):
    sched = mca.ref_schedule(top, **su.SCHEDULE)
    d = su.loop_inputs()
    d = dict(d, e=d["es"])
    b = su.LOOP_SHAPE[0]
    n, dim = cu.LOOP_VQ_CASE[:2]
    cb, _ = vu.case_data(cu.LOOP_VQ_CASE)
    real_q = mgv.ref_vq(n, dim, cb)
    seen = []

    class RecQ(torch.nn.Module):
        def forward(self, z):
            seen.append(z.numpy().copy())
            return real_q(z)

    c, uc = torch.zeros(b, 1), torch.ones(b, 1)
    out = {}

    # the eta of the original-steps case: 1 - a_prev - sigma^2 >= 0 at every index in the reference's own fp32
    orig_eta = None
    for eta in su.ORIG_ETAS:
        s = ddim_sampler(ddim_mod, ddim_model(ldm, sched, d, b), d, su.S, eta)
        sig = s.ddim_sigmas_for_original_num_steps
        if bool(((1. - sched.alphas_cumprod_prev - sig ** 2) >= 0).all()):
            orig_eta = eta
            break
    assert orig_eta is not None, "no eta > 0 keeps 1 - a_prev - sigma^2 >= 0 on the short schedule: eta = 0 only"
    out["orig_eta"] = np.float64(orig_eta)
    out["orig_sigmas"] = sig.numpy()
    full = lambda v: torch.full((1, 1, 1, 1), v)                       # noqa: E731
    out["orig_scalars"] = np.stack([np.asarray([
        float(full(sched.sqrt_one_minus_alphas_cumprod[i])), float(full(sched.alphas_cumprod[i]).sqrt()),
        float((1. - full(sched.alphas_cumprod_prev[i]) - full(sig[i]) ** 2).sqrt()),
        float(full(sched.alphas_cumprod_prev[i]).sqrt()), float(full(sig[i]))], dtype=np.float32)
        for i in range(su.T)])

    for case in su.DDIM_CASES:
        eta = 1.0 if case.endswith("eta1") else orig_eta if case in ("orig_eta", "orig_timesteps", "orig_decode") \
            else 0.0
        st = ddim_model(ldm, sched, d, b, quantizer=RecQ())
        s = ddim_sampler(ddim_mod, st, d, su.S, eta)
        calls = record_calls(s)
        kw = dict(log_every_t=1)
        if case.startswith("mask"):
            kind = case[5:] if case[5:] in su.MASK_KINDS else "b1hw"
            kw.update(mask=T(d["mask_" + kind]), x0=T(d["x0"]))
        if case.endswith("cfg"):
            kw.update(unconditional_guidance_scale=su.GUIDANCE, unconditional_conditioning=uc)
        if case.startswith("corrector"):
            corr = Corrector(d["add"])
            kw.update(score_corrector=corr, corrector_kwargs={"scale": 0.5})
        if case == "dropout_eta1":
            kw.update(noise_dropout=su.LOOP_DROP)
        if case.startswith("orig"):
            kw.update(ddim_use_original_steps=True)
        if case == "orig_timesteps":
            kw.update(timesteps=su.ORIG_TIMESTEPS)
        del DROPPED[:], seen[:]
        torch.manual_seed(su.drop_seed(su.LOOP_SHAPE, su.LOOP_DROP))
        with mg.quiet(), torch.no_grad():
            if case == "orig_decode":
                ddim_mod.noise_like = lambda shape, device, repeat=False: T(d["nz"][st.cur]).clone()
                x = s.decode(T(d["xT"]).clone(), c, su.ORIG_TIMESTEPS, use_original_steps=True)
                inter = {"x_inter": [None] + [cl[1] for cl in calls], "pred_x0": [None] + [cl[2] for cl in calls]}
                assert torch.equal(x, calls[-1][1]) and len(calls) == su.ORIG_TIMESTEPS
            else:
                x, inter = s.ddim_sampling(c, su.LOOP_SHAPE, x_T=T(d["xT"]).clone(), quantize_denoised=case == "mask_quantize",
                                           **kw)
        steps = su.ORIG_TIMESTEPS if case in ("orig_timesteps", "orig_decode") else su.T if case.startswith("orig") \
            else su.S
        assert len(inter["x_inter"]) == steps + 1 and torch.equal(x, inter["x_inter"][-1])
        out[case + "_x_inter"] = np.stack([t.numpy() for t in inter["x_inter"][1:]])
        out[case + "_pred_x0"] = np.stack([t.numpy() for t in inter["pred_x0"][1:]])
        if case == "dropout_eta1":
            assert len(DROPPED) == su.S
            out[case + "_keep"] = np.stack([keep_of(*r) for r in DROPPED])      # by loop counter
        if case == "mask_quantize":
            assert len(seen) == su.S
            for i, zin in enumerate(seen):
                g = vu.rel_gap(zin, cb)
                assert g.min() >= vu.GAP_MIN, f"quantize step {i}: near-tie row ({g.min():.2e}); change the seed"
        print(f"ddim {case}: eta {eta}, |x| max {np.abs(out[case + '_x_inter']).max():.3f}")
    save("so_ddim_loops.npz", out)


def gen_ancestral(ldm, top, ddim_mod):
    sched = mca.ref_schedule(top, **su.SCHEDULE)
    d = su.loop_inputs()
    b = su.LOOP_SHAPE[0]
    out = {}
    for tsteps, ncond in su.COND_SCHEDULES:
        f = types.SimpleNamespace(num_timesteps=tsteps, num_timesteps_cond=ncond)
        ldm.LatentDiffusion.make_cond_schedule(f)
        out[f"cond_ids_{tsteps}_{ncond}"] = f.cond_ids.numpy()

    def stand(shorten=False, dropout=0.0, corrector=None):
        st = mca.make_stand(ldm, sched)
        for name in ("progressive_denoising", "sample", "sample_log", "make_cond_schedule"):
            setattr(type(st), name, getattr(ldm.LatentDiffusion, name))
        st.cur, st.conds, st.k = None, [], [su.T]
        st.channels, st.image_size = su.LOOP_SHAPE[1], su.LOOP_SHAPE[2]
        st.model = types.SimpleNamespace(conditioning_key="concat")
        st.shorten_cond_schedule = shorten
        if shorten:
            st.num_timesteps_cond = su.NUM_TIMESTEPS_COND
            st.make_cond_schedule()

        def apply_model(x_, t_, c_, return_ids=False):
            st.cur = int(t_[0])
            if torch.is_tensor(c_):
                st.conds.append(c_.numpy().copy())
            return T(d["es"][st.cur]).clone()

        def q_sample(x_start, t, noise=None):
            if noise is not None:                       # the conditioning of loop timestep k (first call of it)
                st.k[0] -= 1
                return ldm.DDPM.q_sample(st, x_start, t, noise=T(d["cn"][st.k[0]]).clone())
            return ldm.DDPM.q_sample(st, x_start, t, noise=T(d["qn"][int(t[0])]).clone())

        def p_sample(x, c, t, return_x0=False, **kw):
            kw = dict(kw, noise_dropout=dropout, score_corrector=corrector, corrector_kwargs={})
            xp = ldm.LatentDiffusion.p_sample(st, x, c, t, **kw)
            if not return_x0:
                return xp
            pm = {k: kw[k] for k in ("clip_denoised", "quantize_denoised", "score_corrector", "corrector_kwargs")
                  if k in kw}
            return xp, st.p_mean_variance(x, c, t, return_x0=True, **pm)[3]

        st.apply_model, st.q_sample, st.p_sample = apply_model, q_sample, p_sample
        ldm.noise_like = lambda shape_, device, repeat=False: T(d["nz"][st.cur]).clone()
        return st

    def seeded():
        del DROPPED[:]
        torch.manual_seed(su.drop_seed(su.LOOP_SHAPE, su.LOOP_DROP))

    mk = dict(mask=T(d["mask_b1hw"]), x0=T(d["x0"]))
    # p_sample_loop with dropout + corrector + mask
    st = stand(dropout=su.LOOP_DROP, corrector=Corrector(d["add"]))
    seeded()
    with mg.quiet(), torch.no_grad():
        img, inter = st.p_sample_loop(None, su.LOOP_SHAPE, return_intermediates=True, x_T=T(d["xT"]).clone(),
                                      verbose=False, log_every_t=1, **mk)
    out["loop_options"] = np.stack([t.numpy() for t in inter[1:]])
    out["loop_options_keep"] = np.stack([keep_of(*r) for r in DROPPED])          # in loop order: t = T-1 .. 0
    # progressive_denoising with dropout + corrector + mask + a temperature list + batch_size
    st = stand(dropout=su.LOOP_DROP, corrector=Corrector(d["add"]))
    seeded()
    with mg.quiet(), torch.no_grad():
        img, inter = st.progressive_denoising(None, su.LOOP_SHAPE[1:], verbose=False, temperture=list(su.TEMP_LIST),
                                              batch_size=b, x_T=T(d["xT"]).clone(), log_every_t=1, **mk)
    assert len(inter) == su.T
    out["prog_options_img"] = img.numpy()
    out["prog_options_x0"] = np.stack([t.numpy() for t in inter])
    out["prog_options_keep"] = np.stack([keep_of(*r) for r in DROPPED])
    # shorten_cond_schedule in both loops: every cond the model received, and the result
    for name in ("loop", "prog"):
        st = stand(shorten=True)
        with mg.quiet(), torch.no_grad():
            if name == "loop":
                img = st.p_sample_loop(T(d["cond"]).clone(), su.LOOP_SHAPE, x_T=T(d["xT"]).clone(), verbose=False)
            else:
                img, _ = st.progressive_denoising(T(d["cond"]).clone(), su.LOOP_SHAPE, verbose=False,
                                                  x_T=T(d["xT"]).clone())
        assert len(st.conds) >= su.T
        conds = st.conds[:su.T] if name == "loop" else st.conds[::2][:su.T]   # prog: p_sample + p_mean_variance
        out[f"shorten_{name}_conds"] = np.stack(conds)
        out[f"shorten_{name}_img"] = img.numpy()
    # sample_log, both branches
    ldm.DDIMSampler = ddim_mod.DDIMSampler
    st = stand()
    ddim_mod.noise_like = lambda shape, device, repeat=False: T(d["nz"][st.cur]).clone()
    with mg.quiet(), torch.no_grad():
        x, inter = st.sample_log(None, b, True, su.S, x_T=T(d["xT"]).clone(), eta=1.0, log_every_t=1)
    out["sample_log_ddim"] = np.stack([t.numpy() for t in inter["x_inter"][1:]])
    assert torch.equal(x, inter["x_inter"][-1])
    with mg.quiet(), torch.no_grad():
        x, inter = st.sample_log(None, b, False, su.S, x_T=T(d["xT"]).clone())
    out["sample_log_ancestral"] = np.stack([t.numpy() for t in inter[1:]])
    assert torch.equal(x, inter[-1])
    save("so_ancestral.npz", out)


def gen_model(ldm, top, ddim_mod):
    with mg.quiet():
        from openai_model.model import UNetModel
        torch.manual_seed(cu.UNET_SEED)
        m = UNetModel(**cu.TINY_UNET_CONCAT)
    mg.reinit_(m, cu.UNET_SEED)
    m.eval()
    d = {k: T(v) for k, v in su.model_inputs().items()}
    sched = mca.ref_schedule(top, **cu.STEP_SCHEDULE)
    st = mca.make_stand(ldm, sched)
    dw = types.SimpleNamespace(diffusion_model=m, conditional_key="hybrid")
    st.apply_model = lambda x, t, c, return_ids=False: top.DiffusionWrapper.forward(dw, x, t, **c)
    it = iter(range(su.MODEL_STEPS))
    st.q_sample = lambda x_start, t, noise=None: ldm.DDPM.q_sample(st, x_start, t, noise=d["qn"][next(it)].clone())
    ddim_mod.noise_like = lambda shape, device, repeat=False: torch.zeros(shape)           # eta = 0
    s = ddim_mod.DDIMSampler(st)
    cond = {"c_concat": [d["m"], d["zi"]], "c_crossattn": [d["ctx"]]}
    with mg.quiet(), torch.no_grad():
        s.make_schedule(su.MODEL_STEPS, ddim_eta=0.0, verbose=False)
        x, inter = s.ddim_sampling(cond, tuple(d["x"].shape), x_T=d["x"].clone(), mask=d["m"], x0=d["zi"],
                                   log_every_t=1)
    assert len(inter["x_inter"]) == su.MODEL_STEPS + 1
    save("so_model.npz", dict(samples=x.numpy(), pred_x0_last=inter["pred_x0"][-1].numpy(),
                              seed=np.int64(cu.UNET_SEED)))


def main():
    ldm, top = mca.install_shims()
    ddim_mod = mg.make_ddim_sampler(None)
    torch.set_num_threads(8)
    wrap_dropout()
    gen_kernel(ldm, top, ddim_mod)
    gen_posterior(ldm, top)
    gen_ddim_loops(ldm, top, ddim_mod)
    gen_ancestral(ldm, top, ddim_mod)
    gen_model(ldm, top, ddim_mod)


if __name__ == "__main__":
    main()
