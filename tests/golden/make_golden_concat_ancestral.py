"""Generate the concat-conditioning / ancestral-sampler fixtures by running the REFERENCE itself (build
container only, CPU).

Run from the repo root:  python tests/golden/make_golden_concat_ancestral.py
Needs the reference checkout make_golden.py points at (read-only), einops and tqdm.  Uses the shims of
make_golden.py (flash_attn / omegaconf / Lightning / torchvision stand-ins, identity ``.half()``) and, to import
``ldm/diffusion/ddpm.py`` (whose absolute imports assume ``ldm/`` is the working directory):

* ``modules.diffusionmodules.util`` is the reference's own ``ldm/modules/diffusionmodules/util.py``;
* ``modules.ema``, ``modules.distributions.distributions``, ``models.autoencoder``, ``diffusion.ddim`` and
  ``PIL`` (when absent) are import-time names only, never called here.

The arithmetic is executed by the reference's own functions, called on a stand-in ``self`` (class ``Stand``):
``LatentDiffusion.p_mean_variance`` / ``p_sample`` / ``p_sample_loop`` and ``DDPM.q_posterior`` /
``predict_start_from_noise`` / ``q_sample`` of ``ldm/diffusion/ddpm.py``, ``DDPM.register_schedule`` and
``DiffusionWrapper.forward`` of ``Diffusion/ddpm.py``, ``openai_model.model.UNetModel``.  What the stand-in
supplies instead of the reference (each a documented quirk):

* ``register_schedule`` of ``Diffusion/ddpm.py`` gets its betas from ``make_beta_schedule`` of
  ``DDIM/diffusion_modules.py`` (``Diffusion/utils.py``'s copy has ``(1 - cosine_s)`` in the cosine schedule
  where CompVis and the reference's other two copies have ``(1 + cosine_s)``);
* the schedule buffers of ``Diffusion/ddpm.py``'s ``register_schedule`` (ldm's copy misspells
  ``posterior_veriance`` when it READS the buffer: the stand-in aliases that name to ``posterior_variance``);
* ``q_sample`` is the reference's ``DDPM.q_sample`` called with recorded GAUSSIAN noise (its own default draws
  ``rand_like``, uniform);
* the module's ``noise_like`` returns recorded noise; ``apply_model`` returns recorded tensors;
* x_prev comes from ``p_sample(return_x0=False)`` and x_recon from ``p_mean_variance(return_x0=True)``
  (``p_sample(return_x0=True)`` multiplies where CompVis adds, ``:1633``);
* for the blend fixture ``p_sample`` is a stub that returns a recorded image, so ``p_sample_loop`` runs only
  its own ``q_sample`` + blend lines (``:1782-1784``).

Inputs are regenerated from seeds (tests/ca_util.py); the fixtures hold the reference's outputs:

* ca_schedule.npz — the twelve schedule buffers per schedule of ca_util.SCHEDULES and v_posterior;
* ca_step.npz — x_prev and x_recon per case of ca_util.STEP_CASES x parameterisation x clip x temperature;
* ca_blend.npz — the blended image per mask shape, binary / fractional, per timestep;
* ca_loop.npz — every intermediate of p_sample_loop (plain, mask / x0, clip_denoised, quantize_denoised);
* unet_tiny_concat.npz — the 9-channel tiny UNet through DiffusionWrapper.forward ('hybrid').
"""
from __future__ import annotations

import importlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg                                    # noqa: E402
import make_golden_vq as mgv                                # noqa: E402
import ca_util as cu                                        # noqa: E402
import vq_util as vu                                        # noqa: E402

OUT = HERE
T = torch.from_numpy


def install_shims():
    mgv.install_shims()
    try:
        import PIL  # noqa: F401
    except ImportError:
        pil = types.ModuleType("PIL")
        pil.Image = pil.ImageDraw = pil.ImageFont = None
        sys.modules["PIL"] = pil

    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__path__ = []
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    with mg.quiet():
        util = importlib.import_module("ldm.modules.diffusionmodules.util")
    stub("modules")
    stub("modules.ema", LitEma=object)
    stub("modules.diffusionmodules")
    sys.modules["modules.diffusionmodules.util"] = util
    stub("modules.distributions")
    stub("modules.distributions.distributions", DiagonalGaussianDistribution=object, normal_kl=None)
    stub("models")
    stub("models.autoencoder", VQModelInterface=object, AutoencoderKL=object, IdentityFirstStage=object)
    stub("diffusion")
    stub("diffusion.ddim", DDIMSampler=object)
    with mg.quiet():
        ldm = importlib.import_module("ldm.diffusion.ddpm")
        from Diffusion import ddpm as top
    return ldm, top


def ref_schedule(top, v_posterior=0.0, **kw):
    class Fake:
        parameterization = "eps"

        def register_buffer(self, name, t, persistent=True):
            setattr(self, name, t)

    f = Fake()
    f.v_posterior = v_posterior
    # the betas are an input: make_beta_schedule of DDIM/diffusion_modules.py (== ldm/modules/diffusionmodules/
    # util.py, the one the mirror follows); Diffusion/utils.py's copy divides the cosine argument by
    # (1 - cosine_s) where CompVis has (1 + cosine_s), which drives the last betas to zero
    top.make_beta_schedule = sys.modules["modules.diffusionmodules.util"].make_beta_schedule
    top.DDPM.register_schedule(f, **kw)
    return f


def make_stand(ldm, sched, parameterization="eps", clip_denoised=False, quantizer=None):
    """The stand-in ``self``: the reference's schedule buffers and the reference's own methods."""
    class Stand:
        pass

    for name in ("p_mean_variance", "p_sample", "p_sample_loop"):
        setattr(Stand, name, getattr(ldm.LatentDiffusion, name))
    for name in ("q_posterior", "predict_start_from_noise"):
        setattr(Stand, name, getattr(ldm.DDPM, name))
    st = Stand()
    for k in cu.OLD_BUFFERS + cu.NEW_BUFFERS:
        setattr(st, k, getattr(sched, k))
    st.posterior_veriance = st.posterior_variance          # the misspelt read of ldm q_posterior
    st.num_timesteps = sched.num_timesteps
    st.parameterization = parameterization
    st.clip_denoised = clip_denoised
    st.shorten_cond_schedule = False
    st.log_every_t = 1
    st.device = torch.device("cpu")
    if quantizer is not None:
        st.first_stage_model = types.SimpleNamespace(quantize=quantizer)
    return st


def gen_schedule(top):
    out = {}
    for name, kw in cu.SCHEDULES.items():
        for v in cu.V_POSTERIORS:
            f = ref_schedule(top, v, **kw)
            for k in cu.OLD_BUFFERS + cu.NEW_BUFFERS:
                out[f"{cu.sched_tag(name, v)}_{k}"] = getattr(f, k).numpy()
    np.savez_compressed(os.path.join(OUT, "ca_schedule.npz"), **out)


def gen_step(ldm, top):
    sched = ref_schedule(top, **cu.STEP_SCHEDULE)
    out = {}
    for shape, t in cu.STEP_CASES:
        x, mo, nz = cu.step_inputs(shape)
        tt = torch.tensor(t, dtype=torch.long)
        for param in cu.STEP_PARAMS:
            for clip in (False, True):
                st = make_stand(ldm, sched, param)
                st.apply_model = lambda x_, t_, c_, return_ids=False: T(mo).clone()
                ldm.noise_like = lambda shape_, device, repeat=False: T(nz).clone()
                with torch.no_grad():
                    *_, xr = st.p_mean_variance(T(x).clone(), None, tt, clip_denoised=clip, return_x0=True)
                    _, _, _, raw = st.p_mean_variance(T(x).clone(), None, tt, clip_denoised=False, return_x0=True)
                if clip:
                    changed = float((xr != raw).float().mean())
                    assert 0.0 < changed < 1.0, f"{shape} {param}: the clamp changes {changed:.2f} of the values"
                for temp in cu.STEP_TEMPS:
                    with torch.no_grad():
                        xp = st.p_sample(T(x).clone(), None, tt, clip_denoised=clip, temperture=temp)
                    tag = cu.step_tag(shape, param, clip, temp)
                    out[tag + "_xprev"] = xp.numpy()
                    out[tag + "_xrecon"] = xr.numpy()
    np.savez_compressed(os.path.join(OUT, "ca_step.npz"), **out)


def gen_blend(ldm, top):
    sched = ref_schedule(top, **cu.LOOP_SCHEDULE)
    x0, qn, imgs = cu.blend_inputs()
    out = {}
    for kind in cu.BLEND_MASKS:
        for binary in (True, False):
            mask = cu.blend_mask(kind, binary)
            st = make_stand(ldm, sched)
            st.p_sample = lambda img, cond, ts, **kw: T(imgs[int(ts[0])]).clone()
            st.q_sample = lambda x_start, t, noise=None: ldm.DDPM.q_sample(st, x_start, t,
                                                                           noise=T(qn[int(t[0])]).clone())
            with torch.no_grad():
                _, inter = st.p_sample_loop(None, cu.BLEND_SHAPE, return_intermediates=True,
                                            x_T=torch.zeros(cu.BLEND_SHAPE), verbose=False, mask=T(mask),
                                            x0=T(x0), log_every_t=1)
            assert len(inter) == cu.LOOP_T + 1
            # inter[1 + k] is the image after timestep T-1-k: store by timestep
            out[f"{kind}_{'bin' if binary else 'frac'}"] = np.stack([inter[cu.LOOP_T - i].numpy()
                                                                    for i in range(cu.LOOP_T)])
    np.savez_compressed(os.path.join(OUT, "ca_blend.npz"), **out)


def gen_loop(ldm, top):
    sched = ref_schedule(top, **cu.LOOP_SCHEDULE)
    d = cu.loop_inputs()
    n, dim = cu.LOOP_VQ_CASE[:2]
    cb, _ = vu.case_data(cu.LOOP_VQ_CASE)
    real_q = mgv.ref_vq(n, dim, cb)
    seen = []

    class RecQ(torch.nn.Module):
        def forward(self, z):
            seen.append(z.numpy().copy())
            return real_q(z)

    out = {}
    for mode in cu.LOOP_MODES:
        st = make_stand(ldm, sched, clip_denoised=(mode == "clip"), quantizer=RecQ())
        cur = [None]

        def apply_model(x_, t_, c_, return_ids=False):
            cur[0] = int(t_[0])
            return T(d["es"][cur[0]]).clone()

        st.apply_model = apply_model
        ldm.noise_like = lambda shape_, device, repeat=False: T(d["nz"][cur[0]]).clone()
        st.q_sample = lambda x_start, t, noise=None: ldm.DDPM.q_sample(st, x_start, t,
                                                                       noise=T(d["qn"][int(t[0])]).clone())
        kw = {}
        if mode == "mask":
            kw = dict(mask=T(d["mask"]), x0=T(d["x0"]))
        del seen[:]
        with mg.quiet(), torch.no_grad():
            img, inter = st.p_sample_loop(None, cu.LOOP_SHAPE, return_intermediates=True, x_T=T(d["xT"]).clone(),
                                          verbose=False, quantize_denoised=(mode == "quantize"), log_every_t=1,
                                          **kw)
        assert len(inter) == cu.LOOP_T + 1 and torch.equal(img, inter[-1])
        if mode == "quantize":
            assert len(seen) == cu.LOOP_T
            for i, zin in enumerate(seen):
                g = vu.rel_gap(zin, cb)
                assert g.min() >= vu.GAP_MIN, f"quantize step {i}: near-tie row ({g.min():.2e}); change the seed"
        out[mode] = np.stack([t.numpy() for t in inter[1:]])
        assert np.isfinite(out[mode]).all()
        print(f"loop {mode}: |x| max {np.abs(out[mode]).max():.3f}")
    np.savez_compressed(os.path.join(OUT, "ca_loop.npz"), **out)


def gen_unet(top):
    with mg.quiet():
        from openai_model.model import UNetModel
        torch.manual_seed(cu.UNET_SEED)
        m = UNetModel(**cu.TINY_UNET_CONCAT)
    mg.reinit_(m, cu.UNET_SEED)
    m.eval()
    d = {k: T(v) for k, v in cu.unet_inputs().items()}
    dw = types.SimpleNamespace(diffusion_model=m)
    out = dict(mg.sd_keys(m), seed=np.int64(cu.UNET_SEED),
               cfg=np.frombuffer(json.dumps(cu.TINY_UNET_CONCAT).encode(), dtype=np.uint8))
    with mg.quiet(), torch.no_grad():
        dw.conditional_key = "hybrid"
        out["y_hybrid"] = top.DiffusionWrapper.forward(dw, d["x"], d["t"], c_concat=[d["m"], d["zi"]],
                                                       c_crossattn=[d["ctx"]]).numpy()
        ref = m(torch.cat([d["x"], d["m"], d["zi"]], 1), d["t"], context=d["ctx"])
        assert torch.equal(ref, T(out["y_hybrid"]))
    np.savez_compressed(os.path.join(OUT, "unet_tiny_concat.npz"), **out)


def main():
    ldm, top = install_shims()
    torch.set_num_threads(8)
    gen_schedule(top)
    gen_step(ldm, top)
    gen_blend(ldm, top)
    gen_loop(ldm, top)
    gen_unet(top)
    for f in sorted(os.listdir(OUT)):
        if (f.startswith("ca_") or f == "unet_tiny_concat.npz") and f.endswith(".npz"):
            print(f, os.path.getsize(os.path.join(OUT, f)))


if __name__ == "__main__":
    main()
