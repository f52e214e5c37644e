"""Generate the patch-wise UNet / tiled encode fixtures (``split_input_params``) by running the REFERENCE itself
(build container only, CPU).

Run from the repo root:  python tests/golden/make_golden_patch.py
Needs the reference checkout make_golden.py points at (read-only), einops and tqdm.  Uses the shims of
make_golden.py and make_golden_concat_ancestral.py (flash_attn / omegaconf / Lightning / torchvision stand-ins,
identity ``.half()``, the import-time names of ``ldm/diffusion/ddpm.py``).

The arithmetic is executed by the reference's own functions, called on a stand-in ``self`` (class ``Stand``):
``LatentDiffusion.apply_model`` / ``encode_first_stage`` / ``get_fold_unfold`` / ``get_weighting`` / ``meshgrid`` and
``DiffusionWrapper.forward`` of ``Diffusion/ddpm.py``, ``openai_model.model.UNetModel``, ``DDIMSampler`` of
``DDIM/ddim.py``, the tiny ``AutoEncoderKL`` / ``VQModelInterface``.  What the stand-in supplies instead of the
reference (each a documented quirk):

* ``delta_border`` takes its first min over the last dim (as written, dim=1 fails in torch.cat for w > 1 — Q14);
* the schedule is the one of make_golden_concat_ancestral.ref_schedule;
* 'concat' conditioning is passed as ``{'c_concat': tensor}``: ``apply_model`` unfolds ``next(iter(cond.values()))``,
  which must be a tensor (the list it builds itself from a bare tensor fails in ``Unfold``);
* ``first_stage_model.encode`` returns a tensor: ``h`` of the VQ interface's ``(h, 0, info)`` tuple, and the moments
  (``posterior.parameters``) of the KL posterior — ``encode_first_stage`` stacks what ``encode`` returns, and neither
  tuples nor distribution objects stack (Q27).

Inputs are regenerated from seeds (tests/patch_util.py); the fixtures hold the reference's outputs, and for each
model the state_dict key order + shapes (``keys``), ``cfg`` and ``seed`` the tests regenerate its weights from:

* patch_tables.npz — weighting and normalisation of ``get_fold_unfold`` per case of patch_util.TABLE_CASES, tie-breaker
  on and off;
* patch_unet_concat.npz / patch_unet_crossattn.npz / patch_unet_adm.npz — ``apply_model`` under ``split_input_params``
  (tie-breaker on and off), a 3-step eta = 0 DDIM loop on the concat model, the same with CFG on the crossattn model;
* patch_encode_kl.npz / patch_encode_vq.npz — the tiled ``encode_first_stage``.
"""
from __future__ import annotations

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
import make_golden_concat_ancestral as mgca                 # noqa: E402
import patch_util as pu                                     # noqa: E402

OUT = HERE
T = torch.from_numpy


def delta_border(self, h, w):
    lower_right_corner = torch.tensor([h - 1, w - 1]).view(1, 1, 2)
    arr = self.meshgrid(h, w) / lower_right_corner
    dist_left_up = torch.min(arr, dim=-1, keepdim=True)[0]
    dist_right_down = torch.min(1 - arr, dim=-1, keepdim=True)[0]
    return torch.min(torch.cat([dist_left_up, dist_right_down], dim=-1), dim=-1)[0]


def make_stand(top, sp, sched=None):
    """The stand-in ``self``: the reference's own tiling methods, the fixed ``delta_border``, and (for the DDIM
    loops) the schedule buffers the sampler reads."""
    class Stand:
        parameterization = "eps"
        device = torch.device("cpu")

    for name in ("apply_model", "encode_first_stage", "get_fold_unfold", "get_weighting", "meshgrid"):
        setattr(Stand, name, getattr(top.LatentDiffusion, name))
    Stand.delta_border = delta_border
    st = Stand()
    st.split_input_params = dict(sp)
    if sched is not None:
        st.num_timesteps = sched.num_timesteps
        for k in ("alphas_cumprod", "alphas_cumprod_prev", "betas"):
            setattr(st, k, getattr(sched, k))
    return st


def build_unet(top, name):
    cfg, seed = pu.MODELS[name]
    with mg.quiet():
        from openai_model.model import UNetModel
        torch.manual_seed(seed)
        m = UNetModel(**cfg)
    mg.reinit_(m, seed)
    m.eval()

    class Wrapper:                       # the reference's DiffusionWrapper.forward on this UNet
        diffusion_model = m
        conditional_key = name

        def __call__(self, *a, **kw):
            return top.DiffusionWrapper.forward(self, *a, **kw)

    out = dict(mg.sd_keys(m), seed=np.int64(seed), cfg=np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8))
    return Wrapper(), out


def save(name, out):
    for k, v in out.items():
        if k.startswith(("y_", "ddim_", "enc_")):
            assert np.isfinite(v).all() and np.abs(v).max() > 1e-3, f"{name}/{k}: degenerate output"
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)


def gen_tables(top):
    out = {}
    for tag, (h, w, ks, stride, df) in pu.TABLE_CASES.items():
        for tie in (True, False):
            st = make_stand(top, pu.split_params(ks, stride, tie))
            with mg.quiet():
                _, _, norm, wt = st.get_fold_unfold(torch.zeros(1, 1, h, w), ks, stride, df=df)
            assert norm.shape == (1, 1, h // df, w // df) and wt.shape[2:4] == (ks[0] // df, ks[1] // df)
            out[f"{tag}_tie{int(tie)}_norm"] = norm[0, 0].numpy()
            out[f"{tag}_tie{int(tie)}_weighting"] = wt[0, 0].numpy()          # [kh, kw, L]
    np.savez_compressed(os.path.join(OUT, "patch_tables.npz"), **out)


def ref_cond(name, d):
    """(cond_stage_key, conditioning as the reference's apply_model takes it)."""
    if name == "concat":
        return "image", {"c_concat": T(d["cc"])}
    if name == "crossattn":
        return "txt", T(d["ctx"])
    return "class_label", T(d["y"])


def gen_unet(top, name, sched):
    model, out = build_unet(top, name)
    d = pu.unet_inputs()
    key, cond = ref_cond(name, d)
    untiled = None
    for tie in ((True, False) if name != "adm" else (True,)):
        st = make_stand(top, pu.split_params(pu.KS, pu.STRIDE, tie), sched)
        st.model, st.cond_stage_key = model, key
        with mg.quiet(), torch.no_grad():
            y = st.apply_model(T(d["x"]), T(d["t"]), cond)
            if untiled is None:
                del st.split_input_params
                untiled = st.apply_model(T(d["x"]), T(d["t"]), cond if name != "concat" else [T(d["cc"])])
        assert y.shape == pu.X_SHAPE
        out[f"y_tie{int(tie)}"] = y.numpy()
    # the blend is not the untiled call (a test that ran the UNet untiled must fail)
    assert (T(out["y_tie1"]) - untiled).abs().max() > 1e-2 * untiled.abs().max()
    if name in ("concat", "crossattn"):
        ddim_mod = mg.make_ddim_sampler(None)
        ddim_mod.noise_like = lambda shape, device, repeat=False: torch.zeros(shape)     # eta = 0: sigma z = 0
        st = make_stand(top, pu.split_params(pu.KS, pu.STRIDE, True), sched)
        st.model, st.cond_stage_key = model, key
        s = ddim_mod.DDIMSampler(st)
        kw = {}
        if name == "crossattn":
            kw = dict(unconditional_guidance_scale=pu.CFG_SCALE, unconditional_conditioning=T(d["uc"]))
        with mg.quiet(), torch.no_grad():
            samples, _ = s.sample(S=pu.DDIM_STEPS, batch_size=2, shape=pu.X_SHAPE[1:], conditioning=cond, eta=0.0,
                                  x_T=T(d["xT"]), verbose=False, **kw)
        out["ddim_samples"] = samples.numpy()
    save(f"patch_unet_{name}", out)


def gen_encode(top):
    with mg.quiet():
        from VAE.autoencoder import AutoEncoderKL
        from vqvae.autoencoder import VQModelInterface
        vae = AutoEncoderKL(ddconfig=dict(pu.TINY_VAE), embed_dim=4, lossconfig={"target": "torch.nn.Identity"})
        vqi = VQModelInterface(ddconfig=dict(pu.TINY_VQ), n_embed=pu.TINY_VQ_CODES, embed_dim=pu.TINY_VQ_EMBED,
                               lossconfig={"target": "torch.nn.Identity"})
    x = T(pu.encode_input())
    sp = pu.split_params(pu.ENC_KS, pu.ENC_STRIDE, True, patch_distributed_vq=True, vqf=pu.ENC_VQF)
    for kind, fs, cfg, enc in (("kl", vae, pu.TINY_VAE, lambda z: vae.encode(z).parameters),
                               ("vq", vqi, pu.TINY_VQ, lambda z: vqi.encode(z)[0])):
        mg.reinit_(fs, pu.ENC_SEEDS[kind])
        fs.eval()
        st = make_stand(top, sp)
        st.first_stage_model = types.SimpleNamespace(encode=enc)
        with mg.quiet(), torch.no_grad():
            tiled = st.encode_first_stage(x)
            whole = enc(x)
        assert tuple(st.split_input_params["original_image_size"]) == pu.ENC_SHAPE[2:]
        assert tiled.shape == whole.shape and (tiled - whole).abs().max() > 1e-3 * whole.abs().max()
        out = dict(mg.sd_keys(fs), seed=np.int64(pu.ENC_SEEDS[kind]), enc_tiled=tiled.numpy(),
                   cfg=np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8))
        save(f"patch_encode_{kind}", out)


def main():
    _, top = mgca.install_shims()
    torch.set_num_threads(8)
    sched = mgca.ref_schedule(top, **pu.SCHEDULE)
    gen_tables(top)
    for name in ("concat", "crossattn", "adm"):
        gen_unet(top, name, sched)
    gen_encode(top)
    for f in sorted(os.listdir(OUT)):
        if f.startswith("patch_") and f.endswith(".npz"):
            print(f, os.path.getsize(os.path.join(OUT, f)))


if __name__ == "__main__":
    main()
