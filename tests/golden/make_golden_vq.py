"""Generate the vector-quantiser fixtures by importing the REFERENCE itself (build container only).

Run from the repo root:  python tests/golden/make_golden_vq.py
Needs the reference checkout make_golden.py points at (read-only) and einops.  Uses the shims of make_golden.py (Lightning / Ema
stand-ins, fp32 ``nonlinearity``, ``lossconfig={"target": "torch.nn.Identity"}``, silenced stdout) and
replaces its ``vqvae.autoencoder`` stub by the reference's real module.

Imports ``vqvae.quantize.VectorQuantize2``, ``vqvae.autoencoder.VQModel`` / ``VQModelInterface``,
``ldm.tamming.quantize.VectorQuantizer2`` (``get_codebook_entry`` / ``unmap_to_all``) and
``DDIM.ddim.DDIMSampler``.  Inputs and codebooks are regenerated from seeds (tests/vq_util.py,
synth.py); the fixtures hold indices (int32), relative fp64 gaps, outputs and seeds only:

* vq_kernel.npz — per case of vq_util.KERNEL_CASES the reference's indices and the per-row gap
  (second-best − best fp64 distance) / (‖z‖² + ‖e_best‖²); asserts the near-tie cap, that the
  reference's fp32 argmin is the fp64 argmin, and that z + (e[idx] − z) recomputed from the indices
  is the reference's z_q bit for bit.
* vq_remap.npz — remap ("extra" / integer unknown index), sane_index_shape, loss (legacy and not),
  get_codebook_entry round trip, constructor kwargs and state_dict keys.
* vq_model.npz — tiny VQModelInterface / VQModel: decode with and without quantisation (plain, scaled,
  tiled), encode.
* vq_ddim.npz — DDIMSampler.sample(quantize_x0=True) with a stub model that returns recorded tensors.
"""
from __future__ import annotations

import inspect
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg                                    # noqa: E402
import vq_util as vu                                        # noqa: E402

OUT = HERE


def install_shims():
    mg.install_shims()
    pl = sys.modules["pytorch_lightning"]
    pl.Trainer = object
    cb = types.ModuleType("pytorch_lightning.callbacks")
    cb.ModelCheckpoint = object
    cb.LearningRateMonitor = object
    pl.callbacks = cb
    sys.modules["pytorch_lightning.callbacks"] = cb
    sys.modules["Ema.ema"].LitEma = object
    del sys.modules["vqvae.autoencoder"]                    # the real one is the subject here
    with mg.quiet():
        import Unet.unet as uu
        import Encoder_Decoder.encoder as ee
        silu = lambda x: x * torch.sigmoid(x)               # noqa: E731  (no fp16 cast)
        uu.nonlinearity = silu
        ee.nonlinearity = silu


def ref_vq(n_e, e_dim, codebook, cls=None, **kw):
    if cls is None:
        from vqvae.quantize import VectorQuantize2 as cls
    with mg.quiet():
        q = cls(n_e=n_e, e_dim=e_dim, beta=0.25, **kw)
    with torch.no_grad():
        q.embedding.weight.copy_(torch.from_numpy(codebook))
    return q.eval()


def gen_kernel():
    out = {}
    for case in vu.KERNEL_CASES:
        n, d, b, h, w = case
        cb, z = vu.case_data(case)
        q = ref_vq(n, d, cb)
        with mg.quiet(), torch.no_grad():
            zq, _, (_, _, idx) = q(torch.from_numpy(z))
        idx = idx.numpy().reshape(-1)
        d64 = vu.dist64(z, cb)
        assert (d64.argmin(1) == idx).all(), f"{case}: the reference's fp32 argmin is not the fp64 argmin"
        gap = vu.rel_gap(z, cb, idx)
        frac = float((gap < vu.GAP_MIN).mean())
        assert frac <= vu.NEAR_TIE_CAP, f"{case}: {frac:.4f} of the rows are near-ties"
        assert np.array_equal(vu.straight_through(z, cb, idx), zq.numpy()), f"{case}: z_q is not z + (e - z)"
        tag = vu.case_tag(case)
        out[tag + "_idx"] = idx.astype(np.int32)
        out[tag + "_gap"] = gap.astype(np.float32)
        print(f"kernel {case}: near-tie rows {frac * 100:.3f} %  min gap {gap.min():.3e}")
    # planted / tie inputs of the tests: the reference returns the planted index (checked here only)
    for case in ((8192, 3, 2, 16, 16), (512, 64, 4, 16, 16)):
        n, d, b, h, w = case
        cb, _ = vu.case_data(case)
        pid = np.random.Generator(np.random.PCG64(5)).integers(0, n, size=b * h * w)
        z = cb[pid] + np.float32(1e-3) * vu.randn(6, b * h * w, d)
        z = np.ascontiguousarray(z.reshape(b, h, w, d).transpose(0, 3, 1, 2))
        with mg.quiet(), torch.no_grad():
            _, _, (_, _, idx) = ref_vq(n, d, cb)(torch.from_numpy(z))
        assert (idx.numpy().reshape(-1) == pid).all(), f"planted {case}"
    np.savez_compressed(os.path.join(OUT, "vq_kernel.npz"), **out)


REMAP_CASE = (64, 4, 2, 4, 4)
REMAP_USED = [10, 20, 30, 40, 50]


def gen_remap():
    from vqvae.quantize import VectorQuantize2
    from vqvae.autoencoder import VQModel, VQModelInterface
    from ldm.tamming.quantize import VectorQuantizer2
    n, d, b, h, w = REMAP_CASE
    cb, z = vu.case_data(REMAP_CASE)
    zt = torch.from_numpy(z)
    out = {"used": np.asarray(REMAP_USED, dtype=np.int64)}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "used.npy")
        np.save(path, out["used"])
        with mg.quiet(), torch.no_grad():
            _, _, (_, _, plain) = ref_vq(n, d, cb)(zt)
            out["idx"] = plain.numpy().astype(np.int32)
            for tag, unk in (("extra", "extra"), ("int", 2)):
                q = ref_vq(n, d, cb, remap=path, unknown_index=unk)
                _, _, (_, _, r) = q(zt)
                assert tuple(r.shape) == (b * h * w, 1)
                out[f"remap_{tag}"] = r.numpy().astype(np.int32)
                qs = ref_vq(n, d, cb, remap=path, unknown_index=unk, sane_index_shape=True)
                _, _, (_, _, rs) = qs(zt)
                assert tuple(rs.shape) == (b, h, w) and np.array_equal(rs.numpy().reshape(-1, 1), r.numpy())
                # get_codebook_entry / unmap_to_all: the CompVis class (the vqvae/ copy lacks them)
                t = ref_vq(n, d, cb, cls=VectorQuantizer2, remap=path, unknown_index=unk)
                back = t.unmap_to_all(r.reshape(b, -1).clone())
                out[f"unmap_{tag}"] = back.numpy().astype(np.int32)
                ent = t.get_codebook_entry(r.reshape(-1).clone(), (b, h, w, d))
                assert np.array_equal(ent.numpy(), cb[back.numpy().reshape(-1)].reshape(b, h, w, d)
                                      .transpose(0, 3, 1, 2))
            known = np.isin(out["idx"], out["used"]).mean()
            assert 0.02 < known < 0.98, known           # both known and unknown indices occur
            for tag, legacy in (("legacy", True), ("nonlegacy", False)):
                _, loss, _ = ref_vq(n, d, cb, legacy=legacy)(zt)
                out[f"loss_{tag}"] = np.float64(loss.item())
    meta = {"vq_kwargs": list(inspect.signature(VectorQuantize2.__init__).parameters)[1:],
            "vqmodel_kwargs": list(inspect.signature(VQModel.__init__).parameters)[1:],
            "vqinterface_kwargs": list(inspect.signature(VQModelInterface.__init__).parameters)[1:]}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "used.npy")
        np.save(path, out["used"])
        with mg.quiet():
            meta["vq_keys"] = list(VectorQuantize2(8, 2, 0.25).state_dict().keys())
            meta["vq_remap_keys"] = list(VectorQuantize2(64, 2, 0.25, remap=path).state_dict().keys())
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(OUT, "vq_remap.npz"), **out)


TINY_VQ = dict(mg.TINY_VAE, double_z=False)
TINY_VQ_EMBED, TINY_VQ_CODES = 3, 64
MODEL_SEED = 61


def gen_model():
    from vqvae.autoencoder import VQModel, VQModelInterface
    kw = dict(ddconfig=dict(TINY_VQ), n_embed=TINY_VQ_CODES, embed_dim=TINY_VQ_EMBED,
              lossconfig={"target": "torch.nn.Identity"})
    with mg.quiet():
        vqi = VQModelInterface(**kw)
        vqm = VQModel(**kw)
    mg.reinit_(vqi, MODEL_SEED)
    vqm.load_state_dict(vqi.state_dict())
    vqi.eval(), vqm.eval()
    cb = vqi.quantize.embedding.weight.detach().numpy()
    sf = 0.5
    h = vu.randn(MODEL_SEED + 1, 2, 3, 8, 8) * np.float32(0.6)
    zs = vu.randn(MODEL_SEED + 2, 2, 3, 8, 8) * np.float32(0.3)          # latent-space (scaled) input
    zt = vu.randn(MODEL_SEED + 3, 2, 3, 12, 12) * np.float32(0.3)        # tiled: 2x2 grid of 8x8 patches
    x = np.random.Generator(np.random.PCG64(MODEL_SEED + 4)).random((2, 3, 16, 16), dtype=np.float32) * 2 - 1
    cids = np.random.Generator(np.random.PCG64(MODEL_SEED + 5)).integers(0, TINY_VQ_CODES, size=(2, 8, 8))
    for name, lat in (("h", h), ("zs", (1.0 / sf * torch.from_numpy(zs)).numpy()),
                      ("zt", (1.0 / sf * torch.from_numpy(zt)).numpy())):
        g = vu.rel_gap(lat, cb)
        assert g.min() >= vu.GAP_MIN, f"{name}: a row is a near-tie ({g.min():.2e}); change the seed"
    out = dict(mg.sd_keys(vqi), seed=np.int64(MODEL_SEED), scale_factor=np.float64(sf), h=h, zs=zs, zt=zt, x=x,
               cids=cids.astype(np.int32),
               cfg=np.frombuffer(json.dumps(TINY_VQ).encode(), dtype=np.uint8))
    sp = {"patch_distributed_vq": True, "ks": (8, 8), "stride": (4, 4), "vqf": 2, "clip_min_weight": 0.01,
          "clip_max_weight": 0.5, "tie_braker": True, "clip_min_tie_weight": 0.01, "clip_max_tie_weight": 0.5}
    out["sp"] = np.frombuffer(json.dumps(sp).encode(), dtype=np.uint8)
    with mg.quiet(), torch.no_grad():
        ht = torch.from_numpy(h)
        out["dec_q"] = vqi.decode(ht).numpy()
        out["dec_nq"] = vqi.decode(ht, force_not_quantize=True).numpy()
        # LatentDiffusion.decode_first_stage composed with the CompVis scaling 1/scale_factor * z
        # (ldm/diffusion/ddpm.py:1095; Diffusion/ddpm.py:728 drops z — SURVEY Q8)
        zz = 1.0 / sf * torch.from_numpy(zs)
        out["ld_dec_q"] = vqi.decode(zz).numpy()
        out["ld_dec_nq"] = vqi.decode(zz, force_not_quantize=True).numpy()
        ent = vqi.quantize.embedding(torch.from_numpy(cids)).permute(0, 3, 1, 2).contiguous()
        out["ld_dec_cids"] = vqi.decode(1.0 / sf * ent, force_not_quantize=True).numpy()
        # encode
        hq, zero, info = vqi.encode(torch.from_numpy(x))
        assert float(zero) == 0.0 and info == (None, None, None)
        out["enc_h"] = hq.numpy()
        # VQModel.encode as written fails after quantising (it prints ``info.shape`` of a tuple,
        # autoencoder.py:134): its three calls are made directly
        quant, _, (_, _, eidx) = vqm.quantize(vqm.quant_conv(vqm.encoder(torch.from_numpy(x))))
        out["enc_idx"] = eidx.numpy().astype(np.int32)
        # tiled decode, composed as make_golden.gen_tiled_decode
        from Diffusion.ddpm import LatentDiffusion as RefLD

        def delta_border(self, hh, ww):
            lower_right_corner = torch.tensor([hh - 1, ww - 1]).view(1, 1, 2)
            arr = self.meshgrid(hh, ww) / lower_right_corner
            dist_left_up = torch.min(arr, dim=-1, keepdim=True)[0]
            dist_right_down = torch.min(1 - arr, dim=-1, keepdim=True)[0]
            return torch.min(torch.cat([dist_left_up, dist_right_down], dim=-1), dim=-1)[0]

        class Stand:
            split_input_params = sp
            meshgrid = RefLD.meshgrid
            get_weighting = RefLD.get_weighting
            get_fold_unfold = RefLD.get_fold_unfold

        Stand.delta_border = delta_border
        st = Stand()
        z = 1.0 / sf * torch.from_numpy(zt)
        ks, stride, uf = sp["ks"], sp["stride"], sp["vqf"]
        fold, unfold, normalization, weighting = st.get_fold_unfold(z, ks, stride, uf=uf)
        zp = unfold(z)
        zp = zp.view((zp.shape[0], -1, ks[0], ks[1], zp.shape[-1]))
        assert zp.shape[-1] == 4
        o = torch.stack([vqi.decode(zp[:, :, :, :, i]) for i in range(zp.shape[-1])], axis=-1)
        o = (o * weighting).view((o.shape[0], -1, o.shape[-1]))
        out["ld_dec_tiled"] = (fold(o) / normalization).numpy()
    np.savez_compressed(os.path.join(OUT, "vq_model.npz"), **out)


DDIM_CASE = (256, 4, 2, 8, 8)
DDIM_STEPS = 4


def gen_ddim():
    fake = mg.gen_schedule.__fake__
    ddim_mod = mg.make_ddim_sampler(fake)
    n, d, b, h, w = DDIM_CASE
    cb, _ = vu.case_data(DDIM_CASE)
    s0 = vu.case_seed(DDIM_CASE)
    xT = vu.randn(s0 + 10, b, d, h, w)
    es = vu.randn(s0 + 11, DDIM_STEPS, b, d, h, w)
    nz = vu.randn(s0 + 12, DDIM_STEPS, b, d, h, w)
    real_q = ref_vq(n, d, cb)
    seen = []

    class RecQ(torch.nn.Module):
        def forward(self, z):
            seen.append(z.numpy().copy())
            return real_q(z)

    class FS:
        quantize = RecQ()

    class M:
        num_timesteps = 1000
        alphas_cumprod = fake.alphas_cumprod
        alphas_cumprod_prev = fake.alphas_cumprod_prev
        betas = fake.betas
        device = torch.device("cpu")
        parameterization = "eps"
        first_stage_model = FS()

        def __init__(self):
            self.calls = 0

        def apply_model(self, x, t, c):
            e = torch.from_numpy(es[self.calls])
            self.calls += 1
            return e

    out = {"seed": np.int64(s0), "steps": np.int64(DDIM_STEPS)}
    for eta in (0.0, 1.0):
        cnt = [0]

        def noise_like(shape, device, repeat=False):
            t = torch.from_numpy(nz[cnt[0]])
            cnt[0] += 1
            return t

        ddim_mod.noise_like = noise_like
        del seen[:]
        s = ddim_mod.DDIMSampler(M())
        with mg.quiet(), torch.no_grad():
            samples, inter = s.sample(S=DDIM_STEPS, batch_size=b, shape=(d, h, w), conditioning=None, eta=eta,
                                      x_T=torch.from_numpy(xT), verbose=False, log_every_t=1, quantize_x0=True)
        assert len(seen) == DDIM_STEPS and len(inter["x_inter"]) == DDIM_STEPS + 1
        for i, zin in enumerate(seen):
            g = vu.rel_gap(zin, cb)
            assert g.min() >= vu.GAP_MIN, f"eta {eta} step {i}: near-tie row ({g.min():.2e}); change the seed"
        tag = f"eta{int(eta)}"
        out[f"{tag}_x_inter"] = np.stack([t.numpy() for t in inter["x_inter"][1:]])
        out[f"{tag}_pred_x0"] = np.stack([t.numpy() for t in inter["pred_x0"][1:]])
        assert np.array_equal(out[f"{tag}_x_inter"][-1], samples.numpy())
    np.savez_compressed(os.path.join(OUT, "vq_ddim.npz"), **out)


def main():
    install_shims()
    torch.set_num_threads(8)
    mg.gen_schedule.__fake__ = _schedule_only()
    gen_kernel()
    gen_remap()
    gen_model()
    gen_ddim()
    for f in sorted(os.listdir(OUT)):
        if f.startswith("vq_") and f.endswith(".npz"):
            print(f, os.path.getsize(os.path.join(OUT, f)))


def _schedule_only():
    """The schedule tables of make_golden.gen_schedule without rewriting schedule.npz."""
    sys.path.insert(0, os.path.join(mg.REF, "DDIM"))
    with mg.quiet():
        from Diffusion.ddpm import DDPM

    class FakeDDPM:
        v_posterior = 0.0
        parameterization = "eps"

        def register_buffer(self, name, t, persistent=True):
            setattr(self, name, t)

    fake = FakeDDPM()
    DDPM.register_schedule(fake, beta_schedule="linear", timesteps=1000, linear_start=0.00085, linear_end=0.012)
    return fake


if __name__ == "__main__":
    main()
