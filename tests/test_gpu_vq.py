"""VQ first stage on the GPU (run with -m gpu): the fused nearest-code search, lookup / remap, the
VQModel / VQModelInterface mirrors, LatentDiffusion with a VQ first stage and DDIM ``quantize_x0``,
against fixtures written by the reference itself (tests/golden/make_golden_vq.py).

Search criterion (per case of vq_util.KERNEL_CASES): on every row whose stored relative fp64 gap
between best and second-best code is >= 1e-5 the index equals the reference's and z_q is bit-equal to
the reference's z + (e - z); on the other rows (at most 1 % of a case) the chosen code's fp64
distance exceeds the minimum by at most 1e-5 (|z|^2 + |e|^2).  1e-5: a k-ordered fp32 dot product
is off by about 1.5e-7 sum|ab| at K <= 1024, so the bound keeps more than a tenfold margin.

Parity limits of the model tests: (rel-L2, max-abs / max), each at most 3.5x the error measured on
MI355X (profiles/vq_parity_errors.txt); the measured values stand next to the limits below."""
import json

import numpy as np
import pytest
import torch

import vq_util as vu
from golden_util import cfg_of, load, weights_of
from gpu_util import check_parity

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

# tag: (rel-L2 limit, max-abs limit)                         # measured on MI355X (rel-L2 / max-abs)
VQ_LIMITS = {
    "tiny VQ decode (quantised) vs reference": (2.5e-3, 3e-3),           # 1.266e-3 / 1.233e-3
    "tiny VQ decode (not quantised) vs reference": (2.5e-3, 3e-3),       # 1.255e-3 / 1.352e-3
    "tiny VQ encode h vs reference": (2.7e-3, 2.6e-3),                    # 7.894e-4 / 7.659e-4
    "LD VQ decode_first_stage vs reference": (2.5e-3, 3e-3),             # 1.415e-3 / 1.378e-3
    "LD VQ decode_first_stage force_not_quantize vs reference": (2.5e-3, 3e-3),   # 1.395e-3 / 1.823e-3
    "LD VQ decode_first_stage predict_cids vs reference": (2.5e-3, 3e-3),         # 9.869e-4 / 9.066e-4
    "LD VQ tiled decode vs reference": (2.5e-3, 3e-3),                    # 1.328e-3 / 1.472e-3
}


def _check(tag, got, ref):
    return check_parity(tag, got, torch.from_numpy(np.asarray(ref)), *VQ_LIMITS[tag])


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _nearest(sdk, cb, z, splits=0):
    from sd_amd import ops
    zq, idx = ops.vq_nearest(_gpu(z), _gpu(cb), splits=splits)
    assert idx.dtype == torch.int64 and idx.shape == (z.shape[0] * z.shape[2] * z.shape[3],)
    assert zq.shape == z.shape and zq.dtype == torch.float32
    return zq.cpu().numpy(), idx.cpu().numpy()


def _planted(case, seed=5):
    n, d, b, h, w = case
    cb, _ = vu.case_data(case)
    pid = np.random.Generator(np.random.PCG64(seed)).integers(0, n, size=b * h * w)
    z = cb[pid] + np.float32(1e-3) * vu.randn(seed + 1, b * h * w, d)
    return cb, np.ascontiguousarray(z.reshape(b, h, w, d).transpose(0, 3, 1, 2)), pid


# ------------------------------------------------------------------ 1. kernel against the reference
@pytest.mark.parametrize("case", vu.KERNEL_CASES, ids=vu.case_tag)
def test_nearest_vs_reference(sdk, case):
    fx = load("vq_kernel")
    tag = vu.case_tag(case)
    ref_idx, gap = fx[tag + "_idx"].astype(np.int64), fx[tag + "_gap"]
    cb, z = vu.case_data(case)
    zq, idx = _nearest(sdk, cb, z)
    assert idx.min() >= 0 and idx.max() < case[0]
    good = gap >= vu.GAP_MIN
    print(f"[vq] {tag}: near-tie rows {(~good).sum()} / {good.size}, index mismatches {(idx != ref_idx).sum()}")
    assert (~good).mean() <= vu.NEAR_TIE_CAP
    assert np.array_equal(idx[good], ref_idx[good])
    ref_zq = vu.rows_of(vu.straight_through(z, cb, ref_idx))
    assert np.array_equal(vu.rows_of(zq)[good].view(np.uint32), ref_zq[good].view(np.uint32))
    # every row (near-ties included): the chosen code is within the bound of the fp64 minimum, and
    # z_q is the straight-through value of the code that was chosen
    d64 = vu.dist64(z, cb)
    rows = vu.rows_of(z).astype(np.float64)
    bound = vu.GAP_MIN * ((rows * rows).sum(1) + (cb[idx].astype(np.float64) ** 2).sum(1))
    assert (d64[np.arange(idx.size), idx] - d64.min(1) <= bound).all()
    assert np.array_equal(zq.view(np.uint32), vu.straight_through(z, cb, idx).view(np.uint32))


# ------------------------------------------------------------------ 2. planted
@pytest.mark.parametrize("case,splits", [((8192, 3, 2, 16, 16), 0), ((512, 64, 4, 16, 16), 0),
                                         ((8192, 3, 2, 16, 16), 3), ((512, 64, 4, 16, 16), 3)],
                         ids=["valu", "mfma", "valu_split3", "mfma_split3"])
def test_nearest_planted(sdk, case, splits):
    cb, z, pid = _planted(case)
    _, idx = _nearest(sdk, cb, z, splits=splits)
    assert np.array_equal(idx, pid)


# ------------------------------------------------------------------ 3. ties
@pytest.mark.parametrize("n,d,m,dups", [(8192, 3, 512, (7, 40, 63)), (512, 64, 96, (7, 40, 63)),
                                        (16384, 4, 16, (7, 40, 63)), (1024, 256, 16, (7, 40, 63)),
                                        (16384, 4, 16, (7, 5000, 16383)), (1024, 256, 16, (7, 500, 1023))],
                         ids=["valu", "mfma", "valu_split", "mfma_split", "valu_cross_split", "mfma_cross_split"])
def test_nearest_ties_lowest_index_wins(sdk, n, d, m, dups):
    from sd_amd import ops
    cb = vu.randn(31, n, d)
    for j in dups[1:]:
        cb[j] = cb[dups[0]]
    z = cb[dups[0]][None, :] + np.float32(1e-3) * vu.randn(32, m, d)
    z = np.ascontiguousarray(z.reshape(1, 1, m, d).transpose(0, 3, 1, 2))
    if m == 16:
        assert ops.lib().sdk_vq_nearest_splits(m, n, d) > 1          # these shapes take the split path
    _, idx = _nearest(sdk, cb, z)
    assert (idx == dups[0]).all(), idx


# ------------------------------------------------------------------ 4. determinism
@pytest.mark.parametrize("case", [(1024, 256, 1, 4, 4), (8192, 3, 2, 16, 16)], ids=vu.case_tag)
def test_nearest_is_deterministic(sdk, case):
    cb, z = vu.case_data(case)
    a = _nearest(sdk, cb, z)
    b = _nearest(sdk, cb, z)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


def test_nearest_nan_row_stays_in_range_and_bad_shapes_raise(sdk):
    from sd_amd import ops
    for case in ((256, 4, 1, 8, 8), (1000, 20, 1, 7, 11), (1024, 256, 1, 4, 4)):
        cb, z = vu.case_data(case)
        z[0, :, 0, 0] = np.nan
        z[0, 0, 1, 1] = np.inf
        _, idx = _nearest(sdk, cb, z)
        assert idx.min() >= 0 and idx.max() < case[0]
    cb, z = vu.case_data((256, 4, 1, 8, 8))
    with pytest.raises(ValueError):
        ops.vq_nearest(_gpu(z), _gpu(cb[:, :3]))
    with pytest.raises(TypeError):
        ops.vq_nearest(torch.from_numpy(z), _gpu(cb))
    with pytest.raises(ValueError):
        ops.vq_nearest(_gpu(vu.randn(1, 1, 257, 2, 2)), _gpu(vu.randn(2, 8, 257)))


# ------------------------------------------------------------------ 5. remap / lookup
def _quantizer(sdk, cb, **kw):
    from sd_amd.vqvae.quantize import VectorQuantize2
    q = VectorQuantize2(cb.shape[0], cb.shape[1], 0.25, **kw)
    q.load_state_dict({"embedding.weight": torch.from_numpy(cb)}, strict=False)
    return q.to(DEV)


def test_remap_against_reference(sdk, tmp_path):
    fx = load("vq_remap")
    case = (64, 4, 2, 4, 4)
    n, d, b, h, w = case
    cb, z = vu.case_data(case)
    path = str(tmp_path / "used.npy")
    np.save(path, fx["used"])
    zg = _gpu(z)
    _, _, (p, me, plain) = _quantizer(sdk, cb)(zg)
    assert p is None and me is None and plain.dtype == torch.int64 and plain.shape == (b * h * w,)
    assert np.array_equal(plain.cpu().numpy(), fx["idx"].astype(np.int64))
    for tag, unk in (("extra", "extra"), ("int", 2)):
        q = _quantizer(sdk, cb, remap=path, unknown_index=unk)
        _, _, (_, _, r) = q(zg)
        assert r.dtype == torch.int64 and r.shape == (b * h * w, 1)
        assert np.array_equal(r.cpu().numpy(), fx[f"remap_{tag}"].astype(np.int64))
        _, _, (_, _, rs) = _quantizer(sdk, cb, remap=path, unknown_index=unk, sane_index_shape=True)(zg)
        assert rs.shape == (b, h, w) and np.array_equal(rs.cpu().numpy().reshape(-1, 1), r.cpu().numpy())
        back = q.unmap_to_all(r.reshape(b, -1))
        assert np.array_equal(back.cpu().numpy(), fx[f"unmap_{tag}"].astype(np.int64))
        ent = q.get_codebook_entry(r.reshape(-1), (b, h, w, d))
        want = cb[fx[f"unmap_{tag}"].reshape(-1)].reshape(b, h, w, d).transpose(0, 3, 1, 2)
        assert np.array_equal(ent.cpu().numpy().view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
    q = _quantizer(sdk, cb, remap=path, unknown_index="random")
    _, _, (_, _, r) = q(zg)
    r = r.cpu().numpy().reshape(-1)
    assert q.re_embed == 5 and r.min() >= 0 and r.max() < q.re_embed
    known = np.isin(fx["idx"], fx["used"])
    pos = {int(v): i for i, v in enumerate(fx["used"])}
    assert all(r[i] == pos[int(fx["idx"][i])] for i in np.nonzero(known)[0])
    _, _, (_, _, s) = _quantizer(sdk, cb, sane_index_shape=True)(zg)
    assert s.shape == (b, h, w)


def test_get_codebook_entry_and_range_check(sdk):
    cb = vu.randn(41, 100, 5)
    q = _quantizer(sdk, cb)
    idx = np.random.Generator(np.random.PCG64(42)).integers(0, 100, size=(2, 3, 7))
    flat = q.get_codebook_entry(_gpu(idx), None)
    assert flat.shape == (2, 3, 7, 5)
    assert np.array_equal(flat.cpu().numpy().view(np.uint32), cb[idx].view(np.uint32))
    nchw = q.get_codebook_entry(_gpu(idx.reshape(-1)), (2, 3, 7, 5))
    assert np.array_equal(nchw.cpu().numpy().view(np.uint32),
                          np.ascontiguousarray(cb[idx].transpose(0, 3, 1, 2)).view(np.uint32))
    for bad in (100, -1):
        idx2 = idx.copy()
        idx2[1, 2, 3] = bad
        with pytest.raises(ValueError):
            q.get_codebook_entry(_gpu(idx2), None)


# ------------------------------------------------------------------ 6. loss
@pytest.mark.parametrize("legacy", [True, False], ids=["legacy", "nonlegacy"])
def test_loss_against_reference(sdk, legacy):
    fx = load("vq_remap")
    cb, z = vu.case_data((64, 4, 2, 4, 4))
    _, loss, _ = _quantizer(sdk, cb, legacy=legacy)(_gpu(z))
    ref = float(fx["loss_legacy" if legacy else "loss_nonlegacy"])
    print(f"[vq] loss legacy={legacy}: {float(loss):.8e} vs {ref:.8e}")
    assert abs(float(loss) - ref) <= 1e-5 * abs(ref)


# ------------------------------------------------------------------ 7. tiny VQModelInterface / VQModel
@pytest.fixture(scope="module")
def tiny(sdk):
    from sd_amd.vqvae.autoencoder import VQModel, VQModelInterface
    fx = load("vq_model")
    kw = dict(ddconfig=cfg_of(fx), n_embed=64, embed_dim=3, lossconfig={"target": "torch.nn.Identity"})
    sd = weights_of(fx)
    vqi, vqm = VQModelInterface(**kw), VQModel(**kw)
    vqi.load_state_dict(sd)
    vqm.load_state_dict(sd)
    return fx, sd, vqi.to(DEV), vqm.to(DEV)


def test_tiny_vq_interface_decode(tiny):
    fx, _, vqi, _ = tiny
    h = _gpu(fx["h"])
    _check("tiny VQ decode (quantised) vs reference", vqi.decode(h), fx["dec_q"])
    _check("tiny VQ decode (not quantised) vs reference", vqi.decode(h, force_not_quantize=True), fx["dec_nq"])
    got = vqi.decode((h, None, None))                       # the encode tuple is accepted
    assert torch.equal(got, vqi.decode(h))


def test_tiny_vq_encode(tiny):
    fx, sd, vqi, vqm = tiny
    x = _gpu(fx["x"])
    h, zero, info = vqi.encode(x)
    assert float(zero) == 0.0 and info == (None, None, None)
    _check("tiny VQ encode h vs reference", h, fx["enc_h"])
    quant, loss, (_, _, idx) = vqm.encode(x)
    assert idx.dtype == torch.int64 and loss.ndim == 0
    # indices against the CPU argmin of the GPU's own h, so fp16 conv error upstream cannot flip them
    cb = sd["quantize.embedding.weight"].numpy()
    hn = h.cpu().numpy()
    gap = vu.rel_gap(hn, cb)
    good = gap >= vu.GAP_MIN
    assert good.mean() >= 1 - vu.NEAR_TIE_CAP
    want = vu.dist64(hn, cb).argmin(1)
    assert np.array_equal(idx.cpu().numpy()[good], want[good])
    assert np.array_equal(quant.cpu().numpy().view(np.uint32),
                          vu.straight_through(hn, cb, idx.cpu().numpy()).view(np.uint32))
    dec, diff, ind = vqm(x, return_pred_indices=True)
    assert dec.shape == x.shape and torch.equal(ind, idx) and torch.equal(diff, loss)


# ------------------------------------------------------------------ 8. LatentDiffusion with a VQ first stage
def test_latent_diffusion_with_vq_first_stage(tiny):
    from sd_amd.Diffusion.ddpm import LatentDiffusion
    from sd_amd.Diffusion.utils import instantiate_from_config
    from sd_amd.vqvae.autoencoder import VQModelInterface
    fx, sd, _, _ = tiny
    sf = float(fx["scale_factor"])
    cfg = {"target": "Diffusion.ddpm.LatentDiffusion",
           "params": {"first_stage_config": {"target": "vqvae.autoencoder.VQModelInterface",
                                             "params": {"ddconfig": cfg_of(fx), "n_embed": 64, "embed_dim": 3,
                                                        "lossconfig": {"target": "torch.nn.Identity"}}},
                      "cond_stage_config": "__is_unconditional__",
                      "unet_config": {"target": "openai_model.model.UNetModel",
                                      "params": cfg_of(load("unet_tiny_uncond"))},
                      "scale_factor": sf, "image_size": 8, "channels": 3}}
    ld = instantiate_from_config(cfg)
    assert type(ld) is LatentDiffusion and type(ld.first_stage_model) is VQModelInterface
    ld.first_stage_model.load_state_dict(sd)
    ld = ld.to(DEV)
    z = _gpu(fx["zs"])
    _check("LD VQ decode_first_stage vs reference", ld.decode_first_stage(z), fx["ld_dec_q"])
    _check("LD VQ decode_first_stage force_not_quantize vs reference",
           ld.decode_first_stage(z, force_not_quantize=True), fx["ld_dec_nq"])
    cids = fx["cids"].astype(np.int64)
    by_index = ld.decode_first_stage(_gpu(cids), predict_cids=True)
    _check("LD VQ decode_first_stage predict_cids vs reference", by_index, fx["ld_dec_cids"])
    logits = 0.1 * vu.randn(3, 2, 64, 8, 8)
    np.put_along_axis(logits, cids[:, None], 5.0, axis=1)
    assert torch.equal(ld.decode_first_stage(_gpu(logits), predict_cids=True), by_index)
    x = _gpu(load("vq_model")["x"])
    h = ld.encode_first_stage(x)
    assert torch.is_tensor(h) and h.shape == (2, 3, 8, 8)
    assert torch.equal(ld.get_first_stage_encoding(h), sf * h)
    ld.split_input_params = json.loads(bytes(fx["sp"]).decode())
    tiled = ld.decode_first_stage(_gpu(fx["zt"]))
    assert tiled.shape == (2, 3, 24, 24)
    _check("LD VQ tiled decode vs reference", tiled, fx["ld_dec_tiled"])


# ------------------------------------------------------------------ 9. DDIM quantize_x0
DDIM_CASE = (256, 4, 2, 8, 8)


def _ddim_setup(sdk):
    from sd_amd.DDIM.ddim import DDIMSampler
    from sd_amd.DDIM.diffusion_modules import register_schedule
    n, d, b, h, w = DDIM_CASE
    cb, _ = vu.case_data(DDIM_CASE)
    s0 = vu.case_seed(DDIM_CASE)
    xT, es, nz = vu.randn(s0 + 10, b, d, h, w), vu.randn(s0 + 11, 4, b, d, h, w), vu.randn(s0 + 12, 4, b, d, h, w)
    sch = register_schedule(1000, 0.00085, 0.012)
    es_g, nz_g = _gpu(es), _gpu(nz)

    class FS:
        quantize = _quantizer(sdk, cb)

    class M:
        num_timesteps = 1000
        alphas_cumprod = sch["alphas_cumprod"]
        device = DEV
        parameterization = "eps"
        first_stage_model = FS()
        calls = 0

        def apply_model(self, x, t, c):
            e = es_g[self.calls % 4]
            self.calls += 1
            return e

    return DDIMSampler(M()), _gpu(xT), (lambda i, shape: nz_g[i]), (b, d, h, w)


@pytest.mark.parametrize("eta", [0.0, 1.0], ids=["eta0", "eta1"])
def test_ddim_quantize_x0_bitexact(sdk, eta):
    fx = load("vq_ddim")
    s, xT, noise_fn, (b, d, h, w) = _ddim_setup(sdk)
    out, inter = s.sample(S=4, batch_size=b, shape=(d, h, w), eta=eta, x_T=xT, verbose=False, log_every_t=1,
                          quantize_x0=True, noise_fn=noise_fn)
    tag = f"eta{int(eta)}"
    assert len(inter["x_inter"]) == 5
    for i in range(4):
        assert np.array_equal(inter["pred_x0"][i + 1].cpu().numpy().view(np.uint32),
                              fx[f"{tag}_pred_x0"][i].view(np.uint32)), f"pred_x0 step {i}"
        assert np.array_equal(inter["x_inter"][i + 1].cpu().numpy().view(np.uint32),
                              fx[f"{tag}_x_inter"][i].view(np.uint32)), f"x_prev step {i}"
    assert torch.equal(out, inter["x_inter"][-1])
    # the same through decode(quantize_denoised=True) (img2img): all four indices from x_T
    if eta == 0.0:
        s.model.calls = 0
        dec = s.decode(xT, None, 4, quantize_denoised=True)
        assert torch.equal(dec, out)


@pytest.mark.parametrize("mode", ["plain", "cfg_noise", "v"])
def test_ddim_xprev_reproduces_ddim_step(sdk, mode):
    from sd_amd import ops
    s, xT, _, shape = _ddim_setup(sdk)
    s.make_schedule(4, ddim_eta=1.0 if mode != "plain" else 0.0, verbose=False)
    sc = s.step_scalars(2)
    x, e, eu, nz = (_gpu(vu.randn(90 + i, *shape)) for i in range(4))
    kw = {}
    if mode == "cfg_noise":
        kw = dict(noise=nz, e_uncond=eu, guidance=7.5, temperature=0.9)
    elif mode == "v":
        kw = dict(noise=nz, v_param=(sc["v_sqrt_a"], sc["v_sqrt_1ma"]))
    xp, p0 = ops.ddim_step(x, e, sc, **kw)
    xp2 = ops.ddim_xprev(p0, e, sc, x=x, **kw)
    assert torch.equal(xp, xp2)
    with pytest.raises(ValueError):
        ops.ddim_xprev(p0, e[:1], sc)


def test_quantize_x0_loop_and_split_search_under_graph_capture(sdk):
    """The whole sample(quantize_x0=True) loop, and the codebook-split search (memset + atomicMin +
    second pass), captured with torch.cuda.graph and replayed: bitwise the eager result."""
    from sd_amd import ops
    s, xT, noise_fn, (b, d, h, w) = _ddim_setup(sdk)
    run = lambda: s.sample(S=4, batch_size=b, shape=(d, h, w), eta=1.0, x_T=xT, verbose=False,     # noqa: E731
                           quantize_x0=True, noise_fn=noise_fn)[0]
    eager = run().clone()
    cb, z = vu.case_data((1024, 256, 1, 4, 4))
    cbg, zg = _gpu(cb), _gpu(z)
    norms = ops.vq_code_norms(cbg)
    assert ops.lib().sdk_vq_nearest_splits(16, 1024, 256) > 1
    zq_e, idx_e = ops.vq_nearest(zg, cbg, norms)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.model.calls = 0
        run()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    s.model.calls = 0
    with torch.cuda.graph(g):
        out = run()
        zq_g, idx_g = ops.vq_nearest(zg, cbg, norms)
    out.zero_()
    idx_g.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    assert torch.equal(idx_g, idx_e) and torch.equal(zq_g, zq_e)
