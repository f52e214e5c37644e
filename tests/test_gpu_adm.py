"""GPU tests of the ADM UNet options: the FiLM GroupNorm (sdk_group_norm_film), the dual-output GroupNorm +
resample (sdk_group_norm_resample), the class-label embedding add (sdk_embedding_add), and the models built from
them against the reference's own fp32 outputs (tests/golden/make_golden_adm.py; limits in adm_util.PARITY_LIMITS,
at most 3.5x the errors measured on MI355X, profiles/adm_unet_parity_errors.txt)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import adm_util as au
import vq_util as vu
from golden_util import cfg_of, load, weights_of
from gpu_util import check_parity, rel_l2

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
EPS = 1e-5


def _gpu(a):
    return torch.from_numpy(a).to(DEV)


def _act(seed, *shape):
    """fp16 NHWC activations with an offset and a spread per channel (so GroupNorm has something to do)."""
    return _gpu(vu.randn(seed, *shape) * 1.5 + 0.5).half()


def _affine(seed, C):
    return _gpu(1.0 + 0.2 * vu.randn(seed, C)), _gpu(0.2 * vu.randn(seed + 1, C))


def _nchw(x):
    return x.float().permute(0, 3, 1, 2)


def _nhwc(x):
    return x.permute(0, 2, 3, 1)


# ------------------------------------------------------------------ (a) GroupNorm + FiLM
FILM_CASES = [((3, 7, 5, 64), None, 1), ((2, 16, 16, 640), 320, 1), ((2, 64, 64, 320), None, 1),
              ((2, 16, 16, 640), 320, 0)]


@pytest.mark.parametrize("shape,split,pad", FILM_CASES)
def test_group_norm_film(sdk, shape, split, pad):
    from sd_amd import ops
    B, H, W, C = shape
    x = _act(9000 + H + C, *shape)
    src = x if split is None else (x[..., :split].contiguous(), x[..., split:].contiguous())
    gamma, beta = _affine(9010 + C, C)
    off, ld = 24, 24 + 2 * C + 40                        # this block's columns inside a wider matrix
    film = _gpu(0.5 * vu.randn(9020 + C, B, ld))
    y = ops.group_norm_film(src, gamma, beta, EPS, film, off, silu=True, pad=pad)
    assert y.shape == (B, H + 2 * pad, W + 2 * pad, C) and y.dtype == torch.float16
    f, g = film[:, off:off + C, None, None], film[:, off + C:off + 2 * C, None, None]
    ref = _nhwc(F.silu(F.group_norm(_nchw(x), 32, gamma, beta, EPS) * (1 + f) + g))
    inner = y[:, pad:pad + H, pad:pad + W]
    e = rel_l2(inner, ref)
    print(f"[film] {shape} split {split} pad {pad}: rel-L2 {e:.3e}")
    assert e < 1e-3
    if pad:
        border = y.clone()
        border[:, pad:pad + H, pad:pad + W] = 0
        assert not bool(border.view(torch.int16).any())  # exactly (+)zero
    # a wrong column offset (scale and shift swapped, or off by C) must not pass
    wrong = _nhwc(F.silu(F.group_norm(_nchw(x), 32, gamma, beta, EPS) * (1 + g) + f))
    assert rel_l2(inner, wrong) > 1e-2
    # f = g = 0: the bits of ops.group_norm
    zero = torch.zeros(B, 2 * C, device=DEV)
    y0 = ops.group_norm_film(src, gamma, beta, EPS, zero, 0, silu=True, pad=pad)
    assert torch.equal(y0.view(torch.int16), ops.group_norm(src, gamma, beta, EPS, silu=True, pad=pad).view(torch.int16))


def test_group_norm_film_rejects_a_short_film_matrix(sdk):
    from sd_amd import ops
    x = _act(9100, 1, 4, 4, 64)
    gamma, beta = _affine(9101, 64)
    with pytest.raises(ValueError, match="film"):
        ops.group_norm_film(x, gamma, beta, EPS, torch.zeros(1, 130, device=DEV), 8)


# ------------------------------------------------------------------ (b) GroupNorm + SiLU + resample, two outputs
RS_SHAPES = [(2, 6, 10, 32), (1, 5, 7, 64), (2, 32, 32, 320)]


def _ulp_distance(a, b):
    """fp16 values as ordered integers: |difference| in units in the last place."""
    def order(t):
        i = t.contiguous().view(torch.int16).int()
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (order(a) - order(b)).abs().max().item()


def _resample_ref(t, mode):
    return F.avg_pool2d(t, 2) if mode == "down" else F.interpolate(t, scale_factor=2, mode="nearest")


@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("shape", RS_SHAPES)
@pytest.mark.parametrize("mode", ["down", "up"])
def test_group_norm_resample(sdk, mode, shape, pad):
    from sd_amd import ops
    B, H, W, C = shape
    x = _act(9200 + H + C, *shape)
    gamma, beta = _affine(9210 + C, C)
    gn = ops.group_norm_affine(x, gamma, beta, EPS)
    ya, yr = ops.group_norm_resample(x, gn, mode, silu=True, pad=pad)
    Ho, Wo = (H // 2, W // 2) if mode == "down" else (2 * H, 2 * W)
    assert ya.shape == (B, Ho + 2 * pad, Wo + 2 * pad, C) and yr.shape == (B, Ho, Wo, C)
    act = F.silu(_nchw(x) * gn[0][:, :, None, None] + gn[1][:, :, None, None])
    e = rel_l2(ya[:, pad:pad + Ho, pad:pad + Wo], _nhwc(_resample_ref(act, mode)))
    print(f"[resample] {mode} {shape} pad {pad}: activated rel-L2 {e:.3e}")
    assert e < 1e-3
    if pad:
        border = ya.clone()
        border[:, pad:pad + Ho, pad:pad + Wo] = 0
        assert not bool(border.view(torch.int16).any())
    if mode == "up":
        ref = _nhwc(F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="nearest")).contiguous()
        assert torch.equal(yr.view(torch.int16), ref.view(torch.int16))
    else:
        ref = _nhwc(F.avg_pool2d(_nchw(x), 2).half())
        d = _ulp_distance(yr, ref)
        print(f"[resample] down {shape}: raw ulp distance {d}")
        assert d <= 1
    # the NULL-output and NULL-affine forms give the same bits
    only_a, none_r = ops.group_norm_resample(x, gn, mode, silu=True, pad=pad, raw=False)
    none_a, only_r = ops.group_norm_resample(x, gn, mode, silu=True, pad=pad, act=False)
    none_a2, raw2 = ops.group_norm_resample(x, None, mode)
    assert none_r is None and none_a is None and none_a2 is None
    assert torch.equal(only_a.view(torch.int16), ya.view(torch.int16))
    assert torch.equal(only_r.view(torch.int16), yr.view(torch.int16))
    assert torch.equal(raw2.view(torch.int16), yr.view(torch.int16))


@pytest.mark.parametrize("mode", ["down", "up"])
def test_group_norm_resample_reads_a_two_source_concat(sdk, mode):
    from sd_amd import ops
    x = _act(9300, 2, 6, 10, 96)
    gamma, beta = _affine(9301, 96)
    src = (x[..., :64].contiguous(), x[..., 64:].contiguous())
    gn = ops.group_norm_affine(src, gamma, beta, EPS)
    one = ops.group_norm_resample(x, gn, mode, pad=1)
    two = ops.group_norm_resample(src, gn, mode, pad=1)
    for a, b in zip(one, two):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_group_norm_resample_rejects_channels_not_a_multiple_of_8(sdk):
    from sd_amd import _lib
    x = torch.zeros(1, 4, 4, 12, dtype=torch.float16, device=DEV)
    out = torch.zeros(1, 8, 8, 12, dtype=torch.float16, device=DEV)
    a = _lib.GroupNormArgs()
    a.src0, a.ld0, a.c_split, a.batch, a.hw, a.channels = x.data_ptr(), 12, 12, 1, 16, 12
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for mode in (_lib.RESAMPLE_AVGPOOL2, _lib.RESAMPLE_NEAREST2):
        rc = _lib.lib().sdk_group_norm_resample(ctypes.byref(a), mode, 1, 4, 4, 0, None,
                                                ctypes.c_void_p(out.data_ptr()), stream)
        assert rc == -1                                  # SDK_EINVAL
    torch.cuda.synchronize()
    assert not bool(out.any())                           # nothing was launched


# ------------------------------------------------------------------ (c) class-label embedding add
def test_embedding_add_bits_and_out_of_range_rows(sdk):
    from sd_amd import ops
    B, D, n = 5, 128, 10
    emb = _gpu(vu.randn(9400, B, D)).half()
    store = _gpu(vu.randn(9401, n + 6, D))               # spare rows: a wrong index reads stale data, not out of bounds
    store[n:] = 1000.0
    table = store[:n]
    ids = torch.tensor([3, 9, 0, 7, 3], device=DEV)
    out = ops.embedding_add(emb, table, ids)
    ref = (emb.float() + table[ids]).half()
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))
    bad = torch.tensor([3, n, 0, -1, 9], device=DEV)
    out = ops.embedding_add(emb, table, bad)
    assert bool(torch.isnan(out[1]).all()) and bool(torch.isnan(out[3]).all())
    good = [0, 2, 4]
    assert torch.equal(out[good].view(torch.int16), (emb[good].float() + table[bad[good]]).half().view(torch.int16))


# ------------------------------------------------------------------ models
def _model(sdk, name):
    from sd_amd.openai_model.model import UNetModel
    z = load(name)
    assert cfg_of(z) == au.FIXTURES[name][0]
    m = UNetModel(**cfg_of(z))
    m.load_state_dict(weights_of(z))
    return m.to(DEV), z


def _inputs(shape=(2, 4, 16, 16)):
    return {k: _gpu(v) for k, v in au.inputs(shape).items()}


def _wrapper(sdk, unet):
    from sd_amd.Diffusion.ddpm import DiffusionWrapper
    dw = DiffusionWrapper.__new__(DiffusionWrapper)
    torch.nn.Module.__init__(dw)
    dw.diffusion_model, dw.conditioning_key, dw._graphed, dw._graphs_on = unet, "adm", None, False
    return dw


@pytest.mark.parametrize("key,shape,tag", [("y", (2, 4, 16, 16), "ADM_FULL vs reference"),
                                           ("y_wide", au.WIDE, "ADM_FULL 8x24 vs reference")])
def test_adm_full_vs_reference(sdk, key, shape, tag):
    m, z = _model(sdk, "unet_tiny_adm_full")
    d = _inputs(shape)
    y = m(d["x"], d["t"], context=d["ctx"], y=d["y"])
    assert y.shape == shape and y.dtype == torch.float32
    check_parity(tag, y, torch.from_numpy(z[key]), *au.PARITY_LIMITS[tag])
    # the labels matter, and a host y gives the same bits as a device y
    assert not torch.equal(y, m(d["x"], d["t"], context=d["ctx"], y=(d["y"] + 1) % 10))
    assert torch.equal(y, m(d["x"], d["t"], context=d["ctx"], y=d["y"].cpu()))


def test_adm_pool_vs_reference(sdk):
    m, z = _model(sdk, "unet_tiny_adm_pool")
    d = _inputs()
    tag = "ADM_POOL vs reference"
    check_parity(tag, m(d["x"], d["t"]), torch.from_numpy(z["y"]), *au.PARITY_LIMITS[tag])


def test_adm_film_only_vs_reference(sdk):
    m, z = _model(sdk, "unet_tiny_adm_film")
    d = _inputs()
    tag = "ADM_FILM_ONLY vs reference"
    check_parity(tag, m(d["x"], d["t"], context=d["ctx"]), torch.from_numpy(z["y"]), *au.PARITY_LIMITS[tag])


def test_adm_wrapper_vs_reference(sdk):
    m, z = _model(sdk, "unet_tiny_adm_wrap")
    d = _inputs()
    tag = "adm wrapper vs reference"
    y = _wrapper(sdk, m)(d["x"], d["t"], c_crossattn=[d["y"]])
    check_parity(tag, y, torch.from_numpy(z["y"]), *au.PARITY_LIMITS[tag])


def test_device_label_out_of_range_gives_nan_rows_not_a_fault(sdk):
    m, _ = _model(sdk, "unet_tiny_adm_wrap")
    d = _inputs()
    y = m(d["x"], d["t"], y=torch.tensor([3, 10], device=DEV))
    assert bool(torch.isfinite(y[0]).all()) and bool(torch.isnan(y[1]).all())


def test_adm_graph_replay_equals_eager_with_new_x_t_and_y(sdk):
    from sd_amd.graphs import GraphedUNet
    m, _ = _model(sdk, "unet_tiny_adm_full")
    d = _inputs()
    calls = [(d["x"], d["t"], d["y"]),
             (d["x"] * 0.5 + 0.25, torch.tensor([500, 37], device=DEV), torch.tensor([0, 6], device=DEV))]
    eager = [m(x, t, context=d["ctx"], y=y).clone() for x, t, y in calls]
    assert not torch.equal(eager[0], eager[1])
    g = GraphedUNet(m)
    for rnd in range(2):                                 # the second round replays only
        for (x, t, y), ref in zip(calls, eager):
            assert torch.equal(g(x, t, d["ctx"], y=y), ref), f"round {rnd}"
    assert len(g.graphs) == 1
    # through the wrapper: use_graphs() on an adm model
    mw, _ = _model(sdk, "unet_tiny_adm_wrap")
    dw = _wrapper(sdk, mw)
    ref = [dw(x, t, c_crossattn=[y]).clone() for x, t, y in calls]
    dw.use_graphs(True)
    for x, t, y in calls + calls:
        assert torch.equal(dw(x, t, c_crossattn=[y]), ref[0] if y is calls[0][2] else ref[1])
    assert len(dw._graphed.graphs) == 1


def test_ddim_sample_with_label_conditioning_and_cfg(sdk):
    """DDIMSampler with classifier-free guidance over class labels (unconditional_conditioning = another
    label tensor): finite, right shape, and equal to a hand-rolled loop over the model."""
    from sd_amd import ops
    from sd_amd.DDIM.ddim import DDIMSampler
    from sd_amd.Diffusion.ddpm import LatentDiffusion
    m, _ = _model(sdk, "unet_tiny_adm_wrap")

    class LD(LatentDiffusion):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.parameterization, self.v_posterior = "eps", 0.
            self.model = _wrapper(sdk, m)
            self.register_schedule(beta_schedule="linear", timesteps=1000, linear_start=0.00085, linear_end=0.012)

    ld = LD().to(DEV)
    xT = _gpu(vu.randn(9500, 2, 4, 16, 16))
    c, uc = torch.tensor([3, 9], device=DEV), torch.tensor([0, 0], device=DEV)
    s = DDIMSampler(ld)
    scale = 3.0
    out, _ = s.sample(S=4, batch_size=2, shape=(4, 16, 16), conditioning=c, eta=0.0, x_T=xT, verbose=False,
                      unconditional_guidance_scale=scale, unconditional_conditioning=uc)
    assert out.shape == xT.shape and bool(torch.isfinite(out).all()) and not torch.equal(out, xT)
    x = xT
    for index in range(3, -1, -1):
        ts = torch.full((4,), int(s.ddim_timesteps[index]), device=DEV, dtype=torch.long)
        both = m(torch.cat([x] * 2), ts, y=torch.cat([uc, c])).float()
        x, _ = ops.ddim_step(x, both[2:].contiguous(), s.step_scalars(index), e_uncond=both[:2].contiguous(),
                             guidance=scale)
    assert torch.equal(out, x)
