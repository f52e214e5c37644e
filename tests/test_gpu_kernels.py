"""HIP kernel parity on the MI355X (run with -m gpu).

Each kernel is called through the C ABI (sd_amd.ops → libsdk_amd.so) and compared
with an fp32 CPU computation of the same op on the same (fp16-rounded) inputs.
Tolerances: fp16 storage with fp32 accumulation → rel-L2 ≤ 2e-3 per op (stated
per test); the DDIM update is bit-exact against the oracle."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_util import rel_l2, max_rel

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops(sdk):
    from sd_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return o


def _rand(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half()


def _conv_ref(x_nhwc, w, b, stride=1, pad=1, upsample=False, gn=None, silu=False):
    x = x_nhwc.float().permute(0, 3, 1, 2)
    if gn is not None:
        sc, sh = gn
        x = x * sc[:, :, None, None] + sh[:, :, None, None]
        x = x.half().float()
    if silu:
        x = F.silu(x).half().float()
    if upsample:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    return F.conv2d(x, w.float(), None if b is None else b.float(), stride=stride, padding=pad).permute(0, 2, 3, 1)


@pytest.fixture(params=["auto", "0", "2", "3", "4", "6", "7", "8", "9", "16", "17", "18", "19", "20", "21",
                        "22", "23", "24", "25", "26", "31", "32", "33", "38", "40"])
def conv_variant(request, sdk):
    """Every conv kernel variant (register-staged 128x128, LDS-DMA 256x256/256x128/128x128)."""
    from sd_amd import ops as o
    old = o.FORCE_VARIANT
    if request.param != "auto":
        o.FORCE_VARIANT = int(request.param)
    yield request.param
    o.FORCE_VARIANT = old


@pytest.mark.parametrize("B,H,W,Cin,Cout,k,stride,up", [
    (2, 16, 16, 64, 128, 3, 1, False),
    (2, 16, 16, 320, 320, 3, 1, False),
    (1, 8, 8, 640, 1280, 3, 1, False),        # split-K path
    (2, 16, 16, 64, 64, 3, 2, False),         # Downsample
    (2, 8, 8, 128, 64, 3, 1, True),           # Upsample folded into the load
    (3, 10, 6, 96, 40, 1, 1, False),          # ragged M, N not a multiple of 128
    (2, 8, 8, 8, 320, 3, 1, False),           # conv_in (8 padded channels)
])
def test_conv(ops, conv_variant, B, H, W, Cin, Cout, k, stride, up):
    x = _rand(B, H, W, Cin, seed=1)
    w = torch.randn(Cout, Cin, k, k) / math.sqrt(Cin * k * k)
    b = torch.randn(Cout) * 0.1
    pc = ops.PackedConv([(w, Cin)], b, device=DEV)
    y = ops.conv2d(pc, x.to(DEV), stride=stride, pad=k // 2, upsample=up)
    ref = _conv_ref(x, w.half(), b, stride=stride, pad=k // 2, upsample=up)
    assert y.shape == ref.shape
    assert rel_l2(y, ref) < 2e-3


def test_conv_gn_silu_concat_fused_skip_rowbias(ops, conv_variant):
    """ResBlock conv2 shape: GN+SiLU prologue over a 2-source concat is tested via conv1,
    the fused 1x1 shortcut segment and the per-(batch, channel) embedding add via conv2."""
    B, H, W, C1, C2, Co = 2, 8, 8, 64, 32, 64
    a, b2 = _rand(B, H, W, C1, seed=2), _rand(B, H, W, C2, seed=3)
    xcat = torch.cat([a, b2], -1)
    gamma, beta = torch.rand(C1 + C2) + 0.5, torch.randn(C1 + C2) * 0.1
    sc, sh = ops.group_norm_affine((a.to(DEV), b2.to(DEV)), gamma.to(DEV), beta.to(DEV), 1e-5)
    xr = xcat.float().permute(0, 3, 1, 2)
    ref_n = F.group_norm(xr, 32, gamma, beta, 1e-5)
    got_n = xr * sc.cpu()[:, :, None, None] + sh.cpu()[:, :, None, None]
    assert rel_l2(got_n, ref_n) < 1e-5
    w1 = torch.randn(Co, C1 + C2, 3, 3) / math.sqrt((C1 + C2) * 9)
    b1 = torch.randn(Co) * 0.1
    emb = torch.randn(B, 200).float()
    pc1 = ops.PackedConv([(w1, C1 + C2)], b1, device=DEV)
    plan = {}
    y1 = ops.conv2d(pc1, (a.to(DEV), b2.to(DEV)), gn=(sc, sh), silu=True, row_bias=(emb.to(DEV), 17), plan_out=plan)
    assert plan["variant"] == 0       # a GN+SiLU prologue: the register-staged kernel, whatever was forced
    ref1 = _conv_ref(xcat, w1.half(), b1, gn=(sc.cpu(), sh.cpu()), silu=True) + emb[:, None, None, 17:17 + Co]
    assert rel_l2(y1, ref1) < 3e-3
    # conv2 with fused 1x1 shortcut over the concat input
    w2 = torch.randn(Co, Co, 3, 3) / math.sqrt(Co * 9)
    ws = torch.randn(Co, C1 + C2, 1, 1) / math.sqrt(C1 + C2)
    bb = torch.randn(Co) * 0.1
    pc2 = ops.PackedConv([(w2, Co), (ws, C1 + C2)], bb, device=DEV)
    y2 = ops.conv2d(pc2, y1, seg2=((a.to(DEV), b2.to(DEV)), None, False))
    ref2 = _conv_ref(y1.cpu(), w2.half(), bb) + _conv_ref(xcat, ws.half(), None, pad=0)
    assert rel_l2(y2, ref2) < 3e-3


def test_linear_residual_geglu_rows_f32(ops, conv_variant):
    M, K, N = 300, 320, 640
    x = _rand(M, K, seed=4)
    w = torch.randn(N, K) / math.sqrt(K)
    b = torch.randn(N) * 0.1
    r = _rand(M, N, seed=5)
    pc = ops.PackedConv([(w, K)], b, device=DEV)
    y = ops.linear(pc, x.to(DEV), residual=r.to(DEV))
    ref = (x.float() @ w.half().float().T + b).half().float() + r.float()
    assert rel_l2(y, ref) < 2e-3
    # GEGLU epilogue: x * gelu(gate) with proj width 2*inner
    inner = 160
    wg = torch.randn(2 * inner, K) / math.sqrt(K)
    bg = torch.randn(2 * inner) * 0.1
    pcg = ops.PackedConv([(wg, K)], bg, geglu=True, device=DEV)
    yg = ops.linear(pcg, x.to(DEV), out_mode=ops.OUT_GEGLU_F16)
    hp = x.float() @ wg.half().float().T + bg
    refg = hp[:, :inner] * F.gelu(hp[:, inner:])
    assert yg.shape == (M, inner)
    assert rel_l2(yg, refg) < 3e-3
    # fp32 rows + A-side SiLU (timestep-embedding projections)
    plan = {}
    y32 = ops.linear(pc, x.to(DEV), silu=True, out_mode=ops.OUT_ROWS_F32, plan_out=plan)
    assert plan["variant"] == 0       # an A-side SiLU: the register-staged kernel, whatever was forced
    ref32 = F.silu(x.float()).half().float() @ w.half().float().T + b
    assert y32.dtype == torch.float32 and rel_l2(y32, ref32) < 2e-3


@pytest.mark.parametrize("M,K,N,split", [(154, 768, 3072, None), (154, 3072, 768, None), (1024, 1280, 1280, 4)])
def test_linear_quick_gelu_act(ops, conv_variant, M, K, N, split):
    """Epilogue activation (CLIP fc1 quick_gelu) after bias, before the residual — every tile
    config, the split-K reduce and the fp32 row output."""
    x = _rand(M, K, seed=41)
    w = torch.randn(N, K) / math.sqrt(K)
    b = torch.randn(N) * 0.1
    r = _rand(M, N, seed=42)
    pc = ops.PackedConv([(w, K)], b, device=DEV)
    h = x.float() @ w.half().float().T + b
    qg = h * torch.sigmoid(1.702 * h)
    x4 = x.to(DEV).view(1, M, 1, K)
    plan = {}
    y = ops.conv2d(pc, x4, ksize=1, pad=0, act=ops.ACT_QUICK_GELU, residual=r.to(DEV).view(1, M, 1, N),
                   split_k=split, plan_out=plan).view(M, N)
    assert plan["variant"] == 0       # an epilogue act: the register-staged kernel, whatever was forced
    assert rel_l2(y, qg.half().float() + r.float()) < 3e-3
    y32 = ops.linear(pc, x.to(DEV), act=ops.ACT_QUICK_GELU, out_mode=ops.OUT_ROWS_F32, plan_out=plan)
    assert plan["variant"] == 0
    assert rel_l2(y32, qg) < 2e-3


def test_conv_nchw_f32_out(ops, conv_variant):
    B, H, W, Cin, Cout = 2, 16, 16, 64, 4
    x = _rand(B, H, W, Cin, seed=6)
    w = torch.randn(Cout, Cin, 3, 3) / math.sqrt(Cin * 9)
    b = torch.randn(Cout) * 0.1
    pc = ops.PackedConv([(w, Cin)], b, device=DEV)
    y = ops.conv2d(pc, x.to(DEV), out_mode=ops.OUT_NCHW_F32)
    ref = _conv_ref(x, w.half(), b).permute(0, 3, 1, 2)
    assert y.shape == (B, Cout, H, W) and y.dtype == torch.float32
    assert rel_l2(y, ref) < 2e-3


@pytest.mark.parametrize("C,HW", [(320, 4096), (2560, 64), (128, 16384), (960, 256), (640, 1024), (1280, 256),
                                  (1920, 256), (320, 1024), (64, 100)])
def test_group_norm_stats(ops, C, HW):
    B = 2
    x = (_rand(B, HW, 1, C, seed=7).float() * 2 + 3).half()       # offset activations
    gamma, beta = torch.rand(C) + 0.5, torch.randn(C) * 0.1
    sc, sh = ops.group_norm_affine(x.to(DEV), gamma.to(DEV), beta.to(DEV), 1e-6)
    xr = x.float().permute(0, 3, 1, 2)
    ref = F.group_norm(xr, 32, gamma, beta, 1e-6)
    got = xr * sc.cpu()[:, :, None, None] + sh.cpu()[:, :, None, None]
    assert rel_l2(got, ref) < 1e-5


@pytest.mark.parametrize("C", [320, 640, 1280, 1024])
def test_layer_norm(ops, C):
    M = 777
    x = _rand(M, C, seed=8)
    g, b = torch.rand(C) + 0.5, torch.randn(C) * 0.1
    y = ops.layer_norm(x.to(DEV), g.to(DEV), b.to(DEV), 1e-5)
    ref = F.layer_norm(x.float(), (C,), g, b, 1e-5)
    assert rel_l2(y, ref) < 1e-3


@pytest.mark.parametrize("M,C,offset", [(70001, 320, 0.0), (9000, 768, 30.0), (8193, 2048, -12.0), (5, 64, 100.0)])
def test_layer_norm_rows_walk_and_offset_mean(ops, M, C, offset):
    """More rows than resident waves (each wave walks rows with the next row prefetched), CLIP's
    768, the 2048 maximum, and rows whose mean is far from 0 relative to their spread (the pivot
    keeps the one-pass variance from cancelling)."""
    g0 = torch.Generator().manual_seed(M + C)
    x = (torch.randn(M, C, generator=g0) + offset).half()
    g, b = torch.rand(C, generator=g0) + 0.5, torch.randn(C, generator=g0) * 0.1
    y = ops.layer_norm(x.to(DEV), g.to(DEV), b.to(DEV), 1e-5)
    ref = F.layer_norm(x.float(), (C,), g, b, 1e-5)
    assert rel_l2(y, ref) < 1e-3


@pytest.mark.parametrize("B,H,nq,nk,d", [
    (2, 8, 300, 300, 40), (1, 8, 256, 77, 80), (1, 8, 64, 64, 160), (2, 5, 200, 77, 64),
    (1, 2, 100, 100, 8), (1, 4, 130, 1024, 16), (1, 8, 4096, 4096, 40),
    # d = 40's pipelined loop: one ragged tile, exactly one / two / three whole tiles, a ragged third
    (1, 8, 100, 20, 40), (1, 4, 70, 64, 40), (1, 4, 200, 128, 40), (2, 4, 70, 192, 40), (1, 4, 257, 150, 40),
])
def test_attention(ops, B, H, nq, nk, d):
    from oracle.unet_ref import attention_core
    q = _rand(B, nq, H, d, seed=9)
    k = _rand(B, nk, H, d, seed=10)
    v = _rand(B, nk, H, d, seed=11)
    s = d ** -0.5
    o = ops.attention(q.view(B * nq, H * d).to(DEV), k.view(B * nk, H * d).to(DEV), v.view(B * nk, H * d).to(DEV),
                      batch=B, heads=H, nq=nq, nk=nk, head_dim=d, scale=s)
    ref = attention_core(q.float(), k.float(), v.float(), s).reshape(B * nq, H * d)
    assert rel_l2(o, ref) < 3e-3


@pytest.mark.parametrize("B,H,n,nk,d,packed", [
    (2, 8, 333, 333, 40, "qkv"), (2, 8, 256, 77, 40, "kv"), (1, 8, 1024, 1024, 80, "qkv"), (1, 5, 100, 77, 64, "kv"),
    (1, 8, 64, 64, 160, "qkv"), (1, 8, 40, 77, 160, "kv"),
])
def test_attention_strided_packed(ops, B, H, n, nk, d, packed):
    """The model's layouts: q|k|v column slices of one projection output (self-attention,
    row stride 3*H*d), or a k|v pair from the cached context projection (cross-attention)."""
    from oracle.unet_ref import attention_core
    C = H * d
    if packed == "qkv":
        qkv = _rand(B * n, 3 * C, seed=21).to(DEV)
        q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    else:
        q = _rand(B * n, C, seed=22).to(DEV)
        kv = _rand(B * nk, 2 * C, seed=23).to(DEV)
        k, v = kv[:, :C], kv[:, C:]
    o = ops.attention(q, k, v, batch=B, heads=H, nq=n, nk=nk, head_dim=d, scale=d ** -0.5)
    ref = attention_core(q.cpu().float().contiguous().view(B, n, H, d), k.cpu().float().contiguous().view(B, nk, H, d),
                         v.cpu().float().contiguous().view(B, nk, H, d), d ** -0.5).reshape(B * n, C)
    assert rel_l2(o, ref) < 3e-3


@pytest.mark.parametrize("B,H,n,d", [(2, 12, 77, 64), (1, 2, 77, 64), (1, 4, 300, 64), (2, 8, 129, 40),
                                      (1, 2, 520, 80)])
def test_attention_causal(ops, B, H, n, d):
    """Causal self-attention (CLIP text tower): key j masked for query i when j > i; diagonal
    tiles masked per element, tiles past a workgroup's last query skipped."""
    q = _rand(B, n, H, d, seed=51)
    k = _rand(B, n, H, d, seed=52)
    v = _rand(B, n, H, d, seed=53)
    s = d ** -0.5
    o = ops.attention(q.view(B * n, H * d).to(DEV), k.view(B * n, H * d).to(DEV), v.view(B * n, H * d).to(DEV),
                      batch=B, heads=H, nq=n, nk=n, head_dim=d, scale=s, causal=True)
    qf, kf, vf = (t.float().transpose(1, 2) for t in (q, k, v))
    att = (qf @ kf.transpose(-1, -2)) * s + torch.full((n, n), float("-inf")).triu(1)
    ref = (att.softmax(-1) @ vf).transpose(1, 2).reshape(B * n, H * d)
    assert rel_l2(o, ref) < 3e-3


@pytest.mark.parametrize("d", [64, 40])
def test_attention_large_logits_rescale(ops, d):
    """Force the online-softmax max to jump in a late key tile (rule: test the rescale branch)."""
    from oracle.unet_ref import attention_core
    B, H, n = 1, 2, 256
    q = _rand(B, n, H, d, seed=12)
    k = _rand(B, n, H, d, seed=13)
    k[:, 200] = q[:, 5] * 4           # spike: row 5's max arrives in tile 3
    v = _rand(B, n, H, d, seed=14)
    o = ops.attention(q.view(B * n, H * d).to(DEV), k.view(B * n, H * d).to(DEV), v.view(B * n, H * d).to(DEV),
                      batch=B, heads=H, nq=n, nk=n, head_dim=d, scale=d ** -0.5)
    ref = attention_core(q.float(), k.float(), v.float(), d ** -0.5).reshape(B * n, H * d)
    assert rel_l2(o, ref) < 3e-3


@pytest.mark.parametrize("eta", [0, 1])
@pytest.mark.parametrize("index", [0, 1, 25, 49])
def test_ddim_step_bitexact(ops, eta, index):
    from golden_util import load
    from oracle import schedule as sch
    z = load("ddim_step")
    tab = sch.ddim_tables(50, float(eta))
    sc = sch.ddim_step_scalars(tab, index)
    x, e, nz = (torch.from_numpy(z[k]).to(DEV) for k in ("x", "e", "noise"))
    xp, p0 = ops.ddim_step(x, e, sc, noise=nz if eta else None)
    assert np.array_equal(xp.cpu().numpy(), z[f"eta{eta}_i{index}_xprev"])
    assert np.array_equal(p0.cpu().numpy(), z[f"eta{eta}_i{index}_pred_x0"])


def test_timestep_embedding(ops):
    from golden_util import load
    from sd_amd.openai_model.utils import timestep_frequencies
    z = load("schedule")
    t = torch.from_numpy(z["temb_t"]).to(DEV)
    e = ops.timestep_embedding(t, timestep_frequencies(320).to(DEV), 320)
    ref = torch.from_numpy(z["temb_320"]).half().float()
    assert (e.float().cpu() - ref).abs().max().item() <= 2e-3


def test_nchw_to_nhwc(ops):
    x = torch.randn(3, 4, 17, 9)
    y = ops.nchw_to_nhwc(x.to(DEV), 8, scale=0.5)
    ref = torch.zeros(3, 17, 9, 8)
    ref[..., :4] = (x * 0.5).permute(0, 2, 3, 1)
    assert torch.equal(y.cpu(), ref.half())


@pytest.mark.parametrize("H,W,C,pad", [(64, 64, 320, 1), (9, 7, 64, 1), (16, 16, 1280, 2)])
def test_group_norm_apply_padded(ops, H, W, C, pad):
    """Zero-bordered GN+SiLU output == F.pad of the unpadded output; a pad-0 3x3 conv over it ==
    the pad-1 conv over the unpadded output (the ResBlock fast path)."""
    x = _rand(2, H, W, C, seed=61).to(DEV)
    g = torch.rand(C, device=DEV) + 0.5
    b = torch.randn(C, device=DEV) * 0.1
    st = ops.group_norm_affine(x, g, b, 1e-5)
    y0 = ops.group_norm_apply(x, st, silu=True)
    yp = ops.group_norm_apply(x, st, silu=True, pad=pad)
    assert yp.shape == (2, H + 2 * pad, W + 2 * pad, C)
    ref = F.pad(y0.permute(0, 3, 1, 2), (pad, pad, pad, pad)).permute(0, 2, 3, 1)
    assert torch.equal(yp, ref)
    if pad == 1:
        w = torch.randn(C, C, 3, 3) / math.sqrt(9 * C)
        pc = ops.PackedConv([(w, C)], torch.zeros(C), device=DEV)
        assert torch.equal(ops.conv2d(pc, yp, pad=0, variant=0), ops.conv2d(pc, y0, pad=1, variant=0)) or \
            rel_l2(ops.conv2d(pc, yp, pad=0), ops.conv2d(pc, y0, pad=1)) < 1e-3


@pytest.mark.parametrize("silu", [True, False])
def test_group_norm_apply_concat(ops, silu):
    B, H, W, C1, C2 = 2, 16, 16, 640, 320
    a, b2 = _rand(B, H, W, C1, seed=15), _rand(B, H, W, C2, seed=16)
    gamma, beta = torch.rand(C1 + C2) + 0.5, torch.randn(C1 + C2) * 0.1
    src = (a.to(DEV), b2.to(DEV))
    gn = ops.group_norm_affine(src, gamma.to(DEV), beta.to(DEV), 1e-5)
    y = ops.group_norm_apply(src, gn, silu=silu)
    xr = torch.cat([a, b2], -1).float().permute(0, 3, 1, 2)
    ref = F.group_norm(xr, 32, gamma, beta, 1e-5)
    if silu:
        ref = F.silu(ref)
    assert y.shape == (B, H, W, C1 + C2)
    assert rel_l2(y, ref.permute(0, 2, 3, 1)) < 1e-3


GLDS_VARIANTS = {2, 3, 4, 6, 7, 16, 17, 18, 19, 22, 23, 24, 25, 26, 31, 32, 33, 38, 40}


def _chunk_stats(y, nch):
    """(mean, M2) per (image, chunk of hw/nch pixels, channel) of an NHWC tensor, in float64."""
    B, H, W, C = y.shape
    t = y.double().reshape(B, nch, H * W // nch, C)
    mean = t.mean(2)
    return mean, ((t - mean[:, :, None]) ** 2).sum(2)


@pytest.mark.parametrize("H,W,Ci,Co,split", [(16, 16, 128, 320, None), (8, 8, 640, 1280, 4), (32, 32, 64, 640, None)])
def test_conv_emits_group_norm_statistics(ops, conv_variant, H, W, Ci, Co, split):
    """The producing conv's epilogue (or its split-K reduce) emits per-chunk channel (mean, M2) of
    the fp16 values it stores (bias, embedding row and residual included, offset channels);
    group_norm merges them instead of a statistics pass: same result as the pass."""
    B = 2
    x = _rand(B, H, W, Ci, seed=H + Ci)
    g = torch.Generator(device="cpu").manual_seed(Co + H)
    w = torch.randn(Co, Ci, 3, 3, generator=g) / math.sqrt(Ci * 9)
    b = torch.randn(Co, generator=g) * 2 + 3                     # channel means far from 0
    emb = torch.randn(B, Co + 16, generator=g)
    res = _rand(B, H, W, Co, seed=H + Co)
    pc = ops.PackedConv([(w, Ci)], b, device=DEV)
    y = ops.conv2d(pc, x.to(DEV), residual=res.to(DEV), row_bias=(emb.to(DEV), 16), split_k=split, gn_stats=True)
    ref = _conv_ref(x, w.half(), b) + emb[:, None, None, 16:] + res.float()
    assert rel_l2(y, ref) < 3e-3
    part = getattr(y, ops.GN_ATTR, None)
    forced = None if conv_variant == "auto" else int(conv_variant)
    # the phased 32x32x16 kernel (8 / 9) emits from its epilogue when its 256-row tiles stay inside one image
    if split or forced is None or forced in GLDS_VARIANTS or (forced in (8, 9) and (H * W) % 256 == 0):
        assert part is not None, "this plan should emit GroupNorm statistics"
    if part is None:
        return
    pp, nch, _ = part
    assert pp.shape == (B, nch, Co, 2) and (H * W) % nch == 0
    mean, m2 = _chunk_stats(y, nch)
    assert torch.allclose(pp[..., 0].double().cpu(), mean.cpu(), rtol=1e-5, atol=1e-4)
    assert rel_l2(pp[..., 1].double().cpu(), m2.cpu()) < 1e-4
    gamma = torch.rand(Co, generator=g).to(DEV) + 0.5
    beta = (torch.randn(Co, generator=g) * 0.1).to(DEV)
    g1 = ops.group_norm(y, gamma, beta, 1e-5, 32, silu=True, pad=1)
    g0 = ops.group_norm(y.clone(), gamma, beta, 1e-5, 32, silu=True, pad=1)    # no partials: statistics pass
    assert rel_l2(g1, g0) < 1e-3
    # modified in place after the conv: the emitted statistics are stale and must not be used
    y.mul_(2.0).add_(1.0)
    g2 = ops.group_norm(y, gamma, beta, 1e-5, 32, silu=True, pad=1)
    g3 = ops.group_norm(y.clone(), gamma, beta, 1e-5, 32, silu=True, pad=1)
    assert torch.equal(g2, g3)


def test_group_norm_concat_from_partials(ops):
    """Output-block GroupNorm over cat(h, skip): both sources carry statistics from different
    producers (different chunkings: an M-tile epilogue and a split-K reduce)."""
    B, H, W = 2, 16, 16
    g = torch.Generator(device="cpu").manual_seed(5)
    x = _rand(B, H, W, 320, seed=51).to(DEV)
    w1 = torch.randn(640, 320, 3, 3, generator=g) / math.sqrt(320 * 9)
    w2 = torch.randn(320, 320, 1, 1, generator=g) / math.sqrt(320)
    pc1 = ops.PackedConv([(w1, 320)], torch.randn(640, generator=g) + 1, device=DEV)
    pc2 = ops.PackedConv([(w2, 320)], torch.randn(320, generator=g) - 2, device=DEV)
    h = ops.conv2d(pc1, x, split_k=2, gn_stats=True)
    skip = ops.conv2d(pc2, x, split_k=1, gn_stats=True)
    assert getattr(h, ops.GN_ATTR, None) is not None and getattr(skip, ops.GN_ATTR, None) is not None
    gamma = torch.rand(960, generator=g).to(DEV) + 0.5
    beta = (torch.randn(960, generator=g) * 0.1).to(DEV)
    y1 = ops.group_norm((h, skip), gamma, beta, 1e-5, 32, silu=True, pad=1)
    y0 = ops.group_norm((h.clone(), skip.clone()), gamma, beta, 1e-5, 32, silu=True, pad=1)
    assert rel_l2(y1, y0) < 1e-3
    ref = F.silu(F.group_norm(torch.cat([h, skip], -1).float().permute(0, 3, 1, 2), 32, gamma, beta, 1e-5))
    ref = F.pad(ref, (1, 1, 1, 1)).permute(0, 2, 3, 1)
    assert rel_l2(y1, ref) < 1e-3


@pytest.mark.parametrize("H,W,C1,C2,pad,silu,offset", [
    (32, 32, 640, 0, 1, True, 3.0),        # one-launch statistics + apply (hw <= 1024), zero-bordered
    (16, 16, 640, 640, 1, True, -2.0),     # fused, 2-source concat (output block in_layers)
    (8, 8, 1280, 1280, 0, False, 0.0),     # fused, contiguous, no SiLU
    (32, 32, 960, 0, 0, True, 0.0),        # fused, 960 channels (cg = 30: 8-group slices)
    (8, 8, 2560, 0, 1, True, 10.0),        # fused, 2560 channels (cg = 80)
    (64, 64, 320, 0, 1, True, 3.0),        # hw = 4096: statistics pass, then the apply pass
    (64, 64, 320, 320, 0, True, 0.0),
    (7, 5, 64, 0, 1, True, 0.0),           # ragged image (rows not a multiple of anything)
])
def test_group_norm_end_to_end(ops, H, W, C1, C2, pad, silu, offset):
    """sdk_group_norm (statistics + apply in one call; one launch at the small levels) vs F.group_norm
    (+ SiLU) in fp32, and bitwise equal to the two-call path (affine, then apply)."""
    B = 3
    a = (_rand(B, H, W, C1, seed=H + C1).float() * 1.5 + offset).half()
    b2 = _rand(B, H, W, C2, seed=H + C2 + 1) if C2 else None
    C = C1 + C2
    g = torch.Generator(device="cpu").manual_seed(C + H)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    src = (a.to(DEV), b2.to(DEV)) if C2 else a.to(DEV)
    y = ops.group_norm(src, gamma.to(DEV), beta.to(DEV), 1e-5, 32, silu=silu, pad=pad)
    assert y.shape == (B, H + 2 * pad, W + 2 * pad, C)
    xr = (torch.cat([a, b2], -1) if C2 else a).float().permute(0, 3, 1, 2)
    ref = F.group_norm(xr, 32, gamma, beta, 1e-5)
    if silu:
        ref = F.silu(ref)
    ref = F.pad(ref, (pad, pad, pad, pad)).permute(0, 2, 3, 1)
    assert rel_l2(y, ref) < 1e-3
    if pad:
        border = torch.ones(H + 2 * pad, W + 2 * pad, dtype=torch.bool)
        border[pad:-pad, pad:-pad] = False
        assert torch.count_nonzero(y[:, border].float()) == 0
    two = ops.group_norm_apply(src, ops.group_norm_affine(src, gamma.to(DEV), beta.to(DEV), 1e-5), silu=silu,
                               pad=pad)
    assert torch.equal(y, two)


@pytest.mark.parametrize("B,N,C,D,nk", [(2, 4096, 320, 40, 77), (2, 1024, 640, 80, 77), (1, 256, 320, 64, 77),
                                        (2, 64, 640, 64, 80), (3, 192, 320, 40, 13)])
def test_cross_attention_block(ops, B, N, C, D, nk):
    """Fused to_q + attention over the cached context K|V + to_out + residual (xattn.hip) against a
    plain fp32 torch restatement (fp16 rounding of q / o / the projection output, as the separate
    launches store them) and against the three-launch path."""
    g = torch.Generator(device="cpu").manual_seed(N + C + nk)
    H = C // D
    t = torch.randn(B * N, C, generator=g).half().to(DEV)
    kv = torch.randn(B * nk, 2 * C, generator=g).half().to(DEV)
    res = torch.randn(B * N, C, generator=g).half().to(DEV)
    wq = torch.randn(C, C, generator=g) / math.sqrt(C)
    wo = torch.randn(C, C, generator=g) / math.sqrt(C)
    bo = torch.randn(C, generator=g) * 0.1
    pcq = ops.PackedConv([(wq, C)], None, device=DEV)
    pco = ops.PackedConv([(wo, C)], bo, device=DEV)
    assert ops.cross_attention_block_supported(C, D, nk, N)
    y = ops.cross_attention_block(t, kv, pcq, pco, batch=B, n_img=N, nk=nk, heads=H, head_dim=D, scale=D ** -0.5,
                                  residual=res)
    q = (t.float() @ wq.half().float().to(DEV).T).half().float().view(B, N, H, D)
    k = kv[:, :C].float().view(B, nk, H, D)
    v = kv[:, C:].float().view(B, nk, H, D)
    att = torch.softmax(torch.einsum("bnhd,bkhd->bhnk", q, k) * D ** -0.5, dim=-1)
    o = torch.einsum("bhnk,bkhd->bnhd", att, v).reshape(B * N, C).half().float()
    ref = (o @ wo.half().float().to(DEV).T + bo.to(DEV)).half().float() + res.float()
    assert rel_l2(y, ref) < 3e-3
    q3 = ops.linear(pcq, t)
    o3 = ops.attention(q3, kv[:, :C], kv[:, C:], batch=B, heads=H, nq=N, nk=nk, head_dim=D, scale=D ** -0.5)
    y3 = ops.linear(pco, o3, residual=res)
    assert rel_l2(y, y3) < 3e-3


@pytest.mark.parametrize("B,N,C,D,nk", [(2, 4096, 320, 40, 77), (2, 1024, 640, 80, 77), (3, 192, 320, 64, 13)])
def test_cross_attention_block_fused_norms(ops, B, N, C, D, nk):
    """norm2 / norm3 folded into the cross-attention kernel (sdk_cross_attention_block_ln) give the
    same bits as layer_norm -> cross_attention_block -> layer_norm, and norm3 matches torch's
    LayerNorm of the block output."""
    g = torch.Generator(device="cpu").manual_seed(7 * N + C + nk)
    H = C // D
    tok = (torch.randn(B * N, C, generator=g) * 2 + 0.5).half().to(DEV)
    kv = torch.randn(B * nk, 2 * C, generator=g).half().to(DEV)
    wq = torch.randn(C, C, generator=g) / math.sqrt(C)
    wo = torch.randn(C, C, generator=g) / math.sqrt(C)
    bo = torch.randn(C, generator=g) * 0.1
    g2, b2 = (1 + 0.1 * torch.randn(C, generator=g)).to(DEV), (0.1 * torch.randn(C, generator=g)).to(DEV)
    g3, b3 = (1 + 0.1 * torch.randn(C, generator=g)).to(DEV), (0.1 * torch.randn(C, generator=g)).to(DEV)
    pcq = ops.PackedConv([(wq, C)], None, device=DEV)
    pco = ops.PackedConv([(wo, C)], bo, device=DEV)
    kw = dict(batch=B, n_img=N, nk=nk, heads=H, head_dim=D, scale=D ** -0.5)
    t2 = ops.layer_norm(tok, g2, b2, 1e-5)
    y_sep = ops.cross_attention_block(t2, kv, pcq, pco, residual=tok, **kw)
    t3_sep = ops.layer_norm(y_sep, g3, b3, 1e-5)
    y, t3 = ops.cross_attention_block(tok, kv, pcq, pco, residual=tok, norm_in=(g2, b2, 1e-5),
                                      norm_out=(g3, b3, 1e-5), **kw)
    torch.cuda.synchronize()
    assert torch.equal(y, y_sep)
    assert torch.equal(t3, t3_sep)
    ref3 = F.layer_norm(y.float(), (C,), g3, b3, 1e-5)
    assert rel_l2(t3, ref3) < 2e-3
    # each norm alone
    y_in = ops.cross_attention_block(tok, kv, pcq, pco, residual=tok, norm_in=(g2, b2, 1e-5), **kw)
    assert torch.equal(y_in, y_sep)
    y_out, t3_out = ops.cross_attention_block(t2, kv, pcq, pco, residual=tok, norm_out=(g3, b3, 1e-5), **kw)
    assert torch.equal(y_out, y_sep) and torch.equal(t3_out, t3_sep)


@pytest.mark.parametrize("B,N,D,nk", [(2, 1024, 80, 77), (2, 64, 64, 80), (1, 192, 80, 13)])
def test_cross_attention_block_640_waves_bitwise(ops, B, N, D, nk):
    """The 640-channel block's 8-wave form (the default: two waves per SIMD) and its 4-wave form (one wave
    per SIMD) give the same bits, with and without the folded norms: per output element the K order of
    both projections and the head math are the same, only the channels per wave differ."""
    from sd_amd._lib import lib
    C = 640
    g = torch.Generator(device="cpu").manual_seed(11 * N + D + nk)
    tok = (torch.randn(B * N, C, generator=g) * 2 + 0.5).half().to(DEV)
    kv = torch.randn(B * nk, 2 * C, generator=g).half().to(DEV)
    pcq = ops.PackedConv([(torch.randn(C, C, generator=g) / math.sqrt(C), C)], None, device=DEV)
    pco = ops.PackedConv([(torch.randn(C, C, generator=g) / math.sqrt(C), C)], torch.randn(C, generator=g) * 0.1,
                         device=DEV)
    gg, bb = (1 + 0.1 * torch.randn(C, generator=g)).to(DEV), (0.1 * torch.randn(C, generator=g)).to(DEV)
    kw = dict(batch=B, n_img=N, nk=nk, heads=C // D, head_dim=D, scale=D ** -0.5, residual=tok)
    outs = {}
    try:
        for waves in (4, 8):
            assert lib().sdk_xattn_debug_waves640(waves) == 0
            y = ops.cross_attention_block(tok, kv, pcq, pco, **kw)
            yn, t3 = ops.cross_attention_block(tok, kv, pcq, pco, norm_in=(gg, bb, 1e-5), norm_out=(gg, bb, 1e-5), **kw)
            torch.cuda.synchronize()
            outs[waves] = (y, yn, t3)
    finally:
        lib().sdk_xattn_debug_waves640(8)
    for a, b in zip(outs[4], outs[8]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("B,N,C,D,nk", [(2, 4096, 320, 40, 77), (2, 1024, 640, 80, 77), (1, 256, 320, 64, 77),
                                        (2, 64, 640, 64, 80), (3, 192, 320, 40, 13)])
def test_cross_attention_block_packed_weights_bitwise(ops, B, N, C, D, nk):
    """Projection weights in the fragment-packed layout (sdk_xattn_pack_weight, w_ld = 0; the default) and in
    the row layout (w_ld = channels) give the same bits, with and without the folded norms."""
    g = torch.Generator(device="cpu").manual_seed(17 * N + C + nk)
    tok = (torch.randn(B * N, C, generator=g) * 2 + 0.5).half().to(DEV)
    kv = torch.randn(B * nk, 2 * C, generator=g).half().to(DEV)
    pcq = ops.PackedConv([(torch.randn(C, C, generator=g) / math.sqrt(C), C)], None, device=DEV)
    pco = ops.PackedConv([(torch.randn(C, C, generator=g) / math.sqrt(C), C)], torch.randn(C, generator=g) * 0.1,
                         device=DEV)
    gg, bb = (1 + 0.1 * torch.randn(C, generator=g)).to(DEV), (0.1 * torch.randn(C, generator=g)).to(DEV)
    kw = dict(batch=B, n_img=N, nk=nk, heads=C // D, head_dim=D, scale=D ** -0.5, residual=tok)
    old = ops.XATTN_PACKED_W
    outs = {}
    try:
        for packed in (False, True):
            ops.XATTN_PACKED_W = packed
            y = ops.cross_attention_block(tok, kv, pcq, pco, **kw)
            yn, t3 = ops.cross_attention_block(tok, kv, pcq, pco, norm_in=(gg, bb, 1e-5), norm_out=(gg, bb, 1e-5), **kw)
            torch.cuda.synchronize()
            outs[packed] = (y, yn, t3)
    finally:
        ops.XATTN_PACKED_W = old
    assert hasattr(pcq, "_xattn_pk") and pcq._xattn_pk.numel() == C * C
    for a_, b_ in zip(outs[False], outs[True]):
        assert torch.equal(a_, b_)


def test_xattn_pack_weight_layout_and_rejects(ops, sdk):
    """The packed layout: piece ((nb * C/32 + ks) * 64 + lane) = W[16 nb + lane % 16, 32 ks + 8 (lane // 16) : +8];
    bad shapes / strides are refused."""
    from sd_amd import _lib
    C = 320
    w = torch.randn(C, C + 8).half().to(DEV)
    pk = torch.empty(C * C, dtype=torch.float16, device=DEV)
    assert _lib.lib().sdk_xattn_pack_weight(w.data_ptr(), C + 8, pk.data_ptr(), C, None) == 0
    torch.cuda.synchronize()
    ref = w[:, :C].cpu().view(C // 16, 16, C // 32, 4, 8).permute(0, 2, 3, 1, 4).reshape(-1)
    assert torch.equal(pk.cpu(), ref)
    assert _lib.lib().sdk_xattn_pack_weight(w.data_ptr(), C + 8, pk.data_ptr(), 1280, None) != 0
    assert _lib.lib().sdk_xattn_pack_weight(w.data_ptr(), C - 8, pk.data_ptr(), C, None) != 0


def test_cross_attention_block_fused_norms_rejects(ops):
    C, D, N, nk = 320, 40, 64, 77
    t = torch.zeros(N, C, dtype=torch.float16, device=DEV)
    kv = torch.zeros(nk, 2 * C, dtype=torch.float16, device=DEV)
    pc = ops.PackedConv([(torch.zeros(C, C), C)], None, device=DEV)
    g = torch.ones(C + 1, device=DEV)
    with pytest.raises(RuntimeError, match="aligned"):
        ops.cross_attention_block(t, kv, pc, pc, batch=1, n_img=N, nk=nk, heads=8, head_dim=D, scale=0.1,
                                  norm_in=(g[1:], g[1:], 1e-5))


def test_cross_attention_block_rejects_unsupported(ops):
    assert not ops.cross_attention_block_supported(1280, 160, 77, 256)
    assert not ops.cross_attention_block_supported(320, 40, 81, 4096)
    assert not ops.cross_attention_block_supported(320, 40, 77, 100)


def test_device_calibration_probes(ops):
    """sdk_probe_*: the measured MFMA / HBM ceilings the bench reports beside the spec peaks are
    plausible for an MI355X (dense fp16 <= 2.5 PFLOP/s spec, HBM <= 8 TB/s spec)."""
    pk = ops.probe_peaks(reps=1)
    for k in ("mfma_16x16x32_f16_tflops", "mfma_32x32x16_f16_tflops"):
        assert 300.0 < pk[k] < 2600.0, pk
    assert 1000.0 < pk["hbm_copy_gbs"] < 8100.0, pk


@pytest.mark.parametrize("B,H,W,Cin,Cout,k,pad,mode", [
    (2, 16, 16, 320, 4, 3, 1, "nchw"),      # UNet conv_out (masked halo)
    (2, 18, 18, 320, 4, 3, 0, "nchw"),      # UNet conv_out on the zero-bordered GN output
    (1, 34, 66, 128, 3, 3, 0, "nchw"),      # VAE conv_out shape (ragged 8x32 patches)
    (3, 9, 40, 64, 8, 3, 1, "nhwc"),        # fp16 NHWC out, 8 outputs
    (2, 12, 12, 192, 5, 1, 0, "rows"),      # 1x1, fp32 rows
])
def test_conv_direct_small_n(ops, B, H, W, Cin, Cout, k, pad, mode):
    """Variant 34 (direct convolution for <= 8 outputs: halo tile in LDS, v_dot2_f32_f16) vs fp32
    torch; the planner picks it by itself for these shapes."""
    x = _rand(B, H, W, Cin, seed=H + Cin)
    w = torch.randn(Cout, Cin, k, k) / math.sqrt(Cin * k * k)
    b = torch.randn(Cout) * 0.1
    pc = ops.PackedConv([(w, Cin)], b, device=DEV)
    om = {"nchw": ops.OUT_NCHW_F32, "nhwc": ops.OUT_NHWC_F16, "rows": ops.OUT_ROWS_F32}[mode]
    y = ops.conv2d(pc, x.to(DEV), pad=pad, out_mode=om)
    y34 = ops.conv2d(pc, x.to(DEV), pad=pad, out_mode=om, variant=34)
    assert torch.equal(y, y34), "the planner must pick the direct variant for <= 8 outputs"
    ref = _conv_ref(x, w.half(), b, pad=pad)
    if mode == "nchw":
        ref = ref.permute(0, 3, 1, 2)
    assert y.shape == ref.shape
    assert rel_l2(y, ref) < 2e-3
    with pytest.raises(RuntimeError):                      # does not fit: a 2-source concat
        ops.conv2d(pc, (x.to(DEV)[..., :Cin // 2].contiguous(), x.to(DEV)[..., Cin // 2:].contiguous()),
                   pad=pad, out_mode=om, variant=34)


@pytest.mark.parametrize("M,K,N,silu,mode,res", [
    (16, 320, 1280, False, "nhwc", False),     # time_embed[0] at the bench batch
    (16, 1280, 1280, True, "nhwc", False),     # time_embed[2] (SiLU on the input)
    (16, 1280, 20160, True, "rows", False),    # the 22 ResBlock emb projections, fp32 rows
    (32, 1280, 2560, True, "rows", False),     # CFG-doubled batch
    (7, 200, 72, False, "nhwc", True),         # ragged M / K / N, residual
    (64, 96, 40, True, "rows", False),         # M = 64 (four row blocks)
])
def test_conv_skinny_rows(ops, M, K, N, silu, mode, res):
    """Variant 35 (skinny GEMM for <= 64 rows: 16 columns per workgroup, K split over 4 waves,
    v_mfma_f32_16x16x32_f16) vs fp32 torch; the planner picks it by itself at M <= 64."""
    x = _rand(M, K, seed=M + K)
    w = torch.randn(N, K) / math.sqrt(K)
    b = torch.randn(N) * 0.1
    pc = ops.PackedConv([(w, K)], b, device=DEV)
    om = {"nhwc": ops.OUT_NHWC_F16, "rows": ops.OUT_ROWS_F32}[mode]
    r = _rand(M, N, seed=3) if res else None
    xd = x.to(DEV)
    y = ops.linear(pc, xd, silu=silu, out_mode=om, residual=None if r is None else r.to(DEV))
    x4 = xd.view(1, M, 1, K)
    y35 = ops.conv2d(pc, x4, ksize=1, pad=0, silu=silu, out_mode=om, variant=35,
                     residual=None if r is None else r.to(DEV).view(1, M, 1, N)).view(M, N)
    assert torch.equal(y, y35), "the planner must pick the skinny variant for <= 64 rows"
    xa = x.float()
    if silu:
        xa = F.silu(xa).half().float()
    ref = xa @ w.half().float().t() + b
    if r is not None:
        ref = ref + r.float()
    assert rel_l2(y.float().cpu(), ref) < 2e-3
    if M > 8:   # the tiled kernels give the same numbers within fp32 summation order
        yt = ops.conv2d(pc, x4, ksize=1, pad=0, silu=silu, out_mode=om, variant=0,
                        residual=None if r is None else r.to(DEV).view(1, M, 1, N)).view(M, N)
        assert rel_l2(y.float(), yt.float()) < 2e-3
    with pytest.raises(RuntimeError):                      # does not fit: 65 rows
        ops.conv2d(pc, _rand(1, 65, 1, K).to(DEV), ksize=1, pad=0, out_mode=om, variant=35)


def test_conv_batch_chunks_over_the_buffer_range(ops, monkeypatch):
    """Sources of >= 2 GiB (the VAE decoder's 256-channel 512x512 maps at B=16) run as batch chunks
    under the LDS-DMA kernels' 31-bit buffer range instead of falling back to the register-staged
    kernel.  Forced here on a small problem by lowering ops.BUF_LIMIT: concat source + fused 1x1
    segment + row bias + residual + GroupNorm statistics, vs the unchunked call."""
    B, H, W = 4, 12, 12
    g = torch.Generator(device="cpu").manual_seed(11)
    xa, xb = _rand(B, H, W, 64, seed=1).to(DEV), _rand(B, H, W, 64, seed=2).to(DEV)
    x2 = _rand(B, H, W, 64, seed=3).to(DEV)
    w1 = torch.randn(192, 128, 3, 3, generator=g) / math.sqrt(128 * 9)
    w2 = torch.randn(192, 64, 1, 1, generator=g) / 8.0
    pc = ops.PackedConv([(w1, 128), (w2, 64)], torch.randn(192, generator=g), device=DEV)
    emb = torch.randn(B, 200, generator=g).to(DEV)
    res = _rand(B, H, W, 192, seed=4).to(DEV)
    kw = dict(seg2=(x2, None, False), row_bias=(emb, 8), residual=res, gn_stats=True)
    ref = ops.conv2d(pc, (xa, xb), **kw)
    monkeypatch.setattr(ops, "BUF_LIMIT", B * H * W * 64 * 2 // 2 + 1)   # two chunks of 2 images
    y = ops.conv2d(pc, (xa, xb), **kw)
    assert y.shape == ref.shape
    assert rel_l2(y, ref) < 1e-3
    p_ref, p_y = getattr(ref, ops.GN_ATTR, None), getattr(y, ops.GN_ATTR, None)
    assert (p_ref is None) == (p_y is None)
    if p_y is not None:
        assert p_y[0].shape == p_ref[0].shape and p_y[1] == p_ref[1]
        assert torch.allclose(p_y[0][..., 0], p_ref[0][..., 0], rtol=1e-3, atol=1e-3)
        gamma = torch.rand(192, generator=g).to(DEV) + 0.5
        beta = torch.zeros(192).to(DEV)
        assert rel_l2(ops.group_norm(y, gamma, beta, 1e-6, 32), ops.group_norm(ref, gamma, beta, 1e-6, 32)) < 2e-3
    yn = ops.conv2d(pc, (xa, xb), seg2=(x2, None, False), out_mode=ops.OUT_NCHW_F32)
    monkeypatch.setattr(ops, "BUF_LIMIT", 2147483647)
    assert rel_l2(yn, ops.conv2d(pc, (xa, xb), seg2=(x2, None, False), out_mode=ops.OUT_NCHW_F32)) < 1e-3


@pytest.mark.parametrize("B,H,W,C,ldx", [(2, 16, 16, 1280, 1280), (3, 8, 12, 320, 328), (1, 5, 7, 64, 64)])
def test_upsample_nearest2x_padded(ops, B, H, W, C, ldx):
    """sdk_upsample_nearest2x_padded (the UNet Upsample's F.interpolate(scale_factor=2, mode="nearest"),
    reference openai_model/model.py:120-131) vs torch, zero border of 1, strided source rows; and the 3x3 conv
    over it with pad 0 equals the conv with the upsample folded into its loads, bit for bit (same variant)."""
    xs = _rand(B, H, W, ldx, seed=H * W + C).to(DEV)
    x = xs[..., :C]
    y = ops.upsample_nearest2x_padded(x, 1)
    ref = F.pad(F.interpolate(x.float().permute(0, 3, 1, 2), scale_factor=2, mode="nearest"), (1, 1, 1, 1))
    assert torch.equal(y.float(), ref.permute(0, 2, 3, 1))
    if C % 64 == 0:
        g = torch.Generator().manual_seed(C)
        w = torch.randn(C, C, 3, 3, generator=g) / math.sqrt(9 * C)
        pc = ops.PackedConv([(w, C)], torch.randn(C, generator=g) * 0.1, device=DEV)
        for v in (22, 2):
            a = ops.conv2d(pc, x.contiguous(), upsample=True, pad=1, variant=v, split_k=1)
            b = ops.conv2d(pc, y, pad=0, variant=v, split_k=1)
            assert torch.equal(a, b), f"variant {v}"

