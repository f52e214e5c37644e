"""The chained SpatialTransformer entry (sdk_proj_norm_qkv, csrc/conv_rowpanel.hip) on the MI355X (run with -m gpu):
tok = proj_in(GroupNorm affine?(x)) and qkv = [q | k | v](norm1(tok)) in one launch, compared BIT FOR BIT with the
three launches it replaces — group_norm(silu=False) -> sdk_token_linear_ln -> conv2d on the q|k|v weight.

Shapes: the smallest at which it can go wrong — part of one wave (16 rows), the panel edge (255 / 256 / 257), image
boundaries inside a 16-row block (300 rows, hw = 100) and two full panels (512 rows, hw = 256); with and without the
GroupNorm affine; contiguous and with row strides larger than the widths, in sentinel-filled buffers whose untouched
bytes are checked afterwards.  One case is also checked against a float64 restatement at the limits
tests/test_gpu_token.py uses for proj_in + LayerNorm and for the GEMM (rel-L2 2e-3).  Then the rejections of the C
entry, and a 320-channel SpatialTransformer run both ways, eagerly and under graph capture + replay."""
import math

import pytest
import torch

from gpu_util import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
C, NQ = 320, 960
ROWPANEL = 49          # conv variant id of conv_rowpanel_kernel
SENT = -7.25           # no output of these cases comes near it
CASES = [(16, 1, 16), (255, 1, 255), (256, 1, 256), (257, 1, 257), (300, 3, 100), (512, 2, 256)]   # rows, images, hw


@pytest.fixture(scope="module")
def ops(sdk):
    from sd_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return o


_CACHE = {}


def _weights(ops):
    """One set of weights and its three packs for every case (computed once, left unchanged)."""
    if "w" not in _CACHE:
        g = torch.Generator().manual_seed(320)
        w_in = (torch.randn(C, C, generator=g) / math.sqrt(C)).half()
        b_in = torch.randn(C, generator=g) * 0.2
        w_qkv = (torch.randn(NQ, C, generator=g) / math.sqrt(C)).half()
        gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
        gn_g, gn_b = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
        dev = torch.device(DEV)
        _CACHE["w"] = dict(w_in=w_in, b_in=b_in, w_qkv=w_qkv, gamma=gamma.to(DEV), beta=beta.to(DEV),
                           gn_g=gn_g.to(DEV), gn_b=gn_b.to(DEV),
                           ptl=ops.PackedTokenLinear(w_in, b_in, dev),
                           pc_qkv=ops.PackedConv([(w_qkv.float(), C)], None, device=dev),
                           ppq=ops.PackedProjQkv(w_in, b_in, w_qkv, dev))
    return _CACHE["w"]


def _reference(ops, rows, nimg, hw, gn):
    """(x [nimg, hw, 1, 320], affine or None, tok, qkv) of today's route, once per case."""
    key = (rows, gn)
    if key not in _CACHE:
        W = _weights(ops)
        g = torch.Generator().manual_seed(rows)
        x = (torch.randn(nimg, hw, 1, C, generator=g) * 1.5 + 0.3).half().to(DEV)
        if gn:
            aff = ops.group_norm_affine(x, W["gn_g"], W["gn_b"], 1e-6, 32)
            xn = ops.group_norm(x, W["gn_g"], W["gn_b"], 1e-6, 32, silu=False)
        else:
            aff, xn = None, x
        tok, t1 = ops.token_linear(W["ptl"], xn.view(rows, C), norm=(W["gamma"], W["beta"], 1e-5))
        # the q|k|v conv of today's route at the level the chain is routed to is the row-panel kernel (variant 49,
        # named by the tuning table; its sums are those of the tiled variants 22 / 38).  The planner's own choice
        # for a 16-row GEMM is a kernel with another summation order, which no route runs at that level
        ops.FORCE_VARIANT = ROWPANEL
        try:
            qkv = ops.linear(W["pc_qkv"], t1)
        finally:
            ops.FORCE_VARIANT = None
        _CACHE[key] = (x, aff, tok, qkv)
    return _CACHE[key]


def _guarded(rows, width, ld):
    buf = torch.full((rows * ld + 64,), SENT, dtype=torch.float16, device=DEV)
    return buf, buf[:rows * ld].view(rows, ld)[:, :width]


def _untouched(buf, rows, width, ld):
    body = buf[:rows * ld].view(rows, ld)
    return bool((body[:, width:] == SENT).all()) and bool((buf[rows * ld:] == SENT).all())


@pytest.mark.parametrize("gn", [False, True], ids=["plain", "gn"])
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("rows,nimg,hw", CASES)
def test_proj_norm_qkv_bits(ops, rows, nimg, hw, strided, gn):
    W = _weights(ops)
    x, aff, tok_ref, qkv_ref = _reference(ops, rows, nimg, hw, gn)
    x2 = x.view(rows, C)
    lds = (C + 8, C + 24, NQ + 16) if strided else (C, C, NQ)
    xbuf, xv = _guarded(rows, C, lds[0])
    xv.copy_(x2)
    tbuf, tv = _guarded(rows, C, lds[1])
    qbuf, qv = _guarded(rows, NQ, lds[2])
    tok, qkv = ops.proj_norm_qkv(W["ppq"], xv, (W["gamma"], W["beta"], 1e-5), gn=aff, hw=hw if gn else None,
                                 tok=tv, qkv=qv)
    torch.cuda.synchronize()
    dt = (tok.float() - tok_ref.float()).abs().max().item()
    dq = (qkv.float() - qkv_ref.float()).abs().max().item()
    print(f"[proj_norm_qkv] rows={rows} hw={hw} gn={gn} strided={strided}: max |diff| tok {dt:.3e} qkv {dq:.3e}",
          flush=True)
    assert torch.equal(tok, tok_ref)
    assert torch.equal(qkv, qkv_ref)
    assert _untouched(tbuf, rows, C, lds[1]) and _untouched(qbuf, rows, NQ, lds[2])
    assert torch.equal(xv, x2) and _untouched(xbuf, rows, C, lds[0])


def test_proj_norm_qkv_vs_float64(ops):
    """The 300-row, 3-image case with the GroupNorm affine against the chain restated in float64 with its fp16
    rounding points (xn, tok, norm1(tok), qkv).  Limits: tests/test_gpu_token.py (rel-L2 2e-3 for proj_in, for the
    LayerNorm it feeds and for a GEMM of this K)."""
    rows, nimg, hw = 300, 3, 100
    W = _weights(ops)
    x, aff, _, _ = _reference(ops, rows, nimg, hw, True)
    tok, qkv = ops.proj_norm_qkv(W["ppq"], x.view(rows, C), (W["gamma"], W["beta"], 1e-5), gn=aff, hw=hw)
    sc, sh = (a.double().cpu() for a in aff)
    xn = (x.view(nimg, hw, C).double().cpu() * sc[:, None] + sh[:, None]).half().double().view(rows, C)
    tok64 = (xn @ W["w_in"].double().T + W["b_in"].double()).half()
    t64 = torch.nn.functional.layer_norm(tok64.double(), (C,), W["gamma"].double().cpu(), W["beta"].double().cpu(),
                                         1e-5).half()
    qkv64 = t64.double() @ W["w_qkv"].double().T
    et, eq = rel_l2(tok, tok64), rel_l2(qkv, qkv64)
    print(f"[proj_norm_qkv] vs float64: rel-L2 tok {et:.2e} qkv {eq:.2e}", flush=True)
    assert et < 2e-3 and eq < 2e-3


def _args(_lib, x, w, b, gb, tok, qkv):
    a = _lib.ProjNormQkvArgs()
    a.x, a.w, a.bias, a.gamma, a.beta = x.data_ptr(), w.data_ptr(), b.data_ptr(), gb.data_ptr(), gb.data_ptr()
    a.tok, a.qkv = tok.data_ptr(), qkv.data_ptr()
    a.x_ld, a.tok_ld, a.qkv_ld = C, C, NQ
    a.rows, a.in_features, a.features, a.qkv_features, a.eps = 64, C, C, NQ, 1e-5
    return a


def test_proj_norm_qkv_rejects(ops, sdk):
    from sd_amd import _lib
    L = _lib.lib()
    assert ops.proj_norm_qkv_supported(320, 320, 960) and not ops.proj_norm_qkv_supported(640, 640, 1920)
    x = torch.zeros(64, C, dtype=torch.float16, device=DEV)
    tok = torch.zeros(64, C, dtype=torch.float16, device=DEV)
    qkv = torch.zeros(64, NQ, dtype=torch.float16, device=DEV)
    w = torch.zeros(C + NQ, C, dtype=torch.float16, device=DEV)
    b = torch.zeros(C + NQ, dtype=torch.float32, device=DEV)
    gb = torch.ones(C, dtype=torch.float32, device=DEV)
    aff = torch.ones(1, C, dtype=torch.float32, device=DEV)

    def rc(**kw):
        a = _args(_lib, x, w, b, gb, tok, qkv)
        for k, v in kw.items():
            setattr(a, k, v)
        return L.sdk_proj_norm_qkv(a, None)

    assert rc() == 0                                             # the base arguments are accepted
    torch.cuda.synchronize()
    for feats in ((640, 640, 1920), (320, 320, 640), (320, 640, 960), (640, 320, 960)):
        assert rc(in_features=feats[0], features=feats[1], qkv_features=feats[2]) != 0
    assert rc(x=x.data_ptr() + 8) != 0 and rc(tok=tok.data_ptr() + 2) != 0 and rc(gamma=gb.data_ptr() + 4) != 0
    assert rc(x_ld=C + 4) != 0 and rc(tok_ld=C + 2) != 0 and rc(qkv_ld=NQ + 12) != 0 and rc(qkv_ld=C) != 0
    assert rc(tok=x.data_ptr()) != 0                             # tok overlaps x
    assert rc(qkv=w.data_ptr()) != 0                             # qkv overlaps the weight
    assert rc(tok=qkv.data_ptr()) != 0                           # the outputs overlap each other
    assert rc(gn_scale=aff.data_ptr(), gn_shift=aff.data_ptr()) != 0             # an affine without hw
    assert rc(gn_scale=aff.data_ptr(), hw=64) != 0                               # a scale without a shift
    assert rc(gn_scale=aff.data_ptr(), gn_shift=aff.data_ptr(), hw=48) != 0      # rows no multiple of hw
    assert rc(gn_scale=aff.data_ptr(), gn_shift=aff.data_ptr(), hw=64) == 0
    assert rc(rows=0) != 0 and rc(w=None) != 0
    torch.cuda.synchronize()


def _transformer():
    from sd_amd.openai_model.attention import SpatialTransformer
    torch.manual_seed(7)
    m = SpatialTransformer(320, 8, 40, depth=1, context_dim=None).half()
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape) * (0.05 if p.dim() > 1 else 0.2))
        m.norm.weight.add_(1.0)
    m._prepare(torch.device(DEV))
    return m, (torch.randn(2, 16, 16, 320) * 1.3).half().to(DEV)


def _eager_and_replayed(m, x):
    with torch.no_grad():
        eager = m._run(x).clone()
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            m._run(x)                                  # warm-up on the capture stream (workspaces, LDS caps)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                y = m._run(x)
        torch.cuda.current_stream().wait_stream(s)
        y.zero_()
        g.replay()
        torch.cuda.synchronize()
    return eager, y.clone()


def test_spatial_transformer_chain_equals_three_launches(ops, monkeypatch):
    """A 320-channel SpatialTransformer, H = W = 16, B = 2 (512 rows): the chained route and the three launches
    (the module switch SD_AMD_PROJ_QKV_CHAIN=0 sets) give equal bits, eagerly and under graph capture + replay."""
    from sd_amd.openai_model import attention
    m, x = _transformer()
    launched = []
    real = ops.proj_norm_qkv
    monkeypatch.setattr(ops, "proj_norm_qkv", lambda *a, **k: (launched.append(1), real(*a, **k))[1])
    outs = {}
    for chain in (True, False):
        monkeypatch.setattr(attention, "PROJ_QKV_CHAIN", chain)
        before = len(launched)
        outs[chain] = _eager_and_replayed(m, x)
        assert len(launched) - before == (3 if chain else 0)      # eager, warm-up and capture: once each
    assert torch.isfinite(outs[True][0].float()).all() and outs[True][0].float().abs().max() > 0
    assert torch.equal(outs[True][0], outs[True][1]) and torch.equal(outs[False][0], outs[False][1])
    assert torch.equal(outs[True][0], outs[False][0])
