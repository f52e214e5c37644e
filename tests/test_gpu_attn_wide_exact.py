"""Exact per-element tests of the wide attention form (csrc/attention_wide.hip, head_dim 168..512) on the MI355X
(run with -m gpu), requested as ``form="wide"`` and through ``"auto"``, each asserted to be what ran (``form_out``).

The inputs are the two families of tests/attn_exact_util.py, unchanged: the one-hot family must reproduce V[f(i)]
bit for bit, the weighted family must be within 1 fp16 ulp of the float64 reference (bound derived in that
module's docstring; it holds with or without the deferred max, every rescale being a power of two).  q / k / v are
strided views into NaN-filled buffers, the output a view inside a sentinel-filled buffer that must keep its bits
everywhere else.  Shapes: tests/attn_wide_util.py.

  wide   168 .. 256   attn_wide_kernel<256>   8 waves share 64 query rows, 32 keys per tile
  wide   264 .. 512   attn_wide_kernel<512>
  auto   d > 160: wide"""
import pytest
import torch

import attn_exact_util as U
import attn_wide_util as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAIRS = [(d, f) for d in W.DIMS for f in W.FORMS]


@pytest.fixture(scope="module")
def ops(sdk):
    from sd_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return o


def _run(ops, c, layout, form):
    q, k, v = U.guarded_qkv(c, layout, DEV)
    rows, cols = c.B * c.nq, c.H * c.d
    buf, out = U.out_buffer(rows, cols, DEV)
    info = {}
    y = ops.attention(q, k, v, batch=c.B, heads=c.H, nq=c.nq, nk=c.nk, head_dim=c.d, scale=U.SCALE, out=out,
                      form=form, form_out=info)
    assert y.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    got, clean = U.split_out(buf, rows, cols)
    return got, clean, info


def test_constants(ops):
    """The util's restatement of the kernel's tile constants is what the package exports."""
    assert (ops.ATTN_WIDE_ROWS, ops.ATTN_WIDE_KT) == (W.ROWS, W.KT)


@pytest.mark.parametrize("d,form", PAIRS, ids=[f"d{d}-{f}" for d, f in PAIRS])
def test_attention_wide_exact(ops, d, form):
    """Both families at nk = 20 / 32 / 65 / 129 (a ragged tile, one whole tile, two tiles and a key, five tiles),
    nq = 5 and 133, batch x heads 2 x 1 and 1 x 3, separate / packed k|v / packed q|k|v rows, the negative one-hot
    winner at the ragged nk.  One-hot: bit-equal.  Weighted: <= 1 fp16 ulp.  ``form_out``: the table's promise,
    grid included."""
    bad, ulps = [], []
    for family, B, H, nq, nk, negative, layout in W.wide_specs():
        c = U.get_case(family, B, H, nq, nk, d, False, negative)
        got, clean, info = _run(ops, c, layout, form)
        tag = f"{c.name} {form} {layout}"
        want = W.expected_info(d, B, H, nq)
        if info != want:
            bad.append(f"{tag}: ran {info}, the table promises {want}")
        if not clean:
            bad.append(f"{tag}: wrote outside the output's extent")
        if got.isnan().any():
            bad.append(f"{tag}: {int(got.isnan().sum())} NaN in the output")
            continue
        if family == "onehot":
            ne = got.view(torch.int16) != c.ref.view(torch.int16)
            if ne.any():
                r, col = (int(x) for x in ne.nonzero()[0])
                bad.append(f"{tag}: {int(ne.sum())} elements differ from V[f(i)], {int(ne.any(1).sum())} rows; first "
                           f"at row {r} (b {r // c.nq}, i {r % c.nq}) col {col}: got {got[r, col].item()}, "
                           f"want {c.ref[r, col].item()}")
        else:
            u = U.ulp_diff(got, c.ref)
            ulps.append(u)
            if u > 1:
                bad.append(f"{tag}: {u} fp16 ulp from the float64 reference (bound 1)")
    print(f"attention wide exact d={d} {form}: weighted max ulp {max(ulps)}")
    assert not bad, "\n".join(bad)


def test_wide_validation(ops):
    """``form="wide"`` at d = 160, ``causal`` at d = 256 and d = 520 raise (SDK_EINVAL) and launch nothing."""
    for d, kw, pat in ((160, dict(form="wide"), "no instantiation"), (256, dict(causal=True), "causal"),
                       (256, dict(causal=True, form="wide"), "causal"), (520, dict(), r"\[8, 512\]"),
                       (256, dict(form="nw4"), "no instantiation")):
        x = torch.zeros(64, d, dtype=torch.float16, device=DEV)
        buf, out = U.out_buffer(64, d, DEV)
        info = {}
        with pytest.raises(RuntimeError, match=r"\(-1\).*" + pat):
            ops.attention(x, x, x, batch=1, heads=1, nq=64, nk=64, head_dim=d, scale=1.0, out=out, form_out=info, **kw)
        torch.cuda.synchronize()
        assert info == {} and U.split_out(buf, 0, 0)[1], (d, kw)


def test_wide_under_graph_capture(ops):
    """The wide launch captures and replays to the exact result; ``form_out`` is the same eagerly and captured."""
    c = U.get_case("onehot", 1, 3, W.NKS[3], W.NKS[3], 512)
    q, k, v = U.guarded_qkv(c, "qkv", DEV)
    eager, cap = {}, {}
    y = ops.attention(q, k, v, batch=1, heads=3, nq=c.nq, nk=c.nk, head_dim=512, scale=U.SCALE, form_out=eager)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        yg = ops.attention(q, k, v, batch=1, heads=3, nq=c.nq, nk=c.nk, head_dim=512, scale=U.SCALE, form_out=cap)
    gr.replay()
    torch.cuda.synchronize()
    assert cap == eager == W.expected_info(512, 1, 3, c.nq)
    assert torch.equal(yg.cpu().view(torch.int16), c.ref.view(torch.int16)) and torch.equal(y, yg)
