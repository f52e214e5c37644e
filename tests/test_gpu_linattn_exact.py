"""Exact tests of linear attention (csrc/linattn.hip, ``ops.linear_attention``) on the MI355X (run with -m gpu).

The selector family of tests/attn_wide_util.py (``LinCase``): every step of the kernel is exact on it, in any
chunking and any summation order, so the output must equal the float64 evaluation of the reference's expressions
bit for bit.  Shapes (tokens, dim_head) = (67, 40), (200, 264), (129, 512), (64, 8) (two, four, three chunks and
one; a ragged last chunk, a ragged 32-column block of d, e blocks past the fourth), heads 1 and 3, batch 2, strided
rows in NaN-filled buffers, the output inside a sentinel-filled buffer."""
import pytest
import torch

import attn_exact_util as U
import attn_wide_util as W

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops(sdk):
    from sd_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return o


@pytest.mark.parametrize("n,d", W.LIN_SHAPES, ids=[f"n{n}-d{d}" for n, d in W.LIN_SHAPES])
@pytest.mark.parametrize("H", W.LIN_HEADS)
def test_linear_attention_exact(ops, n, d, H):
    c = W.get_lin_case(W.LIN_BATCH, H, n, d)
    c.check_conditions()
    q, k, v = W.lin_guarded(c, DEV)
    rows, cols = c.B * n, H * d
    buf, out = U.out_buffer(rows, cols, DEV)
    y = ops.linear_attention(q, k, v, batch=c.B, heads=H, n=n, dim_head=d, out=out)
    assert y.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    got, clean = U.split_out(buf, rows, cols)
    assert clean, "wrote outside the output's extent"
    assert not got.isnan().any(), f"{int(got.isnan().sum())} NaN in the output"
    ne = got.view(torch.int16) != c.ref.view(torch.int16)
    if ne.any():
        r, col = (int(x) for x in ne.nonzero()[0])
        pytest.fail(f"{c.name}: {int(ne.sum())} elements differ; first at row {r} col {col}: got {got[r, col].item()}, "
                    f"want {c.ref[r, col].item()}")


def test_linear_attention_twice_bitwise(ops):
    """Two evaluations on random data agree bit for bit (fixed chunk order, no floating-point atomics), and
    agree with the fp32 evaluation of the reference's expressions to fp16 accuracy."""
    B, H, n, d = 2, 3, 200, 264
    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(B * n, H * d, generator=g).half().to(DEV) for _ in range(3))
    y0 = ops.linear_attention(q, k, v, batch=B, heads=H, n=n, dim_head=d).clone()
    y1 = ops.linear_attention(q, k, v, batch=B, heads=H, n=n, dim_head=d)
    torch.cuda.synchronize()
    assert torch.equal(y0.view(torch.int16), y1.view(torch.int16))
    q4, k4, v4 = (t.cpu().double().view(B, n, H, d) for t in (q, k, v))
    ctx = torch.einsum("bnhd,bnhe->bhde", torch.softmax(k4, dim=1), v4)
    ref = torch.einsum("bhde,bnhd->bnhe", ctx, q4).reshape(B * n, H * d)
    rel = ((y1.cpu().double() - ref).norm() / ref.norm()).item()
    print(f"linear attention random data: rel-L2 {rel:.3e}")
    # three fp16 roundings (P, ctx, out), each <= 2^-11 relative per element and independent: the L2 norms add
    # in quadrature to at most sqrt(3) * 2^-11 = 8.5e-4
    assert rel < 3 ** 0.5 * 2.0 ** -11


def test_linear_attention_validation(ops):
    x = torch.zeros(64, 520, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match=r"\[8, 512\]"):
        ops.linear_attention(x, x, x, batch=1, heads=1, n=64, dim_head=520)
    with pytest.raises(RuntimeError, match=r"\[8, 512\]"):
        ops.linear_attention(x, x, x, batch=1, heads=1, n=64, dim_head=12)
