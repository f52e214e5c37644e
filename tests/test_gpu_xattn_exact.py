"""Exact per-element tests of the fused cross-attention block (xattn.hip) on the MI355X (run with -m gpu).

The one-hot attention family (tests/attn_exact_util.py) runs through to_q -> attention over K|V -> to_out +
bias + residual with signed, non-involutive permutation matrices for Wq and Wo (a transposed weight gives
another answer), an integer bias and an integer residual: out = res + bias + (+-V[f(i)])[perm], every step an
integer below 2048, so the output must EQUAL the float64 reference bit for bit.  Bit equality holds although
the kernel multiplies the scores by c = scale * log2(e), which is 1 only to within an fp32 ulp: the winner's
scaled score is also the row maximum, so its P is exp2(0) = 1, the losers stay >= 63 below it, and the row sum is 1.
t / kv / res are views into NaN-filled buffers, out a view inside a sentinel-filled buffer."""
import pytest
import torch

import attn_exact_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = [(C, D, n, nk) for C, D in U.XATTN_SHAPES for n in U.XATTN_N for nk in U.XATTN_NK]


@pytest.fixture(scope="module")
def ops(sdk):
    from sd_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return o


_PC = {}


def _weights(ops, C):
    if C not in _PC:
        wq, wo, bias = U.xattn_weights(C)
        _PC[C] = (ops.PackedConv([(wq.float(), C)], None, device=DEV), ops.PackedConv([(wo.float(), C)], bias.float(), device=DEV))
    return _PC[C]


@pytest.mark.parametrize("C,D,n_img,nk", CASES, ids=[f"c{C}d{D}-n{n}-k{nk}" for C, D, n, nk in CASES])
def test_cross_attention_block_exact(ops, C, D, n_img, nk):
    """batch 2; packed and row weight layouts; both wave counts at 640 channels; at the ragged nk also the
    negative winner (the zero K rows of LDS past nk would win without the key mask)."""
    from sd_amd._lib import lib
    B = 2
    pcq, pco = _weights(ops, C)
    bad = []
    for negative in ((False, True) if nk < 80 else (False,)):
        c = U.XCase(B, n_img, C, D, nk, negative)
        t, kv, res = U.guarded(c.t, 8, DEV), U.guarded(c.kv, 8, DEV), U.guarded(c.res, 16, DEV)
        old = ops.XATTN_PACKED_W
        try:
            for packed in (True, False):
                for waves in ((8, 4) if C == 640 else (4,)):
                    if C == 640:
                        assert lib().sdk_xattn_debug_waves640(waves) == 0
                    ops.XATTN_PACKED_W = packed
                    buf, out = U.out_buffer(B * n_img, C, DEV, pad=8)
                    y = ops.cross_attention_block(t, kv, pcq, pco, batch=B, n_img=n_img, nk=nk, heads=C // D,
                                                  head_dim=D, scale=U.SCALE, residual=res, out=out)
                    assert y.data_ptr() == out.data_ptr()
                    torch.cuda.synchronize()
                    got, clean = U.split_out(buf, B * n_img, C)
                    tag = f"{c.name} packed={packed} waves={waves}"
                    if not clean:
                        bad.append(f"{tag}: wrote outside the output's extent")
                    if got.isnan().any():
                        bad.append(f"{tag}: {int(got.isnan().sum())} NaN in the output")
                        continue
                    ne = got.view(torch.int16) != c.ref.view(torch.int16)
                    if ne.any():
                        r, col = (int(x) for x in ne.nonzero()[0])
                        bad.append(f"{tag}: {int(ne.sum())} elements differ in {int(ne.any(1).sum())} rows; first at "
                                   f"row {r} col {col}: got {got[r, col].item()}, want {c.ref[r, col].item()}")
        finally:
            ops.XATTN_PACKED_W = old
            lib().sdk_xattn_debug_waves640(8)
    assert not bad, "\n".join(bad)
