"""CPU checks of the inputs of tests/test_gpu_attn_wide_exact.py and tests/test_gpu_linattn_exact.py: every case
the GPU tests use is built here, so an inexact input fails on the CPU and not on the GPU."""
import pytest
import torch

import attn_exact_util as U
import attn_wide_util as W


@pytest.mark.parametrize("d", W.DIMS)
def test_wide_cases_build(d):
    """Every (family, shape) of ``wide_specs`` meets its exactness conditions (``Case`` raises InexactCase
    otherwise); the one-hot reference is V[f(i)], the weighted spread stays below the deferral headroom."""
    specs = W.wide_specs()
    assert {s[6] for s in specs} == {"sep", "kv", "qkv"}
    assert {(s[1], s[2]) for s in specs} == set(W.BH)
    assert {s[4] for s in specs} == set(W.NKS) and {s[3] for s in specs} >= {W.NQ_SMALL, W.NQ_BIG}
    for family, B, H, nq, nk, negative, layout in specs:
        c = U.get_case(family, B, H, nq, nk, d, False, negative)
        assert c.ref.shape == (B * nq, H * d) and not c.ref.isnan().any()
        if family == "weighted":
            assert c.spread < 8 and nk * 4 ** c.spread * U.VMAX < 2 ** 24
        if layout == "qkv":
            assert nq == nk


def test_wide_shapes_cover_the_kernel():
    """nk: a ragged single tile, one whole tile, two tiles plus a key, more tiles than twice the ring's slots;
    nq: below one wave's share and two workgroups plus a ragged one; both instantiations, each with a padded
    and its full head dim."""
    ragged, one, two1, many = W.NKS
    assert ragged < W.KT and one == W.KT and two1 == 2 * W.KT + 1 and many > 4 * W.KT and many % W.KT
    assert W.NQ_SMALL < 16 and W.NQ_BIG > 2 * W.ROWS and W.NQ_BIG % W.ROWS
    assert {W.padded(d) for d in W.DIMS} == {256, 512}
    assert 168 in W.DIMS and 256 in W.DIMS and 264 in W.DIMS and 512 in W.DIMS
    assert W.expected_info(512, 2, 3, 133)["grid"] == 18


@pytest.mark.parametrize("n,d", W.LIN_SHAPES)
def test_linear_cases_build(n, d):
    """The selector family's conditions: k is 0 / -64, cnt(d) in {1, 2, 4, 8} members per channel, v an integer in
    [1, 15], three +-1 per row of q; the float64 evaluation of the reference's expressions equals the exact
    rational, which fp16 holds."""
    for H in W.LIN_HEADS:
        c = W.get_lin_case(W.LIN_BATCH, H, n, d)
        c.check_conditions()
        assert set(c.k.unique().tolist()) == {W.KOFF, 0.0}
        assert c.v.min().item() >= 1 and c.v.max().item() <= 15 and torch.equal(c.v, c.v.round())
        assert set(c.cnt.unique().tolist()) <= set(float(x) for x in W.CNTS)
        assert c.ref.shape == (W.LIN_BATCH * n, H * d)
        # an fp32 emulation in chunks of 64 tokens with fp16 P (the kernel's arithmetic) gives the same bits
        kk, vv = c.k.float(), c.v.float()
        ms, dens, ctxs = [], [], []
        for s in range(0, n, 64):
            a = kk[:, s:s + 64] * 1.4426950408889634
            m = a.max(1, keepdim=True).values
            p = torch.exp2(a - m)
            ms.append(m)
            dens.append(p.sum(1, keepdim=True))
            ctxs.append(torch.einsum("bnhd,bnhe->bhde", p.half().float(), vv[:, s:s + 64]))
        mg = torch.stack(ms).max(0).values
        den = sum(torch.exp2(m - mg) * dn for m, dn in zip(ms, dens))
        ctx = sum(torch.exp2(m - mg).permute(0, 2, 3, 1) * cx for m, cx in zip(ms, ctxs))
        ctx = (ctx * (1.0 / den).permute(0, 2, 3, 1)).half().float()
        out = torch.einsum("bhde,bnhd->bnhe", ctx, c.q.float()).reshape(W.LIN_BATCH * n, H * d).half()
        assert torch.equal(out.view(torch.int16), c.ref.view(torch.int16))
