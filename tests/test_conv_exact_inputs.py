"""CPU checks of the exact-arithmetic conv cases (tests/conv_exact_util.py): every case is exact, covers
the tile edges it claims, and the SiLU / GELU value sets round as the GPU test assumes.  No GPU, and
nothing of the product package."""
import math

import pytest
import torch
import torch.nn.functional as F

import conv_exact_util as U


@pytest.mark.parametrize("name", U.ALL_CASES)
def test_case_is_exact(name):
    """|ref| < 2048, integral, float32 == float64 and the fp16 round trip is the identity (asserted by
    ``reference`` while the case is built; restated here on the stored reference), for the value before
    the residual add as well as the final one."""
    c = U.get_case(name)
    ref = c.ref
    assert ref.dtype == torch.float32 and ref.abs().max().item() < U.LIMIT
    assert torch.equal(ref, ref.round()) and torch.equal(ref.half().float(), ref)
    pre64, y64 = U._reference(c, torch.float64)
    assert torch.equal(y64, ref.double()) and pre64.abs().max().item() < U.LIMIT
    assert U._abs_bound(c) < 2 ** 24
    assert ref.abs().max().item() > 16, "a reference this small would not exercise the accumulation"
    for s in c.srcs + (c.srcs2 or []):
        assert s.dtype == torch.float16
    assert torch.equal(c.w.half().float(), c.w)


def test_inexact_case_is_a_test_error():
    """Inputs that break the conditions raise InexactCase (a test error), not a comparison failure."""
    g = U._gen("inexact")
    x = U._ints(g, (1, 4, 4, 64), -3, 3)
    w = U._weight(g, 16, 64, 1)
    with pytest.raises(U.InexactCase, match="limit"):
        U.Case("too-large", srcs=[x * 200], w=w)
    with pytest.raises(U.InexactCase, match="integral"):
        U.Case("fractional", srcs=[x * 0.5], w=w)
    with pytest.raises(U.InexactCase, match="float32"):
        # 2^24 + odd is not a float32: a huge bias that the embedding row cancels in float64 only
        U.Case("cancel", srcs=[x], w=w, bias=torch.full((16,), 2.0 ** 24), row_bias=(torch.full((1, 16), -2.0 ** 24), 0))


@pytest.mark.parametrize("name", U.ALL_CASES)
def test_case_covers_the_tiles_it_claims(name):
    """>= 2 M-tiles and >= 2 N-tiles with ragged last tiles for each claimed BM x BN; M > 64 and
    Cout > 8 for the tile cases, so neither the skinny nor the direct plan pre-empts."""
    c = U.get_case(name)
    M, N = c.M, c.cout
    if c.tiles:
        assert M > 64 and N > 8
    for bm, bn in c.tiles:
        assert -(-M // bm) >= 2, (bm, M)
        assert (M % bm != 0) == c.ragged_m, (bm, M)
        if c.ragged_n:
            assert -(-N // bn) >= 2 and N % bn != 0, (bn, N)
    if name in ("A", "B", "C", "D-odd", "D-even"):
        B, Ho, Wo, _ = c.out_shape
        assert (B, Ho, Wo, N) == (2, 13, 11, 328)
        assert Ho * Wo < 256 < 2 * Ho * Wo            # the first 256-row tile straddles the two images
        assert M % 128 == 30 and M % 256 == 30
        assert {N % 128, N % 256} == {72} and {N % 160, N % 320} == {8}
    if name == "E":
        assert c.out_shape == (2, 14, 12, 328)
    if name == "A":
        assert c.srcs[0].shape[-1] % 64 == 8          # a ragged 64-channel K block
    if name == "K":
        assert c.out_shape[1] == 256 and all(256 % bm == 0 for bm, _ in U.TILE.values())


def test_variant_tables():
    assert [v for v in U.VARIANT_IDS if v != "auto"] == [str(v) for v in sorted(U.TILE)]
    assert U.GEGLU_OK <= set(U.TILE)
    assert {U.TILE[v] for v in U.GEGLU_OK} >= {(128, 256), (256, 256)}     # what case J claims


def test_silu_value_set_rounds_to_integers():
    """silu(v) for v in SILU_SET is {0, 0, 12, ..., 16} after fp16 rounding, for the exact sigmoid and
    for any sigmoid within 1e-4 of it (the kernels use exp and a reciprocal approximation)."""
    v = torch.tensor(U.SILU_SET, dtype=torch.float64)
    want = torch.tensor(U.SILU_OUT, dtype=torch.float64)
    sig = torch.sigmoid(v)
    for err in (0.0, 1e-4, -1e-4):
        got = (v * (sig * (1.0 + err))).half().double()
        assert torch.equal(got, want), (err, got)
    assert torch.equal(F.silu(v).half().double(), want)
    assert torch.equal(F.silu(v.float()).half().double(), want)


def test_gelu_value_set_rounds_to_identity():
    """gelu(g) rounds to g in fp16 for g in 6..13, exact erf form and tanh approximation alike, and
    a * gelu(g) rounds to a * g for every integer a the GEGLU case can produce."""
    g = torch.tensor(U.GELU_SET, dtype=torch.float64)
    erf = 0.5 * g * (1.0 + torch.erf(g / math.sqrt(2.0)))
    tanh = 0.5 * g * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (g + 0.044715 * g ** 3)))
    for y in (erf, tanh, F.gelu(g.float()).double()):
        assert torch.equal(y.half().double(), g)
    a = torch.arange(-157, 158, dtype=torch.float64)[:, None]            # |a| * 13 < 2048
    assert torch.equal((a * erf).half().double(), a * g)
    c = U.get_case("J")
    inner = c.nout
    assert torch.equal(c.w[inner:], torch.zeros_like(c.w[inner:]))
    assert set(c.bias[inner:].tolist()) <= set(U.GELU_SET) and len(set(c.bias[inner:].tolist())) == 8


def test_expected_variant_rule():
    a, f, j, k = (U.get_case(n) for n in ("A", "F-40_32-k3", "J", "K"))
    assert U.expected_variant(a, "auto") is None and U.expected_variant(a, "22") == 22
    assert U.expected_variant(f, "22") == 0 and U.expected_variant(f, "auto") == 0
    assert U.expected_variant(j, "22") == "geglu" and U.expected_variant(j, "40") == 40
    assert U.expected_variant(k, "0") == "tile" and U.expected_variant(k, "7") == 7
    assert U.expected_variant(U.get_case("M"), "auto") == 34 and U.expected_variant(U.get_case("N-res"), "auto") == 35


def test_canary_buffers_and_report():
    """The guarded buffers, the sentinel check and the mismatch report, on the CPU."""
    c = U.get_case("A")
    x = U.guarded_nhwc(c.srcs[0], 88, "cpu")
    assert torch.equal(x, c.srcs[0]) and x.stride(2) == 88 and not x.is_contiguous()
    assert torch.isnan(x._base).sum().item() == x._base.numel() - x.numel()
    r = U.guarded_residual(c.residual, 344, "cpu")
    assert r.shape[-1] == 344 and torch.equal(r[..., :328], c.residual) and torch.isnan(r[..., 328:]).all()
    buf, out = U.out_buffer(c, "cpu")
    assert out.shape == (2, 13, 11, 352) and out.data_ptr() == buf.data_ptr()
    out[..., :328] = c.ref.half()
    got, clean = U.split_out(c, buf)
    assert clean and U.mismatch_report(c, got, c.ref, {"variant": 22, "split_k": 1}) is None
    buf[2, 0, 0, 0] = 1.0                                  # a write past the last image
    assert not U.split_out(c, buf)[1]
    buf[2, 0, 0, 0] = U.SENTINEL
    buf[0, 3, 3, 328] = 0.0                                # a write past cout
    assert not U.split_out(c, buf)[1]
    bad = c.ref.clone()
    bad[1, 12, 10, 327] += 1                               # the last element: last M-tile, last N-tile
    bad[1, 12, 10, 326] = float("nan")
    rep = U.mismatch_report(c, bad, c.ref, {"variant": 22, "split_k": 2})
    assert "2 of" in rep and "variant 22 split_k 2" in rep and "M-tile 1, N-tile 1 of the 256x320" in rep
    assert "(b=1, oy=12, ox=10, n=326): got nan" in rep
    rep = U.mismatch_report(c, bad, c.ref, {"variant": 31, "split_k": 1})
    assert "M-tile 2, N-tile 2 of the 128x160" in rep
    assert U.tile_of(U.get_case("J"), 40, 0, 0, 0, 191) == (0, 1)      # x column 191 is packed row 351
    with pytest.raises(AssertionError, match="N-tile"):
        U.assert_exact(c, bad, {"variant": 0, "split_k": 1})
