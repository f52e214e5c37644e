"""CPU checks of the exact GroupNorm-statistics and LayerNorm cases (tests/gn_stats_exact_util.py,
tests/ln_exact_util.py): the exactness conditions of every data family, the representability of the synthetic
partials, the route every case claims (through the host-only ``sdk_group_norm_plan``), and that correct fp32 row
math stays inside what the GPU LayerNorm test asserts.  No device is touched."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_exact_util as CU
import gn_stats_exact_util as G
import ln_exact_util as L

IDS = [c.name for c in G.CASES]


def _families(case):
    for fam in G.FAMILIES:
        for rot in (G.spike_rounds(case) if fam == "spike" else [0]):
            yield fam, rot, G.data(case, fam, rot)


@pytest.mark.parametrize("case", G.CASES, ids=IDS)
def test_case_inputs_are_exact(case):
    """fp16 holds the data, the pivot-shifted fp32 sums cannot round, the reference's terms are exact doubles, and
    the spike reaches every position and channel it lists."""
    assert case.C % case.groups == 0 and case.cg <= 256 and all(ci % 8 == 0 for ci in case.cins)
    seen = set()
    for fam, rot, x in _families(case):
        assert x.shape == (case.B, case.hw, case.C)
        G.sources(case, x)
        G.check_pivot_sums(case, x)
        mean, var = G.exact_stats(x, case.groups)
        assert (var >= 0).all()
        if fam == "constant":
            assert torch.count_nonzero(var) == 0
        if fam == "offset":                      # a sum without the pivot leaves fp32's integers
            assert (x.double() ** 2).sum(1).min().item() > 2 ** 24, "every channel's sum x^2 must leave fp32's integers"
        if fam == "spike":
            base = x.mode(1).values
            for b, p, ch in (x != base[:, None, :]).nonzero().tolist():
                seen.add((p, ch))
            assert ((x != base[:, None, :]).sum((1, 2)) == 1).all(), "one spike per image"
    pos, chs = case.spike_positions(), case.spike_channels()
    assert {p for p, _ in seen} == set(pos) and 0 in pos and case.hw - 1 in pos
    assert {ch for _, ch in seen} == set(chs)


@pytest.mark.parametrize("case", [c for c in G.CASES if c.nch], ids=[c.name for c in G.CASES if c.nch])
def test_synthetic_partials_are_representable_and_describe_the_tensor(case):
    """chunk_partials raises InexactCase unless every (mean, M2) is an fp32 value; their float64 merge is the
    statistics of the tensor."""
    for n, ci in zip(case.nch, case.cins):
        assert n > 0 and case.hw % n == 0
    for fam, rot, x in _families(case):
        parts = G.case_partials(case, x)
        assert [tuple(p.shape) for p in parts] == [(case.B, n, ci, 2) for n, ci in zip(case.nch, case.cins)]
        mean, var = G.merge_partials(parts, case.hw, case.groups)
        em, ev = G.exact_stats(x, case.groups)
        assert torch.allclose(mean, em, rtol=1e-13, atol=1e-13), (case.name, fam)
        assert torch.allclose(var, ev, rtol=1e-12, atol=1e-13), (case.name, fam)


def test_inexact_inputs_raise_their_own_error():
    x = torch.arange(3 * 8, dtype=torch.int64).reshape(1, 3, 8)
    with pytest.raises(CU.InexactCase):
        G.chunk_partials(x, 1)                                   # 3 rows: the mean is a third
    with pytest.raises(CU.InexactCase):
        G.chunk_partials(torch.tensor([0, 4097, 0, 0]).reshape(1, 4, 1), 1)      # M2 needs more than 24 bits
    c = G.CASE["slice-7x5-c64"]
    with pytest.raises(CU.InexactCase):
        G.check_pivot_sums(c, torch.tensor([[[0], [17]]]))
    with pytest.raises(CU.InexactCase):
        G.sources(c, torch.full((c.B, c.hw, c.C), 2049, dtype=torch.int64))


def test_bounds_are_the_derived_ones():
    f64 = lambda v: torch.tensor([[v]], dtype=torch.float64)
    a = G.Affine(f64(3.0), f64(4.0), 0.25, torch.tensor([1.5]), torch.tensor([-1.0]), 1)
    r = 1.0 / np.sqrt(4.0 + 0.25)
    near = lambda v, w: abs(v - w) <= 4e-16 * abs(w)
    assert near(a.scale.item(), 1.5 * r) and near(a.shift.item(), -1.0 - 3.0 * 1.5 * r)
    assert near(a.bound_scale.item(), 2.0 ** -23 * 1.5 * r * (1 + 2.0 ** -10))
    assert near(a.bound_shift.item(), (2.0 ** -22 * 3.0 * 1.5 * r + 2.0 ** -24 * (1.0 + 4.5 * r)) * (1 + 2.0 ** -10) +
                2.0 ** -44 * 2048 * 1.5 * r)
    # what the listed one-line errors do, against the bound: an unbiased variance at 8x8, cg 10; a dropped eps
    n = 640.0
    assert abs(np.sqrt((n - 1) / n) - 1) > 100 * 2.0 ** -23
    assert abs(np.sqrt(1.0 / (1.0 + 1e-6)) - 1) > 2 * 2.0 ** -23
    assert G.tile_s(256) == 128 and G.tile_s(128) == 64 and G.REDUCE_S == 252


def _plan(sdk, case):
    from sd_amd import _lib
    a = _lib.GroupNormArgs()
    a.src0, a.scale, a.shift = 0x1000, 0x2000, 0x3000
    a.c_split, a.ld0 = case.c_split, case.c_split + 24
    if len(case.cins) > 1:
        a.src1, a.ld1 = 0x4000, case.cins[1] + 24
    a.batch, a.hw, a.channels, a.groups, a.eps = case.B, case.hw, case.C, case.groups, 1e-5
    info = _lib.GroupNormPlanInfo()
    n0, n1 = case.nch or (0, 0)
    rc = sdk.library().sdk_group_norm_plan(C.byref(a), 1, int(case.want_apply), case.H, case.W, case.pad, n0, n1, 1,
                                           C.byref(info))
    assert rc == 0, sdk.library().sdk_last_error()
    return {"stats": _lib.GN_STATS[info.stats], "apply": _lib.GN_APPLY[info.apply], "launches": info.launches,
            "workspace_bytes": info.workspace_bytes}


@pytest.mark.parametrize("case", G.CASES, ids=IDS)
def test_case_plans_the_route_it_claims(sdk, case):
    assert _plan(sdk, case) == case.plan
    if case.stats == "chunked":
        assert case.plan["workspace_bytes"] == sdk.library().sdk_group_norm_workspace(case.B, case.hw, case.C) > 0


def test_case_list_reaches_every_route_and_edge():
    assert {(c.stats, c.apply_form) for c in G.CASES} == G.COMBOS
    by = lambda stats, form=None: [c for c in G.CASES if c.stats == stats and form in (None, c.apply_form)]
    # slice: idle threads, a vector count that does not divide 512, c_split inside a slice, the widest slice
    sl = {G.fused_slice(c.C, c.groups) for c in by("slice")}
    assert {8, 120, 24, 504} <= sl and all(0 < s <= 512 for s in sl)
    assert any(len(c.cins) > 1 and c.c_split % G.fused_slice(c.C, c.groups) for c in by("slice", "none"))
    assert all(c.hw <= G.GN_SLICE_MAX_HW for c in by("slice"))
    assert all(c.hw <= G.GN_SLICE_APPLY_MAX_HW for c in by("slice", "in_stats"))
    # chunked: hw > 1024 or no admissible slice; ry 32 with a ragged chunk, nv 2, tpc 64 / 2 / 1, a concat
    ch = by("chunked")
    assert all(c.hw > 1024 or G.fused_slice(c.C, c.groups) == 0 for c in ch)
    geo = {c.name: G.chunk_geom(c.B, c.hw, c.C) for c in ch}
    assert geo["chunked-103x10-c64"] == (1, 32, 256, 5) and 1030 % 256 == 6
    assert geo["chunked-103x10-c2560"][:2] == (2, 1)
    assert {G.finalize_tpc(c.cg) for c in ch} >= {64, 2, 1}
    assert any(len(c.cins) > 1 for c in ch)
    # partials: chunk counts, unequal concat chunkings, c_split inside a group / a channel slice, idle lanes
    fin = by("parts", "none")
    assert {c.nch[0] for c in fin} >= {1, 2, 3, 16, 64}
    assert any(len(c.cins) > 1 and c.nch[0] != c.nch[1] for c in fin)
    assert any(len(c.cins) > 1 and c.c_split % c.cg for c in fin)
    assert any(G.finalize_tpc(c.cg) > c.nch[0] for c in fin) and any(G.finalize_tpc(c.cg) == 1 for c in fin)
    ap = by("parts", "in_stats")
    assert all(c.hw <= G.GN_PARTS_SINGLE_MAX_HW and max(c.nch) <= G.GNP_MAXCH and G.part_slice(c.C, c.groups) for c in ap)
    assert {c.pad for c in ap} == {0, 1} and {c.nch[0] for c in ap} >= {1, 2, 3, 16}
    assert any(len(c.cins) > 1 and c.c_split % G.part_slice(c.C, c.groups) for c in ap)
    assert any(G.part_slice(c.C, c.groups) < c.C for c in ap)
    splits = [G.part_row_splits(c.B, c.H, c.W, c.pad, c.C, c.groups) + ((c.H + 2 * c.pad) * (c.W + 2 * c.pad),) for c in ap]
    assert any(n > 1 and npix % rows for rows, n, npix in splits)      # a ragged last row split


def test_selector_convs_are_exact():
    for k in (1, 3):
        kw = G.selector_conv(f"tile-k{k}", 2, 16, 16, 64, 328, k)
        c = CU.Case(f"sel-k{k}", **kw)                          # reference() raises InexactCase otherwise
        assert c.ref.abs().max().item() <= 16 and c.out_shape == (2, 16, 16, 328)
        assert torch.equal((kw["w"] != 0).sum((1, 2, 3)), torch.ones(328, dtype=torch.long))
    y = CU.Case("sel-chk", **G.selector_conv("tile-k3", 2, 16, 16, 64, 328, 3)).ref
    part = torch.stack([y.double().reshape(2, 4, 64, 328).mean(2),
                        y.double().reshape(2, 4, 64, 328).var(2, unbiased=False) * 64], -1).float()
    assert G.check_chunk_stats(part, y, 0) == (0.0, 0.0)        # 64-row chunks of integers: exact in fp32
    swapped = part[:, [1, 0, 2, 3]]
    with pytest.raises(AssertionError):
        G.check_chunk_stats(swapped, y, G.REDUCE_S)             # a swapped chunk leaves every merged statistic alone
    m0, v0 = G.merge_partials([part], 256, 8)
    m1, v1 = G.merge_partials([swapped.contiguous()], 256, 8)
    assert torch.allclose(m0, m1, rtol=1e-14, atol=1e-14) and torch.allclose(v0, v1, rtol=1e-13)


# --------------------------------------------------------------------------- LayerNorm

def test_layer_norm_case_table():
    assert all(L.kernel_of(c) == k for c, k in L.KERNEL_OF.items())
    assert set(L.KERNEL_OF.values()) == {"quad<10>", "quad<20>", "row<1>", "row<2>", "row<4>"}
    assert all(c % 8 == 0 and c <= 2048 for c in L.COLS)
    assert any((c // 8) % 64 for c in L.COLS if c > 512)        # a last 64-lane set that is partly empty
    # the capped grids: 2048 blocks of 4 rows, of 64 rows in the quad form; one more step than the grid holds
    assert L.WALK[8] > 2 * 4 * 2048 and L.WALK[320] > 64 * 2048 and L.WALK[8] % 4 and L.WALK[320] % 16


@pytest.mark.parametrize("cols", L.COLS)
@pytest.mark.parametrize("family", L.FAMILIES)
def test_layer_norm_fp32_row_math_meets_the_gpu_assertions(family, cols):
    """The fp32 restatement of ln_row_stats / ln_apply8 (same pivot, same operation order) is within one fp16 ulp
    of the float64 reference, and at every row count the GPU test runs it differs in at least one element fewer than
    that test allows (in none where 0.5 % of the elements is less than two): the device's rsqrtf may differ from the
    correctly rounded one by an fp32 ulp.  The flips are not evenly spread: var = s2 / n - dm^2 cancels when the pivot
    is far from the mean, an error common to the whole row, so single rows of the offset family reach 0.4 %."""
    rows = [max(L.ROWS)] + ([L.WALK[cols]] if cols in L.WALK and family == "hashed" else [])
    for r in rows:
        x, gamma, beta, ref = L.case(family, r, cols)
        assert x[min(2, x.shape[0] - 1)].unique().numel() == 1                  # the constant row
        if family == "offset":
            d = (x.double().mean(1) - x[:, 0])[3:]
            assert (d > 10).all()                                               # mean far from the pivot (sigma 2.6)
        dist = (L.ordered(L.emulate(x, gamma, beta)) - L.ordered(ref)).abs()
        assert int(dist.max()) <= 1, (family, cols, r)
        for n in (L.ROWS if r == max(L.ROWS) else [r]):
            flips, cap = int((dist[:n] != 0).sum()), int(L.MAX_DIFFER * n * cols)
            assert flips <= max(0, cap - 1), (family, cols, n, flips, cap)
        assert ref.float().abs().min().item() >= 0.5                           # no output near zero

