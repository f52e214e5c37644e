"""Exact tests of the GroupNorm statistics on the MI355X, one per route the host plan picks (run with -m gpu).

Part A: every route of csrc/norm.hip to (scale, shift) — gn_stats_fused_kernel<false|true>, gn_partial_kernel +
gn_finalize_kernel, gn_finalize_part_kernel, gn_apply_part_kernel — on integer data whose pivot-shifted fp32 sums
are exact, against an exact-sum float64 reference under the bounds derived in tests/gn_stats_exact_util.py (three
fp32 roundings).  Part B: the per-chunk (mean, M2) the convs emit, chunk by chunk, on selector convs whose stored
output is a known small integer.  Every case first asserts the plan, so a case that stops exercising its route fails
instead of passing on another one.  Sources are views into NaN-filled buffers, outputs views into sentinel-filled
ones.  The largest error / bound ratios are printed (``[gn-exact]`` lines; profiles/gn_stats_exact_errors.txt)."""
import ctypes as C

import pytest
import torch

import conv_exact_util as U
import gn_stats_exact_util as G
from test_gpu_conv_exact import INLAUNCH_VARIANTS
from test_gpu_kernels import GLDS_VARIANTS

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT16 = U.SENTINEL


@pytest.fixture(scope="module")
def ops(sdk):
    from sd_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return o


# --------------------------------------------------------------------------- Part A

def _device_sources(case, x):
    """The sources as views into NaN-filled buffers (ld0 != ld1, both > C), and the buffers."""
    srcs = G.sources(case, x)
    views = [U.guarded_nhwc(s, s.shape[-1] + (24, 40)[i], DEV) for i, s in enumerate(srcs)]
    return views[0] if len(views) == 1 else tuple(views)


def _attach(ops, src, parts):
    for t, p in zip(src if isinstance(src, tuple) else (src,), parts):
        setattr(t, ops.GN_ATTR, (p.to(DEV).contiguous(), p.shape[1], t._version))


def _guarded(B, Cc):
    buf = torch.full((B + 2, Cc), G.SENT32, dtype=torch.float32, device=DEV)
    return buf, buf[1:B + 1]


def _run(ops, case, src, gamma, beta, eps):
    """One call of the case's entry point with (scale, shift) and y inside sentinel-filled buffers (the C entry the
    ops wrapper of that name calls, with the wrapper's own argument block: the wrappers allocate their outputs
    themselves).  Returns (scale, shift, y or None, guards clean)."""
    B, H, W, Cc, pad = case.B, case.H, case.W, case.C, case.pad
    g = gamma.to(DEV) if gamma is not None else torch.ones(Cc, device=DEV)
    b = beta.to(DEV) if beta is not None else torch.zeros(Cc, device=DEV)
    args, shape, _, _ = ops._gn_args(src, g, b, eps, case.groups)
    assert shape == (B, H, W, Cc)
    if gamma is None:
        args.gamma = args.beta = None
    sbuf, scale = _guarded(B, Cc)
    hbuf, shift = _guarded(B, Cc)
    args.scale, args.shift = scale.data_ptr(), shift.data_ptr()
    p0, n0, p1, n1 = ops._producer_parts(src)
    assert (n0, n1) == (case.nch or (0, 0)), "the partials the case attached are the ones the call sees"
    lib, y, ybuf = ops.lib(), None, None
    if case.entry == "affine":
        ops.check(lib.sdk_group_norm_affine(C.byref(args), ops._stream()), "group_norm_affine")
    elif case.entry == "scale_shift":
        ops.check(lib.sdk_group_norm_finalize(C.byref(args), ops._ptr(p0), n0, ops._ptr(p1), n1, ops._stream()),
                  "group_norm_finalize")
    else:
        # a sentinel image before and after the batch and 8 sentinel columns after every pixel's channels (ld_y > C)
        ybuf = torch.full((B + 2, H + 2 * pad, W + 2 * pad, Cc + 8), SENT16, dtype=torch.float16, device=DEV)
        y = ybuf[1:B + 1, :, :, :Cc]
        ops.check(lib.sdk_group_norm(C.byref(args), 0, ops._ptr(y), Cc + 8, H, W, pad, ops._ptr(p0), n0, ops._ptr(p1),
                                     n1, ops._stream()), "group_norm")
    torch.cuda.synchronize()
    clean = all(bool((t[0] == G.SENT32).all()) and bool((t[-1] == G.SENT32).all()) for t in (sbuf, hbuf))
    if ybuf is not None:
        clean = (clean and bool((ybuf[0] == SENT16).all()) and bool((ybuf[-1] == SENT16).all()) and
                 bool((ybuf[..., Cc:] == SENT16).all()))
    return scale, shift, y, clean


def _plan_of(ops, case, src):
    return ops.group_norm_plan(src, groups=case.groups, pad=case.pad, apply=case.want_apply,
                               parts=case.nch if case.nch else 0)


_WORST = {}


def _note(route, rs, rh):
    w = _WORST.setdefault(route, [0.0, 0.0])
    w[0], w[1] = max(w[0], rs), max(w[1], rh)


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    """One line per route and emitter after the module ran: the largest error / bound ratio seen."""
    yield
    for route, (a, b) in sorted(_WORST.items()):
        print(f"\n[gn-exact] {route}: largest error / bound {a:.3f} (scale or mean), {b:.3f} (shift or M2)", flush=True)


def _check_y(case, x, ref, y, what, exempt=False):
    """The applied output: within 1 fp16 ulp of the float64 value rounded once — on every element, or, for a
    (family, eps) of G.ULP_EXEMPT (``exempt``), on every element whose E is below half an ulp — and always inside
    [fp16(y64 - E), fp16(y64 + E)], with a zero border."""
    lo, hi, single = ref.y_interval(x, case)
    got = y.cpu()
    assert got.shape == lo.shape
    bad = ~((got.float() >= lo.float()) & (got.float() <= hi.float()))        # NaN and the sentinel are outside
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.numel()} outputs outside the interval; first at "
                           f"{bad.nonzero()[0].tolist()}: got {got[bad][0].item()} want [{lo[bad][0].item()}, "
                           f"{hi[bad][0].item()}]")
    if case.pad:
        p = case.pad
        border = torch.ones(case.H + 2 * p, case.W + 2 * p, dtype=torch.bool)
        border[p:-p, p:-p] = False
        assert torch.count_nonzero(got[:, border].float()) == 0, f"{what}: the border is not zero"
    dist = (_ordered(got) - _ordered(ref.y_once)).abs()
    must = ref.y_tight if exempt else torch.ones_like(ref.y_tight)
    far = (dist > 1) & must
    assert not far.any(), (f"{what}: {int(far.sum())} of {int(must.sum())} outputs more than 1 fp16 ulp from the float64 "
                           f"value rounded once; first at {far.nonzero()[0].tolist()}: got {got[far][0].item()} want "
                           f"{ref.y_once[far][0].item()} ({int(dist[far][0])} ulp)")
    print(f"[gn-exact] {what}: y at most {int(dist.max())} fp16 ulp from float64 rounded once"
          f"{f' (exempt pair: 1 ulp asserted on {100 * must.double().mean().item():.1f} % of the elements)' if exempt else ''}"
          f"; {100 * single:.2f} % of the intervals are one fp16 value", flush=True)


def _ordered(h):
    """fp16 tensor -> integers whose difference counts fp16 units in the last place."""
    i = h.contiguous().view(torch.int16).int()
    return torch.where(i < 0, -(i & 0x7fff), i)


@pytest.mark.parametrize("family", G.FAMILIES)
@pytest.mark.parametrize("case", G.CASES, ids=[c.name for c in G.CASES])
def test_group_norm_statistics_exact(ops, case, family):
    """One route of the host plan on one data family, at eps 1e-6 / 1e-5 / 0.25 with the hashed affine and once with
    gamma = beta = NULL (the spike family once per rotation of its positions through the batch): the plan, then
    (scale, shift) within the three-rounding bounds, then — where the case applies — y within 1 fp16 ulp of the
    float64 value rounded once, a zero border and untouched guards.  The one exception to the 1-ulp bound is the
    enumerated G.ULP_EXEMPT (offset and constant at every eps, spike at eps <= 1e-5), where an fp32 affine cannot meet
    it (tests/gn_stats_exact_util.py): there it holds on the elements whose error bound is below half an ulp, and the
    interval on all."""
    gamma, beta = G.affine_params(case)
    route = f"{case.stats}/{case.apply_form}"
    runs = [(rot, eps, False) for rot in (G.spike_rounds(case) if family == "spike" else [0]) for eps in G.EPS]
    runs.append((0, 1e-5, True))                                  # gamma = beta = NULL
    src_of = {}
    for rot, eps, null in runs:
        x = G.data(case, family, rot)
        if rot not in src_of:
            src = _device_sources(case, x)
            parts = G.case_partials(case, x) if case.nch else None
            if parts:
                _attach(ops, src, parts)
            src_of[rot] = (src, parts)
        src, parts = src_of[rot]
        assert _plan_of(ops, case, src) == case.plan              # the route, before any number
        gm, bt = (None, None) if null else (gamma, beta)
        ref = G.reference(case, x, eps, gm, bt, parts)
        scale, shift, y, clean = _run(ops, case, src, gm, bt, eps)
        what = f"{case.name} {family} rot {rot} eps {eps}{' null affine' if null else ''}"
        assert clean, f"{what}: wrote outside (scale, shift) or y"
        in_lds = case.stats == "slice" and case.apply_form == "in_stats"     # the affine may stay in the workgroup
        if not (in_lds and bool((scale == G.SENT32).all()) and bool((shift == G.SENT32).all())):
            rs, rh = ref.ratios(scale, shift)
            _note(route, rs, rh)
            assert rs <= 1.0 and rh <= 1.0, f"{what}: (scale, shift) off by {rs:.3g} / {rh:.3g} of the bound"
            if family == "constant":                              # variance 0: gamma / sqrt(eps), nothing NaN or Inf
                want = (1.0 if gm is None else gm.double()) / float(torch.tensor(eps, dtype=torch.float32)) ** 0.5
                assert ((scale.double().cpu() - want).abs() <= ref.bound_scale).all()
        if y is None:
            continue
        _check_y(case, x, ref, y, what, exempt=(family, eps) in G.ULP_EXEMPT)
        if in_lds and not null:
            # the same bits as group_norm_apply on the affine of the statistics-only route
            aff = ops.group_norm_affine(src, gamma.to(DEV), beta.to(DEV), eps, case.groups)
            rs, rh = ref.ratios(*aff)
            _note("slice/none", rs, rh)
            assert rs <= 1.0 and rh <= 1.0, f"{what}: the statistics-only affine is off"
            two = ops.group_norm_apply(src, aff, silu=False, pad=case.pad)
            assert torch.equal(y, two), f"{what}: differs from affine + apply"


def _parts_case(ops, name, family="hashed"):
    case = G.CASE[name]
    x = G.data(case, family)
    src = _device_sources(case, x)
    return case, x, src


@pytest.mark.parametrize("name", ["parts-16x16-c64-n16", "papply-16x16-c64-n2-pad1"])
def test_partials_are_followed_not_recomputed(ops, name):
    """Partials that deliberately describe OTHER data than the tensor holds: the result follows the partials, so no
    statistics pass ran.  Then the staleness rule: after an in-place edit the result follows the tensor."""
    case, x, src = _parts_case(ops, name)
    other = G.data(case, "offset")
    parts = G.case_partials(case, other)
    _attach(ops, src, parts)
    gamma, beta = G.affine_params(case)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    assert _plan_of(ops, case, src) == case.plan
    ref_parts = G.reference(case, other, 1e-5, gamma, beta, parts)
    ref_own = G.reference(case, x, 1e-5, gamma, beta)
    assert (ref_parts.scale - ref_own.scale).abs().min().item() > 1e-2 * ref_own.scale.abs().max().item()
    if case.want_apply:
        y = ops.group_norm(src, gd, bd, 1e-5, case.groups, silu=False, pad=case.pad)
        _check_y(case, x, ref_parts, y, f"{name}: follows the partials")
    else:
        sc, sh = ops.group_norm_scale_shift(src, gd, bd, 1e-5, case.groups)
        assert max(ref_parts.ratios(sc, sh)) <= 1.0, f"{name}: does not follow the partials"
    src.add_(0)                                                   # same values, the version counter moved
    stale = dict(case.plan, stats="slice", apply="flat" if case.want_apply else "none",
                 launches=2 if case.want_apply else 1)
    assert ops.group_norm_plan(src, groups=case.groups, pad=case.pad, apply=case.want_apply) == stale
    if case.want_apply:
        y = ops.group_norm(src, gd, bd, 1e-5, case.groups, silu=False, pad=case.pad)
        _check_y(case, x, ref_own, y, f"{name}: stale partials")
    else:
        sc, sh = ops.group_norm_scale_shift(src, gd, bd, 1e-5, case.groups)
        assert max(ref_own.ratios(sc, sh)) <= 1.0, f"{name}: used stale partials"


# --------------------------------------------------------------------------- Part B

EMITTING = ["auto"] + [str(v) for v in sorted(GLDS_VARIANTS | {8, 9})]
_SEL = {}


def _sel(ops, name, B, H, W, cin, cout, k, epilogue=True):
    """A selector conv (its exact reference, guarded device inputs, packed weights), built once."""
    if name not in _SEL:
        c = U.Case(f"sel-{name}", **G.selector_conv(name, B, H, W, cin, cout, k, epilogue))
        assert c.ref.abs().max().item() <= 16
        d = {"x": U.guarded_nhwc(c.srcs[0], cin + 24, DEV), "pc": ops.PackedConv([(c.w, cin)], c.bias, device=DEV)}
        if epilogue:
            d["row_bias"] = (c.row_bias[0].to(DEV), c.row_bias[1])
            d["residual"] = U.guarded_residual(c.residual, cout + 16, DEV)
        _SEL[name] = (c, d)
    return _SEL[name]


def _emit(ops, c, d, variant, split_k):
    """Run with gn_stats (statistics attach only to an output as wide as Cout: a plain tensor); returns
    (y on the device, plan, partials [B, nch, Cout, 2], nch)."""
    plan = {}
    y = ops.conv2d(d["pc"], d["x"], ksize=c.ksize, pad=c.pad, row_bias=d.get("row_bias"), residual=d.get("residual"),
                   variant=None if variant == "auto" else int(variant), split_k=split_k, gn_stats=True, plan_out=plan)
    torch.cuda.synchronize()
    part = getattr(y, ops.GN_ATTR, None)
    assert part is not None and plan["gn_chunks"] > 0, f"{c.name} variant {variant}: plan {plan} should emit statistics"
    pp, nch, _ = part
    assert nch == plan["gn_chunks"] and pp.shape == (c.out_shape[0], nch, c.cout, 2)
    U.assert_exact(c, y.float().cpu(), plan)
    return y, plan, pp, nch


def _note_chunks(route, rm, rq):
    w = _WORST.setdefault(f"emitter {route}", [0.0, 0.0])
    w[0], w[1] = max(w[0], rm), max(w[1], rq)


def _finalize_emitted(ops, ys, hw, groups, what, single=None):
    """group_norm_scale_shift on the emitted partials (and group_norm where ``single`` = (H, W) names a case of the
    single-launch form) against the float64 merge of those same fp32 partials, under Part A's bounds."""
    parts = [getattr(t, ops.GN_ATTR)[0].cpu() for t in ys]
    Cc = sum(p.shape[2] for p in parts)
    src = ys[0] if len(ys) == 1 else tuple(ys)
    s = G.seed_of(what)
    gamma = (0.5 + G.hashed(s, 1, Cc, 1 << 20)[0].double() / (1 << 20)).float()
    beta = (G.hashed_ints(s + 1, 1, Cc, -(1 << 20), 1 << 20)[0].double() / (1 << 20)).float()
    for eps in G.EPS:
        ref = G.Affine(*G.merge_partials(parts, hw, groups), eps, gamma, beta, Cc // groups, amax=16.0)
        plan = ops.group_norm_plan(src, groups=groups, apply=False)
        assert plan == {"stats": "parts", "apply": "none", "launches": 1, "workspace_bytes": 0}, plan
        sc, sh = ops.group_norm_scale_shift(src, gamma.to(DEV), beta.to(DEV), eps, groups)
        rs, rh = ref.ratios(sc, sh)
        _note("parts/none (emitted)", rs, rh)
        assert rs <= 1.0 and rh <= 1.0, f"{what} eps {eps}: finalize of the emitted partials off by {rs:.3g} / {rh:.3g}"
        if single is not None:
            H, W = single
            plan = ops.group_norm_plan(src, groups=groups, pad=1)
            assert plan == {"stats": "parts", "apply": "in_stats", "launches": 1, "workspace_bytes": 0}, plan
            y = ops.group_norm(src, gamma.to(DEV), beta.to(DEV), eps, groups, silu=False, pad=1)
            x = torch.cat([t.cpu().reshape(t.shape[0], hw, -1) for t in ys], -1).long()
            yc = G.GnCase(what, "group_norm", x.shape[0], H, W, [Cc], ("parts", "in_stats", 1), groups=groups, pad=1,
                          nch=(1, 0))
            _check_y(yc, x, ref, y, f"{what} eps {eps}: single launch")


@pytest.mark.parametrize("k", [3, 1], ids=["3x3", "1x1"])
@pytest.mark.parametrize("variant", EMITTING)
def test_tile_epilogue_statistics_exact(ops, variant, k):
    """B = 2, 16x16 (256 rows per image), Cin 64 -> Cout 328 (a ragged last N tile for every BN): one chunk per
    M-tile.  A 128-row tile is at most 8 blocks, a 256-row tile 16: s = 8 * TBM / 16."""
    c, d = _sel(ops, f"tile-k{k}", 2, 16, 16, 64, 328, k)
    y, plan, pp, nch = _emit(ops, c, d, variant, 1)
    if variant != "auto":
        assert plan["variant"] == int(variant), plan
    assert plan["split_k"] == 1, plan
    tbm = U.TILE[plan["variant"]][0]
    assert nch == 256 // tbm, plan
    rm, rq = G.check_chunk_stats(pp, y, G.tile_s(tbm), what=f"tile epilogue variant {plan['variant']} {k}x{k}")
    _note_chunks(f"tile epilogue {tbm}-row", rm, rq)
    if variant in ("auto", "2", "4"):
        _finalize_emitted(ops, [y], 256, 8, f"tile-{variant}-k{k}-g8")                     # cg 41
        _finalize_emitted(ops, [y], 256, 41, f"tile-{variant}-k{k}-g41", single=(16, 16))  # cg 8: slices of 8 channels


@pytest.mark.parametrize("split", [2, 3])
@pytest.mark.parametrize("H,W", [(16, 16), (12, 14)], ids=["16x16", "12x14"])
def test_split_k_reduce_statistics_exact(ops, H, W, split):
    """16x16: 4 chunks of 64 rows (2 rows per row lane).  12x14: one chunk of 168 rows, the 32 row lanes hold 6 or 5:
    a Chan merge of unequal counts.  s = 4 + 8 * 31: the lane's own pair, then 31 sequential merges."""
    c, d = _sel(ops, f"split-{H}x{W}", 2, H, W, 64, 328, 3)
    y, plan, pp, nch = _emit(ops, c, d, "auto", split)
    assert plan["split_k"] == split and nch == (4 if H * W % 64 == 0 else 1), plan
    rm, rq = G.check_chunk_stats(pp, y, G.REDUCE_S, what=f"split-K {split} reduce {H}x{W}")
    _note_chunks("split-K reduce", rm, rq)
    _finalize_emitted(ops, [y], H * W, 8, f"split{split}-{H}x{W}-g8")


@pytest.mark.parametrize("variant", INLAUNCH_VARIANTS)
def test_inlaunch_split_k_statistics_exact(ops, variant):
    """split_k = -2: the two K halves combine inside the launch and the combining tile emits, like an unsplit tile."""
    c, d = _sel(ops, "tile-k3", 2, 16, 16, 64, 328, 3)
    y, plan, pp, nch = _emit(ops, c, d, str(variant), -2)
    assert plan["variant"] == variant and plan["split_k"] == 2, plan
    tbm = U.TILE[variant][0]
    assert nch == 256 // tbm, plan
    rm, rq = G.check_chunk_stats(pp, y, G.tile_s(tbm), what=f"in-launch split-K variant {variant}")
    _note_chunks(f"in-launch split-K {tbm}-row", rm, rq)
    torch.cuda.synchronize()
    assert int(ops.WORKSPACE.counters(DEV).abs().sum().item()) == 0


def test_concat_of_two_producers_finalizes_exactly(ops):
    """cat(h, skip) at 16x16: h from a split-K reduce (4 chunks of 64 rows), skip from an M-tile epilogue (1 or 2
    chunks): different chunkings merged per source, then across the concat's groups."""
    ch, dh = _sel(ops, "cat-h", 2, 16, 16, 64, 640, 3)
    cs, ds = _sel(ops, "cat-skip", 2, 16, 16, 64, 320, 1, epilogue=False)
    h, plan_h, ph, nh = _emit(ops, ch, dh, "auto", 2)
    skip, plan_s, ps, ns = _emit(ops, cs, ds, "22", 1)
    assert plan_h["split_k"] == 2 and nh == 4 and plan_s["variant"] == 22 and ns == 256 // U.TILE[22][0] != nh
    G.check_chunk_stats(ph, h, G.REDUCE_S, what="concat: split-K producer")
    G.check_chunk_stats(ps, skip, G.tile_s(U.TILE[22][0]), what="concat: M-tile producer")
    _finalize_emitted(ops, [h, skip], 256, 32, "concat-two-producers", single=(16, 16))
