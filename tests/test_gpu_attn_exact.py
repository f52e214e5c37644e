"""Exact per-element tests of the flash attention kernel on the MI355X (run with -m gpu), under every
kernel form that attention.hip instantiates, each asserted to be the one that ran (``form_out``).

Inputs: tests/attn_exact_util.py.  The one-hot family must reproduce V[f(i)] bit for bit (a dropped or
doubled key, a mask off by one position, a skipped rescale or a wrong head / column chunk changes an
integer); the weighted family must be within 1 fp16 ulp of the float64 reference (it weighs the QK^T
side, every column of it).  q / k / v are strided views into NaN-filled buffers (separate, packed k|v,
packed q|k|v; NaN rows before the first and after the last batch), the output a view with row stride
heads*d + 4 inside a sentinel-filled buffer that must keep its bits everywhere else.

(form, d) -> launch<DQK, DV, waves, query blocks, stagger, seed column>, each row run and asserted below
(the causal kernels are attn_fwd_kernel<DQK, DV, waves, 1, true>: never staggered, never seeded):

  nw4       8, 16        <16, 32, 4, 1>            also causal (d = 16)
  nw4       24, 32       <32, 32, 4, 1>            also causal (d = 32); d == DV at 32: explicit row sum
  nw4       40, 48       <48, 64, 4, 1>            also causal (d = 40)
  nw4       56, 64       <64, 64, 4, 1>            also causal (d = 64)
  nw4       72, 80       <80, 96, 4, 1>            also causal (d = 80)
  nw4       96           <96, 96, 4, 1>            also causal
  nw4       128          <128, 128, 4, 1>          also causal
  nw4       152, 160     <160, 160, 4, 1>          also causal (d = 160)
  nw8       40           <48, 64, 8, 1, false, 40> causal: <48, 64, 8, 1, true>
  nw8       48           <48, 64, 8, 1>
  nw8       56, 64       <64, 64, 8, 1>            also causal (d = 64)
  nw8       72, 80       <80, 96, 8, 1>            also causal (d = 80)
  nw8_stag  40           <48, 64, 8, 1, true, 40>
  nw8_stag  48           <48, 64, 8, 1, true>
  nw8_stag  56, 64       <64, 64, 8, 1, true>
  nw8_stag  72, 80       <80, 96, 8, 1, true>
  qb2       40, 48       <48, 64, 4, 2>            no causal form
  auto      d <= 32, d > 80: nw4;  40, 48: nw8;  56 .. 80: nw8_stag

Observed on the MI355X: see ``test_attention_exact``'s docstring."""
import pytest
import torch

import attn_exact_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda"
FORMS = ("auto", "nw4", "nw8", "nw8_stag", "qb2")
PAIRS = [(d, f) for d in U.ALL_DIMS for f in FORMS if f == "auto" or d in U.FORM_DIMS[f]]
CAUSAL_FULL = (40, 64, 80)
CAUSAL_PAIRS = ([(d, f) for d in CAUSAL_FULL for f in ("nw4", "nw8", "nw8_stag", "auto")] +
                [(d, "nw4") for d in (16, 32, 96, 128, 160)])


@pytest.fixture(scope="module")
def ops(sdk):
    from sd_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return o


def _run(ops, c, layout, form):
    """Launch a case; returns (logical output on the CPU, canaries clean, form_out)."""
    q, k, v = U.guarded_qkv(c, layout, DEV)
    rows, cols = c.B * c.nq, c.H * c.d
    buf, out = U.out_buffer(rows, cols, DEV)
    info = {}
    y = ops.attention(q, k, v, batch=c.B, heads=c.H, nq=c.nq, nk=c.nk, head_dim=c.d, scale=U.SCALE, out=out,
                      causal=c.causal, form=form, form_out=info)
    assert y.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    got, clean = U.split_out(buf, rows, cols)
    return got, clean, info


def _check(c, form, layout, got, clean, info, bad):
    """Appends what is wrong with one launch to ``bad``; returns the weighted family's ulp distance."""
    want = U.expected_info(form, c.d, c.causal)
    want["grid"] = -(-c.nq // (32 * want["waves"] * want["qblocks"])) * c.H * c.B
    tag = f"{c.name} {form} {layout}"
    if info != want:
        bad.append(f"{tag}: ran {info}, the table promises {want}")
    if not clean:
        bad.append(f"{tag}: wrote outside the output's extent")
    if got.isnan().any():
        bad.append(f"{tag}: {int(got.isnan().sum())} NaN in the output")
        return None
    if c.family == "onehot":
        ne = got.view(torch.int16) != c.ref.view(torch.int16)
        if ne.any():
            r, col = (int(x) for x in ne.nonzero()[0])
            bad.append(f"{tag}: {int(ne.sum())} elements differ from V[f(i)], {int(ne.any(1).sum())} rows; first at "
                       f"row {r} (b {r // c.nq}, i {r % c.nq}) col {col}: got {got[r, col].item()}, "
                       f"want {c.ref[r, col].item()}")
        return None
    u = U.ulp_diff(got, c.ref)
    if u > 1:
        bad.append(f"{tag}: {u} fp16 ulp from the float64 reference (bound 1)")
    return u


@pytest.mark.parametrize("d,form", PAIRS, ids=[f"d{d}-{f}" for d, f in PAIRS])
def test_attention_exact(ops, d, form):
    """Both families at nk = 20 / 64 / 129 / 257 (one ragged tile, one whole tile, three tiles with a 1-key
    tail, five tiles: the third fetch(t + 2) and the wrap of the 2- and 3-stage rings), nq = ROWS + 69,
    batch 2 x heads 3 (a grid that is no multiple of 8), the negative one-hot winner at the ragged nk, nq = 5,
    a 4-block grid and packed q|k|v.  One-hot: bit-equal.  Weighted: <= 1 fp16 ulp.

    Observed (MI355X): the weighted family is NOT always bit-equal to the float64 reference's fp16.  The
    largest distance was 0 ulp at d = 8 .. 32, 56, 72 and 96 (every form; d = 40 under the 8-wave and qb2
    forms) and 1 ulp at d = 48, 64, 80, 128, 152, 160 and at d = 40 with 4 waves: the fp32 product of the
    numerator with the rounded reciprocal, rounded again to fp16, against one rounding of the quotient.  The
    bound is the derived 1 ulp either way.  The negative one-hot winner first produced NaN rows at d = 152 / 160
    and under qb2: tile 0 multiplied the zero accumulators by exp2(-m), which is inf for a first-tile maximum
    below -128 (fixed in attention.hip: tile 0 has nothing to rescale)."""
    bad, ulps = [], []
    for family, B, H, nq, nk, negative, layout in U.noncausal_specs(form, d):
        c = U.get_case(family, B, H, nq, nk, d, False, negative)
        got, clean, info = _run(ops, c, layout, form)
        u = _check(c, form, layout, got, clean, info, bad)
        if u is not None:
            ulps.append(u)
    print(f"attention exact d={d} {form}: weighted max ulp {max(ulps)}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("d,form", CAUSAL_PAIRS, ids=[f"d{d}-{f}" for d, f in CAUSAL_PAIRS])
def test_attention_exact_causal(ops, d, form):
    """nq = nk = 77 / 129 / 325 and nq != nk both ways at d = 40 / 64 / 80; the other head dims' causal
    instantiations at n = 129.  Diagonal rows win at key i with every later key (i + 1 and the next tile's
    first key included) scoring >= 64 above it; code rows win at f(i) <= i.  A staggered request runs the
    plain 8-wave causal kernel and says so (stagger 0)."""
    bad, ulps = [], []
    for family, B, H, nq, nk, layout in U.causal_specs(d, d in CAUSAL_FULL):
        c = U.get_case(family, B, H, nq, nk, d, True)
        got, clean, info = _run(ops, c, layout, form)
        u = _check(c, form, layout, got, clean, info, bad)
        if u is not None:
            ulps.append(u)
    print(f"attention exact causal d={d} {form}: weighted max ulp {max(ulps)}")
    assert not bad, "\n".join(bad)


def test_auto_runs_todays_defaults(ops):
    """``form=None`` with ``form_out``: d = 40 -> 8 waves, -m in column 40, no stagger; d = 64 and 80 ->
    staggered; d = 160 -> 4 waves (stated in literals, not through the util's table)."""
    want = {40: dict(form="nw8", dqk=48, dv=64, waves=8, qblocks=1, stagger=0, seed_col=40, causal=0, grid=12),
            64: dict(form="nw8_stag", dqk=64, dv=64, waves=8, qblocks=1, stagger=1, seed_col=0, causal=0, grid=12),
            80: dict(form="nw8_stag", dqk=80, dv=96, waves=8, qblocks=1, stagger=1, seed_col=0, causal=0, grid=12),
            160: dict(form="nw4", dqk=160, dv=160, waves=4, qblocks=1, stagger=0, seed_col=0, causal=0, grid=18)}
    for d, w in want.items():
        c = U.get_case("onehot", 2, 3, 325, 129, d)
        q, k, v = U.guarded_qkv(c, "sep", DEV)
        info = {}
        y = ops.attention(q, k, v, batch=2, heads=3, nq=325, nk=129, head_dim=d, scale=U.SCALE, form_out=info)
        assert info == w, (d, info)
        assert torch.equal(y.cpu().view(torch.int16), c.ref.view(torch.int16)), d


def test_form_without_instantiation_is_an_error(ops):
    """Every (form, d) outside the table, and qb2 with causal, raise (SDK_EINVAL) and launch nothing: the
    output keeps its sentinel."""
    for form in ("nw8", "nw8_stag", "qb2"):
        for d in U.ALL_DIMS:
            if d in U.FORM_DIMS[form]:
                continue
            x = torch.zeros(64, d, dtype=torch.float16, device=DEV)
            buf, out = U.out_buffer(64, d, DEV)
            info = {}
            with pytest.raises(RuntimeError, match=r"\(-1\).*no instantiation"):
                ops.attention(x, x, x, batch=1, heads=1, nq=64, nk=64, head_dim=d, scale=1.0, out=out, form=form,
                              form_out=info)
            torch.cuda.synchronize()
            assert info == {} and U.split_out(buf, 0, 0)[1], (form, d)
    x = torch.zeros(64, 40, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match="causal needs the one-block-per-wave form"):
        ops.attention(x, x, x, batch=1, heads=1, nq=64, nk=64, head_dim=40, scale=1.0, causal=True, form="qb2")
    with pytest.raises(KeyError):
        ops.attention(x, x, x, batch=1, heads=1, nq=64, nk=64, head_dim=40, scale=1.0, form="nw16")


def test_form_out_costs_nothing_and_survives_graph_capture(ops):
    """``form_out`` is filled from host integers before the launch: the same dict eagerly and under
    capture, and the captured launch replays to the exact result."""
    c = U.get_case("onehot", 2, 3, 325, 129, 64)
    q, k, v = U.guarded_qkv(c, "kv", DEV)
    eager = {}
    y = ops.attention(q, k, v, batch=2, heads=3, nq=325, nk=129, head_dim=64, scale=U.SCALE, form="nw8_stag",
                      form_out=eager)
    assert eager == dict(U.expected_info("nw8_stag", 64), grid=12)
    cap = {}
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        yg = ops.attention(q, k, v, batch=2, heads=3, nq=325, nk=129, head_dim=64, scale=U.SCALE, form="nw8_stag",
                           form_out=cap)
    assert cap == eager
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(yg.cpu().view(torch.int16), c.ref.view(torch.int16)) and torch.equal(y, yg)
