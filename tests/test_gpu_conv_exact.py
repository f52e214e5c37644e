"""Exact per-element tests of the implicit-GEMM conv / token GEMM on the MI355X (run with -m gpu).

Integer-valued inputs (tests/conv_exact_util.py) make every fp32 accumulation order and every fp16
rounding exact, so each output must EQUAL the float64 CPU reference element for element, under every
tile variant, split-K scheme and tile order.  Every case also
  * reads back the launched plan (``plan_out``) and asserts it by build_params' honoured-variant rule:
    a forced tile variant runs when the operand is transform-free (and the variant GEGLU-capable for a
    GEGLU output), otherwise the plan is variant 0 (or, for GEGLU, a capable one); a passed split_k is
    the reported one;
  * reads its sources and residual out of NaN-filled buffers (an image of NaN rows before and after,
    NaN in the channel gap ld > cin), so a read of an element the conv does not own poisons an output;
  * writes through ``out=`` into a sentinel-filled buffer wider than Cout with one extra image, which
    must be bit-unchanged outside the output's logical extent."""
import contextlib

import pytest
import torch

import conv_exact_util as U
from test_gpu_inlaunch_splitk import TILE_VARIANTS

pytestmark = pytest.mark.gpu
DEV = "cuda"
INLAUNCH_VARIANTS = tuple(TILE_VARIANTS) + (38, 40)      # build_params accepts the 8-wave tiles too


@pytest.fixture(scope="module")
def ops(sdk):
    from sd_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return o


@contextlib.contextmanager
def _forced(ops, variant):
    """ops.linear has no ``variant`` keyword: force through the module switch, as ``conv_variant`` does."""
    old = ops.FORCE_VARIANT
    ops.FORCE_VARIANT = variant
    try:
        yield
    finally:
        ops.FORCE_VARIANT = old


_DEVICE = {}


def _device_case(ops, c):
    """Guarded device inputs and packed weights of a case, built once (per case, not per variant)."""
    d = _DEVICE.get(c.name)
    if d is not None:
        return d
    d = {}
    lds = (24, 40)                                         # channel gaps: ld0 != ld1
    d["x"] = [U.guarded_nhwc(s, s.shape[-1] + lds[i], DEV) for i, s in enumerate(c.srcs)]
    if c.srcs2 is not None:
        d["x2"] = [U.guarded_nhwc(s, s.shape[-1] + lds[1 - i], DEV) for i, s in enumerate(c.srcs2)]
    if c.per_image:
        nb, N, K = c.w.shape
        w = torch.zeros(nb, -(-N // 128) * 128, K, dtype=torch.float16)
        w[:, :N] = c.w.half()
        d["pc"] = ops.PerImageWeights(w.to(DEV), N, c.bias.to(DEV))
    else:
        segs = [(c.w, c.w.shape[1])]
        if c.srcs2 is not None:
            segs.append((c.w2, c.w2.shape[1]))
        d["pc"] = ops.PackedConv(segs, c.bias, geglu=c.geglu, device=DEV)
    if c.gn is not None:
        d["gn"] = (c.gn[0].to(DEV).contiguous(), c.gn[1].to(DEV).contiguous())
    if c.row_bias is not None:
        d["row_bias"] = (c.row_bias[0].to(DEV), c.row_bias[1])
    if c.residual is not None:
        d["residual"] = U.guarded_residual(c.residual, c.nout + 16, DEV)
    _DEVICE[c.name] = d
    return d


def _src(xs):
    return xs[0] if len(xs) == 1 else tuple(xs)


def _run(ops, c, forced, split_k=None):
    """Launch the case; returns (logical output on the CPU, canaries clean, plan)."""
    d = _device_case(ops, c)
    buf, out = U.out_buffer(c, DEV)
    plan = {}
    variant = None if forced == "auto" else int(forced)
    if c.api == "linear":
        assert split_k is None and c.gn is None
        B, H, _, K = c.srcs[0].shape
        x2d = d["x"][0].as_strided((B * H, K), (d["x"][0].stride(1), 1))
        res = d.get("residual")
        with _forced(ops, variant):
            y = ops.linear(d["pc"], x2d, silu=c.silu, residual=None if res is None else res.view(B * H, -1),
                           out_mode=c.out_mode, out=out.view(B * H, -1), n_img=H if c.per_image else None,
                           plan_out=plan)
    else:
        seg2 = None if c.srcs2 is None else (_src(d["x2"]), None, False)
        y = ops.conv2d(d["pc"], _src(d["x"]), ksize=c.ksize, stride=c.stride, pad=c.pad, pad_end=c.pad_end,
                       upsample=c.upsample, gn=d.get("gn"), silu=c.silu, seg2=seg2, row_bias=d.get("row_bias"),
                       residual=d.get("residual"), out_mode=c.out_mode, out=out, variant=variant, split_k=split_k,
                       plan_out=plan)
    assert y.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    got, clean = U.split_out(c, buf)
    return got, clean, plan


def _params(cases):
    return [pytest.param(n, v, id=f"{n}-{v}") for n in cases for v in U.variants_of(n)]


@pytest.mark.parametrize("name,forced", _params(U.CONV_CASES))
def test_conv_exact(ops, name, forced):
    """Cases A-G and I-N (conv_exact_util._build says what each one pins)."""
    c = U.get_case(name)
    got, clean, plan = _run(ops, c, forced)
    U.check_plan(c, forced, plan)
    if name == "I":
        assert plan["split_k"] == 1, plan                 # Cout % 8 != 0 cannot split
    U.assert_exact(c, got, plan)
    assert clean, f"{name} forced {forced}: wrote outside the output's extent; plan {plan}"


@pytest.mark.parametrize("name,forced", _params(U.SPLIT_CASES))
def test_token_gemm_exact_under_every_split(ops, name, forced):
    """Case H: M = 300, K = 1280, N = 648 with bias and residual, split_k 1 / 2 / 4 (fp32 slabs + reduce)
    and -2 (combined in the launch; LDS-DMA tile variants only): each equals the reference, reports the
    requested split, and all have identical bits."""
    c = U.get_case(name)
    outs = []
    for sp in U.SPLITS:
        if sp == -2 and (forced == "auto" or int(forced) not in INLAUNCH_VARIANTS):
            continue
        got, clean, plan = _run(ops, c, forced, split_k=sp)
        U.check_plan(c, forced, plan, split_k=sp)
        U.assert_exact(c, got, plan)
        assert clean, f"{name} forced {forced} split_k {sp}: wrote outside the output's extent; plan {plan}"
        outs.append(got)
    assert len(outs) >= 3 and all(torch.equal(o, outs[0]) for o in outs[1:])
    torch.cuda.synchronize()
    assert int(ops.WORKSPACE.counters(DEV).abs().sum().item()) == 0


@pytest.mark.parametrize("forced", [v for v in U.VARIANT_IDS if v != "auto"])
def test_tile_order_groups_exact(ops, forced):
    """Case E unsplit under tile groups of 2 M-panels (sdk_conv_args.tile_group_m): its three 128-row
    panels make one full group and a shorter last one, its two 256-row panels one group; every tile is
    still computed once and lands in its place."""
    c = U.get_case("E")
    ops.TILE_GROUP_M = 2
    try:
        got, clean, plan = _run(ops, c, forced, split_k=1)
    finally:
        ops.TILE_GROUP_M = None
    U.check_plan(c, forced, plan, split_k=1)
    U.assert_exact(c, got, plan)
    assert clean, f"E forced {forced}, tile groups of 2: wrote outside the output's extent; plan {plan}"


def test_per_image_weights_tile_must_divide_the_image(ops):
    """Case K's rule, stated once: a forced tile variant is honoured when its BM divides the rows of an
    image (every BM divides 256 today, so none of the 25 ids raises there); with 128 rows per image the
    256-row tiles cannot, and the plan falls back to a 128-row tile — never a tile across two images'
    weights (no tile at all is the error test_gpu_reassoc already states)."""
    c = U.get_case("K")
    w = _device_case(ops, c)["pc"].weight[:, :, :64].contiguous()
    pc = ops.PerImageWeights(w, 128)
    x = torch.zeros(3 * 128, 64, dtype=torch.float16, device=DEV)
    for v in (2, 22, 4):
        plan = {}
        with _forced(ops, v):
            ops.linear(pc, x, n_img=128, plan_out=plan)
        assert 128 % U.TILE[plan["variant"]][0] == 0 and plan["variant"] != 0, plan
    assert plan["variant"] == 4


def test_plan_out_costs_nothing_and_survives_graph_capture(ops):
    """``plan_out`` is filled from host integers before the launch: the same dict contents eagerly and
    under capture, and the captured conv replays to the exact result."""
    c = U.get_case("B")
    d = _device_case(ops, c)
    eager = {}
    y = ops.conv2d(d["pc"], d["x"][0], pad=0, variant=22, plan_out=eager)
    assert eager["variant"] == 22 and set(eager) == {"variant", "split_k", "grid_tiles", "gn_chunks"}
    cap = {}
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        yg = ops.conv2d(d["pc"], d["x"][0], pad=0, variant=22, plan_out=cap)
    assert cap == eager
    gr.replay()
    torch.cuda.synchronize()
    U.assert_exact(c, yg.float().cpu(), cap)
    assert torch.equal(y, yg)
