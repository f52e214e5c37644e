"""Exact tests of the fused GEGLU feed-forward (sdk_feed_forward / sdk_ff_pack, csrc/ff.hip) on the MI355X
(run with -m gpu).

Integer family (tests/ff_exact_util.py): every output must EQUAL the float64 reference, for every row count /
feature count the kernel branches on (one iteration, odd iteration counts, ragged last row block), with the
residual off / on / aliased to the output, b1 / b2 present or NULL and row strides (320, 320, 320) or
(328, 336, 344).  Every operand is guarded: t and res are views into NaN-filled buffers (2 rows before, 130
after, the padding columns), the output is a view into a sentinel-filled buffer of the same geometry that
must be bit-unchanged outside the payload and fully overwritten inside, and the packed blob is prefilled
with 0xFF (fp16 NaNs) and followed by a 4-KiB tail that the pack must leave alone.

Pointwise family: one-hot rows read a * gelu(g) itself over a grid of gates in [-8, 8], within the
erf-equivalent error PW_E of the float64 reference; the two-GEMM path on the same input lies within one fp16
ulp of the fused kernel."""
import ctypes as C

import pytest
import torch

import ff_exact_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda"
TAIL = 4096
B1B2 = [(True, True), (False, False), (True, False), (False, True)]


@pytest.fixture(scope="module")
def ops(sdk):
    from sd_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return o


@pytest.fixture(scope="module")
def L(ops):
    from sd_amd import _lib
    return _lib


_PACKED, _INPUT = {}, {}


def _pack(L, w1, b1, w2, F):
    """Pack through the C ABI from exact-size allocations into a 0xFF-prefilled blob + tail; returns the blob
    (tail included) after asserting the tail is untouched."""
    lib = L.lib()
    n = lib.sdk_ff_packed_bytes(U.C, F)
    assert n > 0 and n % 16 == 0
    blob = torch.full((n + TAIL,), 0xFF, dtype=torch.uint8, device=DEV)
    w1d, w2d = w1.to(DEV).contiguous(), w2.to(DEV).contiguous()
    b1d = b1.to(DEV).contiguous() if b1 is not None else None
    rc = lib.sdk_ff_pack(w1d.data_ptr(), b1d.data_ptr() if b1d is not None else None, w2d.data_ptr(),
                         blob.data_ptr(), U.C, F, None)
    torch.cuda.synchronize()
    assert rc == 0, lib.sdk_last_error()
    assert bool((blob[n:] == 0xFF).all()), "sdk_ff_pack wrote past sdk_ff_packed_bytes"
    return blob


def _packed(L, c, has_b1):
    k = (c.F, has_b1, c.name.startswith("ff-pointwise"))
    if k not in _PACKED:
        _PACKED[k] = _pack(L, c.w1, c.b1, c.w2, c.F)
    return _PACKED[k]


def _guarded(key, t, ld):
    """Read-only guarded device input, built once per module."""
    if key not in _INPUT:
        _INPUT[key] = U.guarded_rows(t, ld, DEV)
    return _INPUT[key]


def _launch(L, c, blob, res_mode, lds, b2):
    """One sdk_feed_forward call on guarded buffers; returns (output buffer, rc)."""
    t_ld, res_ld, out_ld = lds
    tag = (c.M, c.F, c.b1 is not None, c.name)
    _, tv = _guarded(("t", t_ld) + tag, c.t, t_ld)
    a = L.FfArgs()
    if res_mode == "alias":
        obuf, ov = U.out_rows(c.M, out_ld, DEV, payload=c.res.to(DEV))
        a.res, a.res_ld = ov.data_ptr(), out_ld
    else:
        obuf, ov = U.out_rows(c.M, out_ld, DEV)
        if res_mode == "res":
            _, rv = _guarded(("res", res_ld) + tag, c.res, res_ld)
            a.res, a.res_ld = rv.data_ptr(), res_ld
    a.t, a.out, a.packed = tv.data_ptr(), ov.data_ptr(), blob.data_ptr()
    a.b2 = b2.data_ptr() if b2 is not None else None
    a.t_ld, a.out_ld = t_ld, out_ld
    a.rows, a.channels, a.features = c.M, U.C, c.F
    rc = L.lib().sdk_feed_forward(C.byref(a), None)
    torch.cuda.synchronize()
    return obuf, rc


def _b2(c):
    return c.b2.to(DEV).contiguous() if c.b2 is not None else None      # an exact-size allocation


@pytest.mark.parametrize("ld", list(U.FF_LDS))
@pytest.mark.parametrize("has_b1,has_b2", B1B2)
@pytest.mark.parametrize("res_mode", U.FF_RES)
@pytest.mark.parametrize("M,F", U.FF_SHAPES)
def test_feed_forward_exact(L, M, F, res_mode, has_b1, has_b2, ld):
    c = U.ff_case(M, F, has_b1, has_b2)
    obuf, rc = _launch(L, c, _packed(L, c, has_b1), res_mode, U.FF_LDS[ld], _b2(c))
    assert rc == 0, L.lib().sdk_last_error()
    got, dirty, unwritten = U.split_rows(obuf, M)
    rep = U.mismatch_report(f"{c.name} res={res_mode} ld={U.FF_LDS[ld]}", got.float(), c.ref[res_mode != "none"].float(),
                            where=U.ff_where)
    assert rep is None, rep
    assert dirty == 0, f"{c.name}: {dirty} cells outside the output's {M} x 320 payload were written"
    assert unwritten == 0


def test_feed_forward_exact_is_deterministic(L):
    c = U.ff_case(300, 1280, True, True)
    blob, b2 = _packed(L, c, True), _b2(c)
    a, _ = _launch(L, c, blob, "res", U.FF_LDS["strided"], b2)
    b, _ = _launch(L, c, blob, "res", U.FF_LDS["strided"], b2)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert torch.equal(_pack(L, c.w1, c.b1, c.w2, c.F), blob)


def test_pack_writes_every_byte_it_owns(L):
    """No 16-bit word of the blob keeps the 0xFF prefill: the W1 / W2 chunks hold small fp16 integers and the b1
    piece small fp32 integers, none of which has a 0xFFFF half."""
    c = U.ff_case(33, 96, True, True)
    blob = _packed(L, c, True)
    n = blob.numel() - TAIL
    words = blob[:n].view(torch.int16)
    assert int((words == -1).sum()) == 0


def _fused_pointwise(L, c):
    obuf, rc = _launch(L, c, _packed(L, c, True), "none", U.FF_LDS["strided"], None)
    assert rc == 0, L.lib().sdk_last_error()
    got, dirty, unwritten = U.split_rows(obuf, c.M)
    assert dirty == 0 and unwritten == 0
    return got


def _where_pw(c):
    return lambda m, ch: U.ff_where(m, ch, feature=int(c.feat[ch])) + f"; a {c.a[m, ch].item()}, g {c.g[m, ch].item()}"


def test_pointwise_gelu_within_the_measured_erf_error(L):
    """out[m, c] = fp16(a gelu(g)) against a 0.5 g (1 + erf(g / sqrt 2)) in float64: within |a| 0.5 |g| PW_E plus
    half an fp16 ulp.  PW_E is twice the E measured on the MI355X (profiles/ff_exact_gelu_errors.txt)."""
    c = U.pointwise_case()
    got = _fused_pointwise(L, c).double()
    E, g, a, ulps, gu, au = U.pointwise_measure(c, got)
    print(f"[ff pointwise] erf-equivalent E {E:.4e} at g = {g}, a = {a}; worst error {ulps:.3f} fp16 ulps of "
          f"a gelu(g) at g = {gu}, a = {au}; asserted E {U.PW_E:.4e}", flush=True)
    one = c.a.abs() == 1
    u1 = ((got - c.ref).abs() / U.fp16_ulp(c.ref)) * one
    print(f"[ff pointwise] |a| = 1: worst error {u1.max().item():.3f} fp16 ulps of gelu(g) at g = "
          f"{c.g.flatten()[int(u1.argmax())].item()}", flush=True)
    for lo, hi in ((-8, -6), (-6, -4), (-4, -2), (-2, 0), (0, 8)):
        sel = (c.g >= lo) & (c.g < hi) if hi < 8 else (c.g >= lo)
        err = (got - c.ref).abs()
        print(f"[ff pointwise]   g in [{lo}, {hi}{')' if hi < 8 else ']'}: worst {(err / U.fp16_ulp(c.ref))[sel].max().item():.3f} "
              f"ulps, worst |error| / |a| {(err / c.a.abs())[sel].max().item():.3e}", flush=True)
    assert U.PW_E < 1e-6
    rep = U.mismatch_report(c.name, got, c.ref, where=_where_pw(c), tol=U.pointwise_tolerance(c, U.PW_E))
    assert rep is None, rep


def test_pointwise_two_gemm_path_within_one_ulp(ops, L):
    """The GEGLU GEMM + output GEMM on the pointwise input: no summation to reorder, so it lies within one fp16
    ulp of the fused kernel (both round a gelu(g) once; their fp32 products may differ in the last bit)."""
    c = U.pointwise_case()
    fused = _fused_pointwise(L, c)
    dev = torch.device(DEV)
    pc1 = ops.PackedConv([(c.w1.float(), U.C)], c.b1, geglu=True, device=dev)
    pc2 = ops.PackedConv([(c.w2.float(), c.F)], None, device=dev)
    two = ops.linear(pc2, ops.linear(pc1, c.t.to(DEV), out_mode=ops.OUT_GEGLU_F16)).cpu()
    d = (two.double() - fused.double()).abs()
    ulp = U.fp16_ulp(torch.maximum(two.double().abs(), fused.double().abs()))
    print(f"[ff pointwise] fused vs two GEMMs: {int((two != fused).sum())} of {two.numel()} elements unequal, "
          f"worst {(d / ulp).max().item():.2f} ulp", flush=True)
    rep = U.mismatch_report("two-GEMM path vs fused", two.double(), fused.double(), where=_where_pw(c), tol=ulp)
    assert rep is None, rep
