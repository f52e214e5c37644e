"""Exact tests of the persistent 320-channel token linear (sdk_token_linear / sdk_token_linear_ln,
csrc/token.hip) on the MI355X (run with -m gpu).

Hashed integer inputs (tests/token_exact_util.py): every output must EQUAL the float64 reference.  The row
counts follow from the device's CU count, read at run time: fewer rows than a block, ragged last blocks, a
second block for some workgroups (the it == 1 wait) and a fourth one (the it >= 2 wait and the ring wrap)
that is also the ragged last block.  Residual off / on / aliased to the output, bias or NULL, row strides
320 / 328 / 344.  x and res are views into NaN-filled buffers (2 rows before, 130 after, the padding columns);
out and out_ln are views into sentinel-filled buffers of the same geometry that must be bit-unchanged outside
the payload; w and bias are exact-size allocations."""
import ctypes as C

import pytest
import torch

import ff_exact_util as U
import token_exact_util as T
from gpu_util import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5


@pytest.fixture(scope="module")
def ops(sdk):
    from sd_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return o


@pytest.fixture(scope="module")
def L(ops):
    from sd_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def cus(ops):
    return torch.cuda.get_device_properties(0).multi_processor_count


_INPUT = {}


def _guarded(key, make):
    if key not in _INPUT:
        _INPUT[key] = make()
    return _INPUT[key]


def _weights(c, with_bias):
    w = _guarded(("w", c.w.data_ptr()), lambda: c.w.to(DEV).contiguous())
    b = _guarded(("b", c.b.data_ptr()), lambda: c.b.to(DEV).contiguous()) if with_bias else None
    return w, b


def _args(L, c, res_mode, with_bias, lds):
    """(args, output buffer, output view) of one call on guarded buffers."""
    x_ld, res_ld, out_ld = lds
    _, xv = _guarded(("x", c.M, x_ld), lambda: U.guarded_rows(c.x, x_ld, DEV))
    w, b = _weights(c, with_bias)
    a = L.TokenLinearArgs()
    if res_mode == "alias":
        obuf, ov = U.out_rows(c.M, out_ld, DEV, payload=c.res.to(DEV))
        a.res, a.res_ld = ov.data_ptr(), out_ld
    else:
        obuf, ov = U.out_rows(c.M, out_ld, DEV)
        if res_mode == "res":
            _, rv = _guarded(("res", c.M, res_ld), lambda: U.guarded_rows(c.res, res_ld, DEV))
            a.res, a.res_ld = rv.data_ptr(), res_ld
    a.x, a.w, a.out = xv.data_ptr(), w.data_ptr(), ov.data_ptr()
    a.bias = b.data_ptr() if b is not None else None
    a.x_ld, a.out_ld = x_ld, out_ld
    a.rows, a.in_features, a.out_features = c.M, U.C, U.C
    return a, obuf, ov


def _check(c, obuf, ref, G, what):
    got, dirty, unwritten = U.split_rows(obuf, c.M)
    rep = U.mismatch_report(what, got.float(), ref.float(), where=T.token_where(c.M, G))
    assert rep is None, rep
    assert dirty == 0, f"{what}: {dirty} cells outside the {c.M} x 320 payload were written"
    assert unwritten == 0
    return got


@pytest.mark.parametrize("ld", list(T.TOKEN_LDS))
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("res_mode", T.TOKEN_RES)
@pytest.mark.parametrize("kind", T.ROW_KINDS)
def test_token_linear_exact(L, cus, kind, res_mode, with_bias, ld):
    c = T.token_case(T.rows_of(kind, cus))
    a, obuf, _ = _args(L, c, res_mode, with_bias, T.TOKEN_LDS[ld])
    rc = L.lib().sdk_token_linear(C.byref(a), None)
    torch.cuda.synchronize()
    assert rc == 0, L.lib().sdk_last_error()
    _check(c, obuf, T.token_ref(c, with_bias, res_mode != "none"), cus,
           f"{c.name} ({kind}, {cus} CUs) res={res_mode} bias={with_bias} ld={T.TOKEN_LDS[ld]}")


@pytest.mark.parametrize("kind", ["33", "it3"])
def test_token_linear_exact_is_deterministic(L, cus, kind):
    c = T.token_case(T.rows_of(kind, cus))
    bufs = []
    for _ in range(2):
        a, obuf, _ = _args(L, c, "res", True, T.TOKEN_LDS["strided-a"])
        assert L.lib().sdk_token_linear(C.byref(a), None) == 0
        torch.cuda.synchronize()
        bufs.append(obuf)
    assert torch.equal(bufs[0].view(torch.int16), bufs[1].view(torch.int16))


def test_token_linear_exact_conv_weight_shape(ops, cus):
    """A [320, 320, 1, 1] conv weight packs to the same exact-size [320, 320] allocation."""
    c = T.token_case(33)
    pk = ops.PackedTokenLinear(c.w.reshape(320, 320, 1, 1), c.b, torch.device(DEV))
    assert pk.w.shape == (320, 320) and pk.w.is_contiguous() and torch.equal(pk.w.cpu(), c.w)
    _, xv = _guarded(("x", c.M, 328), lambda: U.guarded_rows(c.x, 328, DEV))
    obuf, ov = U.out_rows(c.M, 344, DEV, payload=c.res.to(DEV))
    ops.token_linear(pk, xv, residual=ov, out=ov)
    torch.cuda.synchronize()
    _check(c, obuf, T.token_ref(c, True, True), cus, "token-M33 through ops.token_linear, conv weight")


@pytest.mark.parametrize("ln_ld", [320, 336])
@pytest.mark.parametrize("res_mode", ["none", "res"])
@pytest.mark.parametrize("kind", T.ROW_KINDS)
def test_token_linear_ln_exact(ops, L, cus, kind, res_mode, ln_ld):
    """norm= form: out equals float64 bit for bit, out_ln is bitwise ops.layer_norm(out) and within 2e-3
    rel-L2 of the float64 LayerNorm; both outputs guarded."""
    c = T.token_case(T.rows_of(kind, cus))
    g = torch.Generator().manual_seed(5)
    gamma, beta = 1 + 0.1 * torch.randn(320, generator=g), 0.1 * torch.randn(320, generator=g)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    lds = T.TOKEN_LDS["strided-b" if ln_ld == 336 else "dense"]
    a, obuf, ov = _args(L, c, res_mode, True, lds)
    lbuf, lv = U.out_rows(c.M, ln_ld, DEV)
    rc = L.lib().sdk_token_linear_ln(C.byref(a), gd.data_ptr(), bd.data_ptr(), EPS, lv.data_ptr(), ln_ld, None)
    torch.cuda.synchronize()
    assert rc == 0, L.lib().sdk_last_error()
    what = f"{c.name} ({kind}, {cus} CUs) ln res={res_mode} ld={lds} ln_ld={ln_ld}"
    ref = T.token_ref(c, True, res_mode != "none")
    _check(c, obuf, ref, cus, what)
    got_ln, dirty, unwritten = U.split_rows(lbuf, c.M)
    assert dirty == 0, f"{what}: {dirty} cells outside out_ln's payload were written"
    assert unwritten == 0
    sep = ops.layer_norm(ov, gd, bd, EPS).cpu()
    rep = U.mismatch_report(what + " out_ln vs layer_norm(out)", got_ln.float(), sep.float(), where=T.token_where(c.M, cus))
    assert rep is None, rep
    assert bool(torch.isfinite(got_ln).all())
    e = rel_l2(got_ln, T.layer_norm_ref(ref, gamma, beta, EPS))
    print(f"[token_linear_ln exact] {what}: out_ln rel-L2 vs float64 {e:.2e}", flush=True)
    assert e < 2e-3
