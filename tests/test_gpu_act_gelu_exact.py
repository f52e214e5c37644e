"""Exact tests of the GELU epilogue of the conv / token GEMM (``SDK_ACT_GELU``, csrc/conv_device.h ``act_fn``) on the
MI355X (run with -m gpu).

Inputs.  ``x`` holds small integers in column pairs (x[:, 2i] == x[:, 2i+1] == a_i in [-3, 3]); row n of ``w`` holds
(c, -c) on every pair (c in {-1, 0, 1}) except one pair s_n, where it holds (u_n, 0) with u_n = +-1; the bias is a
half-integer in [-5, 5].  Every K element takes part in the sum, every product and partial sum is an integer below
3 K < 2^24 (exact in fp32 in any order, under any split), and the pre-activation is exactly
h[m, n] = u_n a[m, s_n] + b_n: an integer or half-integer in [-8, 8].  A K element dropped or read twice moves h by an
integer.

Bound.  The kernel's fp32 gelu must lie within tol = 0.5 |h| E of gelu64(h) = 0.5 h (1 + erf(h / sqrt 2)) in float64,
with E = 2.75e-7, the erf-equivalent error tests/test_gpu_ff_exact.py asserts for ``gelu_erf``
(profiles/ff_exact_gelu_errors.txt: 1.4e-7 measured).  What the kernel stores is that value pushed through its
roundings, all monotone: fp16(g) for the fp16 output, fp16(fp16(g) + r) with the residual, g or fl32(g + r) for the fp32
rows.  So the stored value must lie between the two ends of [gelu64 - tol, gelu64 + tol] pushed through the same
roundings: the bound on top of one fp16 rounding (two with the residual), and without one for the fp32 rows.

Quick GELU in place of the exact one fails every case: at h = 1 the two differ by 4.5e-3 (nine fp16 ulps of 0.84, four
orders above the bound), at h = 2 by 2.0e-2 (profiles/act_gelu_mutation_check.txt).

Shapes.  (K, N) = (128, 512) and (1024, 4096), the OpenCLIP c_fc GEMM, have 2 and 16 K tiles: too few for a 4-way
split (the planner wants kt / 4 >= 8).  (2048, 512) has 32, so it also runs under split_k = 4: the split-K reduce's
own act_fn call, for both output modes.

Operands are views into NaN-filled buffers and the output a view into a sentinel-filled one
(tests/conv_exact_util.py)."""
import math
import zlib

import numpy as np
import pytest
import torch

import conv_exact_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda"
E_ERF = 2.75e-7

SHAPES = [(128, 512), (1024, 4096), (2048, 512)]
MS = [77, 154]


@pytest.fixture(scope="module")
def ops(sdk):
    from sd_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return o


class GeluCase:
    """One (M, K, N): CPU inputs and the float64 pre-activation, built once and left unchanged."""

    def __init__(self, M, K, N):
        self.M, self.K, self.N = M, K, N
        g = torch.Generator().manual_seed(zlib.crc32(f"act-gelu-{M}-{K}-{N}".encode()))
        P = K // 2
        a = torch.randint(-3, 4, (M, P), generator=g)
        c = torch.randint(-1, 2, (N, P), generator=g)
        s = torch.randint(0, P, (N,), generator=g)
        u = torch.randint(0, 2, (N,), generator=g) * 2 - 1
        w = torch.stack([c, -c], -1)
        w[torch.arange(N), s, 0] = u
        w[torch.arange(N), s, 1] = 0
        self.x = a.repeat_interleave(2, 1).to(torch.float16)                  # [M, K]
        self.w = w.reshape(N, K).to(torch.float32)
        self.b = torch.randint(-10, 11, (N,), generator=g).to(torch.float32) / 2
        self.r = torch.randint(-50, 51, (M, N), generator=g).to(torch.float16)
        h = self.x.double() @ self.w.double().T + self.b.double()
        closed = u.double()[None, :] * a.double()[:, s] + self.b.double()[None, :]
        if not torch.equal(h, closed):
            raise U.InexactCase("the pre-activation is not u a + b")
        if not (h.abs().max() <= 8 and torch.equal(2 * h, (2 * h).round())):
            raise U.InexactCase("the pre-activation is not a half-integer in [-8, 8]")
        if not (self.x.double().abs() @ self.w.double().abs().T).max() < 2 ** 24:
            raise U.InexactCase("a partial sum can reach 2^24")
        if not (h == 1).any():
            raise U.InexactCase("no pre-activation equals 1")
        self.h = h
        self.gelu = 0.5 * h * (1 + torch.special.erf(h / math.sqrt(2.0)))
        self.tol = 0.5 * h.abs() * E_ERF


_CASES = {}


def case(M, K, N):
    if (M, K, N) not in _CASES:
        _CASES[(M, K, N)] = GeluCase(M, K, N)
    return _CASES[(M, K, N)]


def test_cases_discriminate_quick_gelu():
    """The inputs themselves (no kernel): quick GELU lies far outside the bound wherever h = 1."""
    c = case(77, 128, 512)
    quick = c.h * torch.sigmoid(1.702 * c.h)
    at1 = c.h == 1
    assert ((quick - c.gelu).abs()[at1] > 4e-3).all()            # 0.8458 vs 0.8413
    at2 = c.h.abs() == 2
    assert at2.any() and ((quick - c.gelu).abs()[at2] > 1.5e-2).all()
    assert c.tol.max() < 1.2e-6


def _f16(t64):
    """float64 -> fp16 in one correctly rounded step (numpy), as float64."""
    return torch.from_numpy(t64.numpy().astype(np.float16).astype(np.float64))


def _stored(g64, r, f16):
    """A float64 gelu value pushed through the kernel's roundings."""
    if f16:
        o = _f16(g64)
        return o if r is None else _f16((o.float() + r.float()).double())     # fp32 add, then fp16, as the kernel
    o = g64.float()
    return (o if r is None else o + r.float()).double()


def _run(ops, c, api, out_mode, split):
    M, K, N = c.M, c.K, c.N
    f16 = out_mode == ops.OUT_NHWC_F16
    pc = ops.PackedConv([(c.w, K)], c.b, device=DEV)
    x4 = U.guarded_nhwc(c.x.view(1, M, 1, K), K + 8, DEV)
    shell = type("S", (), {"out_shape": (1, M, 1, N), "out_mode": out_mode})
    buf, out = U.out_buffer(shell, DEV)
    plan = {}
    if api == "linear":
        r = None
        # rows of stride K + 8 in, the full-width row view out (out_ld comes from its last dimension)
        y = ops.linear(pc, x4[0, :, 0, :], act=ops.ACT_GELU, out_mode=out_mode, out=out[0, :, 0, :], split_k=split,
                       plan_out=plan)
        assert y.data_ptr() == out.data_ptr()
    else:
        r = c.r
        res = U.guarded_residual(c.r.view(1, M, 1, N), N + 24, DEV)
        ops.conv2d(pc, x4, ksize=1, pad=0, act=ops.ACT_GELU, residual=res, out_mode=out_mode, out=out,
                   split_k=split, plan_out=plan)
    torch.cuda.synchronize()
    assert plan["variant"] == 0, plan          # an epilogue activation: the register-staged kernel
    if split is not None:
        assert plan["split_k"] == split, plan
    got, clean = U.split_out(shell, buf)
    assert clean, "wrote outside the output view"
    got = got.view(M, N).double()
    assert torch.isfinite(got).all()
    lo = _stored(c.gelu - c.tol, r, f16)
    hi = _stored(c.gelu + c.tol, r, f16)
    bad = ~((got >= lo) & (got <= hi))
    tag = f"{api} M={M} K={K} N={N} {'f16' if f16 else 'rows32'} split={split}"
    if not f16 and r is None:
        frac = ((got - c.gelu).abs() / c.tol.clamp_min(1e-30))[c.h != 0].max().item()
        print(f"[act gelu] {tag}: worst error {frac:.4f} of the bound", flush=True)
    else:
        nominal = _stored(c.gelu, r, f16)
        print(f"[act gelu] {tag}: {int((got != nominal).sum())} of {got.numel()} elements off the nominal rounding",
              flush=True)
    if bad.any():
        m, n = bad.nonzero()[0].tolist()
        raise AssertionError(f"{tag}: {int(bad.sum())} of {got.numel()} elements outside the bound; first (m={m}, "
                             f"n={n}): h {c.h[m, n].item()}, got {got[m, n].item()!r}, allowed [{lo[m, n].item()!r}, "
                             f"{hi[m, n].item()!r}], gelu64 {c.gelu[m, n].item()!r}")


def _splits(K):
    return [None, 4] if (K // 64) // 4 >= 8 else [None]


PARAMS = [(M, K, N, sp) for M in MS for (K, N) in SHAPES for sp in _splits(K)]


@pytest.mark.parametrize("out_mode", ["f16", "rows32"])
@pytest.mark.parametrize("M,K,N,split", PARAMS)
def test_linear_act_gelu_exact(ops, M, K, N, split, out_mode):
    mode = ops.OUT_NHWC_F16 if out_mode == "f16" else ops.OUT_ROWS_F32
    _run(ops, case(M, K, N), "linear", mode, split)


@pytest.mark.parametrize("out_mode", ["f16", "rows32"])
@pytest.mark.parametrize("M,K,N,split", PARAMS)
def test_conv1x1_act_gelu_residual_exact(ops, M, K, N, split, out_mode):
    mode = ops.OUT_NHWC_F16 if out_mode == "f16" else ops.OUT_ROWS_F32
    _run(ops, case(M, K, N), "conv2d", mode, split)


def test_unknown_act_and_geglu_combination_are_refused(ops):
    c = case(77, 128, 512)
    pc = ops.PackedConv([(c.w, c.K)], c.b, device=DEV)
    x = c.x.to(DEV)
    with pytest.raises(RuntimeError, match=r"failed \(-1\): conv2d: unknown act"):      # SDK_EINVAL
        ops.linear(pc, x, act=3)
    pcg = ops.PackedConv([(c.w, c.K)], c.b, geglu=True, device=DEV)
    with pytest.raises(RuntimeError, match=r"failed \(-1\): conv2d: act does not combine with the GEGLU"):
        ops.linear(pcg, x, act=ops.ACT_GELU, out_mode=ops.OUT_GEGLU_F16)
    assert ops.ACT_GELU == 2
