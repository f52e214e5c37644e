"""Exact GroupNorm apply tests that first assert which form the host plan routes to (run with -m gpu).

Inputs are small integers and the affine is drawn from {0.5, 1, 2, -1} x [-4, 4], so every product and sum is
exact in fp16 whether or not the compiler fuses the multiply-add: without SiLU the kernels must equal the same
expression evaluated by torch on the CPU, element for element.  With SiLU the fast reciprocal / exponential err by a
few fp32 units in the last place — far below half an fp16 unit — so they can only flip the final rounding: every
element is within one fp16 unit in the last place of F.silu of the exact affine computed in fp64 and rounded once.
All forms go through one device helper, so they also agree with each other bit for bit."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_util import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"

# form the plan must name, (B, H, W, C), pad
APPLY_CASES = [
    ("flat", (2, 9, 7, 64), 1),
    ("flat", (2, 12, 12, 96), 0),
    ("row", (1, 128, 128, 32), 1),
    ("row", (1, 128, 130, 32), 2),          # ragged width
    ("stride", (1, 128, 128, 32), 0),       # unpadded grid-stride form
    ("stride", (2, 16, 16, 8), 1),          # padded: one 8-channel vector per pixel has no flat reciprocal
    ("stride", (1, 128, 128, 8), 1),        # padded, >= 128x128: no exact row reciprocal either
]
# every case as one tensor, and as a 2-source concat split at half the channels where the halves are vectors of 8
CASES = [(f, s, p, c) for (f, s, p) in APPLY_CASES for c in (False, True) if not c or s[3] % 16 == 0]
IDS = [f"{f}-{'x'.join(map(str, s))}-pad{p}{'-concat' if c else ''}" for f, s, p, c in CASES]


@pytest.fixture(scope="module")
def ops(sdk):
    from sd_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return o


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """x fp16 [B, H, W, C], (scale, shift) fp32 [B, C], the exact affine fp32 [B, H, W, C] and the key of each
    element's (x, scale, shift) triple — all on the CPU, computed once per shape."""
    B, H, W, C = shape
    b, y, x, c = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(W), torch.arange(C), indexing="ij")
    xv = (7 * b + 3 * y + 5 * x + c) % 17 - 8
    bb, cc = torch.meshgrid(torch.arange(B), torch.arange(C), indexing="ij")
    si = (bb + cc) % 4
    scale = torch.tensor([0.5, 1.0, 2.0, -1.0])[si]
    shift = ((3 * bb + cc) % 9 - 4).float()
    aff = xv.float() * scale[:, None, None, :] + shift[:, None, None, :]
    key = ((xv + 8) * 4 + si[:, None, None, :]) * 9 + (shift.long()[:, None, None, :] + 4)
    return xv.half(), (scale.contiguous(), shift.contiguous()), aff, key


def _src(x, concat):
    x = x.to(DEV)
    if not concat:
        return x
    h = x.shape[-1] // 2
    return x[..., :h].contiguous(), x[..., h:].contiguous()


def _padded(t, pad):
    return F.pad(t, (0, 0, pad, pad, pad, pad))


def _ordered(h):
    """fp16 tensor -> integers whose difference counts fp16 units in the last place."""
    i = h.contiguous().view(torch.int16).int()
    return torch.where(i < 0, -(i & 0x7fff), i)


@functools.lru_cache(maxsize=None)
def _flat_bits(silu):
    """(x, scale, shift) triple -> output bits, from the flat form's runs (every triple maps to one value there)."""
    from sd_amd import ops
    table = torch.full((17 * 4 * 9,), -1, dtype=torch.int32)
    for form, shape, pad in APPLY_CASES[:2]:
        x, gn, _, key = _inputs(shape)
        assert ops.group_norm_plan(x.to(DEV), pad=pad, stats=False)["apply"] == "flat"
        y = ops.group_norm_apply(x.to(DEV), tuple(t.to(DEV) for t in gn), silu=silu, pad=pad).cpu()
        H, W = shape[1:3]
        bits = y[:, pad:pad + H, pad:pad + W].contiguous().view(torch.int16).int() & 0xffff
        table[key.reshape(-1)] = bits.reshape(-1)
        assert torch.equal(table[key], bits), "one triple gave two values inside the flat form"
    return table


@pytest.mark.parametrize("form, shape, pad, concat", CASES, ids=IDS)
@pytest.mark.parametrize("silu", [False, True], ids=["affine", "silu"])
def test_group_norm_apply_exact(ops, form, shape, pad, concat, silu):
    B, H, W, C = shape
    x, gn, aff, key = _inputs(shape)
    src = _src(x, concat)
    assert ops.group_norm_plan(src, pad=pad, stats=False) == {"stats": "given", "apply": form, "launches": 1,
                                                              "workspace_bytes": 0}
    y = ops.group_norm_apply(src, tuple(t.to(DEV) for t in gn), silu=silu, pad=pad).cpu()
    assert y.shape == (B, H + 2 * pad, W + 2 * pad, C)
    inner = y[:, pad:pad + H, pad:pad + W]
    if pad:
        border = torch.ones(H + 2 * pad, W + 2 * pad, dtype=torch.bool)
        border[pad:-pad, pad:-pad] = False
        assert torch.count_nonzero(y[:, border].float()) == 0
    if not silu:
        assert torch.equal(y, _padded(aff, pad).half())
    else:
        ref = torch.from_numpy(F.silu(aff.double()).numpy().astype(np.float16))    # fp64, rounded once
        ulp = (_ordered(inner) - _ordered(ref)).abs().max().item()
        print(f"silu: max distance from the once-rounded fp64 value {ulp} fp16 ulp")
        assert ulp <= 1
    table = _flat_bits(silu)
    want = table[key]
    assert int(want.min()) >= 0, "a triple the flat runs never saw"
    assert torch.equal(inner.contiguous().view(torch.int16).int() & 0xffff, want), "forms disagree in bits"


@pytest.mark.parametrize("form, shape, pad, concat", CASES, ids=IDS)
def test_group_norm_whole_matches_two_calls(ops, form, shape, pad, concat):
    """ops.group_norm against F.group_norm (+ SiLU), and bit for bit against affine-then-apply wherever the plan
    gives both routes the same statistics kernel."""
    B, H, W, C = shape
    groups = min(32, C)
    g = torch.Generator().manual_seed(H * W + C + pad)
    x = (torch.randn(B, H, W, C, generator=g) * 1.5 + 1.0).half()
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    src = _src(x, concat)
    whole = ops.group_norm_plan(src, groups=groups, pad=pad)
    half = ops.group_norm_plan(src, groups=groups, pad=pad, apply=False)
    assert whole["apply"] in (form, "in_stats") and half["apply"] == "none"
    assert whole["stats"] == ("slice" if H * W <= 1024 else "chunked")
    y = ops.group_norm(src, gamma.to(DEV), beta.to(DEV), 1e-5, groups, silu=True, pad=pad)
    ref = F.silu(F.group_norm(x.float().permute(0, 3, 1, 2), groups, gamma, beta, 1e-5))
    ref = F.pad(ref, (pad, pad, pad, pad)).permute(0, 2, 3, 1)
    err = rel_l2(y, ref)
    print(f"group_norm {shape} pad {pad}: rel_l2 {err:.2e}")
    assert err < 1e-3
    if whole["stats"] == half["stats"]:
        two = ops.group_norm_apply(src, ops.group_norm_affine(src, gamma.to(DEV), beta.to(DEV), 1e-5, groups),
                                   silu=True, pad=pad)
        assert torch.equal(y, two)


EX_CASES = [((2, 6, 10, 64), 1), ((1, 5, 7, 16), 0)]    # the second: the odd-size floor of the pooling


@pytest.mark.parametrize("shape, pad", EX_CASES)
@pytest.mark.parametrize("mode", ["up", "down"])
def test_group_norm_resample_exact(ops, shape, pad, mode):
    """Both outputs exact: the affine values are multiples of 0.5 below 32, so the mean of four is a multiple of
    0.125, which fp16 holds exactly at these magnitudes (and the raw mean of four integers likewise)."""
    B, H, W, C = shape
    x, gn, aff, _ = _inputs(shape)
    ya, yr = ops.group_norm_resample(x.to(DEV), tuple(t.to(DEV) for t in gn), mode, silu=False, pad=pad)

    def resample(t):
        t = t.float().permute(0, 3, 1, 2)
        t = F.avg_pool2d(t, 2) if mode == "down" else F.interpolate(t, scale_factor=2, mode="nearest")
        return t.permute(0, 2, 3, 1)
    assert torch.equal(ya.cpu(), _padded(resample(aff), pad).half())
    assert torch.equal(yr.cpu(), resample(x).half())


@pytest.mark.parametrize("shape, pad", EX_CASES)
@pytest.mark.parametrize("extras", [False, True], ids=["plain", "bias+residual"])
def test_group_norm_apply_ex_exact(ops, shape, pad, extras):
    B, H, W, C = shape
    x, gn, aff, _ = _inputs(shape)
    pb = res = None
    ref = aff
    if extras:
        b, y, xx, c = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(W), torch.arange(C), indexing="ij")
        pb = ((torch.arange(B)[:, None] + 2 * torch.arange(C)[None, :]) % 5 - 2).float()
        res = ((b + y + xx + c) % 7 - 3).half()
        ref = aff + pb[:, None, None, :] + res.float()
    y = ops.group_norm_apply_ex(x.to(DEV), tuple(t.to(DEV) for t in gn), silu=False,
                                post_bias=None if pb is None else pb.to(DEV),
                                residual=None if res is None else res.to(DEV))
    assert torch.equal(y.cpu(), ref.half())
