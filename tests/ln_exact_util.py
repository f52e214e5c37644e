"""Exact-input cases for sdk_layer_norm (csrc/norm.hip layer_norm_kernel<1|2|4>, layer_norm_quad_kernel<10|20>; the
row math is ln_row_stats / ln_apply8 / ln_quad_stats / ln_quad_apply of csrc/common.h).
tests/test_gpu_layer_norm_exact.py runs them on the GPU, tests/test_gn_stats_inputs.py checks them on the CPU.
Nothing of the product package is imported here.

Rows are small integers stored as fp16, so the kernel's pivot-shifted sums s1 = sum (x - x0), s2 = sum (x - x0)^2
(x0 = the row's first element) are integers below 2^24: exact in fp32 whatever the lane layout or shuffle order.
Everything after them is a fixed sequence of fp32 operations (contraction off, the fused steps written as fmaf),
which ``emulate`` restates operation for operation; only rsqrtf (not correctly rounded on the device) can differ,
by an fp32 ulp.  The float64 reference (``reference``) takes the mean and the biased variance from the exact integer
sums and rounds (x - mean) / sqrt(var + eps) * gamma + beta to fp16 once.

What the GPU test asserts is a property of correct fp32 row math on THESE inputs, which the CPU test establishes with
``emulate``: every element within one fp16 ulp of the reference, at most 0.5 % of them different at all.  beta is
drawn from +-[4, 5) so that no output is small against the fp32 error of its terms (|t gamma| <= 3 for the hashed
rows): near zero an fp16 ulp is arbitrarily small and no fp32 kernel could be within one."""
import numpy as np
import torch

from conv_exact_util import SENTINEL, InexactCase
from ff_exact_util import hashed, hashed_ints, seed_of

EPS = 1e-5
PRE, POST = 2, 66                  # guard rows before / after the payload (66 > the 64 rows of a quad-form block)
# columns -> the instantiation sdk_layer_norm picks for them
KERNEL_OF = {320: "quad<10>", 640: "quad<20>", 8: "row<1>", 64: "row<1>", 504: "row<1>", 520: "row<2>", 768: "row<2>",
             1016: "row<2>", 1032: "row<4>", 1280: "row<4>", 2040: "row<4>", 2048: "row<4>"}
COLS = tuple(KERNEL_OF)
ROWS = (1, 5, 63, 64, 65)
# more rows than the capped grid holds: waves walk, and the last step prefetches a row past the end
WALK = {8: 4 * 2048 * 2 + 3, 320: 16 * 4 * 2048 + 17}
WALK_PERIOD = 4099                 # the walking cases repeat the rows of a [4099, cols] base (a prime: no alignment
                                   # with the 4- / 64-row blocks), so their reference is computed once for 4099 rows
FAMILIES = ("hashed", "offset")
MAX_DIFFER = 0.005


def kernel_of(cols):
    """The launch rule of sdk_layer_norm, restated."""
    if cols in (320, 640):
        return f"quad<{cols // 32}>"
    c8 = cols // 8
    return "row<1>" if c8 <= 64 else "row<2>" if c8 <= 128 else "row<4>"


def rows_data(family, rows, cols):
    """int64 [rows, cols]: hashed integers in [-8, 8]; or 8 + [-4, 4] with the row's first element (the kernel's
    pivot) at -8, so the row mean lies 16 (six standard deviations) from it.  Row min(2, rows - 1) is constant
    (variance 0)."""
    s = seed_of(f"ln-{family}-{cols}")
    if family == "hashed":
        x = hashed_ints(s, rows, cols, -8, 8)
    else:
        x = 8 + hashed_ints(s, rows, cols, -4, 4)
        x[:, 0] = -8
    x[min(2, rows - 1), :] = 5
    return x


def params(cols):
    """(gamma, beta) fp32 [cols]: gamma in [0.5, 1.5), beta in +-[4, 5), multiples of 2^-16; beta[0] < 0, the sign of
    the offset family's pivot column (t = -6 there), so that output stays away from zero too."""
    s = seed_of(f"ln-affine-{cols}")
    gamma = 0.5 + hashed(s, 1, cols, 1 << 16)[0].double() / (1 << 16)
    beta = (4.0 + hashed(s + 1, 1, cols, 1 << 16)[0].double() / (1 << 16)) * (2 * hashed(s + 2, 1, cols, 2)[0] - 1)
    beta[0] = -beta[0].abs()
    return gamma.float(), beta.float()


def reference(x, gamma, beta, eps=EPS):
    """fp16 [rows, cols]: float64 from exact integer sums, rounded once."""
    rows, cols = x.shape
    s1, s2 = x.sum(1), (x * x).sum(1)
    num = cols * s2 - s1 * s1
    if not (num.max().item() < 2 ** 53):
        raise InexactCase("the variance numerator is not an exact double")
    mean, var = s1.double() / cols, num.double() / float(cols * cols)
    r = 1.0 / torch.sqrt(var + float(np.float32(eps)))
    y = (x.double() - mean[:, None]) * r[:, None] * gamma.double()[None, :] + beta.double()[None, :]
    return torch.from_numpy(y.numpy().astype(np.float16))


def _fma32(a, b, c):
    """fmaf on float32 arrays: the product of two fp32 values is exact in float64; the sum rounds to 53 bits before
    24, which differs from one rounding only on a 2^-29 sliver."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emulate(x, gamma, beta, eps=EPS):
    """fp16 [rows, cols]: ln_row_stats / ln_quad_stats and ln_apply8 / ln_quad_apply in float32, same pivot, same
    operation order (the two forms differ only in which lanes hold which elements, and the sums are exact)."""
    f32 = np.float32
    xv = x.numpy().astype(np.float32)
    rows, cols = xv.shape
    x0 = xv[:, :1]
    d = xv - x0
    if np.abs(d).max() > 64 or (d.astype(np.float64) ** 2).sum(1).max() >= 2 ** 24:
        raise InexactCase("the pivot-shifted sums are not exact in fp32")
    s1 = d.astype(np.float64).sum(1).astype(f32)
    s2 = (d.astype(np.float64) ** 2).sum(1).astype(f32)
    inv_n = f32(1.0) / f32(cols)
    dm = s1 * inv_n
    var = np.maximum(_fma32(-dm, dm, s2 * inv_n), f32(0.0))
    mean = x0[:, 0] + dm
    rstd = (1.0 / np.sqrt((var + f32(eps)).astype(np.float64))).astype(f32)
    t = (xv - mean[:, None]) * rstd[:, None]
    g, b = gamma.numpy()[None, :], beta.numpy()[None, :]
    return torch.from_numpy(_fma32(t, np.broadcast_to(g, t.shape), np.broadcast_to(b, t.shape)).astype(np.float16))


def ordered(h):
    """fp16 tensor -> integers whose difference counts fp16 units in the last place."""
    i = h.contiguous().view(torch.int16).int()
    return torch.where(i < 0, -(i & 0x7fff), i)


def compare(got, ref):
    """(largest distance in fp16 ulps, share of elements that differ at all); NaN counts as far."""
    if torch.isnan(got.float()).any():
        return 1 << 16, 1.0
    dist = (ordered(got) - ordered(ref)).abs()
    return int(dist.max().item()), (dist != 0).double().mean().item()


_REF = {}


def case(family, rows, cols):
    """(x int64, gamma, beta, reference fp16), built once per process (shared: do not modify).  The walking cases
    return their [WALK_PERIOD, cols] base; row r of the problem is base row r % WALK_PERIOD."""
    base_rows = min(rows, WALK_PERIOD)
    key = (family, base_rows, cols)
    if key not in _REF:
        x = rows_data(family, base_rows, cols)
        if not torch.equal(x.half().long(), x):
            raise InexactCase("the rows are not exact in fp16")
        gamma, beta = params(cols)
        _REF[key] = (x, gamma, beta, reference(x, gamma, beta))
    return _REF[key]


# --------------------------------------------------------------------------- guarded buffers (after ff_exact_util)

def guarded_rows(t, ld, device):
    """(buffer, view): ``t`` [M, cols] fp16 inside a NaN-filled [PRE + M + POST, ld] buffer."""
    M, cols = t.shape
    buf = torch.full((PRE + M + POST, ld), float("nan"), dtype=torch.float16, device=device)
    view = buf[PRE:PRE + M, :cols]
    view.copy_(t)
    return buf, view


def out_rows(M, cols, ld, device):
    """(buffer, the output view [M, cols]): sentinel-filled [PRE + M + POST, ld]."""
    buf = torch.full((PRE + M + POST, ld), SENTINEL, dtype=torch.float16, device=device)
    return buf, buf[PRE:PRE + M, :cols]


def guards_hit(buf, M, cols):
    """Cells outside the view that lost the sentinel (counted on the buffer's device)."""
    hit = buf != SENTINEL
    hit[PRE:PRE + M, :cols] = False
    return int(hit.sum().item())
