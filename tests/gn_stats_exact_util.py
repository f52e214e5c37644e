"""Exact cases for the GroupNorm statistics (csrc/norm.hip) and for the per-chunk statistics the convs emit
(csrc/conv_tile.h gn_block_stats / gn_tile_store, csrc/conv_small.hip splitk_reduce_gn_kernel).
tests/test_gpu_gn_stats_exact.py runs them on the GPU, tests/test_gn_stats_inputs.py checks the inputs and the
claimed routes on the CPU.  Nothing of the product package is imported here.

Why the comparison can be this tight
------------------------------------
Inputs are small integers stored as fp16 (|x| <= 8; the offset family 1024 + [-4, 4], the spike |x| <= 16).  Every
statistics kernel subtracts a pivot (the channel's value at pixel 0 of the image) first, so each d = x - piv is an
integer with |d| <= 16, and the fp32 sums of d (<= 16 n) and d^2 (<= 256 n) over the n <= 16384 pixels a thread or a
workgroup adds stay below 2^24: they are exact in any order.  From there every kernel works in double until it rounds
three times: rstd -> fp32, gamma * rstd -> fp32 (the scale), and beta - (float)mean * scale -> fp32 (the shift).

The reference (``exact_stats`` / ``Affine``) takes sum x and sum x^2 over the group as exact int64 sums, forms
mean = S1 / n and the biased variance (n S2 - S1^2) / n^2 with one float64 rounding each (numerator and denominator
are exact doubles: both are asserted below 2^53), r = 1 / sqrt(var + eps) in float64 with eps, gamma, beta the fp32
values the kernel is given, and scale_ref = gamma r, shift_ref = beta - mean gamma r.

The bounds (u = 2^-24, the fp32 unit roundoff; the kernel's double arithmetic errs by ~1e-15 relative)
  scale = fl(gamma * fl(r)):  r(1 + d1) gamma (1 + d2), |di| <= u            => |scale - scale_ref| <= (2u + u^2) |scale_ref|
                                                                                                  = 2^-23 |scale_ref| (1 + 2^-25)
  shift = fl(beta - fl(mean) * scale), the product rounded (unfused) or not (fused):
          fl(mean) = mean (1 + d3); scale = scale_ref (1 + d4), |d4| <= 2u + u^2; the product's own rounding d5:
          |fl(mean) scale (1 + d5) - mean scale_ref| <= (4u + O(u^2)) |mean scale_ref| = 2^-22 |mean scale_ref| (1 + O(u))
          and the subtraction rounds once: u |shift| <= u (|shift_ref| + 2^-22 |mean scale_ref|)
                                                              => |shift - shift_ref| <= 2^-22 |mean scale_ref| + 2^-24 |shift_ref|  (1 + O(u))
Every O(u) term and the double arithmetic is below 2^-20 relative; the common slack (1 + 2^-10) covers them with
room.  These are ``Affine.bound_scale`` / ``bound_shift``; the GPU test asserts them and records the largest error /
bound ratio it saw.
The one absolute term: the kernels' double mean is a sum of per-channel (and per-chunk) means, each a rounded
quotient, so its error is relative to the largest |x| it adds (A), not to the mean — a group whose integers sum to
exactly 0 gets a mean of ~1e-17 A, not 0.  With at most 256 channels x 64 chunks, each term within 2^-52 A after its
division and its addition, the mean is within 2^-52 * 2^8 = 2^-44 A (the chunks of a channel merge before the
channels do: their 2^6 terms add to the same order).  bound_shift gets + 2^-44 A |scale_ref|: seven decimal orders
below the 2^-22 term unless the mean is below 1e-6 A.

The apply forms (``y_interval``, ``ULP_EXEMPT``).  The assertion is the issue's: without SiLU every element of y is
within 1 fp16 ulp of the float64 value y64 = x scale_ref + shift_ref rounded once.  It is asserted on every element of
every run, with one enumerated exception: the (family, eps) pairs of ``ULP_EXEMPT``, where an fp32 affine cannot meet
it.  y = fp16(fl32(x * scale + shift)), and the fp32 value can be off by
E = |x| bound_scale + bound_shift + u (|x scale_ref| + |y64|)(1 + 2^-10) (the affine's own bounds and the two fp32
roundings of an unfused multiply-add).  In the offset family shift ~ -1024 scale (E ~ 1e-4, above the ulp of every
output below 0.1); a constant image has scale = gamma / sqrt(eps) and shift ~ -mean scale, in the thousands at
eps <= 1e-5 and still ~16 at eps = 0.25 while its outputs are beta in [-1, 1]; the spike family is a constant image
but for one pixel (var ~ 144 / n), so the same holds at eps <= 1e-5 and no longer at 0.25.  A correct kernel measured
up to 2992 ulp there (profiles/gn_stats_exact_errors.txt).  In the exempt runs the 1-ulp bound is still asserted on
every element whose E is below half an fp16 ulp of y64 (there it follows from the roundings), and every element must
lie in [fp16(y64 - E), fp16(y64 + E)] (the fp16 rounding is monotonic), which is what the arithmetic allows and never
wider.

Producer partials (``chunk_partials``): per (image, chunk of 2^k rows, channel) the (mean, M2) of integer data are
S / 2^k and (2^k Q - S^2) / 2^k — exact in fp32 (asserted: ``InexactCase``).  The reference of the routes that merge
partials (``merge_partials``) is the float64 merge of the fp32 partials GIVEN, which for these partials equals the
statistics of the tensor (tests/test_gn_stats_inputs.py asserts that).

What the convs emit (``check_chunk_stats``)
  gn_block_stats: a lane holds RPL = 2^a rows of a channel pair: a0 = sum x is an integer, m = a0 / RPL exact, every
  d = x - m a multiple of 1/RPL with |d| <= 32, q = sum d^2 a multiple of 1/RPL^2 below RPL * 1024: <= 22 bits.  Each
  xor merge pairs EQUAL counts n = 2^b: the mean of two means halves the granule (<= 32 rows: 1/32, 9 bits), and
  d^2 * (n/2) with d a multiple of 1/n is a multiple of 1/(2n) below 2^15 (<= 21 bits).  So a block's pair is exact.
  gn_tile_store merges the tile's TBM/BR blocks sequentially with weights BR/(n + BR) = 1/2, 1/3, 1/4 ... and the
  split-K reduce its 32 row lanes with nb/(na + nb): not exact.  Those get
      |mean - mean64| <= s u A,   |M2 - M264| <= s u 4 R A^2
  with A = max |y| of the chunk, R its rows, s the fp32 operations on the longest dependent path of the route (8 per
  merge on the M2 path: dl, n + nb, the division, dl * dl, * n, * f, q + ., r.y + .):
      tile epilogue: TBM/16 blocks at most (16-row blocks of the 16x16-MFMA tiles)      s = 8 * TBM / 16
      split-K reduce: the lane's own (mean, M2) 4, then 31 merges                         s = 4 + 8 * 31
"""
import numpy as np
import torch

from conv_exact_util import InexactCase
from ff_exact_util import fp16_ulp, hashed, hashed_ints, seed_of

U32 = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10
DBL_MEAN = 2.0 ** -44               # see "The one absolute term" in the docstring
EPS = (1e-6, 1e-5, 0.25)
FAMILIES = ("hashed", "offset", "constant", "spike")
# the (family, eps) pairs whose applied output an fp32 affine cannot hold within 1 fp16 ulp of float64 (docstring, "The
# apply forms"); everywhere else — the hashed family, the spike at eps 0.25, what the convs emit — the bound is asserted
ULP_EXEMPT = frozenset([("offset", 1e-6), ("offset", 1e-5), ("offset", 0.25),
                        ("constant", 1e-6), ("constant", 1e-5), ("constant", 0.25),
                        ("spike", 1e-6), ("spike", 1e-5)])
SENT32 = -777.5                     # prefill of the fp32 (scale, shift) buffers
REDUCE_S = 4 + 8 * 31


def tile_s(tbm):
    return 8 * tbm // 16


# --------------------------------------------------------------------------- the planner's geometry, restated

GN_SLICE_MAX_HW, GN_SLICE_APPLY_MAX_HW, GN_PARTS_SINGLE_MAX_HW = 1024, 64, 256
GNP_MAXCS, GNP_MAXCH, GN_U, GNF_T = 256, 16, 8, 512


def fused_slice(channels, groups):
    """Channels of one workgroup of the single-launch statistics (0: not applicable)."""
    cg = channels // groups
    for g in range(1, groups + 1):
        if groups % g == 0 and (g * cg) % 8 == 0:
            return g * cg if g * cg <= 512 else 0
    return 0


def part_slice(channels, groups):
    """Channels of one workgroup of gn_apply_part_kernel (0: not applicable)."""
    cg = channels // groups
    best = 0
    for g in range(1, groups + 1):
        if groups % g == 0 and (g * cg) % 8 == 0 and g * cg <= GNP_MAXCS:
            best = g * cg
    return best


def part_row_splits(batch, h, w, pad, channels, groups):
    """(rows per split, splits) of gn_apply_part_kernel's grid over the (padded) output image."""
    cs = part_slice(channels, groups)
    slices = channels // cs
    npix = (h + 2 * pad) * (w + 2 * pad)
    splits = max(1, (npix * (cs // 8) + 2047) // 2048)
    want = -(-512 // (slices * batch))
    splits = min(max(splits, want), max(1, npix // 16))
    rows_per = -(-npix // splits)
    return rows_per, -(-npix // rows_per)


def chunk_geom(batch, hw, channels):
    """(nv, ry, chunk_rows, nchunks) of the chunked statistics pass."""
    c8 = channels // 8
    nv = -(-c8 // 256)
    ry = 1 if nv > 1 else max(1, 256 // c8)
    step = ry * GN_U
    want = max(1, -(-1536 // max(batch, 1)))
    per = max(1, -(-hw // want))
    chunk_rows = -(-per // step) * step
    return nv, ry, chunk_rows, -(-hw // chunk_rows)


def finalize_tpc(cg):
    tpc = 64
    while tpc > 1 and tpc * cg > 256:
        tpc >>= 1
    return tpc


# --------------------------------------------------------------------------- the cases

class GnCase:
    """One GroupNorm problem and the route it claims.  ``entry``: "affine" (group_norm_affine: a statistics pass),
    "scale_shift" (group_norm_scale_shift: from partials), "group_norm" (statistics + apply; from partials when
    ``nch`` is given).  ``plan``: (stats, apply, launches) the host plan must name."""

    def __init__(self, name, entry, B, H, W, cins, plan, groups=32, pad=0, nch=None):
        self.name, self.entry, self.B, self.H, self.W, self.cins = name, entry, B, H, W, tuple(cins)
        self.groups, self.pad, self.nch = groups, pad, nch
        self.hw, self.C, self.cg = H * W, sum(cins), sum(cins) // groups
        self.c_split = cins[0]
        self.stats, self.apply_form, self.launches = plan
        assert entry in ("affine", "scale_shift", "group_norm") and (entry == "group_norm") == (self.apply_form != "none")
        assert (nch is not None) == (self.stats == "parts")

    @property
    def want_apply(self):
        return self.entry == "group_norm"

    @property
    def plan(self):
        ws = self.B * chunk_geom(self.B, self.hw, self.C)[3] * self.C * 8 if self.stats == "chunked" else 0
        return {"stats": self.stats, "apply": self.apply_form, "launches": self.launches, "workspace_bytes": ws}

    def spike_positions(self):
        """Pixels at the edges of the route's work split (docstring of each branch), deduplicated, in range."""
        hw = self.hw
        if self.stats == "slice":
            # thread (r0, v) reads pixels r0, r0 + rp, ... in rounds of 8: the first / last pixel of row set 0, the
            # first pixel of the second round, the last row set's first and last pixel
            rp = GNF_T // (fused_slice(self.C, self.groups) // 8)
            cand = [0, hw - 1, rp - 1, rp, 8 * rp - 1, 8 * rp, (hw - 1) // rp * rp, hw // 2]
        else:
            # first and last pixel of the first, a middle and the (ragged) last chunk
            if self.stats == "chunked":
                rows = chunk_geom(self.B, hw, self.C)[2]
            else:
                rows = hw // self.nch[0]
            n = -(-hw // rows)
            mid = n // 2
            cand = [0, rows - 1, mid * rows, min(hw, (mid + 1) * rows) - 1, (n - 1) * rows, hw - 1]
            if self.stats == "parts" and len(self.cins) > 1:
                r1 = hw // self.nch[1]
                cand += [r1 - 1, hw - r1]
        out = []
        for p in cand:
            if 0 <= p < hw and p not in out:
                out.append(p)
        return out

    def spike_channels(self):
        if len(self.cins) > 1:
            return [self.c_split - 1, self.c_split]          # last channel of source 0, first of source 1
        return [0, self.C - 1, (self.C // 2) | 1]


S, K, P = "slice", "chunked", "parts"
CASES = [
    # ---- slice, statistics only (gn_stats_fused_kernel<false>)
    GnCase("slice-7x5-c64", "affine", 3, 7, 5, [64], (S, "none", 1)),                 # slice 8: 504 threads idle
    GnCase("slice-32x32-c960", "affine", 2, 32, 32, [960], (S, "none", 1)),          # cg 30, slice 120: 15 vectors
    GnCase("slice-33x31-c8+88", "affine", 2, 33, 31, [8, 88], (S, "none", 1)),       # cg 3: c_split inside slice 0
    # the widest slice (504); 25 pixels, so that the offset family's sum x^2 of one channel passes 2^24
    GnCase("slice-5x5-c504-g2", "affine", 2, 5, 5, [504], (S, "none", 1), groups=2),
    # ---- slice with apply (gn_stats_fused_kernel<true>)
    GnCase("fused-8x8-c1280-pad0", "group_norm", 2, 8, 8, [1280], (S, "in_stats", 1)),
    GnCase("fused-8x8-c1280-pad1", "group_norm", 2, 8, 8, [1280], (S, "in_stats", 1), pad=1),
    GnCase("fused-8x8-c1280+1280-pad0", "group_norm", 2, 8, 8, [1280, 1280], (S, "in_stats", 1)),
    GnCase("fused-8x8-c1280+1280-pad1", "group_norm", 2, 8, 8, [1280, 1280], (S, "in_stats", 1), pad=1),
    GnCase("fused-7x5-c64-pad1", "group_norm", 3, 7, 5, [64], (S, "in_stats", 1), pad=1),
    # ---- slice statistics, then an apply launch
    GnCase("slice-12x12-c96-flat", "group_norm", 2, 12, 12, [96], (S, "flat", 2)),
    GnCase("slice-16x16-c8-stride", "group_norm", 2, 16, 16, [8], (S, "stride", 2), groups=8, pad=1),
    # ---- chunked (gn_partial_kernel + gn_finalize_kernel)
    GnCase("chunked-103x10-c64", "affine", 2, 103, 10, [64], (K, "none", 2)),        # cg 2: tpc 64; ry 32, ragged chunk
    GnCase("chunked-103x10-c2560", "affine", 1, 103, 10, [2560], (K, "none", 2)),    # nv 2, ry 1
    GnCase("chunked-9x7-c520-g8", "affine", 2, 9, 7, [520], (K, "none", 2), groups=8),       # cg 65: no slice; tpc 2
    GnCase("chunked-35x30-c272-g2", "affine", 2, 35, 30, [272], (K, "none", 2), groups=2),   # cg 136: tpc 1
    GnCase("chunked-103x10-c24+40", "affine", 2, 103, 10, [24, 40], (K, "none", 2), groups=8),
    GnCase("chunked-35x30-c64-flat", "group_norm", 2, 35, 30, [64], (K, "flat", 3), pad=1),
    GnCase("chunked-128x128-c32-row", "group_norm", 1, 128, 128, [32], (K, "row", 3), pad=1),
    GnCase("chunked-128x128-c32-stride", "group_norm", 1, 128, 128, [32], (K, "stride", 3)),
    # ---- partials -> gn_finalize_part_kernel
    GnCase("parts-16x16-c64-n1", "scale_shift", 2, 16, 16, [64], (P, "none", 1), nch=(1, 0)),      # tpc 64 > nch
    GnCase("parts-16x16-c64-n2", "scale_shift", 3, 16, 16, [64], (P, "none", 1), nch=(2, 0)),
    GnCase("parts-12x16-c64-n3", "scale_shift", 2, 12, 16, [64], (P, "none", 1), nch=(3, 0)),      # Chan weights 1/3
    GnCase("parts-16x16-c64-n16", "scale_shift", 2, 16, 16, [64], (P, "none", 1), nch=(16, 0)),
    GnCase("parts-32x32-c64-n64", "scale_shift", 2, 32, 32, [64], (P, "none", 1), nch=(64, 0)),    # every lane a chunk
    GnCase("parts-16x16-c272-g2-n16", "scale_shift", 2, 16, 16, [272], (P, "none", 1), groups=2, nch=(16, 0)),  # tpc 1
    GnCase("parts-12x16-c40-g8-n3", "scale_shift", 2, 12, 16, [40], (P, "none", 1), groups=8, nch=(3, 0)),      # cg 5
    GnCase("parts-16x16-c64+32-n4,1", "scale_shift", 2, 16, 16, [64, 32], (P, "none", 1), nch=(4, 1)),
    GnCase("parts-16x16-c8+88-n16,2", "scale_shift", 2, 16, 16, [8, 88], (P, "none", 1), nch=(16, 2)),  # split in group 2
    # ---- partials -> gn_apply_part_kernel
    GnCase("papply-16x16-c64-n1-pad0", "group_norm", 2, 16, 16, [64], (P, "in_stats", 1), nch=(1, 0)),
    GnCase("papply-16x16-c64-n2-pad1", "group_norm", 3, 16, 16, [64], (P, "in_stats", 1), nch=(2, 0), pad=1),
    GnCase("papply-12x16-c64-n3-pad1", "group_norm", 2, 12, 16, [64], (P, "in_stats", 1), nch=(3, 0), pad=1),  # 252 px
    GnCase("papply-16x16-c640-n16-pad1", "group_norm", 2, 16, 16, [640], (P, "in_stats", 1), nch=(16, 0), pad=1),
    GnCase("papply-16x16-c8+88-n16,2-pad0", "group_norm", 2, 16, 16, [8, 88], (P, "in_stats", 1), nch=(16, 2)),
    GnCase("papply-16x16-c320+160-n4,1-pad1", "group_norm", 2, 16, 16, [320, 160], (P, "in_stats", 1), nch=(4, 1),
           pad=1),                                                                  # slices of 120: 320 inside one
    GnCase("papply-8x8-c64-n1-pad1", "group_norm", 2, 8, 8, [64], (P, "in_stats", 1), nch=(1, 0), pad=1),
    # ---- partials, then an apply launch
    GnCase("parts-16x16-c640-n32-flat", "group_norm", 2, 16, 16, [640], (P, "flat", 2), nch=(32, 0), pad=1),
    GnCase("parts-32x32-c64-n4-flat", "group_norm", 2, 32, 32, [64], (P, "flat", 2), nch=(4, 0), pad=1),
    GnCase("parts-128x128-c32-n64-row", "group_norm", 1, 128, 128, [32], (P, "row", 2), nch=(64, 0), pad=1),
    GnCase("parts-16x16-c8-n32-stride", "group_norm", 2, 16, 16, [8], (P, "stride", 2), groups=8, nch=(32, 0), pad=1),
]
CASE = {c.name: c for c in CASES}
# every (stats, apply) pair the planner can return for a statistics request: a slice never meets the row form
# (hw <= 1024 < 128 * 128) and only slice / parts have a single-launch form
COMBOS = {(S, "none"), (S, "in_stats"), (S, "flat"), (S, "stride"), (K, "none"), (K, "flat"), (K, "row"), (K, "stride"),
          (P, "none"), (P, "in_stats"), (P, "flat"), (P, "row"), (P, "stride")}


# --------------------------------------------------------------------------- data

_DATA = {}


def data(case, family, rot=0):
    """int64 [B, hw, C] (shared: do not modify).  ``rot`` rotates the spike's positions through the batch."""
    key = (case.name, family, rot if family == "spike" else 0)
    if key in _DATA:
        return _DATA[key]
    B, hw, C = case.B, case.hw, case.C
    s = seed_of(f"gn-{case.name}-{family}")
    if family == "hashed":
        x = torch.stack([hashed_ints(s + b, hw, C, -8, 8) for b in range(B)])
    elif family == "offset":
        x = torch.stack([1024 + hashed_ints(s + b, hw, C, -4, 4) for b in range(B)])
    else:
        lo = 8 if family == "constant" else 4
        v = hashed_ints(s, B, case.groups, -lo, lo).repeat_interleave(case.cg, 1)       # equal inside a group
        x = v[:, None, :].expand(B, hw, C).clone()
        if family == "spike":
            pos, chs = case.spike_positions(), case.spike_channels()
            for b in range(B):
                i = rot + b
                p, ch = pos[i % len(pos)], chs[i % len(chs)]
                x[b, p, ch] += 12 if i % 2 == 0 else -12
    if x.abs().max().item() > 2048 or (family != "offset" and x.abs().max().item() > 16):
        raise InexactCase(f"{case.name} {family}: |x| out of range")
    _DATA[key] = x
    return x


def spike_rounds(case):
    """Rotations that put every spike position and every spike channel into some image (image b of rotation r takes
    position and channel r + b, each modulo its list)."""
    n = max(len(case.spike_positions()), len(case.spike_channels()))
    return list(range(0, n, case.B))


def sources(case, x):
    """The 1 or 2 fp16 [B, H, W, Ci] sources of x."""
    out, c0 = [], 0
    for ci in case.cins:
        out.append(x[:, :, c0:c0 + ci].reshape(case.B, case.H, case.W, ci).half())
        c0 += ci
    if not torch.equal(torch.cat([o.reshape(case.B, case.hw, -1) for o in out], -1).long(), x):
        raise InexactCase(f"{case.name}: the data is not exact in fp16")
    return out


def affine_params(case, null=False):
    """(gamma, beta) fp32 [C]: gamma in [0.5, 1.5), beta in [-1, 1], multiples of 2^-20; None, None for ``null``."""
    if null:
        return None, None
    s = seed_of(f"gn-{case.name}-affine")
    gamma = (0.5 + hashed(s, 1, case.C, 1 << 20)[0].double() / (1 << 20)).float()
    beta = (hashed_ints(s + 1, 1, case.C, -(1 << 20), 1 << 20)[0].double() / (1 << 20)).float()
    return gamma, beta


# --------------------------------------------------------------------------- references and bounds

def check_pivot_sums(case, x):
    """The fp32 sums of the pivot-shifted values stay exact: |d| <= 16, and 256 * (pixels one workgroup adds per
    channel) < 2^24."""
    d = x - x[:, :1, :]
    if d.abs().max().item() > 16:
        raise InexactCase(f"{case.name}: |x - pivot| exceeds 16")
    if not (d * d).sum(1).max().item() < 2 ** 24:
        raise InexactCase(f"{case.name}: sum d^2 reaches 2^24")


def exact_stats(x, groups):
    """(mean, var) float64 [B, groups]: biased variance from exact int64 sums, one float64 rounding each."""
    B, hw, C = x.shape
    cg = C // groups
    n = hw * cg
    t = x.reshape(B, hw, groups, cg)
    s1, s2 = t.sum((1, 3)), (t * t).sum((1, 3))
    if not (s2.max().item() * n < 2 ** 62):
        raise InexactCase("n * sum x^2 overflows int64")
    num = n * s2 - s1 * s1
    if not (num.max().item() < 2 ** 53 and n * n < 2 ** 53 and s1.abs().max().item() < 2 ** 53):
        raise InexactCase("a term of the variance is not an exact double")
    return s1.double() / n, num.double() / float(n * n)


def chunk_partials(xs, nch):
    """fp32 [B, nch, Cs, 2]: (mean, M2) per (image, chunk of hw / nch rows, channel) of int64 xs [B, hw, Cs]."""
    B, hw, Cs = xs.shape
    rows = hw // nch
    if rows * nch != hw or rows & (rows - 1):
        raise InexactCase(f"chunks of {hw}/{nch} rows are not a power of two")
    t = xs.reshape(B, nch, rows, Cs)
    s, q = t.sum(2), (t * t).sum(2)
    want = torch.stack([s.double() / rows, (rows * q - s * s).double() / rows], -1)
    p = want.float()
    if not torch.equal(p.double(), want):
        raise InexactCase("a chunk's (mean, M2) is not representable in fp32")
    return p


def case_partials(case, x):
    """The partials of each source, chunked as the case says."""
    out, c0 = [], 0
    for ci, n in zip(case.cins, case.nch):
        out.append(chunk_partials(x[:, :, c0:c0 + ci], n))
        c0 += ci
    return out


def merge_partials(parts, hw, groups):
    """(mean, var) float64 [B, groups] from the fp32 partials GIVEN (one [B, nch_i, C_i, 2] per source)."""
    means, m2s = [], []
    for p in parts:
        m, q = p[..., 0].double(), p[..., 1].double()
        rows = hw / p.shape[1]
        mc = m.mean(1)
        means.append(mc)
        m2s.append(q.sum(1) + rows * ((m - mc[:, None]) ** 2).sum(1))
    mc, qc = torch.cat(means, -1), torch.cat(m2s, -1)
    B, C = mc.shape
    cg = C // groups
    mc, qc = mc.reshape(B, groups, cg), qc.reshape(B, groups, cg)
    mg = mc.mean(2)
    m2g = qc.sum(2) + hw * ((mc - mg[:, :, None]) ** 2).sum(2)
    return mg, m2g / (hw * cg)


class Affine:
    """scale_ref, shift_ref, the group mean per channel (float64 [B, C]) and the two bounds."""

    def __init__(self, mean, var, eps, gamma, beta, cg, amax=2048.0):
        """``amax``: max |x| of the data (float or [B, 1]); 2048 is the families' limit."""
        B = mean.shape[0]
        C = mean.shape[1] * cg
        e = float(np.float32(eps))
        g = torch.ones(C, dtype=torch.float64) if gamma is None else gamma.double()
        b = torch.zeros(C, dtype=torch.float64) if beta is None else beta.double()
        r = 1.0 / torch.sqrt(var + e)
        self.mean = mean.repeat_interleave(cg, 1)
        self.scale = g[None, :] * r.repeat_interleave(cg, 1)
        self.shift = b[None, :] - self.mean * self.scale
        self.bound_scale = 2.0 ** -23 * self.scale.abs() * SLACK
        self.bound_shift = (2.0 ** -22 * (self.mean * self.scale).abs() + 2.0 ** -24 * self.shift.abs()) * SLACK
        self.bound_shift = self.bound_shift + DBL_MEAN * amax * self.scale.abs()
        assert self.scale.shape == (B, C)

    def ratios(self, scale, shift):
        """(max |scale - ref| / bound, max |shift - ref| / bound); NaN / Inf give inf."""
        sc, sh = scale.double().cpu(), shift.double().cpu()
        if not (torch.isfinite(sc).all() and torch.isfinite(sh).all()):
            return float("inf"), float("inf")
        rs = ((sc - self.scale).abs() / self.bound_scale).max().item()
        tiny = torch.finfo(torch.float64).tiny
        rh = ((sh - self.shift).abs() / self.bound_shift.clamp_min(tiny)).max().item()
        return rs, rh

    def y_interval(self, x, case):
        """(lo, hi) fp16 [B, H + 2 pad, W + 2 pad, C] the applied output must lie in (zero border), and the share of
        elements whose interval is a single value."""
        B, hw, C = x.shape
        xd = x.double()
        xs = xd * self.scale[:, None, :]
        y = xs + self.shift[:, None, :]
        E = xd.abs() * self.bound_scale[:, None, :] + self.bound_shift[:, None, :] + U32 * (xs.abs() + y.abs()) * SLACK
        lo = torch.from_numpy((y - E).numpy().astype(np.float16))
        hi = torch.from_numpy((y + E).numpy().astype(np.float16))
        p = case.pad
        shape = (B, case.H, case.W, C)
        pad = lambda t: torch.nn.functional.pad(t.reshape(shape), (0, 0, p, p, p, p))
        self.y_once = pad(torch.from_numpy(y.numpy().astype(np.float16)))       # float64 rounded once
        # where E is below half an fp16 ulp of y64 the 1-ulp bound follows from the roundings (the border: exact 0)
        self.y_tight = torch.nn.functional.pad((E < 0.5 * fp16_ulp(y)).reshape(shape), (0, 0, p, p, p, p), value=True)
        return pad(lo), pad(hi), (lo == hi).double().mean().item()


def reference(case, x, eps, gamma, beta, parts=None):
    """The case's Affine: from the partials for the routes that merge them, else from the exact sums."""
    if parts is not None:
        mean, var = merge_partials(parts, case.hw, case.groups)
    else:
        mean, var = exact_stats(x, case.groups)
    return Affine(mean, var, eps, gamma, beta, case.cg, x.abs().amax((1, 2)).double()[:, None])


# --------------------------------------------------------------------------- what the convs emit

def phase_major(y):
    """[B, 2H, 2W, C] -> [B, 4 H W, C]: an image's pixels in the phase form's chunk order."""
    b, h2, w2, ch = y.shape
    return y.reshape(b, h2 // 2, 2, w2 // 2, 2, ch).permute(0, 2, 4, 1, 3, 5).reshape(b, h2 * w2, ch)


def check_chunk_stats(part, y, s, phase=False, what=""):
    """Every (image, chunk, channel) pair of ``part`` fp32 [B, nch, C, 2] against the float64 (mean, M2) of the stored
    rows of exactly that chunk of ``y`` [B, H, W, C] (phase-major for the phase form), within s u A and s u 4 R A^2
    (s == 0: equality).  Returns the largest (mean error, M2 error) / bound (the absolute errors when s == 0)."""
    part, y = part.double().cpu(), y.double().cpu()
    B, nch, C, _ = part.shape
    rows_img = phase_major(y) if phase else y.reshape(B, -1, C)
    R = rows_img.shape[1] // nch
    assert R * nch == rows_img.shape[1], f"{what}: {nch} chunks do not divide {rows_img.shape[1]} rows"
    t = rows_img.reshape(B, nch, R, C)
    if not torch.equal(t, t.round()) or t.abs().max().item() > 2048:
        raise InexactCase(f"{what}: the stored output is not a small integer")
    mean = t.mean(2)
    m2 = ((t - mean[:, :, None]) ** 2).sum(2)
    A = t.abs().amax((2, 3), keepdim=False)[:, :, None].clamp_min(1.0)             # per (image, chunk)
    em, eq = (part[..., 0] - mean).abs(), (part[..., 1] - m2).abs()
    assert torch.isfinite(part).all(), f"{what}: a partial is not finite"
    if s == 0:
        bad = (em != 0) | (eq != 0)
        rm, rq = em.max().item(), eq.max().item()
    else:
        bm, bq = s * U32 * A, s * U32 * 4 * R * A * A
        bad = (em > bm) | (eq > bq)
        rm, rq = (em / bm).max().item(), (eq / bq).max().item()
    if bad.any():
        b, k, c = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} (image, chunk, channel) pairs off; first "
                             f"(image {b}, chunk {k} of {nch} x {R} rows, channel {c}): got ({part[b, k, c, 0].item()!r}, "
                             f"{part[b, k, c, 1].item()!r}) want ({mean[b, k, c].item()!r}, {m2[b, k, c].item()!r}), "
                             f"s = {s}")
    return rm, rq


def selector_conv(name, B, H, W, cin, cout, k, epilogue=True):
    """A conv whose stored fp16 output is a small integer the test knows (|y| <= 16): each output channel's weight is
    one-hot on one (input channel, tap); x in [-6, 6], bias and the embedding row in [-3, 3], the residual in
    [-4, 4].  Returns the keyword arguments of conv_exact_util.Case."""
    s = seed_of(f"gn-sel-{name}")
    x = hashed_ints(s, B * H * W, cin, -6, 6).reshape(B, H, W, cin).half()
    sel = hashed(s + 1, 1, cout, cin * k * k)[0]
    w = torch.zeros(cout, cin * k * k)
    w[torch.arange(cout), sel] = 1.0
    kw = dict(srcs=[x], w=w.reshape(cout, cin, k, k), ksize=k, pad=k // 2,
              bias=hashed_ints(s + 2, 1, cout, -3, 3)[0].float())
    if epilogue:
        kw["row_bias"] = (hashed_ints(s + 3, B, cout + 24, -3, 3).float(), 17)
        kw["residual"] = hashed_ints(s + 4, B * H * W, cout, -4, 4).reshape(B, H, W, cout).half()
    return kw
