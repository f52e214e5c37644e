"""Exact-arithmetic cases for the fused GEGLU feed-forward (csrc/ff.hip) and the helpers it shares with the
token linear's cases (tests/token_exact_util.py): hashed integer inputs, NaN / sentinel guarded row buffers.
tests/test_gpu_ff_exact.py runs the cases on the GPU, tests/test_ff_exact_inputs.py checks them on the CPU.
Nothing of the product package is imported here.

out = res + W2 (a * gelu(g)) + b2, [a | g] = t W1^T + b1, with three fp16 roundings: h = a gelu(g),
acc + b2, then + res.

Integer family.  t, W1's `a` rows, W2, b1, b2 and res are small integers picked by a hash of (case, row,
column), so every token, feature and channel is distinct.  A gate row of W1 has at most three +-1 entries and
a per-feature offset (in b1, or as the weight of a pilot column whose t is 1 in every row) that puts g into
  ON    g >= 6:  1 - erf(6 / sqrt 2) = 2e-9 < 2^-25, so gelu(g) is g in fp32 and h = fp16(a g);
  OFF   g <= -8: |a gelu(g)| < 2^15 * 8 * 6.3e-16 is below half the smallest fp16 subnormal, h = +-0;
  ZERO  an empty gate row and zero offset: g = 0, h = +-0.
Every partial sum of both GEMMs (bounded by the sum of |terms|) and a g stay below 2^24, |acc + b2| and the
final sum below 65504: each fp16 rounding is one correct rounding of an exactly known integer, and the
float64 reference applies the same three.  The kernel must EQUAL it (``==``: the kernel's off-gate h is -0).

Pointwise family.  One-hot t rows and one-hot W2 rows make out[m, c] = fp16(a gelu(g)) for a single
(a, g) = (W1[f, col], W1[F + f, col] + b1[F + f]): it reads gelu itself, over a grid of fp16-exact g in [-8, 8].

``reference`` functions raise ``InexactCase`` when a case breaks its own conditions."""
import math
import zlib

import numpy as np
import torch

from conv_exact_util import SENTINEL, InexactCase

C = 320                     # model channels
PRE, POST = 2, 130          # guard rows before / after the payload (130 > the feed-forward's 128-row block)
F16_MAX = 65504.0
ON, OFF, ZERO = 1, 2, 0
PILOT = 317                 # the column whose t is 1 in every row

_M1, _M2, _M3 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def seed_of(name):
    return zlib.crc32(name.encode())


def hash_u64(seed, rows, cols):
    """splitmix64 of (seed, row, column): uint64 [len(rows), len(cols)]."""
    with np.errstate(over="ignore"):
        r = np.asarray(rows, dtype=np.uint64)[:, None] * np.uint64(_M1)
        c = np.asarray(cols, dtype=np.uint64)[None, :] * np.uint64(_M2)
        x = r + c + np.uint64(seed) * np.uint64(_M3) + np.uint64(_M1)
        x ^= x >> np.uint64(30)
        x *= np.uint64(_M2)
        x ^= x >> np.uint64(27)
        x *= np.uint64(_M3)
        x ^= x >> np.uint64(31)
    return x


def hashed(seed, nr, nc, n):
    """int64 [nr, nc] in [0, n) by the hash of (seed, row, column)."""
    h = hash_u64(seed, np.arange(nr), np.arange(nc)) >> np.uint64(20)
    return torch.from_numpy((h % np.uint64(n)).astype(np.int64))


def hashed_ints(seed, nr, nc, lo, hi):
    return hashed(seed, nr, nc, hi - lo + 1) + lo


def hashed_pick(seed, nr, nc, values):
    return torch.tensor(values, dtype=torch.float64)[hashed(seed, nr, nc, len(values))]


# --------------------------------------------------------------------------- the integer family

FF_MS = (1, 33, 128, 129, 300)
FF_FS = (32, 64, 96, 1280)
# every F with M = 129 and M = 300, every M with F = 96, F = 1280 with M = 33
FF_SHAPES = sorted({(m, f) for m in (129, 300) for f in FF_FS} | {(m, 96) for m in FF_MS} | {(33, 1280)})
FF_RES = ("none", "res", "alias")
FF_LDS = {"dense": (320, 320, 320), "strided": (328, 336, 344)}      # (t_ld, res_ld, out_ld)


class FFInputs:
    """CPU inputs of one integer case: t [M, 320], w1 [2F, 320], w2 [320, F] fp16; b1 [2F], b2 [320] fp32 or
    None; res [M, 320] fp16; cls [F] (ON / OFF / ZERO)."""

    def __init__(self, M, F, has_b1=True, has_b2=True):
        self.name = f"ff-M{M}-F{F}-b1{int(has_b1)}-b2{int(has_b2)}"
        self.M, self.F = M, F
        s = seed_of(f"ff-F{F}-b1{int(has_b1)}")           # rows are hashed by their index: M only truncates
        t = hashed_ints(s + 1, M, C, -2, 2)
        t[:, PILOT] = 1
        fb, r = torch.arange(F) // 16, torch.arange(F) % 16
        # ON / OFF alternate over the groups of 4 features (slot 8 (l/32) + j <-> feature 8 (j/4) + 4 (l/32) + j%4
        # maps a lane half's 4 registers to one group) and over the blocks; one ZERO feature per block
        cls = torch.where((r // 4 + fb) % 2 == 0, ON, OFF)
        cls[16 * torch.arange(F // 16) + hashed(s + 2, F // 16, 1, 16)[:, 0]] = ZERO
        off = torch.where(cls == ON, 12 + hashed(s + 3, F, 1, 4)[:, 0], -(14 + hashed(s + 4, F, 1, 4)[:, 0]))
        off[cls == ZERO] = 0
        w1 = torch.zeros(2 * F, C, dtype=torch.int64)
        w1[:F] = hashed_pick(s + 5, F, C, (-2, -1, 1, 2)).long()          # dense: every column reaches every feature
        cols = hashed(s + 6, F, 3, C - 1)
        cols = cols + (cols >= PILOT)                                      # never the pilot column
        sign = hashed(s + 7, F, 3, 2) * 2 - 1
        n = hashed(s + 8, F, 1, 4)[:, 0]                                   # 0 .. 3 entries
        for k in range(3):
            use = (n > k) & (cls != ZERO)
            f = torch.arange(F)[use]
            w1[F + f, cols[use, k]] = sign[use, k]
        b1 = None
        if has_b1:
            b1 = torch.cat([hashed_ints(s + 9, F, 1, -8, 8)[:, 0], off]).float()
        else:
            w1[F:, PILOT] = off
        density = min(1.0, 48.0 / F)
        w2 = hashed_pick(s + 10, C, F, (-2, -1, 1, 2)).long()
        w2 = w2 * (hashed(s + 11, C, F, 1 << 20) < int(density * (1 << 20)))
        self.t, self.w1, self.w2 = t.half(), w1.half(), w2.half()
        self.b1 = b1
        self.b2 = hashed_ints(s + 12, 1, C, -2000, 2000)[0].float() if has_b2 else None
        self.res = hashed_ints(s + 13, M, C, -2000, 2000).half()
        self.cls = cls


def _need(ok, msg):
    if not ok:
        raise InexactCase(msg)


def _ff_conditions(c, with_res, on_min=6.0):
    """Float64 evaluation with every condition checked; returns (h, acc + b2 as fp16, final) as float64.
    ``on_min`` is the ON class's lower bound (6: below it gelu(g) is no longer g in fp32, which the check of h
    against fp16(a g) then reports)."""
    F = c.F
    t, w1, w2 = c.t.double(), c.w1.double(), c.w2.double()
    b1 = c.b1.double() if c.b1 is not None else torch.zeros(2 * F, dtype=torch.float64)
    b2 = c.b2.double() if c.b2 is not None else torch.zeros(C, dtype=torch.float64)
    for what, v in (("t", t), ("w1", w1), ("w2", w2), ("b1", b1), ("b2", b2), ("res", c.res.double())):
        _need(torch.equal(v, v.round()), f"{c.name}: {what} is not integral")
    _need((t.abs() @ w1.abs().T + b1.abs()).max().item() < 2 ** 24, f"{c.name}: a partial sum of t W1^T can reach 2^24")
    y = t @ w1.T + b1
    a, g = y[:, :F], y[:, F:]
    on, off, zero = (c.cls == ON)[None, :], (c.cls == OFF)[None, :], (c.cls == ZERO)[None, :]
    _need(bool(((g >= on_min) | ~on).all()), f"{c.name}: an ON gate is below {on_min:g}")
    _need(bool(((g <= -8) | ~off).all()), f"{c.name}: an OFF gate is above -8")
    _need(bool(((g == 0) | ~zero).all()), f"{c.name}: a ZERO gate is not 0")
    _need(a.abs().max().item() < 2 ** 15, f"{c.name}: |a| reaches 2^15 (the OFF class needs less)")
    _need((a * g).abs().max().item() < 2 ** 24, f"{c.name}: a g can reach 2^24")
    h = (a * 0.5 * g * (1.0 + torch.erf(g / math.sqrt(2.0)))).float().half()      # fp32, then the fp16 rounding
    expect = torch.where(on, a * g, torch.zeros_like(a))
    _need(expect.abs().max().item() < F16_MAX, f"{c.name}: h overflows fp16")
    _need(torch.equal(h.double(), expect.float().half().double()), f"{c.name}: fp16(a gelu(g)) is not fp16(a g) / 0")
    h = h.double()
    _need((h.abs() @ w2.abs().T + b2.abs()).max().item() < 2 ** 24, f"{c.name}: a partial sum of h W2^T can reach 2^24")
    acc = h @ w2.T + b2
    _need(acc.abs().max().item() < F16_MAX, f"{c.name}: |acc + b2| reaches 65504")
    pre = acc.float().half().double()
    out = pre
    if with_res:
        s = pre + c.res.double()
        _need(s.abs().max().item() < F16_MAX, f"{c.name}: |acc + b2 + res| reaches 65504")
        out = s.float().half().double()
    return h, pre, out


def ff_reference(c, with_res, on_min=6.0):
    """fp16 reference [M, 320]; raises InexactCase unless the conditions hold."""
    return _ff_conditions(c, with_res, on_min)[2].half()


def ff_reference_f32(c, with_res, perm_seed):
    """The same evaluation in float32 with both summations in a permuted order (exactness makes it equal)."""
    F = c.F
    g = torch.Generator().manual_seed(perm_seed)
    p1, p2 = torch.randperm(C, generator=g), torch.randperm(F, generator=g)
    y = torch.zeros(c.M, 2 * F)
    for ks in torch.chunk(p1, 5):                                           # explicit partial sums
        y = y + c.t.float()[:, ks] @ c.w1.float()[:, ks].T
    if c.b1 is not None:
        y = y + c.b1
    h = (y[:, :F] * torch.nn.functional.gelu(y[:, F:])).half().float()
    acc = torch.zeros(c.M, C)
    for ks in torch.chunk(p2, 4):
        acc = acc + h[:, ks] @ c.w2.float()[:, ks].T
    if c.b2 is not None:
        acc = acc + c.b2
    out = acc.half()
    if with_res:
        out = (out.float() + c.res.float()).half()
    return out


_FF = {}


def ff_case(M, F, has_b1=True, has_b2=True):
    """The inputs and both references, built once per process (shared: do not modify)."""
    k = (M, F, has_b1, has_b2)
    if k not in _FF:
        c = FFInputs(M, F, has_b1, has_b2)
        c.ref = {False: ff_reference(c, False), True: ff_reference(c, True)}
        _FF[k] = c
    return _FF[k]


# --------------------------------------------------------------------------- the pointwise family

PW_F, PW_M = 320, 320
PW_A = (1.0, -1.0, 8.0, 1024.0)
# fp16-exact gates in [-8, 8]: every multiple of 1/8 (the integers and the steps of 1/8 in [-6, -2] among
# them), -0, and every multiple of 1/256 inside (-4, 4).  The fine steps are what sees an erf error of the
# centre: there a gelu(g) is far above its fp16 ulp, and an error of 1e-6 shows only where the exact value
# lies that close to a rounding boundary - about one g in a hundred
PW_G = (tuple(k / 8.0 for k in range(-64, 65)) + (-0.0,) +
        tuple(k / 256.0 for k in range(-1023, 1024) if k % 32))
# the erf-equivalent error of csrc/common.h erf_fast as the fp16 output shows it, measured on the MI355X
# (profiles/ff_exact_gelu_errors.txt); the test asserts twice that, which has to stay below 1e-6
PW_E_MEASURED = 1.3744e-7
PW_E = 2 * PW_E_MEASURED


class PointwiseCase:
    """t = one-hot rows (row m -> column m), W2 = one-hot rows (channel c -> feature (7 c + 3) % 320), so
    out[m, c] = fp16(a gelu(g)) with a = w1[f, m] and g = w1[F + f, m] + b1[F + f]."""

    def __init__(self, gates=PW_G):
        s = seed_of("ff-pointwise")
        F = PW_F
        self.name, self.M, self.F = "ff-pointwise", PW_M, F
        self.t = torch.eye(PW_M, C).half()
        self.feat = (7 * torch.arange(C) + 3) % F
        w2 = torch.zeros(C, F)
        w2[torch.arange(C), self.feat] = 1
        self.w2 = w2.half()
        # (a, g) per (feature, column): a walk of stride 7919 through the grid, so every pair is read (12 times)
        k = (torch.arange(F * C).view(F, C) * 7919 + s) % (len(gates) * len(PW_A))
        a = torch.tensor(PW_A, dtype=torch.float64)[k // len(gates)]
        g = torch.tensor(gates, dtype=torch.float64)[k % len(gates)]
        boff = (hashed_ints(s + 3, F, 1, -8, 8)[:, 0] / 8.0).double()        # b1 of the gate rows: multiples of 1/8
        wg = g - boff[:, None]                                # -0 stays -0 where b1 is 0
        self.w1 = torch.cat([a, wg]).half()
        self.b1 = torch.cat([torch.zeros(F, dtype=torch.float64), boff]).float()
        _need(torch.equal(self.w1.double(), torch.cat([a, wg])), "pointwise: W1 is not fp16-exact")
        # [M, C] views of (a, g) of each output element, float64
        self.a = a[self.feat][:, :PW_M].T.contiguous()
        self.g = (self.w1.double()[F:] + boff[:, None])[self.feat][:, :PW_M].T.contiguous()
        _need(bool((self.g.abs() <= 8).all()), "pointwise: a gate leaves [-8, 8]")
        self.ref = self.a * 0.5 * self.g * (1.0 + torch.erf(self.g / math.sqrt(2.0)))
        self.b2, self.res = None, None


def fp16_ulp(x):
    """The fp16 spacing at |x| (float64 tensor): 2^(floor(log2 |x|) - 10), 2^-24 in the subnormal range."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -14)))
    return torch.exp2(e - 10)


def pointwise_tolerance(c, E):
    """|a| 0.5 |g| E for the erf error plus half an fp16 ulp of the reference h (taken at |ref| + the first
    term, where the fp32 value that is rounded can lie)."""
    d = c.a.abs() * 0.5 * c.g.abs() * E
    return d + 0.5 * fp16_ulp(c.ref.abs() + d)


def pointwise_measure(c, got):
    """(E, worst g, its a, worst error in fp16 ulps of gelu(g)): E is the smallest erf-equivalent error that
    satisfies ``pointwise_tolerance`` for ``got`` [M, C] (float64), as far as the fp16 output shows it."""
    err = (got - c.ref).abs()
    scale = c.a.abs() * 0.5 * c.g.abs()
    e = ((err - 0.5 * fp16_ulp(c.ref)).clamp_min(0) / scale.clamp_min(1e-30)) * (scale > 0)
    i = int(e.argmax())
    ulps = err / fp16_ulp(c.ref)
    j = int(ulps.argmax())
    return (e.flatten()[i].item(), c.g.flatten()[i].item(), c.a.flatten()[i].item(),
            ulps.flatten()[j].item(), c.g.flatten()[j].item(), c.a.flatten()[j].item())


_PW = []


def pointwise_case():
    if not _PW:
        _PW.append(PointwiseCase())
    return _PW[0]


# --------------------------------------------------------------------------- guarded row buffers

def guarded_rows(t, ld, device):
    """(buffer, view): ``t`` [M, 320] fp16 inside a NaN-filled [PRE + M + POST, ld] buffer."""
    M = t.shape[0]
    buf = torch.full((PRE + M + POST, ld), float("nan"), dtype=torch.float16, device=device)
    view = buf[PRE:PRE + M, :C]
    view.copy_(t)
    return buf, view


def out_rows(M, ld, device, payload=None):
    """(buffer, the output view [M, 320]): sentinel-filled [PRE + M + POST, ld]; ``payload`` (the residual of an
    in-place call) goes into the view."""
    buf = torch.full((PRE + M + POST, ld), SENTINEL, dtype=torch.float16, device=device)
    view = buf[PRE:PRE + M, :C]
    if payload is not None:
        view.copy_(payload)
    return buf, view


def split_rows(buf, M):
    """(payload [M, 320] fp16 on the CPU, guard cells that lost the sentinel, payload cells that still hold it)."""
    b = buf.cpu()
    got = b[PRE:PRE + M, :C].contiguous()
    hit = b != SENTINEL
    hit[PRE:PRE + M, :C] = False
    return got, int(hit.sum()), int((got == SENTINEL).sum())


# --------------------------------------------------------------------------- comparison and report

def ff_where(m, ch, feature=None):
    """Who computes out[m, ch] in ff_geglu_kernel (and, for a known feature, who computes that h)."""
    row = ch % 32
    s = (f"workgroup {m // 128}, wave pair {m % 128 // 32}, lane token {m % 32}; channel half {ch // 160} "
         f"(waves +{4 * (ch // 160)}), output block {ch % 160 // 32}, lane half {row // 4 % 2}, "
         f"accumulator register {4 * (row // 8) + row % 4}")
    if feature is not None:
        fb, r = feature // 16, feature % 16
        hh, j = r // 4 % 2, 4 * (r // 8) + r % 4
        s += (f"; feature {feature}: block {fb} (iteration {fb // 2}, ring slot {fb // 2 % 2}, wave half {fb % 2}), "
              f"lane half {hh}, register j {j}, W2 slot {8 * hh + j}")
    return s


def mismatch_report(name, got, ref, where=None, first=5, tol=None):
    """None when ``got`` == ``ref`` element for element (-0 == 0; NaN never equals) or, with ``tol``, lies within
    it; else a report of the first wrong (row, channel)s."""
    if tol is None:
        bad = ~(got == ref)
    else:
        bad = ~((got - ref).abs() <= tol)
    nbad = int(bad.sum())
    if nbad == 0:
        return None
    rows = bad.any(1).nonzero().flatten()
    lines = [f"{name}: {nbad} of {ref.numel()} elements differ, in {rows.numel()} rows "
             f"({rows[0].item()} .. {rows[-1].item()}) and {int(bad.any(0).sum())} channels"]
    for m, ch in bad.nonzero()[:first].tolist():
        lines.append(f"  (row {m}, channel {ch}): got {got[m, ch].item()!r} want {ref[m, ch].item()!r}")
        if where is not None:
            lines.append(f"    {where(m, ch)}")
    return "\n".join(lines)
