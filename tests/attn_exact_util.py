"""Exact-arithmetic inputs for the flash attention kernel (csrc/attention.hip) and the fused
cross-attention block (csrc/xattn.hip).  CPU only: nothing here imports the product package.

``SCALE`` = float32(1 / log2(e)): the kernel's c = scale * log2(e) is then 1 to within an fp32 ulp, so
half(q * c) == q for the small integers used here and every score is an exact integer in the exp2
domain (P = 2^(s - m)).

One-hot family (``onehot``): K rows are +-1 codes of the key index over all d columns, query row i is
A * code(f(i)); the winner f(i) beats every other key by >= 64, so every loser's P (<= 2^-56 against
any admissible running max, which lies at most 8 below the true one) rounds to fp16 zero, the
winner's P is a power of two, what an earlier tile left in the accumulators is rescaled by <= 2^-64
(below half an fp32 ulp of the winner's term), and the output row must EQUAL V[f(i)] bit for bit.
V is an integer code < 2048 of (batch, key, head, column).

Weighted family (``weighted``): Q has 2-3 entries of +-1 per row in columns that rotate with the row, K
is dense in {-1, 0, 1}, V an integer in [1, VMAX].  The scores of a row spread over S <= 6 < 8 = the
kernel's deferral headroom, so its running max is the first tile's max and never moves, P = 2^(s - m)
lies in [2^-S, 2^S] (exact in fp16), and every partial sum of P V and of P is a multiple of 2^-S below
nk * 2^S * VMAX: exact in fp32, in any order, when nk * 4^S * VMAX < 2^24 (asserted per case).  The
output is then the correctly rounded fp32 product of that exact numerator with the fp32 reciprocal of
the exact denominator, rounded once more to fp16: within 1 fp16 ulp of the float64 quotient's fp16."""
import math

import torch

SCALE = float(torch.tensor(1.0 / 1.4426950408889634, dtype=torch.float32))
KT = 64            # keys per tile of the kernel
GAP = 64           # one-hot: the winner's margin in the exp2 domain
VMAX = 15
NAN = float("nan")
SENTINEL = -1234.0


class InexactCase(Exception):
    """A case that does not meet its exactness conditions: a test error, not a comparison failure."""


# ----------------------------------------------------------------------------- forms
# form -> {head dims} and the template arguments (DQK, DV, waves, query blocks, stagger, seed column)
FORM_DIMS = {
    "nw4": (8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 96, 128, 152, 160),
    "nw8": (40, 48, 56, 64, 72, 80),
    "nw8_stag": (40, 48, 56, 64, 72, 80),
    "qb2": (40, 48),
}
ALL_DIMS = FORM_DIMS["nw4"]


def _pad(d):
    """(DQK, DV) of a head dim."""
    for hi, dqk, dv in ((16, 16, 32), (32, 32, 32), (48, 48, 64), (64, 64, 64), (80, 80, 96), (96, 96, 96),
                        (128, 128, 128), (160, 160, 160)):
        if d <= hi:
            return dqk, dv
    raise ValueError(d)


def auto_form(d):
    """Today's default form of a head dim (no tuning knob in the environment)."""
    if d <= 32 or d > 80:
        return "nw4"
    return "nw8" if d <= 48 else "nw8_stag"


def expected_info(form, d, causal=False):
    """What ``form_out`` must report for a legal (form, d): the instantiation table of attention.hip."""
    f = auto_form(d) if form == "auto" else form
    assert d in FORM_DIMS[f], (form, d)
    dqk, dv = _pad(d)
    waves = 4 if f in ("nw4", "qb2") else 8
    stag = 1 if f == "nw8_stag" and not causal else 0
    seed = 40 if d == 40 and waves == 8 and not causal else 0
    return dict(form=f, dqk=dqk, dv=dv, waves=waves, qblocks=2 if f == "qb2" else 1, stagger=stag, seed_col=seed,
                causal=1 if causal else 0)


def rows_of(form, d):
    """Query rows per workgroup."""
    e = expected_info(form, d)
    return 32 * e["waves"] * e["qblocks"]


# ----------------------------------------------------------------------------- codes
def _sign_codes(n, d, const_cols):
    """[n, d] +-1 codes of 0..n-1: column c carries bit c % period of the index (flipped in every other
    repeat, so a column is not a copy of another); with ``const_cols`` one slot of the period is +1 for
    every key.  Distinct indices differ in at least one column.  2^d < n (d = 8, n = 257): codes with one
    zero, at column j % d, and the bits of j // d in the other columns (equal norms again)."""
    nbits = max(1, (n - 1).bit_length())
    j = torch.arange(n).view(n, 1)
    c = torch.arange(d).view(1, d)
    if nbits + (1 if const_cols else 0) > d:
        if const_cols or (1 << (d - 1)) * d < n:
            raise InexactCase(f"no room for {n} distinct codes in {d} columns")
        slot = (c - j % d - 1) % d                     # 0..d-2 for the non-zero columns, d-1 at the zero
        code = 1 - 2 * (((j // d) >> slot.clamp(max=d - 2)) & 1)
        return torch.where(slot == d - 1, torch.zeros_like(code), code).double(), torch.zeros(d, dtype=torch.bool)
    period = nbits + (1 if const_cols else 0)
    slot, rep = c % period, c // period
    code = 1 - 2 * (((j >> slot.clamp(max=nbits - 1)) & 1) ^ (rep & 1))
    is_const = (slot == nbits).expand(1, d).reshape(d)
    code = torch.where(is_const.view(1, d), torch.ones_like(code), code)
    return code.double(), is_const


def _amplitude(codes, is_const):
    """Smallest power of two A with A * (self score - best other score) >= GAP for every key."""
    u = codes[:, ~is_const] @ codes[:, ~is_const].T
    n = u.shape[0]
    self_s = u.diagonal().clone()
    u.fill_diagonal_(-1e9)
    unit = (self_s - u.max(dim=1).values).min().item() if n > 1 else 1.0
    if unit <= 0:
        raise InexactCase("codes are not distinct")
    return 2 ** max(0, math.ceil(math.log2(GAP / unit)))


def v_codes(B, nk, H, d):
    b = torch.arange(B).view(B, 1, 1, 1)
    j = torch.arange(nk).view(1, nk, 1, 1)
    h = torch.arange(H).view(1, 1, H, 1)
    c = torch.arange(d).view(1, 1, 1, d)
    return ((37 * j + 11 * c + 401 * h + 997 * b) % 2039).double()


# ----------------------------------------------------------------------------- cases
class Case:
    """q [B, nq, H, d], k / v [B, nk, H, d] as float64 integers; ``ref`` [B*nq, H*d] fp16.
    one-hot: ``win`` [B, H, nq] the winning key, ``traps`` [(i, key)] (causal)."""

    def __init__(self, family, B, H, nq, nk, d, causal=False, negative=False):
        self.family, self.B, self.H, self.nq, self.nk, self.d = family, B, H, nq, nk, d
        self.causal, self.negative = causal, negative
        self.name = f"{family}{'-neg' if negative else ''}{'-causal' if causal else ''}-b{B}h{H}q{nq}k{nk}d{d}"
        self.ntiles = -(-nk // KT)
        self.win = self.traps = None
        if family == "onehot":
            _build_causal_onehot(self) if causal else _build_onehot(self)
        elif family == "weighted":
            _build_weighted(self)
        else:
            raise ValueError(family)
        for n, t, lim in (("q", self.q, 65504), ("k", self.k, 2048), ("v", self.v, 2048)):
            if not torch.equal(t, t.round()):
                raise InexactCase(f"{self.name}: {n} is not integral")
            if not torch.equal(t.half().double(), t) or t.abs().max().item() > lim:
                raise InexactCase(f"{self.name}: {n} is not an fp16 integer within the limit {lim}")
        self.q, self.k, self.v = self.q.half(), self.k.half(), self.v.half()     # exact (checked above)
        self.check_conditions()
        self.ref = reference(self, torch.float64)[2].half()
        if family == "onehot":
            idx = self.win.permute(0, 2, 1)                                           # [B, nq, H]
            vw = torch.gather(self.v, 1, idx.unsqueeze(-1).expand(B, nq, H, d))
            if not torch.equal(self.ref, vw.reshape(B * nq, H * d)):
                raise InexactCase(f"{self.name}: the float64 softmax is not V[f(i)]")

    def scores(self, dtype=torch.float64):
        """[B, H, nq, nk] integer scores in the exp2 domain; masked ones are -inf."""
        s = torch.einsum("bihc,bjhc->bhij", self.q.to(dtype), self.k.to(dtype))
        if self.causal:
            i = torch.arange(self.nq).view(-1, 1)
            j = torch.arange(self.nk).view(1, -1)
            s = s.masked_fill(j > i, float("-inf"))
        return s

    def check_conditions(self):
        s = self.scores()
        if s.abs()[s.isfinite()].max().item() >= 2 ** 24:
            raise InexactCase(f"{self.name}: a score leaves the fp32 integers")
        if self.d == 40 and not self.causal and s.abs()[s.isfinite()].max().item() > 2048:
            # the non-causal 8-wave d = 40 forms keep the running max as an fp16 in Q's padding column
            raise InexactCase(f"{self.name}: a running max would not be an fp16 integer")
        top2 = s.topk(min(2, self.nk), dim=-1).values
        if self.family == "onehot":
            if not torch.equal(s.argmax(-1), self.win):
                raise InexactCase(f"{self.name}: the intended winner does not win")
            if self.nk > 1 and (top2[..., 0] - top2[..., 1]).min().item() < GAP:
                raise InexactCase(f"{self.name}: one-hot gap below {GAP}")
            self.min_gap = (top2[..., 0] - top2[..., 1]).min().item() if self.nk > 1 else math.inf
            if self.negative and top2[..., 0].max().item() > -GAP:
                raise InexactCase(f"{self.name}: winning score above {-GAP}")
        else:
            lo = s.masked_fill(~s.isfinite(), float("inf")).min(-1).values
            self.spread = int((top2[..., 0] - lo).max().item())
            if self.spread >= 8:
                raise InexactCase(f"{self.name}: score spread {self.spread} reaches the deferral headroom")
            if self.nk * 4 ** self.spread * self.v.max().item() >= 2 ** 24:
                raise InexactCase(f"{self.name}: nk * 4^S * Vmax = {self.nk * 4 ** self.spread * int(self.v.max())} "
                                  f"leaves the fp32 integers (S = {self.spread})")
            if self.v.min().item() < 1:
                raise InexactCase(f"{self.name}: V must be positive (no cancellation)")


def reference(c, dtype):
    """(numerator [B*nq, H*d], denominator [B*nq, H], quotient [B*nq, H*d]) of softmax_2(s) V in ``dtype``,
    P taken against the first tile's maximum, as the kernel does whenever no score exceeds it by more
    than 8 (the weighted family); the quotient does not depend on that choice."""
    s = c.scores(dtype)
    if c.family == "weighted":
        m = s[..., :KT].max(-1, keepdim=True).values
    else:
        m = s.max(-1, keepdim=True).values
    p = torch.exp2(s - m)
    num = torch.einsum("bhij,bjhc->bihc", p, c.v.to(dtype))
    den = p.sum(-1).permute(0, 2, 1)                                                   # [B, nq, H]
    out = num / den.unsqueeze(-1)
    return (num.reshape(c.B * c.nq, c.H * c.d), den.reshape(c.B * c.nq, c.H),
            out.reshape(c.B * c.nq, c.H * c.d))


def winner_tile_plan(i, ntiles):
    """Tile of row i's winner: within every 32-row wave a third of the rows win in tile 0 (the running max
    never moves again), a third in the last tile (forced rescale after tile 0's decoys) and a third in a
    tile that rotates with the row and the wave."""
    r, w = i % 32, i // 32
    kind = r % 3
    return 0 if kind == 0 else ntiles - 1 if kind == 1 else (r // 3 + w) % ntiles


def _build_onehot(c):
    B, H, nq, nk, d = c.B, c.H, c.nq, c.nk, c.d
    codes, is_const = _sign_codes(nk, d, c.negative)
    A = _amplitude(codes, is_const)
    win = torch.empty(B, H, nq, dtype=torch.long)
    for i in range(nq):
        t = winner_tile_plan(i, c.ntiles)
        size = min(KT, nk - t * KT)
        for b in range(B):
            for h in range(H):
                win[b, h, i] = t * KT + (7 * i + 3 * h + 5 * b + 1) % size
    q = A * codes[win]                                                                # [B, H, nq, d]
    if c.negative:
        # every score drops by bias * (number of constant columns): the winner ends at <= -GAP, below the
        # score 0 of the zero K rows that the buffer range check supplies past nk
        ncst, dbits = int(is_const.sum()), int((~is_const).sum())
        bias = 32 * math.ceil((A * dbits + GAP) / (32 * ncst))
        q[..., is_const] = -float(bias)
    c.q = q.permute(0, 2, 1, 3).contiguous()
    c.k = codes.view(1, nk, 1, d).expand(B, nk, H, d).contiguous()
    c.v = v_codes(B, nk, H, d)
    c.win, c.amplitude = win, A


def _build_causal_onehot(c):
    """Two ramp columns next to the codes: K[j, d-1] = j and K[j, d-2] = j // 64.
    'diagonal' rows look at the first ramp only (q = 64 there): the score is 64 j, the winner is the
    last visible key min(i, nk - 1), and EVERY later key (i + 1 and the next tile's first key
    included) scores at least 64 above it and must be masked.
    'code' rows (i % 4 == 2, i < nk) pick f(i) <= i in their own tile by its code and weigh the tile ramp by
    W = 2 A dc + 64: earlier tiles are lower by >= 64, the next tile's first key higher by >= 64."""
    B, H, nq, nk, d = c.B, c.H, c.nq, c.nk, c.d
    dc = d - 2
    codes, is_const = _sign_codes(nk, dc, False)
    A = _amplitude(codes, is_const)
    W = 2 * A * dc + GAP
    k = torch.zeros(nk, d, dtype=torch.float64)
    k[:, :dc] = codes
    k[:, d - 1] = torch.arange(nk)
    k[:, d - 2] = torch.arange(nk) // KT
    q = torch.zeros(B, H, nq, d, dtype=torch.float64)
    win = torch.empty(B, H, nq, dtype=torch.long)
    traps, kinds = [], []
    for i in range(nq):
        last = min(i, nk - 1)
        code_row = i % 4 == 2 and i < nk
        kinds.append("code" if code_row else "diag")
        if code_row:
            t0 = KT * (i // KT)
            for b in range(B):
                for h in range(H):
                    f = t0 + (5 * i + 3 * h + b + 1) % (i - t0 + 1)
                    win[b, h, i] = f
                    q[b, h, i, :dc] = A * codes[f]
            q[:, :, i, d - 2] = W
        else:
            win[:, :, i] = last
            q[:, :, i, d - 1] = GAP
            if i + 1 < nk:
                traps.append((i, i + 1))
        nxt = KT * (i // KT + 1)
        if nxt < nk:
            traps.append((i, nxt))
    c.q = q.permute(0, 2, 1, 3).contiguous()
    c.k = k.view(1, nk, 1, d).expand(B, nk, H, d).contiguous()
    c.v = v_codes(B, nk, H, d)
    c.win, c.traps, c.kinds, c.amplitude = win, traps, kinds, A


def trap_margins(c):
    """For every (row, trap key) of a causal one-hot case: (trap key - row, unmasked trap score - winner's
    score) minimised over batch and head."""
    un = torch.einsum("bihc,bjhc->bhij", c.q.double(), c.k.double())
    s = c.scores()
    best = s.max(-1).values
    return [(j - i, (un[:, :, i, j] - best[:, :, i]).min().item()) for i, j in c.traps]


def _build_weighted(c):
    B, H, nq, nk, d = c.B, c.H, c.nq, c.nk, c.d
    g = torch.Generator().manual_seed(1000 * d + nk + 7 * nq + (1 if c.causal else 0))
    c.k = torch.randint(-1, 2, (B, nk, H, d), generator=g).double()
    c.v = torch.randint(1, VMAX + 1, (B, nk, H, d), generator=g).double()
    q = torch.zeros(B, nq, H, d, dtype=torch.float64)
    for i in range(nq):
        n = 3 if i % 3 == 0 else 2
        for h in range(H):
            for e in range(n):
                col = (2 * i + 5 * h + e) % d
                q[:, i, h, col] = 1.0 if (i + e + h) % 2 == 0 else -1.0
    if B > 1:
        q[1:] = 0.0 - q[1:]
    c.q = q


_CASES = {}


def get_case(family, B, H, nq, nk, d, causal=False, negative=False):
    """Built once and shared by the forms of a head dim; only the latest head dim's cases are kept."""
    key = (family, B, H, nq, nk, d, causal, negative)
    if key not in _CASES:
        if any(k[5] != d for k in _CASES):
            _CASES.clear()
        _CASES[key] = Case(*key)
    return _CASES[key]


# ----------------------------------------------------------------------------- shapes of the GPU tests
NKS = (20, 64, 129, 257)
CAUSAL_N = (77, 129, 325)
BATCH, HEADS = 2, 3


def noncausal_specs(form, d):
    """(family, B, H, nq, nk, negative, layout) for one (form, d): both families at every nk with
    nq = ROWS + 69 (a full workgroup, then two full waves, a 5-row wave and empty waves), the negative
    one-hot winner at the ragged nk, one nq = 5 case, one grid below 8 blocks and one nq == nk packed qkv."""
    rows = rows_of(form, d)
    nq = rows + 69
    out = []
    for n, nk in enumerate(NKS):
        lay = ("sep", "kv")[n % 2]
        out.append(("onehot", BATCH, HEADS, nq, nk, False, lay))
        out.append(("weighted", BATCH, HEADS, nq, nk, False, ("kv", "sep")[n % 2]))
    for nk in (20, 129):
        if nk == 129 and d < 16:
            continue                                       # 8 code bits and the constant column need 9 columns
        out.append(("onehot", BATCH, HEADS, nq, nk, True, "sep"))
    out.append(("onehot", BATCH, HEADS, 5, 129, False, "kv"))
    out.append(("weighted", 1, 2, rows + 5, 257, False, "sep"))         # 4 blocks: xcd_remap with q = 0
    out.append(("onehot", 1, HEADS, 129, 129, False, "qkv"))
    out.append(("weighted", BATCH, HEADS, 77, 77, False, "qkv"))
    return out


def causal_specs(d, full):
    """(family, B, H, nq, nk, layout): ``full`` = the head dims the issue names (every n, one nq != nk)."""
    out = []
    for n in (CAUSAL_N if full else (129,)):
        out.append(("onehot", BATCH, HEADS, n, n, "qkv" if n == 129 else "sep"))
    out.append(("weighted", BATCH, HEADS, 129, 129, "sep"))
    if full:
        out.append(("onehot", BATCH, HEADS, 90, 77, "kv"))               # rows 77.. see every key; ragged tile
        out.append(("onehot", BATCH, HEADS, 70, 129, "sep"))             # tiles past the last query row skipped
    return out


# ----------------------------------------------------------------------------- guards
def guarded(x2d, gap, dev, pre=3, post=2):
    """x2d [rows, cols] placed in a NaN-filled fp16 buffer [pre + rows + post, cols + gap]; returns the view."""
    rows, cols = x2d.shape
    buf = torch.full((pre + rows + post, cols + gap), NAN, dtype=torch.float16)
    buf[pre:pre + rows, :cols] = x2d.half()
    return buf.to(dev)[pre:pre + rows, :cols]


def guarded_qkv(c, layout, dev):
    """Device views (q, k, v) of a case in NaN-guarded buffers: 'sep' three buffers with gaps 8 / 16 / 24,
    'kv' a packed k|v buffer (gap 8) and q alone, 'qkv' one packed q|k|v buffer (nq == nk, gap 16)."""
    C = c.H * c.d
    q2, k2, v2 = c.q.reshape(c.B * c.nq, C), c.k.reshape(c.B * c.nk, C), c.v.reshape(c.B * c.nk, C)
    if layout == "sep":
        return guarded(q2, 8, dev), guarded(k2, 16, dev), guarded(v2, 24, dev)
    if layout == "kv":
        kv = guarded(torch.cat([k2, v2], 1), 8, dev)
        return guarded(q2, 24, dev), kv[:, :C], kv[:, C:]
    assert layout == "qkv" and c.nq == c.nk
    qkv = guarded(torch.cat([q2, k2, v2], 1), 16, dev)
    return qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]


def out_buffer(rows, cols, dev, pad=4, pre=1, post=2):
    """(buffer, view): the view [rows, cols] has row stride cols + pad inside a sentinel-filled buffer."""
    buf = torch.full((pre + rows + post, cols + pad), SENTINEL, dtype=torch.float16, device=dev)
    return buf, buf[pre:pre + rows, :cols]


def split_out(buf, rows, cols, pre=1):
    """(logical output on the CPU, True when everything outside it still holds the sentinel's bits)."""
    b = buf.cpu()
    got = b[pre:pre + rows, :cols].clone()
    b[pre:pre + rows, :cols] = SENTINEL
    clean = torch.equal(b.view(torch.int16), torch.full_like(b, SENTINEL).view(torch.int16))
    return got, clean


def ulp_index(t):
    """fp16 -> an integer that is monotone in the value with step 1 per ulp."""
    bits = t.contiguous().view(torch.int16).int()
    return torch.where(bits < 0, -(bits & 0x7fff), bits)


def ulp_diff(got, ref):
    if got.isnan().any():
        return math.inf
    return (ulp_index(got) - ulp_index(ref)).abs().max().item()


# ----------------------------------------------------------------------------- fused cross-attention block
XATTN_SHAPES = ((320, 40), (320, 64), (640, 64), (640, 80))      # (channels, head_dim) of xattn.hip
XATTN_N = (64, 192)
XATTN_NK = (13, 77, 80)


def signed_permutation(C, mul, add, run):
    """[C, C] weight with W[n, (mul n + add) % C] = +-1 (the sign flips every ``run`` rows): a permutation that
    is not its own inverse, so W and W^T give different answers."""
    n = torch.arange(C)
    perm = (mul * n + add) % C
    sign = 1.0 - 2.0 * ((n // run) % 2).double()
    w = torch.zeros(C, C, dtype=torch.float64)
    w[n, perm] = sign
    if torch.equal(perm[perm], n) or torch.equal(w, w.T) or len(set(perm.tolist())) != C:
        raise InexactCase("the permutation must be a non-involutive bijection")
    return w, perm, sign


_XW = {}


def xattn_weights(C):
    """(Wq, Wo, bias) of a channel count: signed permutations and an integer bias in [-8, 8]."""
    if C not in _XW:
        wq = signed_permutation(C, 7, 3, 3)[0]
        wo = signed_permutation(C, 13, 5, 5)[0]
        bias = ((torch.arange(C) * 5) % 17 - 8).double()
        _XW[C] = (wq, wo, bias)
    return _XW[C]


class XCase:
    """The one-hot family through to_q -> attention -> to_out + bias + residual: t is the family's Q pushed
    back through Wq (so t Wq^T IS that Q, exactly), V a code < 1009, bias and residual small integers.  Every
    step is an integer below 2048: q and o round to fp16 exactly, the winner's P is exp2(0) = 1 against a
    row sum of 1 (the losers' P <= 2^-64 vanish in fp32 next to it), and o Wo^T + bias and the residual add
    are exact.  ``ref`` [B*n_img, C] fp16 = res + bias + (+-V[f(i)])[perm]."""

    def __init__(self, B, n_img, C, D, nk, negative=False):
        H = C // D
        base = Case("onehot", B, H, n_img, nk, D, False, negative)
        self.name = f"xattn-{base.name}-c{C}"
        self.B, self.n_img, self.C, self.D, self.nk, self.H = B, n_img, C, D, nk, H
        wq, wo, bias = xattn_weights(C)
        M = B * n_img
        q2 = base.q.double().reshape(M, C)
        self.t = q2 @ wq                                    # t Wq^T = q2 Wq Wq^T = q2
        v = v_codes(B, nk, H, D) % 1009
        self.kv = torch.cat([base.k.double().reshape(B * nk, C), v.reshape(B * nk, C)], 1)
        m = torch.arange(M).view(M, 1)
        n = torch.arange(C).view(1, C)
        self.res = ((3 * m + 7 * n) % 33 - 16).double()
        self.win = base.win
        o = torch.gather(v, 1, base.win.permute(0, 2, 1).unsqueeze(-1).expand(B, n_img, H, D)).reshape(M, C)
        pre = o @ wo.T + bias
        ref = pre + self.res
        if not torch.equal(self.t @ wq.T, q2):
            raise InexactCase(f"{self.name}: t Wq^T is not the family's Q")
        for nme, x in (("t", self.t), ("kv", self.kv), ("res", self.res), ("o Wo^T + bias", pre), ("out", ref)):
            if not torch.equal(x, x.round()) or x.abs().max().item() > 2048:
                raise InexactCase(f"{self.name}: {nme} is not an integer within 2048")
        self.ref = ref.half()
