"""Cases of the exact tests of the wide attention form (csrc/attention_wide.hip) and of linear attention
(csrc/linattn.hip).  CPU only: nothing here imports the product package.

Wide attention reuses the two families of ``attn_exact_util`` unchanged (``Case``, scale ``SCALE``); both are
independent of the kernel's key-tile size, and the 1-ulp bound of the weighted family holds with or without the
deferred max because every rescale is a power of two.  ``KT`` / ``ROWS`` restate the kernel's constants
(SDK_ATTN_WIDE_KT / SDK_ATTN_WIDE_ROWS; the GPU test compares them with ``ops.ATTN_WIDE_KT`` / ``ATTN_WIDE_ROWS``).

Linear attention, the selector family (``LinCase``): k is 0 on the cnt(d) in {1, 2, 4, 8} member tokens of
channel d and -64 elsewhere, v an integer in [1, 15], q has three +-1 entries per row.  The softmax over the
tokens is then 1/cnt on the members and e^-64 / cnt < 2^-90 elsewhere: that rounds to fp16 zero as P, and stays
below half an fp32 ulp of any sum >= 1 in the column sums and in the combination of chunks (a chunk without a
member has maximum -64 and weight 2^-92 against the others).  ctx[d][e] = (sum of v over the members) / cnt is a
multiple of 1/8 that fp16 holds exactly, and out = q ctx a multiple of 1/8 below 64: every step is exact, in any
chunking and any order, so the kernel must reproduce the float64 result bit for bit."""
import torch

import attn_exact_util as U

KT = 32            # keys per tile of the wide kernel
ROWS = 64          # query rows per workgroup
DIMS = (168, 256, 264, 320, 512)
FORMS = ("wide", "auto")
# a ragged single tile, exactly one tile, two tiles plus one key, five tiles (every slot of the K / V ring is
# refilled twice and the t + 2 prefetch runs three times)
NKS = (KT - 12, KT, 2 * KT + 1, 4 * KT + 1)
NQ_SMALL, NQ_BIG = 5, ROWS + 69
BH = ((2, 1), (1, 3))


def padded(d):
    """The instantiation <DQK, DV> of a head dim."""
    assert 168 <= d <= 512 and d % 8 == 0, d
    return 256 if d <= 256 else 512


def expected_info(d, B, H, nq):
    D = padded(d)
    return dict(form="wide", dqk=D, dv=D, waves=8, qblocks=ROWS // 32, stagger=0, seed_col=0, causal=0,
                grid=-(-nq // ROWS) * H * B)


def wide_specs():
    """(family, B, H, nq, nk, negative, layout): both families at every nk with nq = ROWS + 69 (two full
    workgroups and a 5-row one), batch x heads alternating 2 x 1 / 1 x 3, the three layouts, the negative one-hot
    winner at the ragged nk, and nq = 5."""
    out = []
    for n, nk in enumerate(NKS):
        b0, h0 = BH[n % 2]
        b1, h1 = BH[(n + 1) % 2]
        out.append(("onehot", b0, h0, NQ_BIG, nk, False, ("sep", "kv")[n % 2]))
        out.append(("weighted", b1, h1, NQ_BIG, nk, False, ("kv", "sep")[n % 2]))
    out.append(("onehot", 2, 1, NQ_BIG, NKS[0], True, "sep"))
    out.append(("onehot", 1, 3, NQ_BIG, NKS[0], True, "kv"))
    out.append(("onehot", 1, 3, NQ_SMALL, NKS[2], False, "kv"))
    out.append(("weighted", 2, 1, NQ_SMALL, NKS[3], False, "sep"))
    out.append(("onehot", 1, 3, NKS[3], NKS[3], False, "qkv"))
    out.append(("weighted", 2, 1, NKS[2], NKS[2], False, "qkv"))
    return out


# ----------------------------------------------------------------------------- linear attention
LIN_SHAPES = ((67, 40), (200, 264), (129, 512), (64, 8))      # (tokens, dim_head)
LIN_HEADS = (1, 3)
LIN_BATCH = 2
KOFF = -64.0
CNTS = (1, 2, 4, 8)


class LinCase:
    """q / k / v [B, n, H, d] fp16; ``ref`` [B*n, H*d] fp16 (exact); ``ref64`` the float64 evaluation of the
    reference's expressions; ``exact`` the rational result in float64."""

    def __init__(self, B, H, n, d):
        self.B, self.H, self.n, self.d = B, H, n, d
        self.name = f"lin-b{B}h{H}n{n}d{d}"
        bb = torch.arange(B).view(B, 1, 1, 1)
        nn_ = torch.arange(n).view(1, n, 1, 1)
        hh = torch.arange(H).view(1, 1, H, 1)
        dd = torch.arange(d).view(1, 1, 1, d)
        cnt = torch.tensor(CNTS)[dd % 4]                                    # [1, 1, 1, d]
        assert n >= max(CNTS)
        member = torch.zeros(B, n, H, d, dtype=torch.bool)
        for i in range(max(CNTS)):
            tok = (5 * dd + 3 * hh + bb + i * (n // cnt)) % n               # [B, 1, H, d]
            member |= (nn_ == tok) & (i < cnt)
        self.cnt = cnt.expand(B, 1, H, d).double()
        self.member = member
        k = torch.where(member, torch.zeros(()), torch.full((), KOFF)).double()
        v = ((3 * nn_ + 7 * dd + 5 * hh + 11 * bb) % 15 + 1).double().expand(B, n, H, d).contiguous()
        q = torch.zeros(B, n, H, d, dtype=torch.float64)
        offs = (0, d // 3 + 1, 2 * (d // 3) + 1)
        for j, off in enumerate(offs):
            col = (nn_ + hh + off) % d                                      # [1, n, H, 1]
            sign = 1.0 - 2.0 * ((nn_ + j + bb) % 2).double()                # [B, n, 1, 1]
            q.scatter_add_(3, col.expand(B, n, H, 1), sign.expand(B, n, H, 1).contiguous())
        self.q, self.k, self.v = q.half(), k.half(), v.half()
        for t64, t16 in ((q, self.q), (k, self.k), (v, self.v)):
            if not torch.equal(t16.double(), t64):
                raise U.InexactCase(f"{self.name}: an input is not an fp16 value")
        # the reference's expressions in float64: softmax over the tokens, two einsums
        p = torch.softmax(k, dim=1)
        ctx = torch.einsum("bnhd,bnhe->bhde", p, v)
        self.ref64 = torch.einsum("bhde,bnhd->bnhe", ctx, q).reshape(B * n, H * d)
        # the exact rational
        if not torch.equal(member.sum(1, keepdim=True).double(), self.cnt):
            raise U.InexactCase(f"{self.name}: a channel has the wrong number of members")
        self.ctx_exact = torch.einsum("bnhd,bnhe->bhde", member.double(), v) / self.cnt.permute(0, 2, 3, 1)
        self.exact = torch.einsum("bhde,bnhd->bnhe", self.ctx_exact, q).reshape(B * n, H * d)
        self.ref = self.exact.half()

    def check_conditions(self):
        c8 = self.ctx_exact * 8
        if not torch.equal(c8, c8.round()) or not torch.equal(self.ctx_exact.half().double(), self.ctx_exact):
            raise U.InexactCase(f"{self.name}: ctx is not a multiple of 1/8 that fp16 holds")
        o8 = self.exact * 8
        if not torch.equal(o8, o8.round()) or self.exact.abs().max().item() >= 64:
            raise U.InexactCase(f"{self.name}: the output is not a multiple of 1/8 below 64")
        if not torch.equal(self.ref.double(), self.exact):
            raise U.InexactCase(f"{self.name}: the output is not an fp16 value")
        if not torch.equal(self.ref64, self.exact):
            raise U.InexactCase(f"{self.name}: the float64 softmax does not give the exact rational")
        if (self.q != 0).sum(-1).min().item() != 3 or self.q.abs().max().item() != 1:
            raise U.InexactCase(f"{self.name}: q must have three +-1 entries per row")


_LIN = {}


def get_lin_case(B, H, n, d):
    key = (B, H, n, d)
    if key not in _LIN:
        _LIN[key] = LinCase(*key)
    return _LIN[key]


def lin_guarded(c, dev):
    """Device views (q, k, v) of a LinCase as strided rows of NaN-filled buffers (gaps 8 / 16 / 24 columns)."""
    C = c.H * c.d
    rows = c.B * c.n
    return (U.guarded(c.q.reshape(rows, C), 8, dev), U.guarded(c.k.reshape(rows, C), 16, dev),
            U.guarded(c.v.reshape(rows, C), 24, dev))
