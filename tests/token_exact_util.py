"""Exact-arithmetic cases for the persistent 320-channel token linear (csrc/token.hip):
out = [res +] x W^T + b with fp16 roundings at acc + b and at + res.  tests/test_gpu_token_exact.py runs them
on the GPU, tests/test_token_exact_inputs.py checks them on the CPU; nothing of the product package is
imported here.

x, W, b and res are integers picked by a hash of (case, row, column) (tests/ff_exact_util.py), every partial
sum (bounded by the sum of |terms|) is below 2^24 and every value that is rounded below 65504, so fp32
accumulation is exact in any order, each fp16 rounding is one correct rounding of a known integer (|b| and
|res| reach 2000, so both roundings are real), and the kernel must EQUAL the float64 reference.

The row counts follow from the persistent grid (one workgroup per CU, 32-token blocks dealt grid-stride,
3-stage ring, a counted vmcnt wait with the branches it == 0, it == 1, it >= 2), for G CUs:
  7, 32, 33, 1000      fewer rows than a block, one block, a 1-row second block, a ragged 8-row block 31
  32 G + 40            workgroups 0 / 1 take a second block (it == 1), the last one of 8 rows
  96 G + 169           workgroups 0 .. 5 reach it == 3 (the it >= 2 branch, the ring back in stage 0); the
                       last block has 9 rows and belongs to workgroup 5 on its fourth block"""
import torch

from conv_exact_util import InexactCase  # noqa: F401  (re-exported for the tests)
from ff_exact_util import C, F16_MAX, _need, hashed_ints, seed_of

BLOCK, STAGES = 32, 3
ROW_KINDS = ("7", "32", "33", "1000", "it1", "it3")
TOKEN_RES = ("none", "res", "alias")
TOKEN_LDS = {"dense": (320, 320, 320), "strided-a": (328, 344, 344), "strided-b": (344, 320, 328)}   # (x, res, out)


def rows_of(kind, G):
    if kind == "it1":
        return BLOCK * G + 40
    if kind == "it3":
        return BLOCK * STAGES * G + BLOCK * 5 + 9
    return int(kind)


def walk(rows, G):
    """(grid, blocks, [it of each block], rows of the last block) of the persistent kernel."""
    nblk = -(-rows // BLOCK)
    grid = min(nblk, G)
    return grid, nblk, [b // grid for b in range(nblk)], rows - (nblk - 1) * BLOCK


class TokenInputs:
    """x [M, 320], w [320, 320] fp16, b [320] fp32, res [M, 320] fp16 (hashed by the global row index, so a
    case of fewer rows is a prefix of a longer one)."""

    def __init__(self, M):
        s = seed_of("token-linear")
        self.name, self.M = f"token-M{M}", M
        self.x = hashed_ints(s + 1, M, C, -8, 8).half()
        self.w = hashed_ints(s + 2, C, C, -8, 8).half()
        self.b = hashed_ints(s + 3, 1, C, -2000, 2000)[0].float()
        self.res = hashed_ints(s + 4, M, C, -2000, 2000).half()
        self.ref = {}


def token_reference(c, with_bias, with_res):
    """fp16 reference [M, 320] from float64; raises InexactCase unless the conditions hold."""
    x, w, b, res = c.x.double(), c.w.double(), c.b.double(), c.res.double()
    for what, v in (("x", x), ("w", w), ("b", b), ("res", res)):
        _need(torch.equal(v, v.round()), f"{c.name}: {what} is not integral")
    bb = b.abs() if with_bias else 0.0
    _need((x.abs() @ w.abs().T + bb).max().item() < 2 ** 24, f"{c.name}: a partial sum can reach 2^24")
    acc = x @ w.T + (b if with_bias else 0.0)
    _need(acc.abs().max().item() < F16_MAX, f"{c.name}: |acc + b| reaches 65504")
    out = acc.float().half()
    if with_res:
        s = out.double() + res
        _need(s.abs().max().item() < F16_MAX, f"{c.name}: |acc + b + res| reaches 65504")
        out = s.float().half()
    return out


def token_reference_f32(c, with_bias, with_res, perm_seed):
    """The same in float32 with the summation in a permuted order and explicit partial sums."""
    p = torch.randperm(C, generator=torch.Generator().manual_seed(perm_seed))
    acc = torch.zeros(c.M, C)
    for ks in torch.chunk(p, 5):
        acc = acc + c.x.float()[:, ks] @ c.w.float()[:, ks].T
    if with_bias:
        acc = acc + c.b
    out = acc.half()
    if with_res:
        out = (out.float() + c.res.float()).half()
    return out


_TOK = {}


def token_case(M):
    if M not in _TOK:
        _TOK[M] = TokenInputs(M)
    return _TOK[M]


def token_ref(c, with_bias, with_res):
    """Computed once per (case, options) and shared: do not modify."""
    k = (with_bias, with_res)
    if k not in c.ref:
        c.ref[k] = token_reference(c, with_bias, with_res)
    return c.ref[k]


def layer_norm_ref(out, gamma, beta, eps):
    """float64 LayerNorm of the fp16 ``out`` rows."""
    return torch.nn.functional.layer_norm(out.double(), (C,), gamma.double(), beta.double(), eps)


def token_where(rows, G):
    """A ``where(row, channel)`` for ff_exact_util.mismatch_report: who computes out[row, channel]."""
    grid, nblk, its, last = walk(rows, G)

    def where(m, ch):
        b = m // BLOCK
        return (f"block {b} of {nblk} ({'ragged, ' + str(last) + ' rows' if b == nblk - 1 and last < BLOCK else 'full'}): "
                f"workgroup {b % grid} of {grid}, it {its[b]} (ring stage {its[b] % STAGES}), tile row {m % BLOCK}; "
                f"wave {ch // 80}, channel block {ch % 80 // 16}, lane quarter {ch % 16 // 4}")
    return where
