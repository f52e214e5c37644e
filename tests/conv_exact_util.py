"""Exact-arithmetic cases for the implicit-GEMM conv / token GEMM (tests/test_gpu_conv_exact.py runs
them on the GPU, tests/test_conv_exact_inputs.py checks the inputs on the CPU).

Activations, weights, bias, embedding row and residual are small integers stored as fp16 / fp32, so
every product and partial sum is an integer below 2^24 and every output an integer below 2048: fp32
accumulation is exact in any order and fp16 rounding in the epilogue is the identity.  The kernel
output therefore has to EQUAL the reference element for element, whatever tile variant, split-K
scheme or tile order ran.  ``reference`` asserts those conditions itself (``InexactCase``), so an
accidentally inexact case is a test error, never a kernel failure.

The reference is torch on the CPU in float64 (F.conv2d / einsum, explicit F.pad, F.interpolate and
torch.cat); nothing of the product package is imported here."""
import zlib

import torch
import torch.nn.functional as F

OUT_NHWC_F16, OUT_NCHW_F32, OUT_GEGLU_F16, OUT_ROWS_F32 = 0, 1, 2, 3     # sdk_amd.h enum sdk_out_mode

# the ids of the `conv_variant` fixture (tests/test_gpu_kernels.py), re-declared
VARIANT_IDS = ["auto", "0", "2", "3", "4", "6", "7", "8", "9", "16", "17", "18", "19", "20", "21", "22", "23", "24",
               "25", "26", "31", "32", "33", "38", "40"]
# BM x BN of each tile variant, re-declared (csrc/conv.h's variant table takes them from the config types;
# tests/test_boundary.py checks this copy against the built library on the CPU)
TILE = {0: (128, 128), 2: (256, 256), 3: (256, 128), 4: (128, 128), 6: (256, 160), 7: (128, 320), 8: (256, 256),
        9: (256, 256), 16: (128, 128), 17: (256, 128), 18: (128, 128), 19: (128, 256), 20: (256, 256),
        21: (256, 256), 22: (256, 320), 23: (128, 320), 24: (256, 160), 25: (128, 256), 26: (128, 128),
        31: (128, 160), 32: (128, 128), 33: (128, 160), 38: (256, 320), 40: (256, 256)}
ALL_TILES = sorted(set(TILE.values()))
# variants whose epilogue can pair the (x, gate) halves of a GEGLU projection (the table's GEGLU column)
GEGLU_OK = {0, 2, 3, 4, 8, 9, 16, 17, 18, 19, 20, 21, 25, 26, 32, 40}
DIRECT, SKINNY = 34, 35

# silu(v) rounds to {0, 0, 12, ..., 16} in fp16 for any sigmoid accurate to 1e-4 (checked on the CPU)
SILU_SET = (-30.0, 0.0, 12.0, 13.0, 14.0, 15.0, 16.0)
SILU_OUT = (0.0, 0.0, 12.0, 13.0, 14.0, 15.0, 16.0)
# gelu(g) rounds to g in fp16 for these gate values
GELU_SET = tuple(float(g) for g in range(6, 14))

SENTINEL = -777.5        # prefill of output buffers: finite, not an integer, so never a valid output
LIMIT = 2048.0           # integers below 2^11 are exact in fp16


class InexactCase(RuntimeError):
    """The case's inputs do not satisfy the exactness conditions: a bug of the test, not of a kernel."""


class Case:
    """One conv / GEMM problem: CPU inputs, call geometry, what it claims to cover, and its reference."""

    def __init__(self, name, **kw):
        self.name = name
        self.srcs = None            # list of 1 or 2 fp16 [B, H, W, C] (the channel concat)
        self.w = None               # fp32 [Cout, Cin, k, k]; per-image weights: [B, Cout, K]
        self.ksize, self.stride, self.pad, self.pad_end, self.upsample = 1, 1, 0, 0, False
        self.gn = None              # (scale, shift) fp32 [B, Cin]
        self.silu = False
        self.srcs2, self.w2 = None, None     # fused 1x1 shortcut segment
        self.bias = None            # fp32 [Cout]
        self.row_bias = None        # (fp32 [B, ld], column offset)
        self.residual = None        # fp16 [B, Ho, Wo, Nout]
        self.out_mode = OUT_NHWC_F16
        self.per_image = False
        self.transform = False      # a prologue / split the LDS-DMA kernels cannot do: the plan must be variant 0
        self.variants = VARIANT_IDS
        self.tiles = ALL_TILES      # BM x BN this case claims >= 2 tiles with ragged last tiles for
        self.ragged_m, self.ragged_n = True, True
        self.api = "conv2d"         # or "linear"
        self.__dict__.update(kw)
        self.ref = reference(self)

    @property
    def geglu(self):
        return self.out_mode == OUT_GEGLU_F16

    @property
    def cout(self):
        return self.w.shape[1] if self.per_image else self.w.shape[0]

    @property
    def nout(self):
        return self.cout // 2 if self.geglu else self.cout

    @property
    def out_shape(self):            # logical [B, Ho, Wo, Nout]
        return tuple(self.ref.shape)

    @property
    def M(self):
        b, ho, wo, _ = self.out_shape
        return b * ho * wo


def _reference(c, dt):
    """(value before the residual add, final value) in dtype ``dt``, logical [B, Ho, Wo, Nout]."""
    x = torch.cat(c.srcs, -1).to(dt).permute(0, 3, 1, 2)
    if c.gn is not None:
        sc, sh = c.gn
        x = x * sc.to(dt)[:, :, None, None] + sh.to(dt)[:, :, None, None]
        if not torch.equal(x.half().to(dt), x):
            raise InexactCase(f"{c.name}: the GroupNorm affine does not round-trip through fp16")
    if c.silu:
        x = F.silu(x).half().to(dt)             # the A operand is an fp16 tensor
    if c.per_image:
        B, H, W, K = c.srcs[0].shape
        y = torch.einsum("bmk,bnk->bmn", x.permute(0, 2, 3, 1).reshape(B, H * W, K), c.w.to(dt))
        y = y.reshape(B, H, W, -1)
    else:
        if c.upsample:
            x = F.interpolate(x, scale_factor=2, mode="nearest")
        x = F.pad(x, (c.pad, c.pad + c.pad_end, c.pad, c.pad + c.pad_end))     # zeros AFTER the transform
        y = F.conv2d(x, c.w.to(dt), stride=c.stride)
        if c.srcs2 is not None:
            y = y + F.conv2d(torch.cat(c.srcs2, -1).to(dt).permute(0, 3, 1, 2), c.w2.to(dt))
        y = y.permute(0, 2, 3, 1)
    if c.bias is not None:
        y = y + c.bias.to(dt)
    if c.row_bias is not None:
        rb, off = c.row_bias
        y = y + rb.to(dt)[:, None, None, off:off + y.shape[-1]]
    if c.geglu:
        inner = y.shape[-1] // 2
        a, g = y[..., :inner], y[..., inner:]
        y = (a * F.gelu(g)).half().to(dt)        # one fp16 rounding of x * gelu(gate)
        if not torch.equal(y, a * g):
            raise InexactCase(f"{c.name}: x * gelu(gate) does not round to x * gate")
    pre = y
    if c.residual is not None:
        y = y + c.residual.to(dt)
    return pre.contiguous(), y.contiguous()


def _abs_bound(c):
    """max over outputs of sum_k |a_k| |w_k| (every partial sum, in any order, stays below it)."""
    x = torch.cat(c.srcs, -1).double().permute(0, 3, 1, 2)
    if c.gn is not None:
        x = x * c.gn[0].double()[:, :, None, None] + c.gn[1].double()[:, :, None, None]
    if c.silu:
        x = F.silu(x)
    x = x.abs()
    if c.per_image:
        B, H, W, K = c.srcs[0].shape
        return torch.einsum("bmk,bnk->bmn", x.permute(0, 2, 3, 1).reshape(B, H * W, K), c.w.double().abs()).max().item()
    if c.upsample:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    x = F.pad(x, (c.pad, c.pad + c.pad_end, c.pad, c.pad + c.pad_end))
    y = F.conv2d(x, c.w.double().abs(), stride=c.stride)
    if c.srcs2 is not None:
        y = y + F.conv2d(torch.cat(c.srcs2, -1).double().abs().permute(0, 3, 1, 2), c.w2.double().abs())
    return y.max().item()


def reference(c):
    """float32 reference [B, Ho, Wo, Nout]; raises InexactCase unless the exactness conditions hold."""
    pre64, y64 = _reference(c, torch.float64)
    pre32, y32 = _reference(c, torch.float32)
    for what, v in (("before the residual", pre64), ("final", y64)):
        if not (v.abs().max().item() < LIMIT):
            raise InexactCase(f"{c.name}: |reference| {what} reaches {v.abs().max().item()} (limit {LIMIT})")
        if not torch.equal(v, v.round()):
            raise InexactCase(f"{c.name}: the reference {what} is not integral")
        if not torch.equal(v.half().double(), v):
            raise InexactCase(f"{c.name}: the reference {what} does not round-trip through fp16")
    if not (torch.equal(pre32.double(), pre64) and torch.equal(y32.double(), y64)):
        raise InexactCase(f"{c.name}: the float32 reference differs from the float64 one")
    if not (_abs_bound(c) < 2 ** 24):
        raise InexactCase(f"{c.name}: a partial sum can reach 2^24")
    return y32


# --------------------------------------------------------------------------- the case matrix

def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _ints(g, shape, lo, hi, dtype=torch.float16):
    return torch.randint(lo, hi + 1, shape, generator=g).to(dtype)


def _pick(g, shape, values):
    v = torch.tensor(values, dtype=torch.float32)
    return v[torch.randint(0, len(values), shape, generator=g)]


def _weight(g, cout, cin, k, density=1.0):
    w = _ints(g, (cout, cin, k, k), -1, 1, torch.float32)
    if density < 1.0:
        w = w * (torch.rand(w.shape, generator=g) < density)
    return w


B0, HO, WO, COUT = 2, 13, 11, 328        # M = 286: every BM has a ragged 30-row last tile, a 256-row tile
                                         # straddles the two images; 328 = 2*128+72 = 256+72 = 2*160+8 = 320+8


def _epilogue(g, B, Ho, Wo, cout, bias=True, row_bias=False, residual=False):
    kw = {}
    if bias:
        kw["bias"] = _ints(g, (cout,), -8, 8, torch.float32)
    if row_bias:
        kw["row_bias"] = (_ints(g, (B, cout + 24), -8, 8, torch.float32), 17)
    if residual:
        kw["residual"] = _ints(g, (B, Ho, Wo, cout), -50, 50)
    return kw


def _conv_case(name, srcs_hw, cins, cout=COUT, k=3, xr=3, density=1.0, epi=(True, False, False), B=B0, **kw):
    g = _gen(name)
    H, W = srcs_hw
    srcs = [_ints(g, (B, H, W, ci), -xr, xr) for ci in cins]
    w = _weight(g, cout, sum(cins), k, density)
    c = dict(srcs=srcs, w=w, ksize=k, **kw)
    up = 2 if kw.get("upsample") else 1
    pad, pe, st = kw.get("pad", 0), kw.get("pad_end", 0), kw.get("stride", 1)
    Ho, Wo = (up * H + 2 * pad + pe - k) // st + 1, (up * W + 2 * pad + pe - k) // st + 1
    c.update(_epilogue(g, B, Ho, Wo, cout, *epi))
    return g, c


def _build(name):
    """Construct the named case (inputs seeded by the name)."""
    kind = name.split("-")[0]
    if kind == "A":        # ragged 64-channel K block (the masked LDS-DMA path), the whole epilogue
        g, c = _conv_case(name, (HO, WO), [72], pad=1, epi=(True, True, True))
    elif kind == "B":      # pad 0, Cin % 64 == 0: the `simple` K loop
        g, c = _conv_case(name, (15, 13), [128], pad=0)
    elif kind == "C":      # stride 2 over more than one M-tile
        g, c = _conv_case(name, (25, 21), [64], pad=1, stride=2)
    elif kind == "D":      # the asymmetric Downsample, odd and even source extents
        hw, cin = {"odd": ((27, 23), 64), "even": ((26, 22), 72)}[name.split("-")[1]]
        g, c = _conv_case(name, hw, [cin], pad=0, pad_end=1, stride=2)
    elif kind == "E":      # folded nearest-x2 upsample, N = 328
        g, c = _conv_case(name, (7, 6), [128], pad=1, upsample=True)
    elif kind == "F":      # 2-source concat, ld0 != ld1
        _, split, k = name.split("-")
        cins = {"64_72": [64, 72], "40_32": [40, 32]}[split]
        k = int(k[1])
        g, c = _conv_case(name, (HO, WO), cins, k=k, pad=k // 2, transform=split == "40_32")
    elif kind == "G":      # 3x3 plus the fused 1x1 shortcut
        if name == "G-simple2":        # pad 0 + a 64 | 64 shortcut: build_params' simple == 2
            g, c = _conv_case(name, (15, 13), [64], pad=0)
            s2 = [64, 64]
        else:                          # pad 1 + a ragged single-source shortcut: not simple
            g, c = _conv_case(name, (HO, WO), [64], pad=1)
            s2 = [72]
        c["srcs2"] = [_ints(g, (B0, HO, WO, ci), -3, 3) for ci in s2]
        c["w2"] = _weight(g, COUT, sum(s2), 1)
    elif kind == "H":      # token GEMM under every split-K scheme
        mode = {"f16": OUT_NHWC_F16, "rows32": OUT_ROWS_F32}[name.split("-")[1]]
        g, c = _conv_case("H", (300, 1), [1280], cout=648, k=1, epi=(True, False, True), B=1, out_mode=mode)
    elif kind == "I":      # NCHW fp32 with Cout % 8 != 0: no split-K
        g, c = _conv_case(name, (HO, WO), [72], cout=12, pad=1, epi=(True, True, True), out_mode=OUT_NCHW_F32,
                          ragged_n=False)
    elif kind == "J":      # GEGLU: zero gate weights, gate bias from GELU_SET -> out[:, j] = a[:, j] * g_j
        g = _gen(name)
        inner, K = 192, 128
        w = _weight(g, 2 * inner, K, 1)
        w[inner:] = 0
        bias = torch.cat([_ints(g, (inner,), -4, 4, torch.float32), _pick(g, (inner,), GELU_SET)])
        c = dict(srcs=[_ints(g, (B0, HO, WO, K), -1, 1)], w=w, bias=bias, out_mode=OUT_GEGLU_F16,
                 tiles=[(128, 256), (256, 256)])
    elif kind == "K":      # per-image weights
        g = _gen(name)
        nb, n_img, K, N = 3, 256, 192, COUT
        c = dict(srcs=[_ints(g, (nb, n_img, 1, K), -3, 3)], w=_ints(g, (nb, N, K), -1, 1, torch.float32),
                 per_image=True, api="linear", ragged_m=False, **_epilogue(g, nb, n_img, 1, N, True, False, True))
    elif kind == "L":      # variant-0 prologues
        sub = name.split("-")[1]
        if sub == "gn":        # power-of-two scales, non-zero integer shifts: padding before the affine fails
            g, c = _conv_case(name, (HO, WO), [72], pad=1, transform=True)
            c["gn"] = (_pick(g, (B0, 72), (1.0, 2.0, 4.0)), _pick(g, (B0, 72), (-3.0, -2.0, -1.0, 1.0, 2.0, 3.0)))
        elif sub == "silu":
            g, c = _conv_case(name, (HO, WO), [72], pad=1, density=0.25, silu=True, transform=True)
            c["srcs"] = [_pick(g, (B0, HO, WO, 72), SILU_SET).half()]
        else:                  # affine lands on SILU_SET, over a 64 | 72 concat
            g, c = _conv_case(name, (HO, WO), [64, 72], pad=1, density=0.15, silu=True, transform=True)
            sc, sh = _pick(g, (B0, 136), (1.0, 2.0, 4.0)), _pick(g, (B0, 136), (-3.0, -2.0, -1.0, 1.0, 2.0, 3.0))
            x = (_pick(g, (B0, HO, WO, 136), SILU_SET) - sh[:, None, None, :]) / sc[:, None, None, :]
            c["srcs"] = [x[..., :64].half(), x[..., 64:].half()]
            c["gn"] = (sc, sh)
    elif kind == "M":      # the direct plan (Cout <= 8)
        g, c = _conv_case(name, (9, 40), [72], cout=5, pad=1, B=3, out_mode=OUT_NCHW_F32,
                          variants=variants_of(name), tiles=[])
    elif kind == "N":      # the skinny plan (M <= 64)
        if name == "N-res":
            g, c = _conv_case(name, (7, 1), [200], cout=72, k=1, B=1, epi=(True, False, True))
        else:
            g, c = _conv_case(name, (64, 1), [96], cout=40, k=1, B=1, silu=True, out_mode=OUT_ROWS_F32)
            c["srcs"] = [_pick(g, (1, 64, 1, 96), SILU_SET).half()]
        c.update(variants=variants_of(name), tiles=[], api="linear")
    else:
        raise KeyError(name)
    return Case(name, **c)


CONV_CASES = ["A", "B", "C", "D-odd", "D-even", "E", "F-64_72-k1", "F-64_72-k3", "F-40_32-k1", "F-40_32-k3",
              "G-simple2", "G-ragged", "I", "J", "K", "L-gn", "L-silu", "L-gn_silu", "M", "N-res", "N-silu32"]
SPLIT_CASES = ["H-f16", "H-rows32"]          # run under split_k in SPLITS (-2: in-launch, tile variants only)
SPLITS = (1, 2, 4, -2)
ALL_CASES = CONV_CASES + SPLIT_CASES

# the direct and skinny plans pre-empt every tile variant: those cases run under "auto" and their own id
_OWN_VARIANTS = {"M": ["auto", str(DIRECT)], "N-res": ["auto", str(SKINNY)], "N-silu32": ["auto", str(SKINNY)]}


def variants_of(name):
    """The ``forced`` ids a case runs under (known without building the case)."""
    return _OWN_VARIANTS.get(name, VARIANT_IDS)


_CACHE = {}


def get_case(name):
    """The case, built once per process (the reference is shared and must not be modified)."""
    if name not in _CACHE:
        _CACHE[name] = _build(name)
    return _CACHE[name]


# --------------------------------------------------------------------------- the honoured-variant rule

def expected_variant(case, forced):
    """What the plan must report: an id, ``"geglu"`` (any GEGLU-capable id), or None (nothing asserted).
    Only build_params' honoured / not-honoured rule, never its scoring."""
    if case.transform:
        return 0
    if forced == "auto":
        return int(case.variants[1]) if len(case.variants) == 2 else None      # direct / skinny
    v = int(forced)
    if case.geglu and v not in GEGLU_OK:
        return "geglu"
    if case.per_image and v == 0:
        return "tile"          # variant 0 has no per-image weights: the planner's LDS-DMA pick
    return v


def check_plan(case, forced, plan, split_k=None):
    want = expected_variant(case, forced)
    got = plan["variant"]
    ctx = f"{case.name} forced {forced}: plan {plan}"
    if want == "geglu":
        assert got in GEGLU_OK and got != int(forced), ctx
    elif want == "tile":
        assert got in TILE and got != 0 and case.M // case.out_shape[0] % TILE[got][0] == 0, ctx
    elif want is not None:
        assert got == want, ctx
    if split_k is not None:
        assert plan["split_k"] == abs(split_k), ctx
    if got in TILE:
        bm, bn = TILE[got]
        assert plan["grid_tiles"] == -(-case.M // bm) * -(-case.cout // bn), ctx


# --------------------------------------------------------------------------- canary buffers

def guarded_nhwc(t, ld, device):
    """``t`` [B, H, W, C] as a view into a NaN-filled [B + 2, H, W, ld] buffer: one image of NaN rows
    before and after, NaN in the channel gap [C, ld)."""
    B, H, W, C = t.shape
    assert ld > C
    buf = torch.full((B + 2, H, W, ld), float("nan"), dtype=t.dtype, device=device)
    buf[1:B + 1, :, :, :C] = t.to(device)
    return buf[1:B + 1, :, :, :C]


def guarded_residual(t, ld, device):
    """The residual at full width ``ld`` (ops.conv2d takes res_ld from the last dimension): NaN in
    columns [C, ld) and in one image before and after."""
    B, H, W, C = t.shape
    buf = torch.full((B + 2, H, W, ld), float("nan"), dtype=t.dtype, device=device)
    buf[1:B + 1, :, :, :C] = t.to(device)
    return buf[1:B + 1]


def out_buffer(case, device, extra=24):
    """(buffer, the ``out=`` view): sentinel-filled, one image more than the batch and, for the row
    layouts, ``extra`` columns more than the output is wide."""
    B, Ho, Wo, N = case.out_shape
    if case.out_mode == OUT_NCHW_F32:
        buf = torch.full((B + 1, N, Ho, Wo), SENTINEL, dtype=torch.float32, device=device)
    else:
        dt = torch.float32 if case.out_mode == OUT_ROWS_F32 else torch.float16
        buf = torch.full((B + 1, Ho, Wo, N + extra), SENTINEL, dtype=dt, device=device)
    return buf, buf[:B]


def split_out(case, buf):
    """(logical output [B, Ho, Wo, N] as float32 on the CPU, True when everything outside it still
    holds the sentinel bit for bit)."""
    B, Ho, Wo, N = case.out_shape
    buf = buf.cpu()
    sent = torch.full((), SENTINEL, dtype=buf.dtype)
    if case.out_mode == OUT_NCHW_F32:
        got = buf[:B].permute(0, 2, 3, 1)
        outside = [buf[B:]]
    else:
        got = buf[:B, :, :, :N]
        outside = [buf[B:], buf[:B, :, :, N:]]
    clean = all(torch.equal(o, sent.expand_as(o)) for o in outside)
    return got.float().contiguous(), clean


# --------------------------------------------------------------------------- comparison and report

def tile_of(case, variant, b, oy, ox, n):
    """(M-tile, N-tile) of an output element under ``variant``'s BM x BN (None for direct / skinny)."""
    if variant not in TILE:
        return None
    bm, bn = TILE[variant]
    _, Ho, Wo, _ = case.out_shape
    m = (b * Ho + oy) * Wo + ox
    if case.geglu:               # packed weight rows: 32 x columns, then their 32 gate columns
        n = 64 * (n // 32) + n % 32
    return m // bm, n // bn


def mismatch_report(case, got, ref, plan, first=5):
    """None when ``got`` equals ``ref`` element for element (-0 == 0; NaN never equals), else a report that
    names the tile of the first wrong element."""
    bad = ~(got == ref)
    nbad = int(bad.sum())
    if nbad == 0:
        return None
    idx = bad.nonzero()[:first].tolist()
    lines = [f"{case.name}: {nbad} of {ref.numel()} elements differ; plan variant {plan.get('variant')} "
             f"split_k {plan.get('split_k')}"]
    for b, oy, ox, n in idx:
        lines.append(f"  (b={b}, oy={oy}, ox={ox}, n={n}): got {got[b, oy, ox, n].item()} want {ref[b, oy, ox, n].item()}")
    v = plan.get("variant")
    t = tile_of(case, v, *idx[0])
    if t is not None:
        lines.append(f"  first in M-tile {t[0]}, N-tile {t[1]} of the {TILE[v][0]}x{TILE[v][1]} tiling")
    else:
        lines.append(f"  first at row {(idx[0][0] * ref.shape[1] + idx[0][1]) * ref.shape[2] + idx[0][2]}, "
                     f"column {idx[0][3]} (variant {v} has no BM x BN tiling)")
    return "\n".join(lines)


def assert_exact(case, got, plan, ref=None):
    rep = mismatch_report(case, got, case.ref if ref is None else ref, plan)
    assert rep is None, rep
