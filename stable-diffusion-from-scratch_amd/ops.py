"""Tensor-level wrappers over the C ABI (libsdk_amd.so).

Activations are NHWC fp16 CUDA tensors ``[B, H, W, C]`` (tokens ``[B, N, C]`` are
the ``W = 1`` case).  A conv source may be a 2-tuple ``(a, b)`` meaning the
channel concat ``cat([a, b], -1)``, read zero-copy by the kernels.

There is no CPU or eager-PyTorch fallback: a non-CUDA tensor raises TypeError,
a library failure raises RuntimeError.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import (ACT_NONE, ACT_QUICK_GELU, ACT_GELU, AttentionArgs, XAttnArgs, XAttnLnArgs, FfArgs, TokenLinearArgs, ProjNormQkvArgs, ConvArgs, ConvPlanInfo, GroupNormArgs,
                   OUT_GEGLU_F16, OUT_NCHW_F32, OUT_NHWC_F16, OUT_ROWS_F32, check, lib)

BK = 64          # K tile of the conv kernel (packed weight column padding)
BN = 128         # packed weight row padding (the kernels clamp reads beyond it)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _need_cuda(t: torch.Tensor, what: str, dtype=torch.float16):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError(f"sd_amd.{what}: expected a CUDA tensor (HIP path only, no CPU fallback)")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"sd_amd.{what}: expected {dtype}, got {t.dtype}")


def need_gpu_sampler(option: str, device):
    """The sampler options added after the plain loops (mask / x0 in DDIM, original steps, ``noise_dropout``,
    ``score_corrector``, ``progressive_denoising``, ``shorten_cond_schedule``) exist only as HIP kernels: on a
    model or tensor that is not on the GPU they stay NotImplementedError, raised before any model call."""
    if torch.device(device).type != "cuda":
        raise NotImplementedError(f"sd_amd: {option} is implemented on the GPU only (HIP kernels, no CPU "
                                  f"fallback); got device '{device}'")


# --------------------------------------------------------------------------- workspace

class _Workspace:
    """Growable scratch buffers (split-K slabs, GroupNorm partials), one per (device, lane).
    Calls of one lane are stream-ordered on one stream, so its buffer is safe to reuse;
    work issued concurrently on another stream must run under another lane
    (``with WORKSPACE.use_lane(i)``).

    A grown buffer is RETIRED, not freed: a HIP graph captured earlier holds the old
    pointer and writes through it on every replay, so its memory must stay owned by this
    workspace for the process lifetime (the superseded sizes sum to less than the final one
    when growth doubles; ``release_retired()`` is for callers that dropped every graph)."""

    def __init__(self):
        self.buf = {}
        self.retired = []
        self.lane = 0

    def release_retired(self):
        self.retired.clear()

    def use_lane(self, lane: int):
        import contextlib

        @contextlib.contextmanager
        def cm():
            prev, self.lane = self.lane, lane
            try:
                yield
            finally:
                self.lane = prev
        return cm()

    def counters(self, device) -> torch.Tensor:
        """The lane's per-tile arrival counters of in-launch split-K convs: zeroed once, and every launch
        leaves them zero (its last arrival resets each), so one fixed buffer serves every call of the lane."""
        key = (torch.device(device).index, self.lane, "cnt")
        c = self.buf.get(key)
        if c is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("sd_amd: tile counters must exist before graph capture (run one warm-up step)")
            c = torch.zeros(TILE_COUNTERS, dtype=torch.int32, device=device)
            self.buf[key] = c
        return c

    def get(self, nbytes: int, device) -> torch.Tensor:
        key = (torch.device(device).index, self.lane)
        b = self.buf.get(key)
        if b is None or b.numel() < nbytes:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("sd_amd: workspace must be sized before graph capture (run one warm-up step)")
            if b is not None:
                self.retired.append(b)
                nbytes = max(nbytes, 2 * b.numel())       # geometric growth bounds the retired total
            b = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
            self.buf[key] = b
        return b


WORKSPACE = _Workspace()
TILE_COUNTERS = 16384     # sdk_amd.h SDK_TILE_COUNTERS


# --------------------------------------------------------------------------- sources

def _as_pair(x):
    if isinstance(x, tuple):
        a, b = x
        return a, b
    return x, None


def src_shape(x):
    a, b = _as_pair(x)
    B, H, W, C0 = a.shape
    return B, H, W, C0 + (b.shape[-1] if b is not None else 0)


def _fill_src(s: "_lib.ConvSrc", x, ksize, stride, pad, upsample, gn, silu):
    a, b = _as_pair(x)
    _need_cuda(a, "conv2d")
    B, H, W, C0 = a.shape
    if a.stride(3) != 1 or (H > 1 and a.stride(1) != W * a.stride(2)) or (B > 1 and a.stride(0) != H * a.stride(1)):
        raise ValueError("sd_amd.conv2d: source must be NHWC with contiguous channels and a uniform pixel stride")
    s.src0 = a.data_ptr()
    s.ld0 = a.stride(2) if a.dim() == 4 else a.stride(1)
    if b is not None:
        _need_cuda(b, "conv2d")
        s.src1 = b.data_ptr()
        s.ld1 = b.stride(2)
        s.c_split = C0
        s.cin = C0 + b.shape[-1]
    else:
        s.src1 = None
        s.ld1 = 0
        s.c_split = C0
        s.cin = C0
    s.h, s.w = H, W
    s.ksize, s.stride, s.pad, s.upsample = ksize, stride, pad, 1 if upsample else 0
    if gn is not None:
        s.gn_scale, s.gn_shift = gn[0].data_ptr(), gn[1].data_ptr()
    else:
        s.gn_scale = s.gn_shift = None
    s.silu = 1 if silu else 0
    return B, H, W


# --------------------------------------------------------------------------- packed weights

class PackedConv:
    """A conv / linear weight packed for the implicit-GEMM kernel.

    ``segments``: list of (weight [N, Cin, k, k] or [N, Cin], cin_src) — cin_src is
    the channel count of the NHWC source feeding that segment (>= Cin; extra
    channels get zero weights).  Packed layout: fp16 [roundup(N,128)][sum_s k*k*roundup(cin_src,64)],
    per segment 64-channel block major, then tap, then channel.  ``geglu`` interleaves the (x, gate) halves of a
    GEGLU projection in 32-row groups so one wave holds both.
    """

    def __init__(self, segments, bias=None, geglu=False, device="cuda"):
        cols, self.seg_geom = [], []
        n_out = None
        for w, cin_src in segments:
            w = w.detach().float()
            if w.dim() == 2:
                w = w[:, :, None, None]
            if w.dim() == 3:                      # Conv1d [N, Cin, 1]
                w = w[:, :, :, None]
            N, Cin, kh, kw = w.shape
            assert kh == kw, "square kernels only"
            if n_out is None:
                n_out = N
            assert N == n_out
            cin_pad = (cin_src + BK - 1) // BK * BK
            wp = torch.zeros(N, kh, kw, cin_pad, dtype=torch.float32, device=w.device)
            wp[:, :, :, :Cin] = w.permute(0, 2, 3, 1)
            # K order: 64-channel block major, tap minor (the kernels' K-step order)
            wp = wp.reshape(N, kh * kw, cin_pad // BK, BK).permute(0, 2, 1, 3)
            cols.append(wp.reshape(N, -1))
            self.seg_geom.append((kh, cin_src))
        Wt = torch.cat(cols, dim=1)
        b = bias.detach().float().clone() if bias is not None else None
        if geglu:
            inner = n_out // 2
            assert inner % 32 == 0
            idx = []
            for q in range(inner // 32):
                idx += list(range(32 * q, 32 * q + 32)) + list(range(inner + 32 * q, inner + 32 * q + 32))
            idx = torch.tensor(idx, device=Wt.device)
            Wt = Wt[idx]
            if b is not None:
                b = b[idx.to(b.device)]
        self.N = n_out
        self.geglu = geglu
        npad = (n_out + BN - 1) // BN * BN
        Wfull = torch.zeros(npad, Wt.shape[1], dtype=torch.float32, device=Wt.device)
        Wfull[:n_out] = Wt
        self.weight = Wfull.to(device=device, dtype=torch.float16).contiguous()
        self.k_total = self.weight.shape[1]
        self.bias = b.to(device=device, dtype=torch.float32).contiguous() if b is not None else None


class PerImageWeights:
    """Per-image GEMM weights for ``linear(..., n_img=)``: ``weight`` fp16 [batch, n_pad, k] (row n of
    image b's matrix, K contiguous; n_pad = roundup(n, 128)), so output rows of image b use matrix b
    (``sdk_conv_args.weight_batch_stride``).  The reassociated cross-attention's per-prompt K_h Wq_h and
    Wo_h V_h^T (openai_model/attention.py)."""

    def __init__(self, weight, n, bias=None):
        assert weight.dim() == 3 and weight.dtype == torch.float16 and weight.is_contiguous()
        assert weight.shape[1] % BN == 0 and weight.shape[2] % BK == 0 and n <= weight.shape[1]
        self.weight = weight
        self.N = n
        self.k_total = weight.shape[2]
        self.bias = bias
        self.geglu = False
        self.seg_geom = [(1, weight.shape[2])]
        self.w_batch_stride = weight.shape[1] * weight.shape[2]


def fold_upsample_weight(w):
    """The four 2x2 phase kernels of ``F.interpolate(scale_factor=2, mode="nearest")`` + conv3x3 pad 1.

    Output pixel (2i+a, 2j+b) reads the low-res rows {i-1, i} (a = 0) or {i, i+1} (a = 1): of its three vertical
    taps two land on the same low-res row, so their weights add (columns alike).  ``w`` [N, Cin, 3, 3] ->
    [4, N, Cin, 2, 2] in w's dtype (phase = 2a + b; tap (dy, dx) multiplies low-res pixel (i-1+a+dy, j-1+b+dx),
    zero outside the image).  Exact: sums only, in the dtype given (float32 for the packed weights, which are then
    rounded to fp16 once)."""
    assert w.dim() == 4 and w.shape[2:] == (3, 3)
    rows = ((w[:, :, 0], w[:, :, 1] + w[:, :, 2]), (w[:, :, 0] + w[:, :, 1], w[:, :, 2]))     # [a][dy] -> [N, Cin, 3]
    out = w.new_empty(4, w.shape[0], w.shape[1], 2, 2)
    for a in range(2):
        for dy in range(2):
            r = rows[a][dy]
            cols = ((r[:, :, 0], r[:, :, 1] + r[:, :, 2]), (r[:, :, 0] + r[:, :, 1], r[:, :, 2]))   # [b][dx]
            for b in range(2):
                for dx in range(2):
                    out[2 * a + b, :, :, dy, dx] = cols[b][dx]
    return out


class PhaseConv:
    """The packed weights of an Upsample's conv in the phase form (``conv2d(..., phase=True)``): the four 2x2
    kernels of ``fold_upsample_weight`` (summed in fp32, rounded to fp16 once), each packed as a ``PackedConv``
    matrix [roundup(N, 128)][4 * roundup(cin_src, 64)], stacked [4, ...] (``sdk_conv_args.weight_batch_stride``
    apart).  Built once from the module's parameters."""

    def __init__(self, weight, cin_src, bias=None, device="cuda"):
        ph = fold_upsample_weight(weight.detach().float())
        packs = [PackedConv([(ph[q], cin_src)], bias if q == 0 else None, device=device) for q in range(4)]
        self.weight = torch.stack([pk.weight for pk in packs]).contiguous()
        self.N, self.k_total, self.bias = packs[0].N, packs[0].k_total, packs[0].bias
        self.geglu = False
        self.seg_geom = [(2, cin_src)]
        self.w_batch_stride = self.weight.shape[1] * self.weight.shape[2]


def _conv_source_files():
    """The conv sources and headers (csrc/conv*), sorted by name: what the tuning-cache key covers."""
    import os
    # SD_AMD_CONV_SOURCE: the csrc directory (or a file inside it) an A/B library (SD_AMD_LIB) was built from (tools only)
    src = os.environ.get("SD_AMD_CONV_SOURCE") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
    if not os.path.isdir(src):
        src = os.path.dirname(src)
    return [os.path.join(src, f) for f in sorted(os.listdir(src)) if f.startswith("conv")]


def _conv_source_hash():
    """sha1 over the name and bytes of every conv source file: any edit of one invalidates a tuning cache."""
    import hashlib
    import os
    h = hashlib.sha1()
    for path in _conv_source_files():
        h.update(os.path.basename(path).encode() + b"\0")
        with open(path, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


class _Autotune:
    """Per-shape choice of conv tile configuration and split-K, measured on the device.

    Enabled by ``enable()`` (UNetModel/AutoEncoderKL.prepare(autotune=True)); the
    first call of each distinct problem times every candidate (HIP events, 3 reps
    after a warm-up; SD_AMD_TUNE_REPS) and caches the fastest.  Never runs under graph capture."""
    VARIANTS = (2, 7, 6, 4, 3, 8, 9, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 31, 32, 33, 34, 35, 38, 40, 49)
    # split -2: two K halves combined inside the launch (sdk_conv_args.split_inlaunch; LDS-DMA tile kernels)
    # (3 and 6: 80 256x256 tiles of a 16x16-level conv x 3 = 240 workgroups, one wave of the 256 CUs)
    SPLITS = (0, 1, 2, 3, 4, 6, 8, 12, 16, -2)
    # unsplit plans: M-panels per tile group (sdk_conv_args.tile_group_m; 1 = M-panel major)
    GROUPS = (1, 8, 16)

    def __init__(self):
        import os
        self.enabled = False
        self.table = {}
        self.timed = 0
        ev = os.environ.get("SD_AMD_TUNE_VARIANTS")       # candidate subset (benchmarking the tuner itself)
        if ev:
            self.VARIANTS = tuple(int(v) for v in ev.split(","))
        self.reps = int(os.environ.get("SD_AMD_TUNE_REPS", "3"))   # timed launches per candidate

    def enable(self, on=True):
        self.enabled = on

    def save(self, path):
        """Write the table as JSON (key tuple -> [variant_hint, split_k, tile_group_m]); a tuning cache
        like MIOpen's find-db: later runs load it and time nothing."""
        import json
        with open(path, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else None,
                       "conv_source": _conv_source_hash(),
                       "entries": [[list(k), list(v)] for k, v in sorted(self.table.items(), key=str)]}, f, indent=0)

    def load(self, path):
        import json
        with open(path) as f:
            d = json.load(f)
        if d.get("conv_source") != _conv_source_hash():
            return 0                     # tuned against other kernel code: re-time everything
        n = 0
        for k, v in d["entries"]:
            self.table[tuple(k)] = tuple(v)
            n += 1
        return n

    def key(self, a, pc, gn=False):
        s0, s1 = a.seg[0], a.seg[1]
        return (a.batch, a.ho, a.wo, a.cout, a.nseg, pc.k_total, a.out_mode, s0.cin, s0.h, s0.w, s0.ksize,
                s0.stride, s0.upsample, s0.c_split, int(bool(s0.gn_scale) or bool(s0.silu)),
                s1.cin if a.nseg > 1 else 0, int(gn), int(bool(a.weight_batch_stride)))

    def choose(self, a, pc, dev, gn=False):
        """``gn``: the output feeds a GroupNorm — candidates are timed emitting the statistics, and
        plans that cannot emit them are dropped (their GroupNorm would pay a statistics pass)."""
        key = self.key(a, pc, gn)
        hit = self.table.get(key)
        if hit is not None or not self.enabled or torch.cuda.is_current_stream_capturing():
            return hit
        cands = self.VARIANTS
        if a.nseg > 1 and (a.seg[1].gn_scale or a.seg[1].silu):
            self.table[key] = (0, 0)
            return self.table[key]
        if a.seg[0].gn_scale or a.seg[0].silu:
            # a transform prologue: the register-staged kernel or the skinny M <= 64 GEMM (SiLU on its A
            # fragments)
            cands = (0, 35)
        best, best_t = (0, 0), float("inf")
        info = ConvPlanInfo()
        stream = _stream()
        emit_any = False
        if gn:                           # is there a candidate at all that emits the statistics?
            for v in cands:
                for sp in self.SPLITS:
                    a.variant_hint = v + 1
                    set_split(a, sp, dev)
                    if lib().sdk_conv2d_plan(C.byref(a), C.byref(info)) == 0 and info.gn_chunks > 0:
                        emit_any = True
        for v in cands:
            for sp in self.SPLITS:
                a.variant_hint = v + 1
                set_split(a, sp, dev)
                if lib().sdk_conv2d_plan(C.byref(a), C.byref(info)) != 0:
                    continue
                if info.variant != v:
                    continue             # the forced variant does not apply: the planner's pick is timed once, as its own id
                if sp == 0 and info.split_k in self.SPLITS[1:]:
                    continue             # the automatic split equals an explicit candidate
                part = None
                if emit_any:
                    if info.gn_chunks == 0:
                        continue
                    part = torch.empty(a.batch, info.gn_chunks, a.cout, 2, dtype=torch.float32, device=dev)
                    a.gn_partial = part.data_ptr()
                else:
                    a.gn_partial = None
                if info.workspace_bytes > 0:
                    ws = WORKSPACE.get(info.workspace_bytes, dev)
                    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
                for gm in (self.GROUPS if info.split_k == 1 else (0,)):
                    a.tile_group_m = gm
                    check(lib().sdk_conv2d(C.byref(a), stream), "conv2d(autotune)")
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(self.reps):
                        lib().sdk_conv2d(C.byref(a), stream)
                    e1.record()
                    e1.synchronize()
                    t = e0.elapsed_time(e1)
                    if t < best_t:
                        best_t, best = t, (v + 1, -2 if sp == -2 else info.split_k, gm)
        a.variant_hint, a.gn_partial, a.tile_group_m = 0, None, 0
        set_split(a, 0, dev)
        self.table[key] = best
        self.timed += 1
        if self.timed % 10 == 0:             # progress (a full re-tune takes minutes)
            import sys
            print(f"sd_amd autotune: {self.timed} conv problems timed", file=sys.stderr, flush=True)
        return best


AUTOTUNE = _Autotune()


def set_split(a, sp, dev):
    """split_k of a ConvArgs; ``sp == -2`` requests the in-launch combine of two K halves (its arrival
    counters: ``WORKSPACE.counters``)."""
    if sp == -2:
        a.split_k, a.split_inlaunch = 2, 1
        a.tile_counters = WORKSPACE.counters(dev).data_ptr()
    else:
        a.split_k, a.split_inlaunch, a.tile_counters = sp, 0, None


# tests / benchmarks: force one tile configuration on every conv call (None = planner / autotuner)
FORCE_VARIANT = None
# tests / benchmarks: M-panels per tile group of unsplit plans (sdk_conv_args.tile_group_m; None = library default)
TILE_GROUP_M = None


# GroupNorm statistics emitted by the producing conv (tensor attribute; see conv2d(gn_stats=True))
GN_ATTR = "_sd_gn_partial"
EMIT_GN_STATS = True      # tests / A/B: False = every GroupNorm runs its own statistics pass


def _claim(out):
    """A caller-supplied ``out`` is about to be overwritten through the C ABI, which does not move
    torch's version counter: drop any GroupNorm statistics a previous producer attached to it, so
    only the plan that writes it now can attach (fresh) ones."""
    if out is not None and hasattr(out, GN_ATTR):
        delattr(out, GN_ATTR)
    return out


# The LDS-DMA conv kernels address a source through a buffer resource (31-bit byte offsets); a source
# of >= 2 GiB (the VAE decoder's 256-channel 512x512 maps at B=16: 2.15 GB) would push the plan onto
# the register-staged kernel (~500 vs ~800 TFLOP/s).  Such convs run as batch chunks under the limit
# (SD_AMD_CONV_CHUNK_LIMIT overrides it: A/B only).
BUF_LIMIT = int(__import__("os").environ.get("SD_AMD_CONV_CHUNK_LIMIT", "2147483647"))


def _src_bytes(x):
    a, b = _as_pair(x)
    B, H, W, _ = a.shape
    ld = max(a.stride(2), b.stride(2) if b is not None else 0)
    return B * H * W * ld * 2


def _bslice(t, b0, b1):
    if t is None:
        return None
    if isinstance(t, tuple):
        return tuple(_bslice(u, b0, b1) for u in t)
    return t[b0:b1]


def _conv2d_batch_chunks(pc, x, seg2, gn, row_bias, residual, out, B, kw):
    big = max(_src_bytes(x), _src_bytes(seg2[0]) if seg2 is not None else 0)
    n = -(-big // BUF_LIMIT)
    while big * 1.0 / n >= BUF_LIMIT or B % n:
        n += 1
        if n >= B:
            n = B
            break
    cb = B // n
    outs = []
    for b0 in range(0, B, cb):
        b1 = min(B, b0 + cb)
        s2 = None if seg2 is None else (_bslice(seg2[0], b0, b1), _bslice(seg2[1], b0, b1), seg2[2])
        rb = None if row_bias is None else (row_bias[0][b0:b1], row_bias[1])
        outs.append(conv2d(pc, _bslice(x, b0, b1), seg2=s2, gn=_bslice(gn, b0, b1), row_bias=rb,
                           residual=_bslice(residual, b0, b1), out=None if out is None else out[b0:b1], **kw))
    full = out if out is not None else torch.cat(outs, 0)
    parts = [getattr(o, GN_ATTR, None) for o in outs]
    if all(pp is not None for pp in parts) and len({pp[1] for pp in parts}) == 1:
        setattr(full, GN_ATTR, (torch.cat([pp[0] for pp in parts], 0), parts[0][1], full._version))
    return full


def _conv_out(pc, x, ksize, stride, pad, pad_end, upsample, phase, out_mode):
    """(Ho, Wo, shape, dtype) of the output of a conv2d call."""
    B, H, W = _as_pair(x)[0].shape[:3]
    lh, lw = (2 * H, 2 * W) if upsample else (H, W)
    Ho = (lh + 2 * pad + pad_end - ksize) // stride + 1
    Wo = (lw + 2 * pad + pad_end - ksize) // stride + 1
    if phase:
        Ho, Wo = 2 * (H - 2), 2 * (W - 2)
    shape = {OUT_GEGLU_F16: (B, Ho, Wo, pc.N // 2), OUT_NCHW_F32: (B, pc.N, Ho, Wo)}.get(out_mode, (B, Ho, Wo, pc.N))
    dt = torch.float16 if out_mode in (OUT_NHWC_F16, OUT_GEGLU_F16) else torch.float32
    return Ho, Wo, shape, dt


def conv2d(pc: PackedConv, x, *, ksize=None, stride=1, pad=None, pad_end=0, upsample=False, gn=None, silu=False,
           seg2=None, bias=True, row_bias=None, residual=None, out_mode=OUT_NHWC_F16, out=None,
           variant=None, split_k=None, act=ACT_NONE, gn_stats=False, plan_out=None, phase=False):
    """Run the implicit-GEMM conv.  ``seg2`` = (x2, gn2, silu2) adds a fused 1x1 K segment.
    ``pad_end`` adds zero rows/cols after the source (asymmetric (0,1,0,1) padding).
    ``row_bias`` = (fp32 tensor [B, ld], column offset) — the per-(batch, channel) add.
    ``variant`` / ``split_k`` force a kernel configuration (benchmarks; default: planner
    or autotuner).  ``gn_stats``: the output feeds a GroupNorm — when the chosen plan can, the
    epilogue also emits its per-chunk channel statistics (attached to the returned tensor,
    consumed by ``group_norm``, which then skips its statistics pass).  ``plan_out``: a dict that
    receives the launched plan (``variant``, ``split_k``, ``grid_tiles``, ``gn_chunks`` of the
    ConvPlanInfo; host integers, so it is safe under graph capture; a conv that runs as batch
    chunks reports its last chunk).  ``phase``: ``pc`` is a ``PhaseConv`` and ``x`` the low-res image with its
    1-pixel zero border (``zero_border``): nearest-x2 + conv3x3 pad 1 as four 2x2 convs, the ordinary
    [B, 2H, 2W, N] output (``sdk_conv_args.upsample_phase``)."""
    _claim(out)
    if phase:
        assert isinstance(pc, PhaseConv) and not isinstance(x, tuple) and not upsample and stride == 1
        ksize, pad, pad_end = 2, 0, 0
    B0 = _as_pair(x)[0].shape[0]
    dev = _as_pair(x)[0].device
    k0 = pc.seg_geom[0][0] if ksize is None else ksize
    Ho, Wo, shape, dt = _conv_out(pc, x, k0, stride, k0 // 2 if pad is None else pad, pad_end, upsample, phase, out_mode)
    if B0 > 1 and (_src_bytes(x) >= BUF_LIMIT or (seg2 is not None and _src_bytes(seg2[0]) >= BUF_LIMIT)):
        if out is None:
            out = torch.empty(shape, dtype=dt, device=dev)
        kw = dict(ksize=ksize, stride=stride, pad=pad, pad_end=pad_end, upsample=upsample, silu=silu, bias=bias,
                  out_mode=out_mode, variant=variant, split_k=split_k, act=act, gn_stats=gn_stats,
                  plan_out=plan_out, phase=phase)
        return _conv2d_batch_chunks(pc, x, seg2, gn, row_bias, residual, out, B0, kw)
    a = ConvArgs()
    if pad is None:
        pad = k0 // 2
    B, H, W = _fill_src(a.seg[0], x, k0, stride, pad, upsample, gn, silu)
    a.seg[0].pad_end = pad_end
    a.upsample_phase = 1 if phase else 0
    a.nseg = 1
    if seg2 is not None:
        x2, gn2, silu2 = seg2
        _fill_src(a.seg[1], x2, 1, 1, 0, False, gn2, silu2)
        a.nseg = 2
    a.batch, a.ho, a.wo, a.cout = B, Ho, Wo, pc.N
    a.act = act
    a.weight = pc.weight.data_ptr()
    a.k_total = pc.k_total
    a.weight_batch_stride = getattr(pc, "w_batch_stride", 0)
    a.bias = pc.bias.data_ptr() if (bias and pc.bias is not None) else None
    if row_bias is not None:
        rb, off = row_bias
        a.row_bias = rb.data_ptr() + 4 * off
        a.row_bias_ld = rb.stride(0)
    if out is None:
        out = torch.empty(shape, dtype=dt, device=dev)
    a.out = out.data_ptr()
    a.out_ld = out.shape[-1] if out_mode != OUT_NCHW_F32 else 0
    a.out_mode = out_mode
    if residual is not None:
        _need_cuda(residual, "conv2d residual")
        a.residual = residual.data_ptr()
        a.res_ld = residual.shape[-1]
    want_gn = gn_stats and EMIT_GN_STATS and out_mode == OUT_NHWC_F16
    tuned = AUTOTUNE.choose(a, pc, dev, want_gn) if (AUTOTUNE.enabled or AUTOTUNE.table) else None
    if tuned is not None:
        a.variant_hint = tuned[0]
        set_split(a, tuned[1], dev)
        a.tile_group_m = tuned[2] if len(tuned) > 2 else 0
    if variant is None:
        variant = FORCE_VARIANT
    if variant is not None:
        if variant + 1 != a.variant_hint:
            # a forced configuration: the tuned split / tile order belong to the tuned variant (an in-launch
            # split may not even exist for this one) -> the planner's split for the forced variant
            set_split(a, 0, dev)
            a.tile_group_m = 0
        a.variant_hint = variant + 1
    if split_k is not None:
        set_split(a, split_k, dev)    # -2: the in-launch combine of two K halves
    if TILE_GROUP_M is not None:
        a.tile_group_m = TILE_GROUP_M
    info = ConvPlanInfo()
    check(lib().sdk_conv2d_plan(C.byref(a), C.byref(info)), "conv2d_plan")
    if plan_out is not None:
        plan_out.update(variant=info.variant, split_k=info.split_k, grid_tiles=info.grid_tiles,
                        gn_chunks=info.gn_chunks)
    if info.workspace_bytes > 0:
        ws = WORKSPACE.get(info.workspace_bytes, dev)
        a.workspace = ws.data_ptr()
        a.workspace_bytes = ws.numel()
    part = None
    if want_gn and info.gn_chunks > 0 and out.shape[-1] == pc.N:
        part = torch.empty(B, info.gn_chunks, pc.N, 2, dtype=torch.float32, device=dev)
        a.gn_partial = part.data_ptr()
    if PROFILER.active:
        # algorithmic HBM bytes: each source tensor, the weights and the output once (+ residual)
        nb = sum(t.numel() * 2 for t in _as_pair(x) if t is not None) + pc.N * pc.k_total * 2
        if seg2 is not None:
            nb += sum(t.numel() * 2 for t in _as_pair(seg2[0]) if t is not None)
        nb += out.numel() * out.element_size() + (residual.numel() * 2 if residual is not None else 0)
        PROFILER.begin("conv", info, shape=(B * Ho * Wo, pc.N, pc.k_total, info.variant, info.split_k), nbytes=nb)
    check(lib().sdk_conv2d(C.byref(a), _stream()), "conv2d")
    if PROFILER.active:
        PROFILER.end()
    if part is not None:
        # the statistics describe `out` as written now: group_norm ignores them once the tensor has
        # been modified in place (its version counter moved)
        setattr(out, GN_ATTR, (part, info.gn_chunks, out._version))
    return out


def linear(pc: PackedConv, x2d, *, silu=False, residual=None, out_mode=OUT_NHWC_F16, out=None, bias=True,
           act=ACT_NONE, n_img=None, plan_out=None, split_k=None):
    """Token GEMM: x2d [M, K] fp16 → [M, N]; a 1x1 conv over an M x 1 image.  ``silu`` applies to
    the input (prologue), ``act`` (``ACT_QUICK_GELU`` / ``ACT_GELU``) to the output (epilogue, before the
    residual).  ``n_img``: rows per image, for a ``PerImageWeights`` pc (the GEMM runs as M / n_img images of
    n_img x 1).  ``plan_out`` / ``split_k``: as for ``conv2d``."""
    _claim(out)
    M = x2d.shape[0]
    nb, rows = (1, M) if n_img is None else (M // n_img, n_img)
    assert nb * rows == M
    if isinstance(pc, PerImageWeights):
        assert n_img is not None and nb == pc.weight.shape[0], "per-image weights: n_img must split M by image"
    x4 = x2d.view(nb, rows, 1, x2d.shape[-1]) if x2d.stride(-1) == 1 and x2d.is_contiguous() else None
    if x4 is None:
        x4 = x2d.as_strided((nb, rows, 1, x2d.shape[1]), (rows * x2d.stride(0), x2d.stride(0), x2d.stride(0), 1))
    res4 = residual.view(nb, rows, 1, residual.shape[-1]) if residual is not None else None
    y = conv2d(pc, x4, ksize=1, pad=0, silu=silu, residual=res4, out_mode=out_mode, bias=bias,
               out=None if out is None else out.view(nb, rows, 1, out.shape[-1]), act=act, plan_out=plan_out,
               split_k=split_k)
    return y.view(M, y.shape[-1])


def segment_softmax(s, nseg, seglen, scale, ld_p=None, out=None):
    """p = softmax over each of the ``nseg`` ``seglen``-column segments of scale * s (fp32 [M, ld] →
    fp16 [M, ld_p], columns from nseg*seglen zero): the reassociated cross-attention's softmax."""
    _need_cuda(s, "segment_softmax", torch.float32)
    assert s.dtype == torch.float32 and s.stride(-1) == 1
    M = s.shape[0]
    ld_p = ld_p or (nseg * seglen + BK - 1) // BK * BK
    if out is None:
        out = torch.empty(M, ld_p, dtype=torch.float16, device=s.device)
    check(lib().sdk_segment_softmax(s.data_ptr(), s.stride(0), out.data_ptr(), out.stride(0), M, nseg, seglen,
                                    float(scale), _stream()), "segment_softmax")
    return out


# --------------------------------------------------------------------------- normalisation

def _gn_args(x, gamma=None, beta=None, eps=0.0, groups=32, gn=None):
    """``(GroupNormArgs, (B, H, W, C), device, gn)`` of x (a tensor or a 2-source concat pair).  With gamma / beta the
    statistics side is filled in too: groups, eps, a workspace and fresh fp32 ``[B, C]`` scale / shift buffers
    (returned as ``gn``); with ``gn`` = (scale, shift) those are the given affine."""
    a0, a1 = _as_pair(x)
    _need_cuda(a0, "group_norm")
    B, H, W, Ch = src_shape(x)
    args = GroupNormArgs()
    args.src0 = a0.data_ptr()
    args.ld0 = a0.stride(2)
    if a1 is not None:
        args.src1 = a1.data_ptr()
        args.ld1 = a1.stride(2)
    args.c_split = a0.shape[-1]
    args.batch, args.hw, args.channels = B, H * W, Ch
    if gamma is not None:
        args.groups, args.eps = groups, eps
        args.gamma, args.beta = gamma.data_ptr(), beta.data_ptr()
        gn = (torch.empty(B, Ch, dtype=torch.float32, device=a0.device),
              torch.empty(B, Ch, dtype=torch.float32, device=a0.device))
        ws = WORKSPACE.get(lib().sdk_group_norm_workspace(B, H * W, Ch), a0.device)
        args.workspace, args.workspace_bytes = ws.data_ptr(), ws.numel()
    if gn is not None:
        args.scale, args.shift = gn[0].data_ptr(), gn[1].data_ptr()
    return args, (B, H, W, Ch), a0.device, gn


def _producer_parts(x):
    """(part0, nch0, part1, nch1) of the statistics the producing convs attached to x's sources, or
    (None, 0, None, 0) unless every source carries current ones (a tensor modified in place since — its
    version counter moved — no longer does)."""
    srcs = [t for t in _as_pair(x) if t is not None]
    parts = [getattr(t, GN_ATTR, None) for t in srcs]
    parts = [pp if pp is not None and pp[2] == t._version else None for pp, t in zip(parts, srcs)]
    if not all(pp is not None for pp in parts):
        return None, 0, None, 0
    p1, n1 = (parts[1][0], parts[1][1]) if len(parts) > 1 else (None, 0)
    return parts[0][0], parts[0][1], p1, n1


def group_norm_plan(x, *, groups=32, pad=0, stats=True, apply=True, parts=None, single_launch=True):
    """The launches GroupNorm takes on x, decided on the host by the planner every GroupNorm entry point routes
    through (``sdk_group_norm_plan``): ``{"stats": "given" | "slice" | "chunked" | "parts", "apply": "none" |
    "in_stats" | "flat" | "row" | "stride", "launches": n, "workspace_bytes": n}``.  ``stats`` / ``apply``: what the
    call computes (``group_norm``: both; ``group_norm_affine`` / ``group_norm_scale_shift``: statistics only;
    ``group_norm_apply``: apply only).  ``parts``: (nch0, nch1) chunk counts of producer statistics, 0 / False for
    none, None = whatever x's sources carry, as ``group_norm`` uses them.  ``single_launch=False``:
    ``group_norm_film``."""
    args, (B, H, W, Ch), _, _ = _gn_args(x)
    args.groups = groups
    args.scale = args.shift = args.src0          # only their presence counts
    if parts is None:
        _, n0, _, n1 = _producer_parts(x)
    else:
        n0, n1 = (parts, parts) if isinstance(parts, int) else parts
    info = _lib.GroupNormPlanInfo()
    check(lib().sdk_group_norm_plan(C.byref(args), int(stats), int(apply), H, W, pad, int(n0), int(n1),
                                    int(single_launch), C.byref(info)), "group_norm_plan")
    return {"stats": _lib.GN_STATS[info.stats], "apply": _lib.GN_APPLY[info.apply], "launches": info.launches,
            "workspace_bytes": info.workspace_bytes}


# zero-bordered GN+SiLU outputs for pad-0 3x3 convs (mask-free gather); 0 = the masked pad-1 path
PREPAD = 1


def gn_conv_pad():
    """(pad written by group_norm_apply, pad of the 3x3 conv that consumes it)."""
    return (1, 0) if PREPAD else (0, 1)


def group_norm_apply(x, gn, silu=True, out=None, pad=0):
    """y = silu?(x*scale + shift) — the normalised (possibly concatenated) input, contiguous NHWC.
    ``pad`` > 0 writes it into a zero-bordered [B, H+2pad, W+2pad, C] image for a pad-0 3x3 conv."""
    args, (B, H, W, Ch), dev, _ = _gn_args(x, gn=gn)
    y = _claim(out) if out is not None else torch.empty(B, H + 2 * pad, W + 2 * pad, Ch, dtype=torch.float16,
                                                          device=dev)
    if PROFILER.active:
        PROFILER.begin("gn_apply", None)
    if pad:
        check(lib().sdk_group_norm_apply_padded(C.byref(args), 1 if silu else 0, _ptr(y), Ch, H, W, pad, _stream()),
              "group_norm_apply_padded")
    else:
        check(lib().sdk_group_norm_apply(C.byref(args), 1 if silu else 0, _ptr(y), Ch, _stream()),
              "group_norm_apply")
    if PROFILER.active:
        PROFILER.end()
    return y


def group_norm_apply_ex(x, gn, silu=True, post_bias=None, residual=None):
    """y = silu?(x*scale + shift) + post_bias[b, c] + residual (DDPM C1 post-activation GroupNorm)."""
    args, (B, H, W, Ch), dev, _ = _gn_args(x, gn=gn)
    y = torch.empty(B, H, W, Ch, dtype=torch.float16, device=dev)
    pb_ld = 0
    if post_bias is not None:
        _need_cuda(post_bias, "group_norm_apply_ex post_bias", torch.float32)
        pb_ld = post_bias.stride(0)
    res_ld = 0
    if residual is not None:
        _need_cuda(residual, "group_norm_apply_ex residual")
        res_ld = residual.shape[-1]
    if PROFILER.active:
        PROFILER.begin("gn_apply", None)
    check(lib().sdk_group_norm_apply_ex(C.byref(args), 1 if silu else 0, _ptr(post_bias), pb_ld, _ptr(residual),
                                        res_ld, _ptr(y), Ch, _stream()), "group_norm_apply_ex")
    if PROFILER.active:
        PROFILER.end()
    return y


def upsample_bilinear2x(x):
    """F.interpolate(scale_factor=2, mode='bilinear', align_corners=True) on NHWC fp16."""
    _need_cuda(x, "upsample_bilinear2x")
    x = x.contiguous()
    B, H, W, Cc = x.shape
    y = torch.empty(B, 2 * H, 2 * W, Cc, dtype=torch.float16, device=x.device)
    check(lib().sdk_upsample_bilinear2x(_ptr(x), _ptr(y), B, H, W, Cc, _stream()), "upsample_bilinear2x")
    return y


def zero_border(x, pad=1):
    """NHWC fp16 x inside a zero border of ``pad``: [B, H + 2pad, W + 2pad, C] (the source of the phase-form
    Upsample conv, ``conv2d(..., phase=True)``)."""
    _need_cuda(x, "zero_border")
    B, H, W, Cc = x.shape
    if x.stride(-1) != 1 or x.stride(1) != W * x.stride(2) or x.stride(0) != H * x.stride(1):
        x = x.contiguous()
    y = torch.empty(B, H + 2 * pad, W + 2 * pad, Cc, dtype=torch.float16, device=x.device)
    check(lib().sdk_zero_border(_ptr(x), x.stride(2), _ptr(y), B, H, W, Cc, pad, _stream()), "zero_border")
    return y


def upsample_nearest2x_padded(x, pad=1):
    """Nearest-x2 upsample of NHWC fp16 x into a zero-bordered [B, 2H + 2pad, 2W + 2pad, C] image (the UNet
    Upsample's interpolate; its 3x3 conv then runs with pad 0 on the unmasked linear issue)."""
    _need_cuda(x, "upsample_nearest2x_padded")
    B, H, W, Cc = x.shape
    if x.stride(-1) != 1 or x.stride(1) != W * x.stride(2) or x.stride(0) != H * x.stride(1):
        x = x.contiguous()
    y = torch.empty(B, 2 * H + 2 * pad, 2 * W + 2 * pad, Cc, dtype=torch.float16, device=x.device)
    check(lib().sdk_upsample_nearest2x_padded(_ptr(x), x.stride(2), _ptr(y), B, H, W, Cc, pad, _stream()),
          "upsample_nearest2x_padded")
    return y


def gelu(x):
    """Exact (erf) GELU, fp16."""
    _need_cuda(x, "gelu")
    x = x.contiguous()
    y = torch.empty_like(x)
    check(lib().sdk_gelu(_ptr(x), _ptr(y), x.numel(), _stream()), "gelu")
    return y


def group_norm_scale_shift(x, gamma, beta, eps, groups=32):
    """Per-(batch, channel) fp32 (scale, shift) [B, C] of GroupNorm(x) from the statistics its producing
    convs emitted (else a statistics pass) — for a 3x3 conv that applies GroupNorm + SiLU to its own
    prologue (``conv2d(gn=(scale, shift), silu=True)`` on the register-staged kernel), so the normalised
    tensor is never written (``sdk_group_norm_finalize``)."""
    args, _, _, gn = _gn_args(x, gamma, beta, eps, groups)
    p0, n0, p1, n1 = _producer_parts(x)
    if PROFILER.active:
        PROFILER.begin("group_norm", None)
    check(lib().sdk_group_norm_finalize(C.byref(args), _ptr(p0), n0, _ptr(p1), n1, _stream()), "group_norm_finalize")
    if PROFILER.active:
        PROFILER.end()
    return gn


def group_norm_affine(x, gamma, beta, eps, groups=32):
    """Per-(batch, channel) (scale, shift) fp32 [B, C] of GroupNorm(x) for the conv prologue."""
    args, _, _, gn = _gn_args(x, gamma, beta, eps, groups)
    if PROFILER.active:
        PROFILER.begin("group_norm", None)
    check(lib().sdk_group_norm_affine(C.byref(args), _stream()), "group_norm_affine")
    if PROFILER.active:
        PROFILER.end()
    return gn


def group_norm(x, gamma, beta, eps, groups=32, silu=True, pad=0, out=None):
    """GroupNorm (+ SiLU) end to end in one C call: statistics (from the producing convs' partials when every
    source carries them) and apply, written contiguous or zero-bordered (``pad``) for a pad-0 3x3 conv.  At the
    UNet's small levels one fused launch; elsewhere the statistics pass then the apply pass (``sdk_group_norm``;
    ``group_norm_plan`` names the forms)."""
    args, (B, H, W, Ch), dev, gn = _gn_args(x, gamma, beta, eps, groups)
    y = _claim(out) if out is not None else torch.empty(B, H + 2 * pad, W + 2 * pad, Ch, dtype=torch.float16,
                                                          device=dev)
    p0, n0, p1, n1 = _producer_parts(x)
    if PROFILER.active:
        PROFILER.begin("group_norm", None)
    check(lib().sdk_group_norm(C.byref(args), 1 if silu else 0, _ptr(y), y.shape[-1], H, W, pad, _ptr(p0), n0,
                               _ptr(p1), n1, _stream()), "group_norm")
    if PROFILER.active:
        PROFILER.end()
    return y


def group_norm_film(x, gamma, beta, eps, film, film_off, groups=32, silu=True, pad=0, out=None):
    """GroupNorm with FiLM conditioning (+ SiLU): ``silu?(GN(x) * (1 + f) + g)`` with ``f = film[:, off:off+C]``,
    ``g = film[:, off+C:off+2C]`` (fp32 ``[B, ld]``, the batched ``emb_layers`` GEMM), folded into the
    per-(batch, channel) affine so x is read once and y written once (``sdk_group_norm_film``)."""
    args, (B, H, W, Ch), dev, gn = _gn_args(x, gamma, beta, eps, groups)
    _need_cuda(film, "group_norm_film film", torch.float32)
    if film.dim() != 2 or film.shape[0] != B or film.stride(1) != 1 or film_off < 0 or \
            film_off + 2 * Ch > film.shape[1]:
        raise ValueError(f"sd_amd.group_norm_film: film {tuple(film.shape)} has no [{B}, {film_off}:{film_off}+2*{Ch}]")
    y = _claim(out) if out is not None else torch.empty(B, H + 2 * pad, W + 2 * pad, Ch, dtype=torch.float16,
                                                          device=dev)
    p0, n0, p1, n1 = _producer_parts(x)
    if PROFILER.active:
        PROFILER.begin("group_norm_film", None)
    check(lib().sdk_group_norm_film(C.byref(args), _ptr(film), film.stride(0), film_off, 1 if silu else 0, _ptr(y),
                                    y.shape[-1], H, W, pad, _ptr(p0), n0, _ptr(p1), n1, _stream()),
          "group_norm_film")
    if PROFILER.active:
        PROFILER.end()
    return y


RESAMPLE_MODES = {"down": _lib.RESAMPLE_AVGPOOL2, "up": _lib.RESAMPLE_NEAREST2}


def group_norm_resample(x, gn, mode, silu=True, pad=0, act=True, raw=True):
    """One read of x, two outputs (``sdk_group_norm_resample``): ``(resample(silu?(x*scale + shift)) zero-bordered
    by pad, resample(x) contiguous)``; ``mode`` 'down' = avg-pool 2x2 stride 2 (odd H / W floor), 'up' = nearest x2.
    ``gn`` = (scale, shift) fp32 ``[B, C]`` or None (raw only); an output not asked for is None."""
    args, (B, H, W, Ch), dev, _ = _gn_args(x, gn=gn)
    if gn is None:
        act = False
    if not act and not raw:
        raise ValueError("sd_amd.group_norm_resample: no output asked for")
    Ho, Wo = (H // 2, W // 2) if mode == "down" else (2 * H, 2 * W)
    ya = torch.empty(B, Ho + 2 * pad, Wo + 2 * pad, Ch, dtype=torch.float16, device=dev) if act else None
    yr = torch.empty(B, Ho, Wo, Ch, dtype=torch.float16, device=dev) if raw else None
    if PROFILER.active:
        PROFILER.begin("group_norm_resample", None)
    check(lib().sdk_group_norm_resample(C.byref(args), RESAMPLE_MODES[mode], 1 if silu else 0, H, W, pad, _ptr(ya),
                                        _ptr(yr), _stream()), "group_norm_resample")
    if PROFILER.active:
        PROFILER.end()
    return ya, yr


def embedding_add(emb, table, ids):
    """``fp16(emb.float() + table[ids])`` — the class-label row added to the timestep embedding
    (``sdk_embedding_add``).  emb fp16 ``[B, D]``, table fp32 ``[n, D]``, ids int64 ``[B]`` on the device; an id
    outside ``[0, n)`` gives a NaN row (the table is never read out of range)."""
    _need_cuda(emb, "embedding_add emb")
    _need_cuda(table, "embedding_add table", torch.float32)
    _need_cuda(ids, "embedding_add ids", torch.int64)
    B, D = emb.shape
    if table.dim() != 2 or table.shape[1] != D or ids.shape != (B,):
        raise ValueError(f"sd_amd.embedding_add: emb {tuple(emb.shape)}, table {tuple(table.shape)}, "
                         f"ids {tuple(ids.shape)}")
    emb, table, ids = emb.contiguous(), table.contiguous(), ids.contiguous()
    out = torch.empty(B, D, dtype=torch.float16, device=emb.device)
    if PROFILER.active:
        PROFILER.begin("embedding_add", None)
    check(lib().sdk_embedding_add(_ptr(emb), _ptr(table), _ptr(ids), _ptr(out), B, D, table.shape[0], _stream()),
          "embedding_add")
    if PROFILER.active:
        PROFILER.end()
    return out


def embedding_rows(ids, table):
    """``table[ids].half()`` — the ClassEmbedder row gather (``sdk_embedding_rows``).  ids int64 ``[n]``, table
    fp32 ``[rows, dim]`` on the device → fp16 ``[n, dim]``; an id outside ``[0, rows)`` raises ValueError (checked
    on the host before the launch: the kernel reads the table by the ids it is given)."""
    _need_cuda(ids, "embedding_rows ids", torch.int64)
    _need_cuda(table, "embedding_rows table", torch.float32)
    if ids.dim() != 1 or ids.numel() < 1 or table.dim() != 2 or table.shape[1] < 1:
        raise ValueError(f"sd_amd.embedding_rows: ids {tuple(ids.shape)} (want [n >= 1]), table {tuple(table.shape)} "
                         "(want [rows, dim >= 1])")
    if ids.device != table.device:
        raise ValueError("sd_amd.embedding_rows: ids and table on different devices")
    lo, hi = int(ids.min()), int(ids.max())
    if lo < 0 or hi >= table.shape[0]:
        raise ValueError(f"sd_amd.embedding_rows: id outside [0, {table.shape[0]}) (min {lo}, max {hi})")
    ids, table = ids.contiguous(), table.contiguous()
    n, dim = ids.shape[0], table.shape[1]
    out = torch.empty(n, dim, dtype=torch.float16, device=table.device)
    check(lib().sdk_embedding_rows(_ptr(ids), _ptr(table), _ptr(out), n, dim, _stream()), "embedding_rows")
    return out


RESIZE_MODES = {"nearest": _lib.RESIZE_NEAREST, "bilinear": _lib.RESIZE_BILINEAR, "bicubic": _lib.RESIZE_BICUBIC,
                "area": _lib.RESIZE_AREA}


def resize2d(x, scale_factor, mode="bilinear", out=None):
    """``F.interpolate(x, scale_factor=scale_factor, mode=mode)`` with torch's defaults (align_corners=False, no
    antialias, the given factor used for the coordinates) on NCHW fp32 (``sdk_resize2d``): ``[B, C, H, W]`` →
    ``[B, C, floor(H * s), floor(W * s)]``.  ``scale_factor``: a number or an (h, w) pair; ``mode``: nearest /
    bilinear / bicubic / area."""
    _need_cuda(x, "resize2d", torch.float32)
    if x.dim() != 4:
        raise ValueError(f"sd_amd.resize2d: expected NCHW, got {tuple(x.shape)}")
    if mode not in RESIZE_MODES:
        raise ValueError(f"sd_amd.resize2d: mode {mode!r} not in {sorted(RESIZE_MODES)}")
    sh, sw = (scale_factor if isinstance(scale_factor, (tuple, list)) else (scale_factor, scale_factor))
    sh, sw = float(sh), float(sw)
    if not (sh > 0 and sw > 0 and math.isfinite(sh) and math.isfinite(sw)):
        raise ValueError(f"sd_amd.resize2d: scale_factor {scale_factor!r} must be positive and finite")
    B, Cc, H, W = x.shape
    Ho, Wo = math.floor(H * sh), math.floor(W * sw)
    if min(B, Cc, H, W, Ho, Wo) < 1:
        raise ValueError(f"sd_amd.resize2d: empty input or output ({tuple(x.shape)} -> {Ho} x {Wo})")
    if B * Cc >= 2 ** 31 or max(H, W, Ho, Wo) >= 2 ** 31:
        raise ValueError("sd_amd.resize2d: sizes exceed int32")
    x = x.contiguous()
    if out is None:
        out = torch.empty(B, Cc, Ho, Wo, dtype=torch.float32, device=x.device)
    else:
        _need_cuda(out, "resize2d out", torch.float32)
        if tuple(out.shape) != (B, Cc, Ho, Wo) or not out.is_contiguous() or out.device != x.device:
            raise ValueError(f"sd_amd.resize2d: out must be contiguous {(B, Cc, Ho, Wo)} on the input's device")
    a = _lib.Resize2dArgs()
    a.x, a.y = x.data_ptr(), out.data_ptr()
    a.planes, a.h, a.w, a.out_h, a.out_w = B * Cc, H, W, Ho, Wo
    a.mode, a.scale_h, a.scale_w = RESIZE_MODES[mode], sh, sw
    if PROFILER.active:
        PROFILER.begin("resize2d", None, nbytes=4 * (x.numel() + out.numel()))
    check(lib().sdk_resize2d(C.byref(a), _stream()), "resize2d")
    if PROFILER.active:
        PROFILER.end()
    return out


def layer_norm(x2d, gamma, beta, eps=1e-5, out=None):
    _need_cuda(x2d, "layer_norm")
    M, Cc = x2d.shape
    y = _claim(out) if out is not None else torch.empty(M, Cc, dtype=torch.float16, device=x2d.device)
    if PROFILER.active:
        PROFILER.begin("layer_norm", None)
    check(lib().sdk_layer_norm(_ptr(x2d), _ptr(y), M, Cc, x2d.stride(0), y.stride(0), _ptr(gamma), _ptr(beta),
                               C.c_float(eps), _stream()), "layer_norm")
    if PROFILER.active:
        PROFILER.end()
    return y


# --------------------------------------------------------------------------- device calibration

def probe_peaks(reps=3):
    """Measured dense fp16 MFMA rate (both MFMA shapes, random operands, every CU busy) and HBM copy
    rate of this device (sdk_probe_*; HIP events, best of ``reps``) — the achievable ceilings next to
    the spec peaks the bench's roofline is quoted against."""
    dev = torch.device("cuda", torch.cuda.current_device())
    seed = torch.randn(32768, device=dev).half()
    nsm = torch.cuda.get_device_properties(dev).multi_processor_count
    sink = torch.empty(4 * nsm * 4, dtype=torch.float32, device=dev)
    out = {}
    # 2 or 4 workgroups of 4 waves per CU (2 / 4 waves per SIMD): the faster is the ceiling
    for m16, iters, name in ((1, 40000, "mfma_16x16x32_f16_tflops"), (0, 20000, "mfma_32x32x16_f16_tflops")):
        top = 0.0
        for blocks in (2 * nsm, 4 * nsm):
            check(lib().sdk_probe_mfma(m16, blocks, 200, _ptr(seed), _ptr(sink), _stream()), "probe_mfma")
            best = float("inf")
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                check(lib().sdk_probe_mfma(m16, blocks, iters, _ptr(seed), _ptr(sink), _stream()), "probe_mfma")
                e1.record()
                e1.synchronize()
                best = min(best, e0.elapsed_time(e1))
            top = max(top, lib().sdk_probe_mfma_flops(m16, blocks, iters) / (best * 1e-3) / 1e12)
        out[name] = round(top, 1)
    # HBM: a 1 GiB copy (read + write counted), the best of a few shapes — loads in flight per thread,
    # non-temporal or default policy, workgroups per CU (the fastest is the device's streaming ceiling)
    nbytes = 1 << 30
    src = torch.empty(nbytes // 2, dtype=torch.float16, device=dev).normal_()
    dst = torch.empty_like(src)
    best_gbs, best_mode = 0.0, 0
    for mode in (0, 1, 2, 3, 1 | (8 << 2), 3 | (8 << 2), 1 | (32 << 2), 3 | (32 << 2), 256, 257, 258, 259):
        check(lib().sdk_probe_copy_ex(_ptr(src), _ptr(dst), nbytes, mode, _stream()), "probe_copy")
        best = float("inf")
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            check(lib().sdk_probe_copy_ex(_ptr(src), _ptr(dst), nbytes, mode, _stream()), "probe_copy")
            e1.record()
            e1.synchronize()
            best = min(best, e0.elapsed_time(e1))
        gbs = 2 * nbytes / (best * 1e-3) / 1e9
        if gbs > best_gbs:
            best_gbs, best_mode = gbs, mode
    out["hbm_copy_gbs"] = round(best_gbs, 1)
    out["hbm_copy_mode"] = {"loads_in_flight": 8 if best_mode & 1 else 4, "nontemporal": bool(best_mode & 2),
                            "form": "flat one pass" if best_mode & 256 else "grid-stride",
                            "workgroups_per_cu": None if best_mode & 256 else ((best_mode >> 2) & 63) or 16}
    del src, dst
    return out


# --------------------------------------------------------------------------- attention

ATTN_FORMS = {"auto": _lib.ATTN_AUTO, "nw4": _lib.ATTN_NW4, "nw8": _lib.ATTN_NW8, "nw8_stag": _lib.ATTN_NW8_STAG,
              "qb2": _lib.ATTN_QB2, "wide": _lib.ATTN_WIDE}
_ATTN_FORM_NAMES = {v: k for k, v in ATTN_FORMS.items()}
# the wide form (head_dim 168..512): query rows per workgroup (grid = ceil(nq / ROWS) * heads * batch) and keys
# per tile of its two-slot K / V ring
ATTN_WIDE_ROWS = _lib.ATTN_WIDE_ROWS
ATTN_WIDE_KT = _lib.ATTN_WIDE_KT


def attention(q, k, v, *, batch, heads, nq, nk, head_dim, scale, out=None, causal=False, form=None, form_out=None):
    """q/k/v: 2-D fp16 views [batch*n, ld] (head h at columns h*head_dim...); ``causal`` masks
    key j > query i.  ``form``: None / "auto" (the head dim's default) or "nw4" / "nw8" / "nw8_stag" /
    "qb2" / "wide" (``sdk_attention_form``; a form without an instantiation at this head dim raises;
    "wide" is head_dim 168..512, non-causal, and what "auto" runs above 160).
    ``form_out``: a dict that receives the launched kernel's form and template arguments (host
    integers, filled before the launch; the same under graph capture)."""
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        _need_cuda(t, "attention " + n)
    if out is None:
        out = torch.empty(batch * nq, heads * head_dim, dtype=torch.float16, device=q.device)
    _claim(out)
    a = AttentionArgs()
    a.q, a.k, a.v, a.o = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    a.q_ld, a.k_ld, a.v_ld, a.o_ld = q.stride(0), k.stride(0), v.stride(0), out.stride(0)
    a.batch, a.heads, a.nq, a.nk, a.head_dim, a.scale = batch, heads, nq, nk, head_dim, scale
    a.causal = 1 if causal else 0
    if PROFILER.active:
        PROFILER.begin("attention", (batch, heads, nq, nk, head_dim))
    if form is None and form_out is None:
        check(lib().sdk_attention(C.byref(a), _stream()), "attention")
    else:
        info = _lib.AttentionFormInfo()
        check(lib().sdk_attention_form(C.byref(a), ATTN_FORMS[form or "auto"], C.byref(info), _stream()), "attention")
        if form_out is not None:
            form_out.update(form=_ATTN_FORM_NAMES[info.form], dqk=info.dqk, dv=info.dv, waves=info.waves,
                            qblocks=info.qblocks, stagger=info.stagger, seed_col=info.seed_col,
                            causal=info.causal, grid=info.grid)
    if PROFILER.active:
        PROFILER.end()
    return out


def linear_attention(q, k, v, *, batch, heads, n, dim_head, out=None):
    """Linear attention (``sdk_linear_attention``): per (batch, head) ``ctx = softmax_n(k)^T v`` then
    ``out = q ctx``.  q/k/v: 2-D fp16 views [batch*n, ld], head h at columns h*dim_head...; dim_head a
    multiple of 8 in [8, 512].  The workspace (chunk partials and the fp16 context) is allocated here."""
    for t, nm in ((q, "q"), (k, "k"), (v, "v")):
        _need_cuda(t, "linear_attention " + nm)
    if out is None:
        out = torch.empty(batch * n, heads * dim_head, dtype=torch.float16, device=q.device)
    _claim(out)
    a = _lib.LinearAttentionArgs()
    a.q, a.k, a.v, a.o = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    a.q_ld, a.k_ld, a.v_ld, a.o_ld = q.stride(0), k.stride(0), v.stride(0), out.stride(0)
    a.batch, a.heads, a.n, a.dim_head = batch, heads, n, dim_head
    nbytes = lib().sdk_linear_attention_workspace_bytes(C.byref(a))
    if nbytes < 0:
        check(-1, "linear_attention")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=q.device)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    if PROFILER.active:
        PROFILER.begin("linear_attention", None)
    check(lib().sdk_linear_attention(C.byref(a), _stream()), "linear_attention")
    if PROFILER.active:
        PROFILER.end()
    return out


def cross_attention_block_supported(channels, head_dim, nk, n_img):
    return bool(lib().sdk_cross_attention_block_supported(channels, head_dim, nk, n_img))


# the block's projection weights in the fragment-packed layout (sdk_xattn_pack_weight: whole 128-B lines per weight
# fetch); False = the row layout (A/B only, same bits)
XATTN_PACKED_W = True


def xattn_packed_weight(pc: PackedConv):
    """The fragment-packed copy of a channels x channels PackedConv for the cross-attention kernel, made once
    and kept on the PackedConv (not inside a graph capture: the first eager evaluation makes it)."""
    pk = getattr(pc, "_xattn_pk", None)
    if pk is None:
        Cc = pc.N
        pk = torch.empty(Cc * Cc, dtype=torch.float16, device=pc.weight.device)
        check(lib().sdk_xattn_pack_weight(pc.weight.data_ptr(), pc.k_total, pk.data_ptr(), Cc, _stream()),
              "xattn_pack_weight")
        pc._xattn_pk = pk
    return pk


def cross_attention_block(t, kv, pc_q: PackedConv, pc_o: PackedConv, *, batch, n_img, nk, heads, head_dim, scale,
                          residual=None, out=None, norm_in=None, norm_out=None, out_ln=None):
    """One-kernel cross-attention block on a cached context K|V: ``to_out(attn(to_q(t), K, V)) + residual``.
    t / residual: [batch*n_img, C] fp16; kv: [batch*nk, >= 2C] fp16 (K | V).

    ``norm_in`` = (gamma, beta, eps): ``t`` is the LayerNorm's INPUT and is normalised inside the
    kernel (BasicTransformerBlock.norm2); ``norm_out`` = (gamma, beta, eps): also returns
    LayerNorm(out) (norm3) — the result is then ``(out, out_ln)``.  Both match ``layer_norm``
    bit for bit."""
    Cc = heads * head_dim
    for x, n in ((t, "t"), (kv, "kv")):
        _need_cuda(x, "cross_attention_block " + n)
    if pc_q.k_total != Cc or pc_o.k_total != Cc or pc_q.N != Cc or pc_o.N != Cc:
        raise ValueError("sd_amd.cross_attention_block: to_q / to_out must be channels x channels")
    if out is None:
        out = torch.empty(batch * n_img, Cc, dtype=torch.float16, device=t.device)
    _claim(out)
    _claim(out_ln)
    a = XAttnArgs()
    a.t, a.kv, a.wq, a.wo = t.data_ptr(), kv.data_ptr(), pc_q.weight.data_ptr(), pc_o.weight.data_ptr()
    packed = XATTN_PACKED_W and (not torch.cuda.is_current_stream_capturing() or
                                 (hasattr(pc_q, "_xattn_pk") and hasattr(pc_o, "_xattn_pk")))
    if packed:
        a.wq, a.wo = xattn_packed_weight(pc_q).data_ptr(), xattn_packed_weight(pc_o).data_ptr()
    a.bias = pc_o.bias.data_ptr() if pc_o.bias is not None else None
    a.res = residual.data_ptr() if residual is not None else None
    a.out = out.data_ptr()
    a.t_ld, a.kv_ld, a.w_ld = t.stride(0), kv.stride(0), 0 if packed else Cc
    a.res_ld = residual.stride(0) if residual is not None else 0
    a.out_ld = out.stride(0)
    a.batch, a.n_img, a.nk, a.channels, a.head_dim, a.scale = batch, n_img, nk, Cc, head_dim, scale
    if PROFILER.active:
        # FLOPs of the three products it replaces (2 projections + attention core)
        PROFILER.begin("cross_attention_block", None)
        PROFILER._cur = PROFILER._cur[:2] + (4.0 * batch * n_img * Cc * Cc + 4.0 * batch * n_img * nk * Cc,) + \
            PROFILER._cur[3:]
    if norm_in is None and norm_out is None:
        check(lib().sdk_cross_attention_block(C.byref(a), _stream()), "cross_attention_block")
    else:
        ln = XAttnLnArgs()
        if norm_in is not None:
            ln.in_gamma, ln.in_beta, ln.in_eps = norm_in[0].data_ptr(), norm_in[1].data_ptr(), norm_in[2]
        if norm_out is not None:
            if out_ln is None:
                out_ln = torch.empty_like(out)
            ln.out_gamma, ln.out_beta, ln.out_eps = norm_out[0].data_ptr(), norm_out[1].data_ptr(), norm_out[2]
            ln.out_ln, ln.out_ln_ld = out_ln.data_ptr(), out_ln.stride(0)
        check(lib().sdk_cross_attention_block_ln(C.byref(a), C.byref(ln), _stream()), "cross_attention_block")
    if PROFILER.active:
        PROFILER.end()
    return (out, out_ln) if norm_out is not None else out


def ff_supported(channels, features):
    return bool(lib().sdk_ff_supported(channels, features))


class PackedFF:
    """The GEGLU FeedForward's weights packed once for ``feed_forward`` (sdk_ff_pack): proj (Linear(C, 2F):
    rows [0, F) = a, [F, 2F) = gate) and the output Linear(F, C)."""

    def __init__(self, w1, b1, w2, b2, device):
        F2, Cc = w1.shape
        self.channels, self.features = Cc, F2 // 2
        if not ff_supported(Cc, self.features):
            raise ValueError(f"sd_amd.PackedFF: unsupported shape channels={Cc} features={self.features}")
        w1h = w1.detach().to(device=device, dtype=torch.float16).contiguous()
        w2h = w2.detach().to(device=device, dtype=torch.float16).contiguous()
        b1f = b1.detach().to(device=device, dtype=torch.float32).contiguous() if b1 is not None else None
        self.b2 = b2.detach().to(device=device, dtype=torch.float32).contiguous() if b2 is not None else None
        nbytes = lib().sdk_ff_packed_bytes(Cc, self.features)
        self.packed = torch.empty(nbytes, dtype=torch.uint8, device=device)
        check(lib().sdk_ff_pack(_ptr(w1h), _ptr(b1f), _ptr(w2h), _ptr(self.packed), Cc, self.features, _stream()),
              "ff_pack")


def feed_forward(pf: PackedFF, t, residual=None, out=None):
    """out = residual + Linear2(GEGLU(t)) in one kernel (t, residual: [M, C] fp16 token rows)."""
    _need_cuda(t, "feed_forward t")
    M, Cc = t.shape
    if Cc != pf.channels or t.stride(-1) != 1:
        raise ValueError("sd_amd.feed_forward: t must be [M, channels] with unit column stride")
    if out is None:
        out = torch.empty(M, Cc, dtype=torch.float16, device=t.device)
    _claim(out)
    a = FfArgs()
    a.t, a.out, a.packed = t.data_ptr(), out.data_ptr(), pf.packed.data_ptr()
    a.b2 = pf.b2.data_ptr() if pf.b2 is not None else None
    if residual is not None:
        _need_cuda(residual, "feed_forward residual")
        a.res, a.res_ld = residual.data_ptr(), residual.stride(0)
    a.t_ld, a.out_ld = t.stride(0), out.stride(0)
    a.rows, a.channels, a.features = M, Cc, pf.features
    if PROFILER.active:
        PROFILER.begin("feed_forward", None, shape=(M, Cc, pf.features))
        PROFILER._cur = PROFILER._cur[:2] + (2.0 * M * Cc * 3 * pf.features,) + PROFILER._cur[3:]
    check(lib().sdk_feed_forward(C.byref(a), _stream()), "feed_forward")
    if PROFILER.active:
        PROFILER.end()
    return out


def token_linear_supported(in_features, out_features):
    return bool(lib().sdk_token_linear_supported(in_features, out_features))


class PackedTokenLinear:
    """A 320 -> 320 Linear / 1x1 conv for ``token_linear`` (sdk_token_linear): fp16 [out][in] weight
    (nn.Linear layout; a [out, in, 1, 1] conv weight is flattened), fp32 bias."""

    def __init__(self, w, b, device):
        w = w.detach().reshape(w.shape[0], -1)
        if not token_linear_supported(w.shape[1], w.shape[0]):
            raise ValueError(f"sd_amd.PackedTokenLinear: unsupported shape {tuple(w.shape)}")
        self.features = w.shape[0]
        self.w = w.to(device=device, dtype=torch.float16).contiguous()
        self.b = b.detach().to(device=device, dtype=torch.float32).contiguous() if b is not None else None


def token_linear(pk: PackedTokenLinear, x, residual=None, out=None, norm=None):
    """out = [residual +] x W^T + b (x, residual: [M, 320] fp16 token rows; out may be residual).
    ``norm=(gamma, beta, eps)`` (fp32 [320]) also returns LayerNorm(out) (sdk_token_linear_ln, the same
    bits as ``layer_norm(out, ...)``): ``(out, out_ln)``."""
    _need_cuda(x, "token_linear x")
    M, K = x.shape
    if K != pk.features or x.stride(-1) != 1:
        raise ValueError("sd_amd.token_linear: x must be [M, 320] with unit column stride")
    if out is None:
        out = torch.empty(M, pk.features, dtype=torch.float16, device=x.device)
    _claim(out)
    a = TokenLinearArgs()
    a.x, a.w, a.out = x.data_ptr(), pk.w.data_ptr(), out.data_ptr()
    a.bias = pk.b.data_ptr() if pk.b is not None else None
    if residual is not None:
        _need_cuda(residual, "token_linear residual")
        if residual.shape != (M, pk.features) or residual.stride(-1) != 1:
            raise ValueError("sd_amd.token_linear: residual must be [M, 320] with unit column stride")
        a.res, a.res_ld = residual.data_ptr(), residual.stride(0)
    a.x_ld, a.out_ld = x.stride(0), out.stride(0)
    a.rows, a.in_features, a.out_features = M, K, pk.features
    if PROFILER.active:
        PROFILER.begin("token_linear", None, shape=(M, pk.features, K))
        PROFILER._cur = PROFILER._cur[:2] + (2.0 * M * K * pk.features,) + PROFILER._cur[3:]
    if norm is None:
        check(lib().sdk_token_linear(C.byref(a), _stream()), "token_linear")
    else:
        g, bt, eps = norm
        _need_cuda(g, "token_linear_ln gamma", torch.float32)
        _need_cuda(bt, "token_linear_ln beta", torch.float32)
        if g.numel() != pk.features or bt.numel() != pk.features:
            raise ValueError("sd_amd.token_linear: norm gamma / beta must have 320 elements")
        out_ln = torch.empty(M, pk.features, dtype=torch.float16, device=x.device)
        check(lib().sdk_token_linear_ln(C.byref(a), g.data_ptr(), bt.data_ptr(), float(eps), out_ln.data_ptr(),
                                        out_ln.stride(0), _stream()), "token_linear_ln")
    if PROFILER.active:
        PROFILER.end()
    return out if norm is None else (out, out_ln)


# ------------------------------------------------------------ SpatialTransformer entry, chained (sdk_proj_norm_qkv)
PROJ_QKV_C, PROJ_QKV_N = 320, 960
PROJ_QKV_PANEL = 256         # rows a workgroup of the chained kernel (and of the row-panel kernel) owns


def proj_qkv_perm():
    """``perm[p]`` = the proj_in output channel whose weight row and bias sit at packed position ``p`` (int64 [320]):
    ``p = 160 c + 16 nb + 4 cg + q`` holds channel ``32 (g // 2) + 8 cg + 4 (g % 2) + q`` with ``g = 10 c + nb`` — the
    order in which a 16x16 MFMA accumulator block (one token and four channels per lane) is, once rounded to fp16,
    half of the same lane's eight-channel operand fragment of the next GEMM."""
    p = torch.arange(PROJ_QKV_C)
    c, r = p // 160, p % 160
    nb, cg, q = r // 16, (r % 16) // 4, r % 4
    g = 10 * c + nb
    return 32 * (g // 2) + 8 * cg + 4 * (g % 2) + q


def proj_qkv_pack(w_in, b_in, w_qkv, b_qkv=None):
    """(weight fp32 [1280, 320], bias fp32 [1280]) of the chained kernel: proj_in's rows permuted by ``proj_qkv_perm``,
    then the q|k|v rows (bias zero where the projections have none)."""
    w_in = w_in.detach().float().reshape(w_in.shape[0], -1)
    w_qkv = w_qkv.detach().float().reshape(w_qkv.shape[0], -1)
    if tuple(w_in.shape) != (PROJ_QKV_C, PROJ_QKV_C) or tuple(w_qkv.shape) != (PROJ_QKV_N, PROJ_QKV_C):
        raise ValueError(f"sd_amd.proj_qkv_pack: unsupported shapes {tuple(w_in.shape)} / {tuple(w_qkv.shape)}")
    perm = proj_qkv_perm().to(w_in.device)
    b_in = torch.zeros(PROJ_QKV_C, device=w_in.device) if b_in is None else b_in.detach().float()
    b_qkv = torch.zeros(PROJ_QKV_N, device=w_in.device) if b_qkv is None else b_qkv.detach().float().to(w_in.device)
    return torch.cat([w_in[perm], w_qkv.to(w_in.device)], 0), torch.cat([b_in[perm], b_qkv], 0)


def proj_qkv_unpack(w, b):
    """Inverse of ``proj_qkv_pack``: (w_in, b_in, w_qkv, b_qkv)."""
    perm = proj_qkv_perm().to(w.device)
    w_in, b_in = torch.empty_like(w[:PROJ_QKV_C]), torch.empty_like(b[:PROJ_QKV_C])
    w_in[perm], b_in[perm] = w[:PROJ_QKV_C], b[:PROJ_QKV_C]
    return w_in, b_in, w[PROJ_QKV_C:], b[PROJ_QKV_C:]


def proj_norm_qkv_supported(in_features, features, qkv_features):
    return bool(lib().sdk_proj_norm_qkv_supported(in_features, features, qkv_features))


_CU_COUNT = {}


def cu_count(dev):
    """Compute units of a device (cached: asked on every routed call)."""
    key = torch.device(dev)
    if key not in _CU_COUNT:
        _CU_COUNT[key] = torch.cuda.get_device_properties(key).multi_processor_count
    return _CU_COUNT[key]


def proj_qkv_chain_fills(rows, cus):
    """The routing rule of the chained kernel, stated once: its 256-row panels must fill the CUs as the row-panel
    kernel's do — one round (``ceil(rows / 256) <= cus``) or a last round that is at least half full.  C5's 96x96
    level (288 panels on 256 CUs: a second round of 32) is where the plain row-panel kernel already loses."""
    panels = (rows + PROJ_QKV_PANEL - 1) // PROJ_QKV_PANEL
    last = panels % cus
    return panels <= cus or last == 0 or 2 * last >= cus


class PackedProjQkv:
    """proj_in (320 -> 320, bias) and the self-attention's concatenated to_q | to_k | to_v (320 -> 960) packed for
    ``proj_norm_qkv``: one fp16 [1280][320] matrix and one fp32 [1280] bias (``proj_qkv_pack``)."""

    def __init__(self, w_in, b_in, w_qkv, device, b_qkv=None):
        w, b = proj_qkv_pack(w_in, b_in, w_qkv, b_qkv)
        self.w = w.to(device=device, dtype=torch.float16).contiguous()
        self.b = b.to(device=device, dtype=torch.float32).contiguous()


def proj_norm_qkv(pk: PackedProjQkv, x, norm, gn=None, hw=None, tok=None, qkv=None):
    """``(tok, qkv)`` with tok = proj_in(xn) and qkv = [q | k | v](LayerNorm(tok)) in one launch; xn = x ([M, 320] fp16
    rows), or with ``gn=(scale, shift)`` (fp32 [M / hw, 320], ``group_norm_affine``) and ``hw`` rows per image the
    GroupNorm of x applied on the way in.  ``norm=(gamma, beta, eps)`` of the LayerNorm (fp32 [320]).  The bits of
    ``group_norm(silu=False)`` -> ``token_linear(norm=)`` -> ``linear`` on the q|k|v weight."""
    _need_cuda(x, "proj_norm_qkv x")
    M, K = x.shape
    if K != PROJ_QKV_C or x.stride(-1) != 1:
        raise ValueError("sd_amd.proj_norm_qkv: x must be [M, 320] with unit column stride")
    g, bt, eps = norm
    _need_cuda(g, "proj_norm_qkv gamma", torch.float32)
    _need_cuda(bt, "proj_norm_qkv beta", torch.float32)
    if g.numel() != PROJ_QKV_C or bt.numel() != PROJ_QKV_C:
        raise ValueError("sd_amd.proj_norm_qkv: norm gamma / beta must have 320 elements")
    if tok is None:
        tok = torch.empty(M, PROJ_QKV_C, dtype=torch.float16, device=x.device)
    if qkv is None:
        qkv = torch.empty(M, PROJ_QKV_N, dtype=torch.float16, device=x.device)
    _claim(tok)
    _claim(qkv)
    a = ProjNormQkvArgs()
    a.x, a.w, a.bias, a.gamma, a.beta = x.data_ptr(), pk.w.data_ptr(), pk.b.data_ptr(), g.data_ptr(), bt.data_ptr()
    a.tok, a.qkv = tok.data_ptr(), qkv.data_ptr()
    a.x_ld, a.tok_ld, a.qkv_ld = x.stride(0), tok.stride(0), qkv.stride(0)
    a.rows, a.in_features, a.features, a.qkv_features = M, K, tok.shape[1], qkv.shape[1]
    a.eps = float(eps)
    if gn is not None:
        sc, sh = gn
        _need_cuda(sc, "proj_norm_qkv gn scale", torch.float32)
        _need_cuda(sh, "proj_norm_qkv gn shift", torch.float32)
        if hw and (not sc.is_contiguous() or not sh.is_contiguous() or sc.numel() != M // hw * PROJ_QKV_C
                   or sh.numel() != sc.numel()):
            raise ValueError("sd_amd.proj_norm_qkv: gn scale / shift must be contiguous fp32 [M / hw, 320]")
        a.gn_scale, a.gn_shift = sc.data_ptr(), sh.data_ptr()
    a.hw = int(hw or 0)
    if PROFILER.active:
        # x in, tok and qkv out: the GroupNorm output and norm1(tok) never cross HBM
        PROFILER.begin("proj_norm_qkv", None, shape=(M, PROJ_QKV_C + PROJ_QKV_N, K),
                       nbytes=2 * M * (K + PROJ_QKV_C + PROJ_QKV_N))
        PROFILER._cur = PROFILER._cur[:2] + (2.0 * M * K * (PROJ_QKV_C + PROJ_QKV_N),) + PROFILER._cur[3:]
    check(lib().sdk_proj_norm_qkv(C.byref(a), _stream()), "proj_norm_qkv")
    if PROFILER.active:
        PROFILER.end()
    return tok, qkv


# --------------------------------------------------------------------------- sampler glue

def token_embedding(ids: torch.Tensor, tok: torch.Tensor, pos: torch.Tensor):
    """CLIP token + position embedding: ids int64 [B, T] → fp16 [B, T, D] (fp32 tables)."""
    _need_cuda(ids, "token_embedding", torch.int64)
    _need_cuda(tok, "token_embedding table", torch.float32)
    _need_cuda(pos, "token_embedding positions", torch.float32)
    B, T = ids.shape
    if T > pos.shape[0]:
        raise ValueError(f"sd_amd.token_embedding: {T} tokens > {pos.shape[0]} positions")
    out = torch.empty(B, T, tok.shape[1], dtype=torch.float16, device=ids.device)
    check(lib().sdk_token_embedding(_ptr(ids.contiguous()), _ptr(tok), _ptr(pos), _ptr(out), B, T, tok.shape[1],
                                    _stream()), "token_embedding")
    return out


def extract_patches(z: torch.Tensor, kh: int, kw: int, sy: int, sx: int):
    """NCHW fp32 [B, C, H, W] → patches [Ly*Lx, B, C, kh, kw] (torch.nn.Unfold patch order)."""
    _need_cuda(z, "extract_patches", torch.float32)
    z = z.contiguous()
    B, Cc, H, W = z.shape
    Ly, Lx = (H - kh) // sy + 1, (W - kw) // sx + 1
    out = torch.empty(Ly * Lx, B, Cc, kh, kw, dtype=torch.float32, device=z.device)
    check(lib().sdk_extract_patches(_ptr(z), _ptr(out), B, Cc, H, W, kh, kw, sy, sx, _stream()), "extract_patches")
    return out


def fold_patches(patches: torch.Tensor, pix_w: torch.Tensor, l_w, H: int, W: int, sy: int, sx: int, Ly: int,
                 Lx: int):
    """[L, B, C, ph, pw] fp32 → normalised weighted overlap-add [B, C, H, W]."""
    _need_cuda(patches, "fold_patches", torch.float32)
    _need_cuda(pix_w, "fold_patches weights", torch.float32)
    patches = patches.contiguous()
    L, B, Cc, ph, pw = patches.shape
    assert L == Ly * Lx
    out = torch.empty(B, Cc, H, W, dtype=torch.float32, device=patches.device)
    check(lib().sdk_fold_patches(_ptr(patches), _ptr(pix_w.contiguous()), _ptr(l_w), _ptr(out), B, Cc, H, W, ph, pw,
                                 sy, sx, Ly, Lx, _stream()), "fold_patches")
    return out


def timestep_embedding(t: torch.Tensor, freqs: torch.Tensor, dim: int):
    _need_cuda(t, "timestep_embedding", torch.int64)
    out = torch.empty(t.shape[0], dim, dtype=torch.float16, device=t.device)
    check(lib().sdk_timestep_embedding(_ptr(t), _ptr(freqs), _ptr(out), t.shape[0], dim, _stream()),
          "timestep_embedding")
    return out


def nchw_to_nhwc(x: torch.Tensor, c_pad: int, scale: float = 1.0):
    _need_cuda(x, "nchw_to_nhwc", torch.float32)
    x = x.contiguous()
    B, Cc, H, W = x.shape
    y = torch.empty(B, H, W, c_pad, dtype=torch.float16, device=x.device)
    check(lib().sdk_nchw_to_nhwc(_ptr(x), _ptr(y), B, Cc, H * W, c_pad, C.c_float(scale), _stream()),
          "nchw_to_nhwc")
    return y


def _drop_scale(what, keep, drop_p, ref, noise):
    """(keep as a contiguous byte tensor or None, fp32(1 / (1 - p))) of the noise dropout: the factor
    ``F.dropout`` multiplies the kept elements by; ``p == 1`` multiplies by 0, as torch returns zeros."""
    p = float(drop_p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"sd_amd.{what}: drop_p must be in [0, 1], got {drop_p}")
    if keep is None:
        if p > 0.0:
            raise ValueError(f"sd_amd.{what}: drop_p > 0 needs keep (one byte per element)")
        return None, 0.0
    if not torch.is_tensor(keep) or not keep.is_cuda or keep.device != ref.device or \
            keep.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f"sd_amd.{what}: keep must be a CUDA uint8 / bool tensor on {ref.device}")
    if keep.shape != ref.shape:
        raise ValueError(f"sd_amd.{what}: keep {tuple(keep.shape)} vs {tuple(ref.shape)}")
    if noise is None:
        raise ValueError(f"sd_amd.{what}: keep needs noise")
    keep = keep.contiguous()
    if keep.dtype == torch.bool:
        keep = keep.view(torch.uint8)
    return keep, (0.0 if p == 1.0 else float(np.float32(1.0 / (1.0 - p))))


def _same_f32(what, ref, **tensors):
    """Each given tensor: CUDA fp32 of ``ref``'s shape on its device, made contiguous."""
    out = {}
    for k, v in tensors.items():
        if v is None:
            out[k] = None
            continue
        if not torch.is_tensor(v) or not v.is_cuda or v.dtype != torch.float32 or v.device != ref.device:
            raise ValueError(f"sd_amd.{what}: {k} must be a CUDA fp32 tensor on {ref.device}")
        if v.shape != ref.shape:
            raise ValueError(f"sd_amd.{what}: {k} {tuple(v.shape)} vs {tuple(ref.shape)}")
        out[k] = v.contiguous()
    return out


def _mask_mode(what, mask, shape):
    """mask_mode of ``sdk_masked_q_sample`` for a mask over an NCHW ``shape``."""
    if len(shape) != 4:
        raise ValueError(f"sd_amd.{what}: the mask blend needs NCHW tensors, got {tuple(shape)}")
    B, Cc, H, W = shape
    modes = {(B, 1, H, W): 0, (1, 1, H, W): 1, (B, Cc, H, W): 2}      # equal shapes index alike
    if tuple(mask.shape) not in modes:
        raise ValueError(f"sd_amd.{what}: mask {tuple(mask.shape)} does not broadcast over {tuple(shape)}")
    return modes[tuple(mask.shape)]


def _ddim_ex(what, ref, x, e, sc, pred_x0_in, noise, e_uncond, guidance, v_param, x_prev, pred_x0, temperature,
             keep, drop_p, blend_x0, blend_noise, blend_mask, blend_sqrt_acp, blend_sqrt_1m_acp, x_next):
    """The one call of ``sdk_ddim_step_ex`` behind ``ddim_step`` / ``ddim_xprev``."""
    t = _same_f32(what, ref, noise=noise, e_uncond=e_uncond)
    noise, e_uncond = t["noise"], t["e_uncond"]
    keep, scale = _drop_scale(what, keep, drop_p, ref, noise)
    ex = _lib.DdimExArgs()
    a = ex.step
    a.x = x.data_ptr() if x is not None else None
    a.e, a.x_prev, a.pred_x0 = e.data_ptr(), x_prev.data_ptr(), pred_x0.data_ptr()
    a.e_uncond = e_uncond.data_ptr() if e_uncond is not None else None
    a.noise = noise.data_ptr() if noise is not None else None
    a.n = ref.numel()
    if not pred_x0_in:
        a.sqrt_one_minus_at = float(sc["sqrt_one_minus_at"])
        a.sqrt_at = float(sc["sqrt_at"])
    a.dir_coef = float(sc["dir_coef"])
    a.sqrt_a_prev = float(sc["sqrt_a_prev"])
    a.sigma = float(sc["sigma"])
    a.temperature = float(temperature)
    a.guidance = float(guidance)
    if v_param is not None:
        a.v_param = 1
        a.v_sqrt_a, a.v_sqrt_1ma = float(v_param[0]), float(v_param[1])
    ex.pred_x0_in = int(pred_x0_in)
    if keep is not None:
        ex.keep, ex.drop_scale = keep.data_ptr(), scale
    if blend_mask is None:
        if blend_x0 is not None or blend_noise is not None or x_next is not None:
            raise ValueError(f"sd_amd.{what}: blend_x0 / blend_noise / x_next need blend_mask")
        check(lib().sdk_ddim_step_ex(C.byref(ex), _stream()), what)
        return None
    if blend_x0 is None or blend_noise is None or blend_sqrt_acp is None or blend_sqrt_1m_acp is None:
        raise ValueError(f"sd_amd.{what}: the blend needs blend_x0, blend_noise, blend_sqrt_acp and blend_sqrt_1m_acp")
    t = _same_f32(what, ref, blend_x0=blend_x0, blend_noise=blend_noise)
    if not torch.is_tensor(blend_mask) or not blend_mask.is_cuda or blend_mask.dtype != torch.float32 or \
            blend_mask.device != ref.device:
        raise ValueError(f"sd_amd.{what}: blend_mask must be a CUDA fp32 tensor on {ref.device}")
    m = ex.blend
    m.mask_mode = _mask_mode(what, blend_mask, ref.shape)
    blend_mask = blend_mask.contiguous()
    if x_next is None:
        x_next = torch.empty_like(ref)
    elif x_next.shape != ref.shape or not x_next.is_contiguous() or x_next.dtype != torch.float32 or \
            x_next.device != ref.device:
        raise ValueError(f"sd_amd.{what}: x_next must be a contiguous CUDA fp32 tensor of x's shape")
    m.x0, m.noise, m.mask, m.out = t["blend_x0"].data_ptr(), t["blend_noise"].data_ptr(), blend_mask.data_ptr(), \
        x_next.data_ptr()
    m.n, m.per_sample, m.hw = ref.numel(), ref.numel() // ref.shape[0], ref.shape[2] * ref.shape[3]
    m.sqrt_acp, m.sqrt_1m_acp = float(blend_sqrt_acp), float(blend_sqrt_1m_acp)
    check(lib().sdk_ddim_step_ex(C.byref(ex), _stream()), what)
    return x_next


def ddim_step(x, e, sc: dict, noise=None, e_uncond=None, guidance=1.0, v_param=None, x_prev=None, pred_x0=None,
              temperature=1.0, *, keep=None, drop_p=0.0, blend_x0=None, blend_noise=None, blend_mask=None,
              blend_sqrt_acp=None, blend_sqrt_1m_acp=None, x_next=None):
    """Fused DDIM update; ``sc`` holds the fp32 scalars (sampler.DDIMSampler computes them).  ``keep`` /
    ``drop_p``: noise dropout (one byte per element; the noise term is multiplied by keep·fp32(1/(1−p))).
    ``blend_mask`` (+ ``blend_x0``, ``blend_noise`` and the NEXT timestep's ``blend_sqrt_acp`` /
    ``blend_sqrt_1m_acp``): the known-region blend of the next loop iteration in the same launch,
    ``x_next = (sa·x0 + s1m·noise)·mask + (1 − mask)·x_prev``; the return is then (x_prev, pred_x0, x_next)."""
    _need_cuda(x, "ddim_step", torch.float32)
    _need_cuda(e, "ddim_step", torch.float32)
    if e.shape != x.shape:
        raise ValueError(f"sd_amd.ddim_step: x {tuple(x.shape)} vs e {tuple(e.shape)}")
    x, e = x.contiguous(), e.contiguous()
    xp = x_prev if x_prev is not None else torch.empty_like(x)
    p0 = pred_x0 if pred_x0 is not None else torch.empty_like(x)
    xn = _ddim_ex("ddim_step", x, x, e, sc, False, noise, e_uncond, guidance, v_param, xp, p0, temperature, keep,
                  drop_p, blend_x0, blend_noise, blend_mask, blend_sqrt_acp, blend_sqrt_1m_acp, x_next)
    return (xp, p0) if xn is None else (xp, p0, xn)


def ddim_xprev(pred_x0, e, sc: dict, x=None, noise=None, e_uncond=None, guidance=1.0, v_param=None, x_prev=None,
               temperature=1.0, *, keep=None, drop_p=0.0, blend_x0=None, blend_noise=None, blend_mask=None,
               blend_sqrt_acp=None, blend_sqrt_1m_acp=None, x_next=None):
    """Second half of ``ddim_step`` with ``pred_x0`` as an input (the quantize_denoised path quantises
    it in between): x_prev = sqrt(a_prev)·pred_x0 + dir_coef·e + sigma·noise·temperature, the same
    fp32 operations in the same order.  ``e`` / ``e_uncond`` / ``guidance`` / ``v_param`` are the
    first call's; ``x`` is needed only with ``v_param``.  ``keep`` / ``drop_p`` / ``blend_*`` as in
    ``ddim_step``; with a blend the return is (x_prev, x_next)."""
    _need_cuda(pred_x0, "ddim_xprev", torch.float32)
    _need_cuda(e, "ddim_xprev", torch.float32)
    if e.shape != pred_x0.shape:
        raise ValueError(f"sd_amd.ddim_xprev: pred_x0 {tuple(pred_x0.shape)} vs e {tuple(e.shape)}")
    pred_x0, e = pred_x0.contiguous(), e.contiguous()
    xp = x_prev if x_prev is not None else torch.empty_like(pred_x0)
    if v_param is not None:
        if x is None:
            raise ValueError("sd_amd.ddim_xprev: v_param needs x")
        _need_cuda(x, "ddim_xprev", torch.float32)
        x = x.contiguous()
    else:
        x = None
    xn = _ddim_ex("ddim_xprev", pred_x0, x, e, sc, True, noise, e_uncond, guidance, v_param, xp, pred_x0, temperature,
                  keep, drop_p, blend_x0, blend_noise, blend_mask, blend_sqrt_acp, blend_sqrt_1m_acp, x_next)
    return xp if xn is None else (xp, xn)


MULTISTEP_FORMS = {"plms": _lib.MULTISTEP_PLMS, "plms_warmup": _lib.MULTISTEP_PLMS_WARMUP, "dpm": _lib.MULTISTEP_DPM}


def multistep_step(x, e, sc: dict, form="plms", history=(), e_next=None, coefs=None, e_uncond=None, guidance=1.0,
                   v_param=None, x_prev=None, pred_x0=None, hist_out=None, *, blend_x0=None, blend_noise=None,
                   blend_mask=None, blend_sqrt_acp=None, blend_sqrt_1m_acp=None, x_next=None):
    """Fused multistep update (``sdk_multistep_step``), one launch.  ``sc``: the eta = 0 scalars of
    ``DDIMSampler.step_scalars``.  ``form`` "plms": ``history`` holds the guided ε of the previous 0-3 steps, most
    recent first, and ``e' = e | (3e − h1)/2 | (23e − 16h1 + 5h2)/12 | (55e − 59h1 + 37h2 − 9h3)/24`` replaces ε in
    the DDIM update; "plms_warmup": ``e' = (e + e_next)/2``; "dpm": ``coefs = (c_x, c_0, c_1)``, ``history`` the
    previous data prediction or empty, ``x_prev = c_x·x + c_0·D (+ c_1·h1)``.  ``hist_out`` (a contiguous CUDA fp32
    tensor of x's shape, or None) receives the guided ε (PLMS) or D (DPM) and may be one of ``history``.
    ``e_uncond`` / ``guidance`` / ``v_param`` / ``x_prev`` / ``pred_x0`` / ``blend_*`` / ``x_next`` as in
    ``ddim_step``.  Returns (x_prev, pred_x0), with a blend (x_prev, pred_x0, x_next)."""
    what = "multistep_step"
    _need_cuda(x, what, torch.float32)
    _need_cuda(e, what, torch.float32)
    if e.shape != x.shape:
        raise ValueError(f"sd_amd.{what}: x {tuple(x.shape)} vs e {tuple(e.shape)}")
    if form not in MULTISTEP_FORMS:
        raise ValueError(f"sd_amd.{what}: form must be one of {sorted(MULTISTEP_FORMS)}, got {form!r}")
    history = list(history)
    most = {"plms": 3, "plms_warmup": 0, "dpm": 1}[form]
    if len(history) > most:
        raise ValueError(f"sd_amd.{what}: form '{form}' takes at most {most} history tensors, got {len(history)}")
    if (form == "plms_warmup") != (e_next is not None):
        raise ValueError(f"sd_amd.{what}: e_next goes with form 'plms_warmup' (and only with it)")
    if (form == "dpm") != (coefs is not None):
        raise ValueError(f"sd_amd.{what}: coefs = (c_x, c_0, c_1) goes with form 'dpm' (and only with it)")
    x, e = x.contiguous(), e.contiguous()
    t = _same_f32(what, x, e_uncond=e_uncond, e_next=e_next, **{f"history[{k}]": h for k, h in enumerate(history)})
    for k, h in enumerate(history):
        if h is None:
            raise ValueError(f"sd_amd.{what}: history[{k}] is None")
    outs = {"x_prev": x_prev, "pred_x0": pred_x0, "hist_out": hist_out, "x_next": x_next}
    for k, v in outs.items():
        if v is not None and (not torch.is_tensor(v) or v.shape != x.shape or not v.is_contiguous() or
                              v.dtype != torch.float32 or v.device != x.device):
            raise ValueError(f"sd_amd.{what}: {k} must be a contiguous CUDA fp32 tensor of x's shape")
    xp = x_prev if x_prev is not None else torch.empty_like(x)
    p0 = pred_x0 if pred_x0 is not None else torch.empty_like(x)
    m = _lib.MultistepArgs()
    a = m.step
    a.x, a.e, a.x_prev, a.pred_x0 = x.data_ptr(), e.data_ptr(), xp.data_ptr(), p0.data_ptr()
    a.e_uncond = t["e_uncond"].data_ptr() if t["e_uncond"] is not None else None
    a.n = x.numel()
    a.sqrt_one_minus_at, a.sqrt_at = float(sc["sqrt_one_minus_at"]), float(sc["sqrt_at"])
    if form != "dpm":
        if float(sc.get("sigma", 0.0)) != 0.0:
            raise ValueError(f"sd_amd.{what}: PLMS is deterministic: the scalars must be those of eta = 0")
        a.dir_coef, a.sqrt_a_prev = float(sc["dir_coef"]), float(sc["sqrt_a_prev"])
    else:
        m.c_x, m.c_0, m.c_1 = (float(c) for c in coefs)
    a.temperature, a.guidance = 1.0, float(guidance)
    if v_param is not None:
        a.v_param = 1
        a.v_sqrt_a, a.v_sqrt_1ma = float(v_param[0]), float(v_param[1])
    m.form, m.nhist = MULTISTEP_FORMS[form], len(history)
    for k in range(len(history)):
        m.hist[k] = t[f"history[{k}]"].data_ptr()
    if e_next is not None:
        m.e_next = t["e_next"].data_ptr()
    if hist_out is not None:
        m.hist_out = hist_out.data_ptr()
    if blend_mask is None:
        if blend_x0 is not None or blend_noise is not None or x_next is not None:
            raise ValueError(f"sd_amd.{what}: blend_x0 / blend_noise / x_next need blend_mask")
        check(lib().sdk_multistep_step(C.byref(m), _stream()), what)
        return xp, p0
    if blend_x0 is None or blend_noise is None or blend_sqrt_acp is None or blend_sqrt_1m_acp is None:
        raise ValueError(f"sd_amd.{what}: the blend needs blend_x0, blend_noise, blend_sqrt_acp and blend_sqrt_1m_acp")
    tb = _same_f32(what, x, blend_x0=blend_x0, blend_noise=blend_noise)
    if not torch.is_tensor(blend_mask) or not blend_mask.is_cuda or blend_mask.dtype != torch.float32 or \
            blend_mask.device != x.device:
        raise ValueError(f"sd_amd.{what}: blend_mask must be a CUDA fp32 tensor on {x.device}")
    b = m.blend
    b.mask_mode = _mask_mode(what, blend_mask, x.shape)
    blend_mask = blend_mask.contiguous()
    xn = x_next if x_next is not None else torch.empty_like(x)
    b.x0, b.noise, b.mask, b.out = tb["blend_x0"].data_ptr(), tb["blend_noise"].data_ptr(), blend_mask.data_ptr(), \
        xn.data_ptr()
    b.n, b.per_sample, b.hw = x.numel(), x.numel() // x.shape[0], x.shape[2] * x.shape[3]
    b.sqrt_acp, b.sqrt_1m_acp = float(blend_sqrt_acp), float(blend_sqrt_1m_acp)
    check(lib().sdk_multistep_step(C.byref(m), _stream()), what)
    return xp, p0, xn


def cfg_combine(e_uncond, e_cond, guidance, out=None):
    """``e_uncond + guidance·(e_cond − e_uncond)`` (``ddim.py:178``) as a tensor: the two fp32 operations of
    the combine fused into ``ddim_step``, so ``ddim_step(x, cfg_combine(u, c, g), sc)`` has the bits of
    ``ddim_step(x, c, sc, e_uncond=u, guidance=g)``."""
    _need_cuda(e_cond, "cfg_combine", torch.float32)
    t = _same_f32("cfg_combine", e_cond, e_uncond=e_uncond)
    if t["e_uncond"] is None:
        raise ValueError("sd_amd.cfg_combine: e_uncond must be a CUDA fp32 tensor")
    e_cond = e_cond.contiguous()
    y = out if out is not None else torch.empty_like(e_cond)
    if y.shape != e_cond.shape or not y.is_contiguous() or y.dtype != torch.float32 or y.device != e_cond.device:
        raise ValueError("sd_amd.cfg_combine: out must be a contiguous CUDA fp32 tensor of e_cond's shape")
    check(lib().sdk_cfg_combine(t["e_uncond"].data_ptr(), e_cond.data_ptr(), y.data_ptr(), e_cond.numel(),
                                C.c_float(float(guidance)), _stream()), "cfg_combine")
    return y


# --------------------------------------------------------------------------- ancestral sampler / concat

def concat_nchw_to_nhwc(srcs, c_pad: int):
    """``nchw_to_nhwc(torch.cat(srcs, 1), c_pad)`` in one pass, without the concatenated fp32 tensor:
    1..4 NCHW fp32 sources of one ``B, H, W`` → NHWC fp16 ``[B, H, W, c_pad]`` (zeros past the channel sum)."""
    srcs = list(srcs)
    if not 1 <= len(srcs) <= 4:
        raise ValueError(f"sd_amd.concat_nchw_to_nhwc: 1..4 sources, got {len(srcs)}")
    for s in srcs:
        _need_cuda(s, "concat_nchw_to_nhwc", torch.float32)
        if s.dim() != 4 or s.shape[0] != srcs[0].shape[0] or s.shape[2:] != srcs[0].shape[2:]:
            raise ValueError("sd_amd.concat_nchw_to_nhwc: sources must be NCHW with the same batch and spatial "
                             f"size, got {[tuple(t.shape) for t in srcs]}")
    srcs = [s.contiguous() for s in srcs]
    B, _, H, W = srcs[0].shape
    csum = sum(s.shape[1] for s in srcs)
    if c_pad < csum:
        raise ValueError(f"sd_amd.concat_nchw_to_nhwc: c_pad {c_pad} below the channel sum {csum}")
    y = torch.empty(B, H, W, c_pad, dtype=torch.float16, device=srcs[0].device)
    a = _lib.ConcatArgs()
    for i, s in enumerate(srcs):
        a.src[i], a.channels[i] = s.data_ptr(), s.shape[1]
    a.nsrc, a.y, a.batch, a.hw, a.c_pad = len(srcs), y.data_ptr(), B, H * W, c_pad
    check(lib().sdk_concat_nchw_to_nhwc(C.byref(a), _stream()), "concat_nchw_to_nhwc")
    return y


def patch_grid(h: int, w: int, ks, stride):
    """Patch geometry of ``split_input_params`` on an ``h x w`` tensor: ``(ks', stride', Ly, Lx)`` with ``ks`` and
    ``stride`` clipped to the tensor (``Diffusion/ddpm.py:818-825``) and ``Ly x Lx`` the ``torch.nn.Unfold`` patch
    grid.  Host arithmetic only."""
    h, w = int(h), int(w)
    ks, stride = (int(ks[0]), int(ks[1])), (int(stride[0]), int(stride[1]))
    if h <= 0 or w <= 0 or min(ks) <= 0 or min(stride) <= 0:
        raise ValueError(f"sd_amd.patch_grid: sizes must be positive, got {h}x{w}, ks {ks}, stride {stride}")
    ks = (min(ks[0], h), min(ks[1], w))
    stride = (min(stride[0], h), min(stride[1], w))
    return ks, stride, (h - ks[0]) // stride[0] + 1, (w - ks[1]) // stride[1] + 1


def patch_pack(srcs, c_pad: int, kh: int, kw: int, sy: int, sx: int, p0: int = 0, np: int = None):
    """``concat_nchw_to_nhwc`` of the ``extract_patches`` output of every source, for the patches
    ``[p0, p0 + np)`` (``np=None``: up to the last one), in one pass without any fp32 patch tensor: 1..4 NCHW fp32
    sources of one ``B, H, W`` → NHWC fp16 ``[np, kh, kw, c_pad]``; patch ``p = l*B + b`` (Unfold order)."""
    srcs = list(srcs)
    if not 1 <= len(srcs) <= 4:
        raise ValueError(f"sd_amd.patch_pack: 1..4 sources, got {len(srcs)}")
    for s in srcs:
        _need_cuda(s, "patch_pack", torch.float32)
        if s.dim() != 4 or s.shape[0] != srcs[0].shape[0] or s.shape[2:] != srcs[0].shape[2:]:
            raise ValueError("sd_amd.patch_pack: sources must be NCHW with the same batch and spatial size, got "
                             f"{[tuple(t.shape) for t in srcs]}")
    srcs = [s.contiguous() for s in srcs]
    B, _, H, W = srcs[0].shape
    csum = sum(s.shape[1] for s in srcs)
    if c_pad < csum:
        raise ValueError(f"sd_amd.patch_pack: c_pad {c_pad} below the channel sum {csum}")
    if not (0 < kh <= H and 0 < kw <= W and sy > 0 and sx > 0):
        raise ValueError(f"sd_amd.patch_pack: patches {kh}x{kw} every ({sy}, {sx}) do not fit {H}x{W}")
    total = ((H - kh) // sy + 1) * ((W - kw) // sx + 1) * B
    if np is None:
        np = total - p0
    if p0 < 0 or np < 1 or p0 + np > total:
        raise ValueError(f"sd_amd.patch_pack: window [{p0}, {p0 + np}) outside the {total} patches")
    y = torch.empty(np, kh, kw, c_pad, dtype=torch.float16, device=srcs[0].device)
    a = _lib.PatchPackArgs()
    for i, s in enumerate(srcs):
        a.src[i], a.channels[i] = s.data_ptr(), s.shape[1]
    a.nsrc, a.y, a.batch, a.h, a.w, a.c_pad = len(srcs), y.data_ptr(), B, H, W, c_pad
    a.kh, a.kw, a.sy, a.sx, a.p0, a.np = kh, kw, sy, sx, p0, np
    check(lib().sdk_patch_pack(C.byref(a), _stream()), "patch_pack")
    return y


def _t_runs(t, batch):
    """``t`` (an int, or one int per sample) → [(first sample, end sample, t)] runs of equal t."""
    ts = [int(t)] * batch if not isinstance(t, (list, tuple)) else [int(v) for v in t]
    if len(ts) != batch:
        raise ValueError(f"sd_amd: {len(ts)} timesteps for a batch of {batch}")
    runs, b0 = [], 0
    for b in range(1, batch + 1):
        if b == batch or ts[b] != ts[b0]:
            runs.append((b0, b, ts[b0]))
            b0 = b
    return runs


def posterior_step(x, model_out, t, tables: dict, noise=None, *, x0_param=False, clip=False, temperature=1.0,
                   stage=0, x_recon_in=None, x_prev=None, x_recon=None, want_x_recon=False, keep=None, drop_p=0.0):
    """Fused ancestral step of ``LatentDiffusion.p_sample`` (see ``sdk_posterior_step``).  ``t``: a host
    int or one per sample (a launch per run of equal t); ``tables``: host fp32 arrays
    ``c_recip, c_recipm1, coef1, coef2, sigma`` indexed by t.  ``stage`` 0: x_prev (and x_recon when
    ``want_x_recon``); 1: x_recon only; 2: x_prev from ``x_recon_in``.  ``keep`` / ``drop_p``: noise dropout
    as in ``ddim_step`` (applied to noise·temperature).  Returns (x_prev, x_recon)."""
    ref = x if x is not None else model_out
    B = ref.shape[0]
    ins = {"x": x, "model_out": model_out, "noise": noise, "x_recon_in": x_recon_in}
    for k, v in ins.items():
        if v is not None:
            _need_cuda(v, "posterior_step " + k, torch.float32)
            if v.shape != ref.shape:
                raise ValueError(f"sd_amd.posterior_step: {k} {tuple(v.shape)} vs {tuple(ref.shape)}")
            ins[k] = v.contiguous()
    if stage != 1 and x_prev is None:
        x_prev = torch.empty_like(ref, memory_format=torch.contiguous_format)
    if (stage == 1 or want_x_recon) and x_recon is None:
        x_recon = torch.empty_like(ref, memory_format=torch.contiguous_format)
    keep, scale = _drop_scale("posterior_step", keep, drop_p, ref, ins["noise"])
    if keep is not None and stage == 1:
        raise ValueError("sd_amd.posterior_step: keep needs a stage that writes x_prev")
    per = ref.numel() // B
    ex = _lib.PosteriorExArgs()
    ex.drop_scale = scale
    a = ex.step
    a.stage, a.x0_param, a.clip, a.temperature = int(stage), int(bool(x0_param)), int(bool(clip)), float(temperature)
    for b0, b1, ti in _t_runs(t, B):
        off = b0 * per * 4
        for k, v in ins.items():
            setattr(a, k, v.data_ptr() + off if v is not None else None)
        a.x_prev = x_prev.data_ptr() + off if x_prev is not None and stage != 1 else None
        a.x_recon = x_recon.data_ptr() + off if x_recon is not None else None
        ex.keep = keep.data_ptr() + b0 * per if keep is not None else None
        a.n = (b1 - b0) * per
        a.c_recip, a.c_recipm1 = float(tables["c_recip"][ti]), float(tables["c_recipm1"][ti])
        a.coef1, a.coef2, a.sigma = float(tables["coef1"][ti]), float(tables["coef2"][ti]), float(tables["sigma"][ti])
        a.nonzero = 0.0 if ti == 0 or noise is None else 1.0      # no noise: x_prev is the posterior mean
        check(lib().sdk_posterior_step_ex(C.byref(ex), _stream()), "posterior_step")
    return x_prev, x_recon


def masked_q_sample(x0, noise, mask, img, t, sqrt_acp, sqrt_1m_acp, out=None):
    """``(sqrt_acp[t]·x0 + sqrt_1m_acp[t]·noise)·mask + (1 − mask)·img`` (``ldm/diffusion/ddpm.py:1783-1784``),
    the mask ``[B,1,H,W]``, ``[1,1,H,W]`` or ``[B,C,H,W]`` broadcast by index.  ``t`` as in
    ``posterior_step``; the tables are host fp32 arrays.  ``out=img`` updates in place."""
    for k, v in (("x0", x0), ("noise", noise), ("mask", mask), ("img", img)):
        _need_cuda(v, "masked_q_sample " + k, torch.float32)
    if x0.dim() != 4 or noise.shape != x0.shape or img.shape != x0.shape:
        raise ValueError("sd_amd.masked_q_sample: x0, noise and img must be one NCHW shape")
    B, Cc, H, W = x0.shape
    mode = _mask_mode("masked_q_sample", mask, x0.shape)
    x0, noise, mask = x0.contiguous(), noise.contiguous(), mask.contiguous()
    if not img.is_contiguous():
        if out is img:
            raise ValueError("sd_amd.masked_q_sample: in-place update needs a contiguous img")
        img = img.contiguous()
    y = out if out is not None else torch.empty_like(img)
    if y.shape != img.shape or not y.is_contiguous() or y.dtype != torch.float32:
        raise ValueError("sd_amd.masked_q_sample: out must be a contiguous fp32 tensor of img's shape")
    per, hw = Cc * H * W, H * W
    a = _lib.MaskedQArgs()
    a.per_sample, a.hw, a.mask_mode = per, hw, mode
    for b0, b1, ti in _t_runs(t, B):
        off = b0 * per * 4
        a.x0, a.noise, a.img, a.out = x0.data_ptr() + off, noise.data_ptr() + off, img.data_ptr() + off, y.data_ptr() + off
        a.mask = mask.data_ptr() + (0 if mode == 1 else b0 * (hw if mode == 0 else per) * 4)
        a.n = (b1 - b0) * per
        a.sqrt_acp, a.sqrt_1m_acp = float(sqrt_acp[ti]), float(sqrt_1m_acp[ti])
        check(lib().sdk_masked_q_sample(C.byref(a), _stream()), "masked_q_sample")
    return y


# --------------------------------------------------------------------------- vector quantiser

def _vq_codebook(codebook, what):
    _need_cuda(codebook, what + " codebook", torch.float32)
    if codebook.dim() != 2 or not codebook.is_contiguous():
        raise ValueError(f"sd_amd.{what}: codebook must be a contiguous [n_e, e_dim] tensor")
    return codebook.shape


def vq_code_norms(codebook: torch.Tensor):
    """‖e_j‖² per code, fp32 [n_e] — computed once per codebook and passed to ``vq_nearest``."""
    N, D = _vq_codebook(codebook, "vq_code_norms")
    norms = torch.empty(N, dtype=torch.float32, device=codebook.device)
    check(lib().sdk_vq_code_norms(_ptr(codebook), _ptr(norms), N, D, _stream()), "vq_code_norms")
    return norms


def vq_nearest(z: torch.Tensor, codebook: torch.Tensor, norms: torch.Tensor = None, splits: int = 0):
    """Nearest code per pixel of NCHW fp32 ``z`` [B, e_dim, H, W] → (z_q NCHW fp32, idx int64 [B·H·W]).
    One fused search (no [M, n_e] distance matrix); lowest index wins ties; z_q = z + (e − z).
    ``splits`` > 0 forces the number of codebook splits (tests), 0 lets the library choose."""
    _need_cuda(z, "vq_nearest", torch.float32)
    N, D = _vq_codebook(codebook, "vq_nearest")
    if z.dim() != 4 or z.shape[1] != D:
        raise ValueError(f"sd_amd.vq_nearest: z {tuple(z.shape)} does not match e_dim {D} (expected [B, {D}, H, W])")
    if not 1 <= D <= 256:
        raise ValueError(f"sd_amd.vq_nearest: e_dim {D} outside [1, 256]")
    if z.numel() == 0:
        raise ValueError("sd_amd.vq_nearest: empty input")
    if norms is None:
        norms = vq_code_norms(codebook)
    _need_cuda(norms, "vq_nearest norms", torch.float32)
    if norms.shape != (N,):
        raise ValueError(f"sd_amd.vq_nearest: norms {tuple(norms.shape)} vs n_e {N}")
    z = z.contiguous()
    B, _, H, W = z.shape
    M = B * H * W
    zq = torch.empty_like(z)
    idx = torch.empty(M, dtype=torch.int64, device=z.device)
    keys = None
    if splits > 1 or (splits <= 0 and lib().sdk_vq_nearest_splits(M, N, D) > 1):
        keys = torch.empty(M, dtype=torch.int64, device=z.device)
    check(lib().sdk_vq_nearest(_ptr(z), _ptr(codebook), _ptr(norms.contiguous()), _ptr(idx), _ptr(zq), B, D, H * W, N,
                               _ptr(keys), M * 8 if keys is not None else 0, int(splits), _stream()), "vq_nearest")
    return zq, idx


def vq_lookup(idx: torch.Tensor, codebook: torch.Tensor, nchw_shape=None):
    """codebook[idx]: int64 indices (any shape, M entries) → fp32 [M, e_dim], or NCHW
    [B, e_dim, H, W] when ``nchw_shape`` = (B, H, W) is given.  Indices must already be inside
    [0, n_e) (``VectorQuantize2.get_codebook_entry`` checks them on the host)."""
    _need_cuda(idx, "vq_lookup", torch.int64)
    N, D = _vq_codebook(codebook, "vq_lookup")
    idx = idx.contiguous().view(-1)
    M = idx.numel()
    if M == 0:
        raise ValueError("sd_amd.vq_lookup: no indices")
    if nchw_shape is not None:
        B, H, W = (int(v) for v in nchw_shape)
        if B * H * W != M:
            raise ValueError(f"sd_amd.vq_lookup: {M} indices do not fill {(B, H, W)}")
        out = torch.empty(B, D, H, W, dtype=torch.float32, device=idx.device)
        hw, nchw = H * W, 1
    else:
        out = torch.empty(M, D, dtype=torch.float32, device=idx.device)
        hw, nchw = 1, 0
    check(lib().sdk_vq_lookup(_ptr(idx), _ptr(codebook), _ptr(out), M, N, D, hw, nchw, _stream()), "vq_lookup")
    return out


def vq_remap(inds: torch.Tensor, used: torch.Tensor, *, to_used: bool, unknown: int = 0, random=None,
             extra: bool = False):
    """Index remap on the device.  ``to_used=True``: position of the first match in ``used`` else
    ``random[i]`` (a pre-drawn int64 tensor) or ``unknown``; ``to_used=False`` (unmap_to_all):
    ``used[inds]``, with ``extra`` an index ≥ len(used) becomes 0 first.  Shape is kept."""
    _need_cuda(inds, "vq_remap", torch.int64)
    _need_cuda(used, "vq_remap used", torch.int64)
    if inds.numel() == 0 or used.dim() != 1 or used.numel() == 0:
        raise ValueError("sd_amd.vq_remap: empty indices or used table")
    src = inds.contiguous()
    if random is not None:
        _need_cuda(random, "vq_remap random", torch.int64)
        if random.numel() != src.numel():
            raise ValueError("sd_amd.vq_remap: random must have one entry per index")
        random = random.contiguous()
    out = torch.empty_like(src)
    check(lib().sdk_vq_remap(_ptr(src), _ptr(used.contiguous()), _ptr(random), _ptr(out), src.numel(), used.numel(),
                             0 if to_used else 1, int(unknown), 1 if extra else 0, _stream()), "vq_remap")
    return out


def diag_gaussian_sample(moments: torch.Tensor, noise=None, scale: float = 1.0, out=None):
    """moments NCHW fp32 [B, 2C, H, W] -> scale * (mean + std * noise) (or scale * mean) [B, C, H, W]."""
    _need_cuda(moments, "diag_gaussian_sample", torch.float32)
    B, C2, H, W = moments.shape
    moments = moments.contiguous()
    if noise is not None:
        _need_cuda(noise, "diag_gaussian_sample noise", torch.float32)
        noise = noise.contiguous()
    z = out if out is not None else torch.empty(B, C2 // 2, H, W, dtype=torch.float32, device=moments.device)
    check(lib().sdk_diag_gaussian_sample(_ptr(moments), _ptr(noise), _ptr(z), B, C2 // 2, H * W, float(scale),
                                         _stream()), "diag_gaussian_sample")
    return z


def stochastic_encode(x0: torch.Tensor, noise: torch.Tensor, sqrt_a: float, sqrt_1ma: float, out=None):
    """sqrt_a * x0 + sqrt_1ma * noise, fp32, bit-identical to the reference's CPU expression."""
    _need_cuda(x0, "stochastic_encode", torch.float32)
    _need_cuda(noise, "stochastic_encode noise", torch.float32)
    x0, noise = x0.contiguous(), noise.contiguous()
    y = out if out is not None else torch.empty_like(x0)
    check(lib().sdk_stochastic_encode(_ptr(x0), _ptr(noise), _ptr(y), x0.numel(), float(sqrt_a), float(sqrt_1ma),
                                      _stream()), "stochastic_encode")
    return y


def ddpm_step(x, eps, noise, inv_sqrt_alpha, coef, sigma, out=None):
    _need_cuda(x, "ddpm_step", torch.float32)
    y = out if out is not None else torch.empty_like(x)
    check(lib().sdk_ddpm_step(_ptr(x), _ptr(eps), _ptr(noise), _ptr(y), x.numel(), C.c_float(inv_sqrt_alpha),
                              C.c_float(coef), C.c_float(sigma), _stream()), "ddpm_step")
    return y


# --------------------------------------------------------------------------- profiling hooks

class _Profiler:
    """Optional per-launch HIP-event timing on the launch stream (bench roofline leg)."""

    def __init__(self):
        self.active = False
        self.records = []
        self.regions = []      # per record: the module region it ran in (None outside any)
        self.region = None     # set by modules around their launches (e.g. "cross_attention")
        self._cur = None

    def start(self):
        self.records = []
        self.regions = []
        self.active = True

    def stop(self):
        self.active = False

    def begin(self, kind, info, shape=None, nbytes=0):
        s = torch.cuda.current_stream()
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record(s)
        flops = info.flops if isinstance(info, ConvPlanInfo) else None
        if kind == "attention" and info is not None:
            b, h, nq, nk, d = info
            flops = 4.0 * b * h * nq * nk * d
            shape = info
        variant = info.variant if isinstance(info, ConvPlanInfo) else None
        self._cur = (kind, variant, flops, e0, shape, nbytes)

    def end(self):
        s = torch.cuda.current_stream()
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record(s)
        kind, variant, flops, e0, shape, nbytes = self._cur
        self.records.append((kind, variant, flops, e0, e1, shape, nbytes))
        self.regions.append(self.region)

    def region_summary(self, region):
        """Totals over the launches of one module region: launches, ms, flops, and per kind."""
        torch.cuda.synchronize()
        tot = {"launches": 0, "ms": 0.0, "flops": 0.0, "by_kind": {}}
        for rec, reg in zip(self.records, self.regions):
            if reg != region:
                continue
            kind, _, flops, e0, e1, _, _ = rec
            ms = e0.elapsed_time(e1)
            k = tot["by_kind"].setdefault(kind, {"launches": 0, "ms": 0.0, "flops": 0.0})
            for d in (tot, k):
                d["launches"] += 1
                d["ms"] += ms
                d["flops"] += flops or 0.0
        return tot

    def shape_table(self):
        """Per (kind, shape) totals: launches, ms, TFLOP/s — where the time goes."""
        torch.cuda.synchronize()
        out = {}
        for kind, variant, flops, e0, e1, shape, _ in self.records:
            d = out.setdefault((kind, shape), [0, 0.0, 0.0])
            d[0] += 1
            d[1] += e0.elapsed_time(e1)
            d[2] += flops or 0.0
        rows = [(k, v[0], v[1], (v[2] / (v[1] * 1e-3) / 1e12) if v[1] > 0 and v[2] else 0.0) for k, v in out.items()]
        return sorted(rows, key=lambda r: -r[2])

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for kind, variant, flops, e0, e1, shape, nbytes in self.records:
            key = kind if variant is None else f"{kind}:{variant}"
            d = out.setdefault(key, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            d["launches"] += 1
            d["bytes"] += nbytes
            d["ms"] += e0.elapsed_time(e1)
            d["flops"] += flops or 0.0
        return out


PROFILER = _Profiler()
