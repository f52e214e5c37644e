"""Record what the conv host planner decides: sdk_conv2d_plan over every variant id, split-K request and
GroupNorm-statistics request for a set of tiny conv / GEMM descriptions, and sdk_kernel_name for ids -1..48.

Run from the repo root:  python tests/golden/make_golden_conv_plans.py
Needs only the built product library (no GPU, no reference checkout: the planner never dereferences a
pointer, so every pointer is a dummy).  SD_AMD_LIB selects another build of the same ABI.

conv_plans.npz was recorded from the library as it stood before the planner, the part launchers and the
kernel names were derived from one variant table; tests/test_boundary.py replays it against the built
library and requires every row to be equal (error message text is not compared).  ``sweep`` and ``CASES``
are what the test imports, so the recorded rows and the replayed rows come from the same descriptions.

Per row: case, variant_hint (0..44), split request (index into SPLITS), gn_partial (0 / 1), the return code
and, on success, variant, split_k, grid_tiles, workspace_bytes, gn_chunks and flops (zeros otherwise).
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(HERE, "conv_plans.npz")

OUT_NHWC_F16, OUT_NCHW_F32, OUT_GEGLU_F16, OUT_ROWS_F32 = 0, 1, 2, 3
HINTS = tuple(range(0, 45))
# (split_k, split_inlaunch): planner's choice, 1..4, and the in-launch request
SPLITS = ((0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (2, 1))
NAME_IDS = tuple(range(-1, 49))
SRC0, SRC1, SRC2, SRC3, WEIGHT, OUTP, RES, WORK, GNP, TCNT, GNS, GNB = (0x1000 * k for k in range(1, 13))

# the product kernel ids, the diagnostic ablations and the ids that never existed or were withdrawn
PRODUCT_IDS = {0, 2, 3, 4, 6, 7, 8, 9, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 31, 32, 33, 34, 35, 38, 40}
DIAGNOSTIC_IDS = {10, 11, 12, 13, 14, 15, 27, 28, 29, 30}
UNKNOWN_IDS = {1, 36, 37, 39, 41, 42, 43}


def _seg(s, h, w, cin, ksize=1, stride=1, pad=0, pad_end=0, c_split=None, src=(SRC0, SRC1)):
    c_split = cin if c_split is None else c_split
    s.src0 = src[0]
    s.c_split, s.cin, s.ld0 = c_split, cin, c_split
    if c_split < cin:
        s.src1, s.ld1 = src[1], cin - c_split
    s.h, s.w, s.ksize, s.stride, s.pad, s.pad_end = h, w, ksize, stride, pad, pad_end
    return ksize * ksize * ((cin + 63) // 64 * 64)          # packed K of the segment


def _conv(_lib, batch, h, w, cin, cout, ksize=3, stride=1, pad=1, pad_end=0, c_split=None, out_mode=OUT_NHWC_F16):
    a = _lib.ConvArgs()
    ho = (h + 2 * pad + pad_end - ksize) // stride + 1
    wo = (w + 2 * pad + pad_end - ksize) // stride + 1
    a.batch, a.ho, a.wo, a.cout, a.nseg = batch, ho, wo, cout, 1
    a.k_total = _seg(a.seg[0], h, w, cin, ksize, stride, pad, pad_end, c_split)
    a.weight, a.out, a.workspace, a.workspace_bytes = WEIGHT, OUTP, WORK, 1 << 40
    a.out_mode = out_mode
    a.out_ld = cout // 2 if out_mode == OUT_GEGLU_F16 else cout
    return a


def _gemm(_lib, m, n, k, **kw):
    return _conv(_lib, 1, m, 1, k, n, ksize=1, pad=0, **kw)


def _residual(a):
    a.residual, a.res_ld = RES, a.cout
    return a


def _shortcut(_lib, concat):
    """3x3 plus a plain 1x1 shortcut segment over the output grid."""
    a = _conv(_lib, 2, 16, 16, 128 if concat else 64, 128, c_split=64 if concat else None)
    a.nseg = 2
    a.k_total += _seg(a.seg[1], 16, 16, 64, src=(SRC2, SRC3))
    return a


def _prologue(_lib):
    a = _conv(_lib, 2, 16, 16, 64, 128)
    a.seg[0].gn_scale, a.seg[0].gn_shift, a.seg[0].silu = GNS, GNB, 1
    return a


def _act(_lib):
    a = _gemm(_lib, 600, 704, 1280)
    a.act = 1
    return a


def _per_image(_lib, rows):
    """Per-image weight matrices over ``rows`` rows per image."""
    a = _conv(_lib, 2, rows, 1, 192, 328, ksize=1, pad=0)
    a.weight_batch_stride = 384 * 192                       # cout padded to 128 rows x K
    return a


def _phase(_lib):
    """The phase form of nearest-x2 + 3x3: 2x2 taps over the zero-bordered 18x18 source, a 32x32 output."""
    a = _conv(_lib, 2, 18, 18, 64, 128, ksize=2, pad=0)
    a.ho = a.wo = 32
    a.upsample_phase = 1
    a.weight_batch_stride = 128 * a.k_total
    return a


CASES = {
    "conv3x3": lambda L: _conv(L, 2, 16, 16, 64, 128),
    "token_gemm": lambda L: _gemm(L, 600, 704, 1280),
    "large_grid": lambda L: _conv(L, 16, 64, 64, 320, 320),
    "shortcut_one_source": lambda L: _shortcut(L, False),
    "shortcut_concat": lambda L: _shortcut(L, True),
    "concat_40_32": lambda L: _conv(L, 2, 16, 16, 72, 128, c_split=40),
    "gn_silu_prologue": _prologue,
    "geglu": lambda L: _gemm(L, 600, 640, 320, out_mode=OUT_GEGLU_F16),
    "quick_gelu": _act,
    "direct": lambda L: _conv(L, 2, 16, 16, 64, 4, out_mode=OUT_NCHW_F32),
    "direct_residual": lambda L: _residual(_conv(L, 2, 16, 16, 64, 4, out_mode=OUT_NCHW_F32)),
    "gemm_m16": lambda L: _gemm(L, 16, 1280, 320),
    "gemm_m65": lambda L: _gemm(L, 65, 1280, 320),
    "rows_f32_cout12": lambda L: _gemm(L, 600, 12, 128, out_mode=OUT_ROWS_F32),
    "per_image_384": lambda L: _per_image(L, 384),      # 128-row tiles fit inside one image, 256-row tiles do not
    "per_image_200": lambda L: _per_image(L, 200),      # no tile fits
    "phase": _phase,
    "phase_residual": lambda L: _residual(_phase(L)),
    "stride2_pad_end": lambda L: _conv(L, 2, 17, 17, 64, 128, stride=2, pad=0, pad_end=1),
}
CASE_NAMES = tuple(CASES)


def sweep(L, _lib):
    """Every row of the sweep as a dict of arrays, in a fixed order."""
    info = _lib.ConvPlanInfo()
    rows = []
    for ci, name in enumerate(CASE_NAMES):
        for hint in HINTS:
            for si, (split, inl) in enumerate(SPLITS):
                for gn in (0, 1):
                    a = CASES[name](_lib)
                    a.variant_hint, a.split_k, a.split_inlaunch = hint, split, inl
                    a.tile_counters = TCNT if inl else None
                    a.gn_partial = GNP if gn else None
                    rc = L.sdk_conv2d_plan(C.byref(a), C.byref(info))
                    ok = rc == 0
                    rows.append((ci, hint, si, gn, rc, info.variant if ok else 0, info.split_k if ok else 0,
                                 info.grid_tiles if ok else 0, info.workspace_bytes if ok else 0,
                                 info.gn_chunks if ok else 0, info.flops if ok else 0.0))
    cols = list(zip(*rows))
    out = {k: np.asarray(cols[i], dtype=np.int32) for i, k in enumerate(
        ("case", "hint", "split_req", "gn_req", "rc", "variant", "split_k", "grid_tiles"))}
    out["workspace_bytes"] = np.asarray(cols[8], dtype=np.int64)
    out["gn_chunks"] = np.asarray(cols[9], dtype=np.int32)
    out["flops"] = np.asarray(cols[10], dtype=np.float64)
    L.sdk_kernel_name.restype = C.c_char_p
    out["kernel_names"] = np.asarray([L.sdk_kernel_name(v) for v in NAME_IDS])
    out["case_names"] = np.asarray([n.encode() for n in CASE_NAMES])
    return out


def check_coverage(g):
    """The sweep reaches every decision the planner makes about a variant id."""
    ok = g["rc"] == 0
    forced = g["hint"] - 1
    case = lambda *names: np.isin(g["case"], [CASE_NAMES.index(n) for n in names])   # noqa: E731
    assert set(g["variant"][ok].tolist()) == PRODUCT_IDS, sorted(set(g["variant"][ok].tolist()) ^ PRODUCT_IDS)
    tile_ids = sorted(PRODUCT_IDS - {0, 34, 35})
    assert (ok & np.isin(forced, tile_ids) & (g["variant"] == 0)).any(), "no forced tile id fell back to 0"
    assert (ok & (g["gn_chunks"] == 0)).any() and (ok & (g["gn_chunks"] > 0)).any()
    inl = g["split_req"] == len(SPLITS) - 1
    assert (inl & ok).any() and (inl & ~ok & ~case("phase", "phase_residual")).any(), "in-launch split"
    assert (case("phase") & ok).any() and (case("phase") & ~ok).any() and not (case("phase_residual") & ok).any()
    assert (case("per_image_384") & ok).any() and not (case("per_image_200") & ok).any()
    assert (ok & (forced == 5)).any() and set(g["variant"][ok & (forced == 5) & case("token_gemm")].tolist()) == {22}
    for ids in (UNKNOWN_IDS, DIAGNOSTIC_IDS):
        sel = np.isin(forced, sorted(ids))
        assert sel.any() and not (sel & ok).any(), ids
    names = dict(zip(NAME_IDS, g["kernel_names"].tolist()))
    assert {v for v, n in names.items() if n != b"unknown"} == PRODUCT_IDS | {5}


def main():
    import sd_amd_loader
    sdk = sd_amd_loader.load()
    from sd_amd import _lib
    assert "SDK_CONV_VARIANT" not in os.environ, "the environment override would be recorded as a forced id"
    g = sweep(sdk.library(), _lib)
    check_coverage(g)
    np.savez_compressed(OUT, **g)
    print("conv_plans", len(g["rc"]), "rows,", int((g["rc"] == 0).sum()), "planned,", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
