"""Host side of the patch-wise UNet / tiled encode (``split_input_params``): the patch geometry, the errors raised
before any model call, ``sdk_patch_pack``'s argument checks (they precede the launch, so no device is needed) and
the weighting / normalisation tables the reference wrote (tests/golden/make_golden_patch.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import patch_util as pu
from golden_util import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ geometry
@pytest.mark.parametrize("args,want", pu.GRID_CASES,
                         ids=["{}x{}_k{}x{}_s{}x{}".format(a[0], a[1], *a[2], *a[3]) for a, _ in pu.GRID_CASES])
def test_patch_grid(sdk, args, want):
    from sd_amd import ops
    assert ops.patch_grid(*args) == want
    ks, stride, Ly, Lx = want
    unfold = torch.nn.Unfold(kernel_size=ks, stride=stride)
    assert unfold(torch.zeros(1, 1, args[0], args[1])).shape[-1] == Ly * Lx        # L as torch.nn.Unfold counts it


def test_patch_grid_rejects_non_positive(sdk):
    from sd_amd import ops
    for bad in ((0, 8, (4, 4), (2, 2)), (8, 8, (0, 4), (2, 2)), (8, 8, (4, 4), (2, 0))):
        with pytest.raises(ValueError):
            ops.patch_grid(*bad)


# ------------------------------------------------------------------ errors before any model call
class _NeverCalled(torch.nn.Module):
    conditioning_key = "crossattn"

    def forward(self, *a, **kw):
        raise AssertionError("the model was called")

    encode = forward


def _ld(sdk, sp, cond_stage_key="txt"):
    from sd_amd.Diffusion.ddpm import LatentDiffusion

    class LD(LatentDiffusion):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.model = self.first_stage_model = _NeverCalled()
            self.cond_stage_key = cond_stage_key
            self.split_input_params = sp

    return LD()


def test_apply_model_refusals(sdk):
    x, t, c = torch.zeros(2, 4, 12, 12), torch.zeros(2, dtype=torch.long), torch.zeros(2, 7, 48)
    with pytest.raises(ValueError, match="return_ids"):
        _ld(sdk, pu.split_params(pu.KS, pu.STRIDE)).apply_model(x, t, c, return_ids=True)
    with pytest.raises(NotImplementedError, match="coordinates_bbox"):
        _ld(sdk, pu.split_params(pu.KS, pu.STRIDE), "coordinates_bbox").apply_model(x, t, c)
    # ragged coverage names the geometry: 12 - 8 is no multiple of 3, and 13 rows leave row 12 uncovered
    with pytest.raises(ValueError, match=r"ks \(8, 8\).*stride \(3, 4\).*12x12"):
        _ld(sdk, pu.split_params(pu.KS, (3, 4))).apply_model(x, t, c)
    with pytest.raises(ValueError, match=r"13x12"):
        _ld(sdk, pu.split_params(pu.KS, pu.STRIDE)).apply_model(torch.zeros(2, 4, 13, 12), t, c)
    # ... also where the clipped grid is a single patch that does not reach the border
    with pytest.raises(ValueError, match=r"stride \(8, 8\)"):
        _ld(sdk, pu.split_params(pu.KS, (8, 8))).apply_model(x, t, c)
    # ... and where the patches reach the border but leave gaps between them (stride > ks)
    with pytest.raises(ValueError, match=r"ks \(2, 8\).*stride \(5, 4\)"):
        _ld(sdk, pu.split_params((2, 8), (5, 4))).apply_model(x, t, c)
    # patch_unet = False and a single covering patch go to the model (which these stand-ins refuse to be)
    for sp in (pu.split_params(pu.KS, pu.STRIDE, patch_unet=False), pu.split_params((16, 16), (4, 4))):
        with pytest.raises(AssertionError, match="the model was called"):
            _ld(sdk, sp).apply_model(x, t, c)


def test_encode_first_stage_refusals(sdk):
    x = torch.zeros(2, 3, 24, 24)
    enc = dict(patch_distributed_vq=True, vqf=pu.ENC_VQF)
    with pytest.raises(ValueError, match="divisible by vqf = 2"):
        _ld(sdk, pu.split_params((15, 16), pu.ENC_STRIDE, **enc)).encode_first_stage(x)
    with pytest.raises(ValueError, match="divisible by vqf = 2"):
        _ld(sdk, pu.split_params(pu.ENC_KS, (8, 1), **enc)).encode_first_stage(x)
    sp = pu.split_params(pu.ENC_KS, (6, 8), **enc)
    with pytest.raises(ValueError, match=r"ks \(16, 16\).*stride \(6, 8\).*24x24"):
        _ld(sdk, sp).encode_first_stage(x)
    assert tuple(sp["original_image_size"]) == (24, 24)          # recorded before the checks, as the reference does
    # not patch_distributed_vq: the untiled encode
    with pytest.raises(AssertionError, match="the model was called"):
        _ld(sdk, pu.split_params(pu.ENC_KS, pu.ENC_STRIDE, patch_distributed_vq=False, vqf=2)).encode_first_stage(x)


# ------------------------------------------------------------------ sdk_patch_pack argument checks (C ABI)
def _pack_args(_lib, **over):
    """A valid call's arguments (B = 2, 12x20, 8x8 every 4: 16 patches) with pointers that are never read: every
    variation below is rejected before the launch."""
    buf = (C.c_float * 4)()
    a = _lib.PatchPackArgs()
    a.src[0], a.channels[0], a.nsrc, a.y = C.addressof(buf), 4, 1, C.addressof(buf)
    a.batch, a.h, a.w, a.c_pad, a.kh, a.kw, a.sy, a.sx, a.p0, a.np = 2, 12, 20, 8, 8, 8, 4, 4, 0, 16
    for k, v in over.items():
        setattr(a, k, v)
    return a


BAD_PACK = [dict(nsrc=0), dict(nsrc=5), dict(y=None), dict(kh=13), dict(kw=21), dict(kh=0), dict(sy=0), dict(sx=-4),
            dict(c_pad=3), dict(p0=-1), dict(np=0), dict(p0=1, np=16), dict(p0=16, np=1), dict(batch=0), dict(h=0)]


@pytest.mark.parametrize("over", BAD_PACK, ids=lambda o: "_".join(f"{k}{v}" for k, v in o.items()))
def test_patch_pack_rejects(sdk, over):
    from sd_amd import _lib
    L = _lib.lib()
    assert L.sdk_patch_pack(C.byref(_pack_args(_lib, **over)), None) == -1          # SDK_EINVAL
    assert b"patch_pack" in L.sdk_last_error()


def test_patch_pack_rejects_null_source_and_struct(sdk):
    from sd_amd import _lib
    L = _lib.lib()
    a = _pack_args(_lib, nsrc=2)                 # the second source is NULL with 0 channels
    assert L.sdk_patch_pack(C.byref(a), None) == -1
    a.src[1] = a.src[0]
    assert L.sdk_patch_pack(C.byref(a), None) == -1          # channels[1] = 0
    assert L.sdk_patch_pack(None, None) == -1


def test_patch_pack_in_header_binding_and_integration_table(sdk):
    from sd_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "sdk_amd.h")).read()
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"\bint sdk_patch_pack\(", header) and "sdk_patch_pack" in _lib.EXPORTS
    assert hasattr(_lib.lib(), "sdk_patch_pack")
    assert re.search(r"^\| `sdk_patch_pack` \|", table, re.M)
    assert callable(ops.patch_pack) and callable(ops.patch_grid)
    # the struct the binding declares is the header's: same field order
    body = re.search(r"typedef struct \{([^}]*)\} sdk_patch_pack_args;", header).group(1)
    names = re.findall(r"(\w+)(?:\[4\])?\s*[,;]", body)
    assert names == [f[0] for f in _lib.PatchPackArgs._fields_]


def test_graph_key_holds_the_patch_window(sdk):
    from sd_amd.graphs import GraphedUNet
    x, t = torch.zeros(2, 4, 12, 12), torch.zeros(5, dtype=torch.long)
    k0 = GraphedUNet._key(x, t, None)
    k1 = GraphedUNet._key(x, t, None, (), None, (8, 8, 4, 4, 0, 5))
    k2 = GraphedUNet._key(x, t, None, (), None, (8, 8, 4, 4, 3, 5))
    assert len({k0, k1, k2}) == 3 and k1 == GraphedUNet._key(x, t, None, (), None, (8, 8, 4, 4, 0, 5))


# ------------------------------------------------------------------ the reference's tables
@pytest.mark.parametrize("tie", [True, False], ids=["tie", "notie"])
@pytest.mark.parametrize("tag", sorted(pu.TABLE_CASES))
def test_weighting_and_normalisation_vs_reference(sdk, tag, tie):
    """``get_weighting`` (pixel (x) patch weights, kept separable) and a NumPy overlap-add against the weighting and
    the ``fold(weighting)`` normalisation that the reference's ``get_fold_unfold`` wrote, bit for bit, for
    uf = df = 1 (apply_model) and df = 2 (encode)."""
    from sd_amd import ops
    from sd_amd.Diffusion.ddpm import LatentDiffusion
    fx = load("patch_tables")
    h, w, ks, stride, df = pu.TABLE_CASES[tag]
    sp = pu.split_params(ks, stride, tie)
    ks2, stride2, Ly, Lx = ops.patch_grid(h, w, ks, stride)
    assert (ks2, stride2) == (tuple(ks), tuple(stride))
    kh, kw = ks[0] // df, ks[1] // df
    pix, lw = LatentDiffusion.get_weighting(_ld(sdk, sp), kh, kw, Ly, Lx, sp)
    assert (lw is not None) == tie and pix.dtype == np.float32
    full = pix[:, :, None] * (lw[None, None, :] if tie else np.ones(Ly * Lx, dtype=np.float32))
    ref_w, ref_n = fx[f"{tag}_tie{int(tie)}_weighting"], fx[f"{tag}_tie{int(tie)}_norm"]
    assert full.shape == ref_w.shape and np.array_equal(full, ref_w)
    norm = pu.overlap_add(pix, lw, h // df, w // df, (stride[0] // df, stride[1] // df), Ly, Lx)
    # both are fp32 sums of the same n <= 4 positive terms (the bit-equal weights of the covering patches) in an
    # order of their own: each is within (n - 1) * 2^-24 of the exact sum, relative, so they differ by <= 6 * 2^-24
    assert (ref_n > 0).all()
    n_cover = -(-ks[0] // stride[0]) * -(-ks[1] // stride[1])
    assert n_cover <= 4
    err = np.abs(norm.astype(np.float64) - ref_n) / ref_n
    print(f"[tables] {tag} tie={tie}: normalisation max rel diff {err.max() / 2.0 ** -24:.2f} x 2^-24")
    assert err.max() <= 2 * (n_cover - 1) * 2.0 ** -24
