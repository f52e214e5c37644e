"""``sdk_patch_pack`` on the GPU, exact (run with -m gpu): the UNet input of a window of patches gathered from
the full-size sources must be bit-equal to ``concat_nchw_to_nhwc`` of ``torch.nn.Unfold`` computed on the CPU.

Source values are integers in [-2048, 2048] (exact in fp16), every source is a view into a NaN-filled buffer (a
read outside it shows as NaN) and the output is a view into a sentinel-filled buffer whose head and tail must stay
intact.  Shapes are the smallest at which each index can go wrong: Ly != Lx, kh != kw with sy != sx, a patch equal to
the image, B = 1, channel sums of 4 / 5 / 7 / 8 over one to four sources, windows that start inside an image's
patches and a ragged last one."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SENTINEL = 12344.0            # exact in fp16, outside the sources' range
GUARD = 64                    # elements before and after a view (keeps a 16-byte aligned view aligned)

# (B, H, W, (kh, kw), (sy, sx))
GEOMS = [(2, 12, 20, (8, 8), (4, 4)),        # Ly = 2, Lx = 4
         (2, 12, 20, (8, 4), (4, 8)),        # kh != kw, sy != sx: Ly = 2, Lx = 3
         (2, 12, 20, (12, 20), (4, 4)),      # the patch is the image
         (1, 12, 20, (8, 8), (4, 4))]        # B = 1
CHANNELS = [(4,), (4, 3, 1), (4, 1), (3, 1, 1, 2)]          # sums 4, 8 (full groups only), 5, 7


def _ints(seed, *shape):
    return np.random.Generator(np.random.PCG64(seed)).integers(-2048, 2049, size=shape).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(geom, chans):
    """(CPU sources, reference [L*B, kh, kw, csum] fp16): Unfold of every source in patch order p = l*B + b,
    concatenated along channels, channels last."""
    B, H, W, (kh, kw), (sy, sx) = geom
    srcs = [torch.from_numpy(_ints(9300 + 17 * i + sum(chans) + kh + sx, B, c, H, W)) for i, c in enumerate(chans)]
    unfold = torch.nn.Unfold(kernel_size=(kh, kw), stride=(sy, sx))
    pats = []
    for s in srcs:
        u = unfold(s)                                                   # [B, C*kh*kw, L]
        u = u.view(B, s.shape[1], kh, kw, u.shape[-1]).permute(4, 0, 1, 2, 3)
        pats.append(u.reshape(-1, s.shape[1], kh, kw))                  # [L*B, C, kh, kw]
    ref = torch.cat(pats, 1).permute(0, 2, 3, 1).contiguous().half()
    assert torch.equal(ref.float(), torch.cat(pats, 1).permute(0, 2, 3, 1))         # the values are fp16-exact
    return srcs, ref


def _guarded(t, fill, guard=GUARD):
    """A contiguous device copy of ``t`` that is a view into a ``fill``-ed buffer, and the buffer."""
    buf = torch.full((t.numel() + 2 * guard,), fill, dtype=t.dtype, device=DEV)
    view = buf[guard:guard + t.numel()].view(t.shape)
    view.copy_(t)
    return view, buf


def _windows(total):
    last = (total - 1) // 5 * 5
    return sorted({(0, total), (3, 5) if total >= 8 else (total - 1, 1), (last, total - last)})


def _pack_into(sdk, srcs, y, geom, c_pad, p0, n):
    from sd_amd import _lib
    B, H, W, (kh, kw), (sy, sx) = geom
    a = _lib.PatchPackArgs()
    for i, s in enumerate(srcs):
        a.src[i], a.channels[i] = s.data_ptr(), s.shape[1]
    a.nsrc, a.y, a.batch, a.h, a.w, a.c_pad = len(srcs), y.data_ptr(), B, H, W, c_pad
    a.kh, a.kw, a.sy, a.sx, a.p0, a.np = kh, kw, sy, sx, p0, n
    _lib.check(_lib.lib().sdk_patch_pack(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "patch_pack")


def _want(ref, c_pad, p0, n):
    out = torch.zeros(n, ref.shape[1], ref.shape[2], c_pad, dtype=torch.float16)
    out[..., :ref.shape[3]] = ref[p0:p0 + n]
    return out


@pytest.mark.parametrize("chans", CHANNELS, ids=lambda c: "c" + "+".join(map(str, c)))
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "b{}_{}x{}_k{}x{}_s{}x{}".format(g[0], g[1], g[2], *g[3], *g[4]))
def test_patch_pack_equals_unfold_concat(sdk, geom, chans):
    from sd_amd import ops
    cpu_srcs, ref = _case(geom, chans)
    B, H, W, (kh, kw), (sy, sx) = geom
    total, csum = ref.shape[0], sum(chans)
    srcs = [_guarded(s, float("nan"))[0] for s in cpu_srcs]
    # c_pad: the next multiple of 8, 16, and the channel sum itself (no multiple of 8: every store is scalar);
    # guard 3 puts the output at a 6-byte offset, so the 16-byte stores are not taken either
    for c_pad, guard in [((csum + 7) // 8 * 8, GUARD), (16, GUARD), (csum, GUARD), ((csum + 7) // 8 * 8, 3)]:
        for p0, n in _windows(total):
            y, buf = _guarded(torch.empty(n, kh, kw, c_pad, dtype=torch.float16), SENTINEL, guard)
            y.fill_(SENTINEL)
            _pack_into(sdk, srcs, y, geom, c_pad, p0, n)
            want = _want(ref, c_pad, p0, n)
            what = f"c_pad {c_pad} guard {guard} window [{p0}, {p0 + n})"
            assert torch.equal(y.cpu().view(torch.int16), want.view(torch.int16)), what
            assert bool((buf[:guard] == SENTINEL).all()) and bool((buf[guard + y.numel():] == SENTINEL).all()), what
    # the public wrapper: its own output, np=None runs to the last patch
    c_pad = (csum + 7) // 8 * 8
    y = ops.patch_pack(srcs, c_pad, kh, kw, sy, sx)
    assert y.dtype == torch.float16 and tuple(y.shape) == (total, kh, kw, c_pad) and y.is_contiguous()
    assert torch.equal(y.cpu().view(torch.int16), _want(ref, c_pad, 0, total).view(torch.int16))
    p0 = total // 2
    y = ops.patch_pack(srcs, c_pad, kh, kw, sy, sx, p0=p0)
    assert torch.equal(y.cpu().view(torch.int16), _want(ref, c_pad, p0, total - p0).view(torch.int16))


def test_patch_pack_equals_the_composition_it_replaces(sdk):
    """``concat_nchw_to_nhwc`` of ``extract_patches`` of every source, on the device, on real-valued sources (the
    fp32 -> fp16 rounding is the same conversion)."""
    from sd_amd import ops
    import vq_util as vu
    B, H, W, (kh, kw), (sy, sx) = GEOMS[0]
    srcs = [torch.from_numpy(vu.randn(9400 + c, B, c, H, W) * np.float32(3.0)).to(DEV) for c in (4, 1, 4)]
    comp = ops.concat_nchw_to_nhwc([ops.extract_patches(s, kh, kw, sy, sx).view(-1, s.shape[1], kh, kw)
                                    for s in srcs], 16)
    assert torch.equal(ops.patch_pack(srcs, 16, kh, kw, sy, sx).view(torch.int16), comp.view(torch.int16))
    assert torch.equal(ops.patch_pack(srcs, 16, kh, kw, sy, sx, 5, 7).view(torch.int16), comp[5:12].view(torch.int16))


def test_patch_pack_wrapper_rejects(sdk):
    from sd_amd import ops
    x = torch.zeros(2, 4, 12, 20, device=DEV)
    for bad in (dict(srcs=[x] * 5, c_pad=24), dict(srcs=[x, torch.zeros(2, 1, 12, 12, device=DEV)]),
                dict(c_pad=3), dict(kh=13), dict(sx=0), dict(p0=-1), dict(p0=10, np=7), dict(np=0)):
        kw = dict(srcs=[x], c_pad=8, kh=8, kw=8, sy=4, sx=4, p0=0, np=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.patch_pack(**kw)
    with pytest.raises(TypeError):
        ops.patch_pack([x.cpu()], 8, 8, 8, 4, 4)
