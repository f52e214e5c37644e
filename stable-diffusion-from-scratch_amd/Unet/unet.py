"""Mirror of ``Unet/unet.py`` VAE building blocks (Normalize, Upsample, Downsample, ResnetBlock), HIP-backed.

Reference semantics kept: GroupNorm eps 1e-6 (``unet.py:9-19``), SiLU after each
norm (``unet.py:23-28``; the reference casts to fp16 first — the device path is
fp16 anyway), nearest-x2 + conv3x3 upsample (``unet.py:34-49``), ResnetBlock with
optional 1x1 ``nin_shortcut`` (``unet.py:74-135``).  The shortcut projection is
fused into conv2 as a second K segment; the identity shortcut is the residual
epilogue of conv2.
"""
from __future__ import annotations

from torch import nn

from .. import ops
from ..packing import gn_norm, pack_res_tail, pack_upsample_conv, prep_norm, run_res_tail, run_upsample_conv


def Normalize(in_channels, num_groups=32):
    return nn.GroupNorm(num_groups=num_groups, num_channels=in_channels, eps=1e-6, affine=True)


UPSAMPLE_MATERIALISE_MAX_BYTES = 8 << 30   # the VAE Upsample's zero-bordered x2 image


class Upsample(nn.Module):
    def __init__(self, in_channels, with_conv):
        super().__init__()
        self.with_conv = with_conv
        self.in_channels = in_channels
        if not with_conv:
            raise NotImplementedError("sd_amd: conv-less VAE Upsample is not on the SD path")
        self.conv = nn.Conv2d(in_channels, in_channels, kernel_size=3, stride=1, padding=1)

    def _prepare(self, dev):
        self._pc, self._ppc = pack_upsample_conv(self.conv, self.in_channels, dev)

    def _run(self, x):
        # The routes: packing.run_upsample_conv.  The materialised image (the A/B switch, and the fallback for
        # channel counts that are no multiple of 64) is at C5 (B = 8, 384 -> 768, 256 channels) a 2.4 GB temporary:
        # above UPSAMPLE_MATERIALISE_MAX_BYTES the folded form runs instead
        return run_upsample_conv(self._pc, self._ppc, x, materialise_max_bytes=UPSAMPLE_MATERIALISE_MAX_BYTES)


class Downsample(nn.Module):
    """Encoder-side downsample (``unet.py:52-71``): F.pad(x, (0,1,0,1)) + conv3x3 s2 p0, run as one
    implicit-GEMM conv with ``pad_end=1`` (the extra bottom/right zero row and column are taps
    that fall outside the source, read as zeros — no padded copy)."""

    def __init__(self, in_channels, with_conv):
        super().__init__()
        self.with_conv = with_conv
        self.in_channels = in_channels
        if with_conv:
            self.conv = nn.Conv2d(in_channels, in_channels, kernel_size=3, stride=2, padding=0)

    def _prepare(self, dev):
        if not self.with_conv:
            raise NotImplementedError("sd_amd: avg-pool Downsample (with_conv=False) is not on the SD path")
        self._pc = ops.PackedConv([(self.conv.weight, self.in_channels)], self.conv.bias, device=dev)

    def _run(self, x):
        return ops.conv2d(self._pc, x, stride=2, pad=0, pad_end=1, gn_stats=True)


class ResnetBlock(nn.Module):
    def __init__(self, *, in_channels, out_channels=None, conv_shortcut=False, dropout, temb_channels=512):
        super().__init__()
        self.in_channels = in_channels
        out_channels = in_channels if out_channels is None else out_channels
        self.out_channels = out_channels
        self.use_conv_shortcut = conv_shortcut
        self.norm1 = Normalize(in_channels)
        self.conv1 = nn.Conv2d(in_channels, out_channels, kernel_size=3, stride=1, padding=1)
        if temb_channels > 0:
            self.temb_proj = nn.Linear(temb_channels, out_channels)
        self.norm2 = Normalize(out_channels)
        self.dropout = nn.Dropout(dropout)
        self.conv2 = nn.Conv2d(out_channels, out_channels, kernel_size=3, stride=1, padding=1)
        if self.in_channels != self.out_channels:
            if self.use_conv_shortcut:
                self.conv_shortcut = nn.Conv2d(in_channels, out_channels, kernel_size=3, stride=1, padding=1)
            else:
                self.nin_shortcut = nn.Conv2d(in_channels, out_channels, kernel_size=1, stride=1, padding=0)

    def _prepare(self, dev):
        prep_norm(self.norm1, dev)
        prep_norm(self.norm2, dev)
        self._pc1 = ops.PackedConv([(self.conv1.weight, self.in_channels)], self.conv1.bias, device=dev)
        skip = getattr(self, "conv_shortcut" if self.use_conv_shortcut else "nin_shortcut", None)
        self._tail = pack_res_tail(self.conv2, skip, self.in_channels, self.out_channels, dev)

    def _run(self, x, temb=None):
        if temb is not None:
            raise NotImplementedError("sd_amd: the VAE ResnetBlock path has no timestep embedding")
        # zero-bordered GN+SiLU outputs: both 3x3 convs run with pad 0 (mask-free gather); both outputs
        # feed a GroupNorm (norm2 / the next block's norm1, an attention norm or norm_out), so the convs
        # emit its statistics from their epilogues (no statistics pass over the tensor)
        gp, cp = ops.gn_conv_pad()
        h = ops.conv2d(self._pc1, gn_norm(self.norm1, x, silu=True, pad=gp), pad=cp, gn_stats=True)
        return run_res_tail(self._tail, gn_norm(self.norm2, h, silu=True, pad=gp), x, cp)
