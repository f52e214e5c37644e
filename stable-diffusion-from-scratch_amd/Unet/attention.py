"""Mirror of ``Unet/attention.py`` — ``make_attention`` and its blocks (first-stage attention):
``FlashAttentionBlock`` (8 heads), ``AttentionBlock`` (one head over all C channels: CompVis' AttnBlock, what
the published KL / VQ first stages were trained with) and ``LinearAttention`` / ``LinearAttentionBlock``.

Reference ``attention.py:221-264``: GroupNorm(32, C) with torch's default eps
1e-5, q/k/v 1x1 convs, 8 heads x C/8 through flash_attn with
its default scale d^-1/2, proj_out 1x1, + x.  Here: GN folded into ONE fused
q|k|v GEMM, ``sdk_attention``, proj_out GEMM with the residual epilogue.

``AttentionBlock`` (reference ``attention.py:76-128``) has the same parameters (``norm``, ``q``, ``k``, ``v``,
``proj_out``) but Normalize's eps 1e-6, ONE head of C channels and scale C^-1/2: a different function of the same
state_dict.  C <= 160 runs the per-wave attention forms, 168 <= C <= 512 the wide form (SDK_ATTN_WIDE).

``LinearAttention`` (``attention.py:131-194``): to_qkv without bias in the channel order (qkv heads c), softmax of
k over the tokens, ``sdk_linear_attention``, to_out with bias; no norm and no residual, as in the reference.
"""
from __future__ import annotations

import torch
from torch import nn

from .. import ops
from ..packing import gn_norm, prep_norm
from .unet import Normalize


class FlashAttentionBlock(nn.Module):
    def __init__(self, in_channels, num_heads=8):
        super().__init__()
        self.in_channels = in_channels
        self.num_heads = num_heads
        self.head_dim = in_channels // num_heads
        assert in_channels % num_heads == 0, "in_channels must be divisible by num_heads"
        self.norm = nn.GroupNorm(32, in_channels)
        self.q = nn.Conv2d(in_channels, in_channels, kernel_size=1)
        self.k = nn.Conv2d(in_channels, in_channels, kernel_size=1)
        self.v = nn.Conv2d(in_channels, in_channels, kernel_size=1)
        self.proj_out = nn.Conv2d(in_channels, in_channels, kernel_size=1)

    def _prepare(self, dev):
        prep_norm(self.norm, dev)
        w = torch.cat([self.q.weight, self.k.weight, self.v.weight], 0)
        b = torch.cat([self.q.bias, self.k.bias, self.v.bias], 0)
        self._pc_qkv = ops.PackedConv([(w, self.in_channels)], b, device=dev)
        self._pc_o = ops.PackedConv([(self.proj_out.weight, self.in_channels)], self.proj_out.bias, device=dev)

    def _run(self, x):
        B, H, W, C = x.shape
        xn = gn_norm(self.norm, x, silu=False)
        qkv = ops.conv2d(self._pc_qkv, xn).view(B * H * W, 3 * C)
        o = ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], batch=B, heads=self.num_heads, nq=H * W,
                          nk=H * W, head_dim=self.head_dim, scale=self.head_dim ** -0.5)
        return ops.conv2d(self._pc_o, o.view(B, H, W, C), residual=x, gn_stats=True)   # feeds a GroupNorm


class AttentionBlock(nn.Module):
    MAX_CHANNELS = 512      # sdk_attention's widest head

    def __init__(self, in_channels):
        super().__init__()
        if in_channels > self.MAX_CHANNELS:
            raise NotImplementedError(f"sd_amd: AttentionBlock runs one head of in_channels <= {self.MAX_CHANNELS} "
                                      f"(got {in_channels})")
        self.in_channels = in_channels
        self.norm = Normalize(in_channels)
        self.q = nn.Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.k = nn.Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.v = nn.Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.proj_out = nn.Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)

    _prepare = FlashAttentionBlock._prepare

    def _run(self, x):
        B, H, W, C = x.shape
        xn = gn_norm(self.norm, x, silu=False)
        qkv = ops.conv2d(self._pc_qkv, xn).view(B * H * W, 3 * C)
        o = ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], batch=B, heads=1, nq=H * W, nk=H * W,
                          head_dim=C, scale=int(C) ** (-0.5))
        return ops.conv2d(self._pc_o, o.view(B, H, W, C), residual=x, gn_stats=True)   # feeds a GroupNorm


class LinearAttention(nn.Module):
    def __init__(self, dim, heads=4, dim_head=32):
        super().__init__()
        if dim_head % 8 or not 8 <= dim_head <= 512:
            raise NotImplementedError(f"sd_amd: LinearAttention needs dim_head a multiple of 8 in [8, 512] (got {dim_head})")
        self.heads = heads
        self.dim_head = dim_head
        self.dim = dim
        hidden_dim = dim_head * heads
        self.to_qkv = nn.Conv2d(dim, hidden_dim * 3, kernel_size=1, bias=False)
        self.to_out = nn.Conv2d(hidden_dim, dim, kernel_size=1)

    def _prepare(self, dev):
        hidden = self.heads * self.dim_head
        self._pc_qkv = ops.PackedConv([(self.to_qkv.weight, self.dim)], None, device=dev)
        self._pc_o = ops.PackedConv([(self.to_out.weight, hidden)], self.to_out.bias, device=dev)

    def _run(self, x):
        B, H, W, C = x.shape
        hid = self.heads * self.dim_head
        qkv = ops.conv2d(self._pc_qkv, x).view(B * H * W, 3 * hid)       # columns: (qkv heads c)
        o = ops.linear_attention(qkv[:, :hid], qkv[:, hid:2 * hid], qkv[:, 2 * hid:], batch=B, heads=self.heads,
                                 n=H * W, dim_head=self.dim_head)
        return ops.conv2d(self._pc_o, o.view(B, H, W, hid), gn_stats=True)          # feeds a ResnetBlock's GroupNorm


class LinearAttentionBlock(LinearAttention):
    """to match AttentionBlock usage"""

    def __init__(self, in_channels):
        super().__init__(dim=in_channels, heads=1, dim_head=in_channels)


def make_attention(in_channels, attention_type="vanilla"):
    """``"single_head"`` (an extension: the reference's own ``make_attention`` has that line commented out) returns
    the one-head ``AttentionBlock`` that CompVis-trained first-stage checkpoints need."""
    assert attention_type in ["vanilla", "linear", "none", "single_head"], f"attention_type {attention_type} not found."
    if attention_type == "vanilla":
        return FlashAttentionBlock(in_channels)
    if attention_type == "single_head":
        return AttentionBlock(in_channels)
    if attention_type == "linear":
        return LinearAttentionBlock(in_channels)
    return nn.Identity(in_channels)
