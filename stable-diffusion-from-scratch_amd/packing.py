"""Host-side packing shared by the module mirrors: the packed-weight lifecycle (``PackedOwner``) and the helpers
every mirror packs and runs with (fp32 norm vectors, the ResBlock's second conv and skip, the nearest-x2 + 3x3
Upsample conv).  No kernel and no C ABI call lives here; everything goes through ``sd_amd.ops``.
"""
from __future__ import annotations

import os

import torch
from torch import nn

from . import ops


class PackedOwner:
    """Mixin (listed BEFORE ``nn.Module`` in the bases) for a module that owns device-side packed copies of its
    parameters: ``ops.PackedConv`` / ``PhaseConv`` / ``PackedFF`` / ``PackedTokenLinear``, fp32 norm vectors,
    embedding tables and whatever its blocks' ``_prepare(dev)`` build.  It adds no parameter, buffer or submodule.

    One key, ``_packed_key``, says what the current packs were built for: a tuple that starts with the device and
    continues with whatever the class needs; ``None`` means nothing valid.  ``ensure_packed(*key)`` calls the
    class's ``_pack(*key)`` when the key differs, ``repack(*key)`` unconditionally (the public ``prepare(device)``
    of the models: call it again after editing parameters in place).

    The packs are invalidated whenever this module's parameters are loaded, by its own ``load_state_dict`` or by any
    ancestor's: ``nn.Module.load_state_dict`` walks the tree through ``_load_from_state_dict``, which is the one
    place overridden here.  Invalidation drops the key, moves ``prepare_generation`` at once (whatever holds
    something derived from the old packs, a ``GraphedUNet``'s graphs, compares it on its next call, with no eager
    forward in between) and calls ``_packs_dropped()`` for state the class keeps beside the packs.

    An owner never writes another owner's state: a parent (``AutoEncoderKL``, ``VQModel``) asks its ``Encoder`` /
    ``Decoder`` to ``ensure_packed`` with the key it needs.

    Rule for every other parameter-derived cache: it is either rebuilt by ``_pack`` or it hangs off an object that
    ``_pack`` replaces.  As audited: ``UNetModel._label_table`` and ``CrossAttention._bo32`` are rebuilt;
    ``CrossAttention._pc_reassoc`` is reset to ``None`` by the block's ``_prepare``; ``PackedConv._xattn_pk`` lives
    on the ``PackedConv`` that ``_prepare`` replaces; a ``ReassocContext`` lives in ``UNetModel._ctx_cache``, which
    ``_packs_dropped`` clears.  Not covered: parameters edited in place (call ``prepare`` again) and dtype casts
    through ``Module._apply``.
    """

    _packed_key = None
    prepare_generation = 0

    def _load_from_state_dict(self, *args, **kwargs):
        self.invalidate_packed()
        return super()._load_from_state_dict(*args, **kwargs)

    def invalidate_packed(self):
        self._packed_key = None
        self.prepare_generation += 1
        self._packs_dropped()

    def _packs_dropped(self):
        """Per-class hook: drop what was derived from the packs just invalidated."""

    @torch.no_grad()
    def repack(self, *key, **pack_args):
        self.invalidate_packed()          # the old packs are about to be replaced; a failed _pack leaves none valid
        self._pack(*key, **pack_args)
        self._packed_key = key

    def ensure_packed(self, *key, **pack_args):
        if self._packed_key != key:
            self.repack(*key, **pack_args)


# ---------------------------------------------------------------------------------------------- norm parameters
def f32(param, dev):
    return param.detach().to(dev, torch.float32).contiguous()


def prep_norm(norm, dev):
    """fp32 device copies of a GroupNorm's or LayerNorm's affine as ``norm._g`` / ``norm._b``."""
    norm._g = f32(norm.weight, dev)
    norm._b = f32(norm.bias, dev)


def gn_affine(gn, x):
    """Per-(batch, channel) (scale, shift) of ``gn(x)`` for a consumer that applies it itself."""
    return ops.group_norm_affine(x, gn._g, gn._b, gn.eps, gn.num_groups)


def gn_scale_shift(gn, x):
    """The same affine from the statistics x's producing convs emitted (else a statistics pass): what ``gn_norm``
    applies, for a consumer that applies it itself."""
    return ops.group_norm_scale_shift(x, gn._g, gn._b, gn.eps, gn.num_groups)


def gn_norm(gn, x, silu=True, pad=0):
    """GroupNorm (+ SiLU) of x materialised, zero-bordered by ``pad`` — one ``sdk_group_norm``."""
    return ops.group_norm(x, gn._g, gn._b, gn.eps, gn.num_groups, silu=silu, pad=pad)


# ------------------------------------------------------------------------- the ResBlock's second conv and its skip
def pack_res_tail(conv2, skip, cin, cout, dev):
    """(mode, packed conv2, packed skip or None) of a residual block's ``conv2(ha) + skip(x)``.  ``skip`` is the
    block's skip module (anything but a Conv2d is the identity): ``"identity"`` adds x as conv2's residual epilogue,
    ``"fused"`` runs a 1x1 skip as a second K segment of the same GEMM, ``"conv3"`` runs a 3x3 skip on its own."""
    if isinstance(skip, nn.Conv2d) and skip.kernel_size[0] == 1:
        return "fused", ops.PackedConv([(conv2.weight, cout), (skip.weight, cin)],
                                       conv2.bias.detach() + skip.bias.detach(), device=dev), None
    pc2 = ops.PackedConv([(conv2.weight, cout)], conv2.bias, device=dev)
    if isinstance(skip, nn.Conv2d):
        return "conv3", pc2, ops.PackedConv([(skip.weight, cin)], skip.bias, device=dev)
    return "identity", pc2, None


def run_res_tail(tail, ha, x, pad):
    """``tail`` from ``pack_res_tail``; ``ha`` the activated input of conv2, ``x`` the skip source.  The output
    feeds a GroupNorm: the conv emits its statistics."""
    mode, pc2, pc_skip = tail
    if mode == "identity":
        return ops.conv2d(pc2, ha, pad=pad, residual=x, gn_stats=True)
    if mode == "fused":
        return ops.conv2d(pc2, ha, pad=pad, seg2=(x, None, False), gn_stats=True)
    return ops.conv2d(pc2, ha, pad=pad, residual=ops.conv2d(pc_skip, x), gn_stats=True)


# ---------------------------------------------------------------------------------- nearest-x2 + conv3x3 Upsample
# Default: the phase form — four 2x2 convs over the zero-bordered low-res image, one per output parity
# (ops.PhaseConv, 4/9 of the FLOPs, no x2 image).  SD_AMD_UPSAMPLE_MATERIALISE=1 restores the previous route for
# A/B runs (the nearest-x2 image written zero-bordered, an unmasked 3x3 conv over it with pad 0; also the fallback
# for channel counts that are no multiple of 64); SD_AMD_UPSAMPLE_FOLD=1 folds the upsample into the 3x3 conv's DMA
# addresses (the folded form ran the 512^2 decoder convs at 730-830 TF/s).
UPSAMPLE_FOLD = os.environ.get("SD_AMD_UPSAMPLE_FOLD", "0") == "1"
UPSAMPLE_MATERIALISE = os.environ.get("SD_AMD_UPSAMPLE_MATERIALISE", "0") == "1"


def upsample_phase_ok(x, padding=1):
    """The phase form needs one NHWC source with whole 64-channel K blocks (and the conv's padding 1)."""
    return not (UPSAMPLE_FOLD or UPSAMPLE_MATERIALISE) and not isinstance(x, tuple) and x.shape[-1] % 64 == 0 \
        and padding == 1


def pack_upsample_conv(conv, channels, dev, padding=1):
    """(PackedConv, PhaseConv or None) of an Upsample's 3x3 conv."""
    pc = ops.PackedConv([(conv.weight, channels)], conv.bias, device=dev)
    ppc = None
    if channels % 64 == 0 and padding == 1 and not (UPSAMPLE_FOLD or UPSAMPLE_MATERIALISE):
        ppc = ops.PhaseConv(conv.weight, channels, conv.bias, device=dev)
    return pc, ppc


def run_upsample_conv(pc, ppc, x, padding=1, materialise_max_bytes=None):
    """Route choice: phase form, else the materialised zero-bordered x2 image, else the folded form.  The
    materialised image is a temporary of B·(2H+2)·(2W+2)·C·2 bytes beside the input and the output; a caller that
    passes ``materialise_max_bytes`` gets the folded form above it.  The output feeds a GroupNorm."""
    if ppc is not None and upsample_phase_ok(x, padding):
        return ops.conv2d(ppc, ops.zero_border(x, 1), phase=True, gn_stats=True)
    fold = UPSAMPLE_FOLD or isinstance(x, tuple) or x.shape[-1] % 8 != 0
    if not fold and materialise_max_bytes is not None:
        n, h, w, c = x.shape
        fold = n * (2 * h + 2) * (2 * w + 2) * c * 2 > materialise_max_bytes
    if fold:
        return ops.conv2d(pc, x, upsample=True, pad=padding, gn_stats=True)
    return ops.conv2d(pc, ops.upsample_nearest2x_padded(x, padding), pad=0, gn_stats=True)
