"""Mirror of ``vqvae/quantize.py`` — VectorQuantize2 (inference) on the HIP path.

``forward`` keeps the reference's signature, asserts, remap / ``sane_index_shape`` handling and
return value ``(z_q, loss, (None, None, indices))`` (``quantize.py:104-181``), with int64 indices.
The reference's [M, n_e] distance matrix + argmin + embedding + straight-through line
(``quantize.py:138-145,160``) is ONE fused search (``sdk_vq_nearest``): fp32 scores
‖e‖² − 2·z·e, lowest index on ties (torch.argmin's rule), z_q = z + (e − z) with the reference's
two roundings, z read in place from NCHW.  ‖e‖² is computed once per codebook and cached;
``load_state_dict`` (or a new weight tensor) invalidates it.

``loss`` follows ``quantize.py:150-156`` with torch reductions on the device (off the hot path;
no gradients: inference only).  ``nearest(z)`` returns only ``(z_q, idx)`` for the decode and
DDIM paths, which never pay for the loss.

Documented extension: ``unmap_to_all`` and ``get_codebook_entry`` are taken from
``ldm/tamming/quantize.py:261-329`` (VectorQuantizer2).  The ``vqvae/`` copy of the class lacks
them although ``Diffusion/ddpm.py:722`` calls ``first_stage_model.quantize.get_codebook_entry``.
Indices outside the codebook raise ValueError (checked on the host).  None of the reference's
``print`` calls are kept.
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from .. import ops
from ..packing import PackedOwner


class VectorQuantize2(PackedOwner, nn.Module):
    def __init__(self, n_e, e_dim, beta, remap=None, unknown_index="random", sane_index_shape=False, legacy=True):
        super().__init__()
        self.n_e = n_e
        self.e_dim = e_dim
        self.beta = beta
        self.legacy = legacy
        self.embedding = nn.Embedding(num_embeddings=self.n_e, embedding_dim=self.e_dim)
        self.remap = remap
        if self.remap is not None:
            self.register_buffer("used", torch.tensor(np.load(self.remap)))
            self.re_embed = self.used.shape[0]
            self.unknown_index = unknown_index          # "random", "extra" or an integer
            if self.unknown_index == "extra":
                self.unknown_index = self.re_embed
                self.re_embed = self.re_embed + 1
        else:
            self.re_embed = n_e
        self.sane_index_shape = sane_index_shape

    def _pack(self, *weight_key):
        self._norms = ops.vq_code_norms(self.embedding.weight.detach())

    def _codebook(self, device):
        """(fp32 contiguous codebook on ``device``, cached ‖e‖²)."""
        w = self.embedding.weight.detach()
        if w.device != device or w.dtype != torch.float32 or not w.is_contiguous():
            raise TypeError("sd_amd.VectorQuantize2: the codebook must be fp32 on the input's device "
                            "(move the module to the GPU)")
        self.ensure_packed(w.device, w.data_ptr(), w._version)
        return w, self._norms

    @torch.no_grad()
    def nearest(self, z):
        """NCHW fp32 ``z`` → (z_q NCHW fp32, idx int64 [B·H·W]); no loss, no remap."""
        if not torch.is_tensor(z) or not z.is_cuda:
            raise TypeError("sd_amd.VectorQuantize2: HIP path only — move inputs to the GPU")
        w, norms = self._codebook(z.device)
        return ops.vq_nearest(z.float(), w, norms)

    def _used(self, device):
        return self.used.to(device=device, dtype=torch.int64)

    @torch.no_grad()
    def remap_to_used(self, inds):
        ishape = inds.shape
        assert len(ishape) > 1
        rnd = None
        unknown = 0
        if self.unknown_index == "random":
            rnd = torch.randint(0, self.re_embed, size=(inds.numel(),)).to(device=inds.device)
        else:
            unknown = int(self.unknown_index)
        return ops.vq_remap(inds.to(torch.int64), self._used(inds.device), to_used=True, unknown=unknown,
                            random=rnd).reshape(ishape)

    @torch.no_grad()
    def unmap_to_all(self, inds):
        ishape = inds.shape
        assert len(ishape) > 1
        inds = inds.to(torch.int64)
        lo, hi = int(inds.min()), int(inds.max())
        if lo < 0 or hi >= self.re_embed:
            raise ValueError(f"sd_amd.VectorQuantize2.unmap_to_all: index outside [0, {self.re_embed})")
        return ops.vq_remap(inds, self._used(inds.device), to_used=False,
                            extra=self.re_embed > self.used.shape[0]).reshape(ishape)

    @torch.no_grad()
    def forward(self, z, temp=None, rescale_logits=False, return_logits=False):
        assert temp is None or temp == 1.0, "Only for interface compatible with Gumbel"
        assert rescale_logits == False, "Only for interface compatible with Gumbel"    # noqa: E712
        assert return_logits == False, "Only for interface compatible with Gumbel"     # noqa: E712
        z = z.float()
        z_q, idx = self.nearest(z)
        B, _, H, W = z.shape
        e = ops.vq_lookup(idx, self.embedding.weight.detach(), nchw_shape=(B, H, W))
        diff = e - z
        if not self.legacy:
            loss = self.beta * torch.mean(diff ** 2) + torch.mean(diff ** 2)
        else:
            loss = torch.mean(torch.mean(diff) ** 2) + self.beta * torch.mean(diff ** 2)
        min_encoding_indices = idx
        if self.remap is not None:
            min_encoding_indices = min_encoding_indices.reshape(B, -1)
            min_encoding_indices = self.remap_to_used(min_encoding_indices)
            min_encoding_indices = min_encoding_indices.reshape(-1, 1)
        if self.sane_index_shape:
            min_encoding_indices = min_encoding_indices.reshape(B, H, W)
        return z_q, loss, (None, None, min_encoding_indices)

    @torch.no_grad()
    def get_codebook_entry(self, indices, shape):
        """``shape`` = (batch, height, width, channel) → NCHW z_q; ``shape=None`` →
        ``indices.shape + (e_dim,)`` (ldm/tamming/quantize.py:314-329)."""
        if not torch.is_tensor(indices) or not indices.is_cuda:
            raise TypeError("sd_amd.VectorQuantize2: HIP path only — move the indices to the GPU")
        indices = indices.to(torch.int64)
        if self.remap is not None:
            if shape is None:
                raise ValueError("sd_amd.VectorQuantize2.get_codebook_entry: remap needs `shape` (as the reference)")
            indices = indices.reshape(shape[0], -1)
            indices = self.unmap_to_all(indices)
            indices = indices.reshape(-1)
        if int(indices.min()) < 0 or int(indices.max()) >= self.n_e:
            raise ValueError(f"sd_amd.VectorQuantize2.get_codebook_entry: index outside [0, {self.n_e})")
        w = self.embedding.weight.detach()
        if shape is not None:
            return ops.vq_lookup(indices, w, nchw_shape=(shape[0], shape[1], shape[2]))
        return ops.vq_lookup(indices, w).view(*indices.shape, self.e_dim)
