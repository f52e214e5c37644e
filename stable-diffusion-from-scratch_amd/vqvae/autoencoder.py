"""Mirror of ``vqvae/autoencoder.py`` — VQModel and VQModelInterface (inference) on the HIP path.

``VQModel.encode(x)`` = Encoder → quant_conv (1x1, folded into the encoder's conv_out as
AutoEncoderKL does, ``double_z=False``) → VectorQuantize2 → ``(quant, emb_loss, info)``
(``autoencoder.py:124-135``); ``VQModel.decode(quant)`` = post_quant_conv → Decoder (``:138-141``),
the 1x1 conv as the 8-channel zero-padded GEMM of ``VAE/autoencoder.py``.
``VQModelInterface.encode`` stops before the quantiser and returns ``(h, 0, (None, None, None))``
(``:446-450``); ``VQModelInterface.decode(h, force_not_quantize=False)`` quantises first unless told
not to, and accepts the encode tuple (``:453-468``).
``decode`` takes AutoEncoderKL's ``pre_scale``: decode_first_stage's ``1/scale_factor · z``.  Without
quantisation it is fused into the layout conversion; with quantisation it multiplies ``h`` before
the search, exactly where the reference multiplies.
Training-only kwargs (``lossconfig``, ``image_key``, ``batch_resize_range``, ``scheduler_config``,
``lr_g_factor``, ``use_ema``) are accepted and ignored; none of the reference's ``print`` calls are kept.
"""
from __future__ import annotations

import torch
from torch import nn

from ..Encoder_Decoder.encoder import Decoder, Encoder, FirstStage
from .quantize import VectorQuantize2 as VectorQuantizer


class VQModel(FirstStage):
    def __init__(self, ddconfig, n_embed, embed_dim, lossconfig=None, ckpt_path=None, ignore_keys=[],
                 image_key="image", colorize_nlabels=None, monitor=None, batch_resize_range=None,
                 scheduler_config=None, lr_g_factor=1.0, remap=None, sane_index_shape=False, use_ema=False):
        super().__init__()
        if ddconfig.get("double_z", True):
            raise ValueError("sd_amd.VQModel: the VQ first stage needs `double_z: False` in ddconfig")
        self.embed_dim = embed_dim
        self.n_embed = n_embed
        self.image_key = image_key
        self.encoder = Encoder(**ddconfig)
        self.decoder = Decoder(**ddconfig)
        self.quantize = VectorQuantizer(n_e=n_embed, e_dim=embed_dim, beta=0.25, remap=remap,
                                        sane_index_shape=sane_index_shape)
        self.quant_conv = nn.Conv2d(ddconfig["z_channels"], embed_dim, 1)
        self.post_quant_conv = nn.Conv2d(embed_dim, ddconfig["z_channels"], 1)
        self.z_channels = ddconfig["z_channels"]
        if colorize_nlabels is not None:
            assert type(colorize_nlabels) == int
            self.register_buffer("colorize", torch.randn(3, colorize_nlabels, 1, 1))
        if monitor is not None:
            self.monitor = monitor
        self.batch_resize_range = batch_resize_range
        self.use_ema = use_ema
        self.scheduler_config = scheduler_config
        self.lr_g_factor = lr_g_factor
        if ckpt_path is not None:
            self.init_from_ckpt(ckpt_path, ignore_keys=ignore_keys)

    @torch.no_grad()
    def _encode_h(self, x):
        """Encoder ∘ quant_conv: NCHW image → fp32 NCHW [B, embed_dim, h, w]."""
        if not torch.is_tensor(x) or not x.is_cuda:
            raise TypeError("sd_amd.VQModel: HIP path only — move inputs to the GPU")
        return self.encoder.encode_packed(x, quant_conv=self.quant_conv)

    @torch.no_grad()
    def _decode_quant(self, quant, pre_scale: float = 1.0):
        if not torch.is_tensor(quant) or not quant.is_cuda:
            raise TypeError("sd_amd.VQModel: HIP path only — move inputs to the GPU")
        return self._decode_packed(quant, pre_scale)

    @torch.no_grad()
    def encode(self, x):
        return self.quantize(self._encode_h(x))

    @torch.no_grad()
    def decode(self, quant, pre_scale: float = 1.0):
        return self._decode_quant(quant, pre_scale)

    @torch.no_grad()
    def forward(self, input, return_pred_indices=False):
        quant, diff, (_, _, ind) = self.encode(input)
        dec = self.decode(quant)
        if return_pred_indices:
            return dec, diff, ind
        return dec, diff


class VQModelInterface(VQModel):
    def __init__(self, embed_dim, *args, **kwargs):
        super().__init__(embed_dim=embed_dim, *args, **kwargs)
        self.embed_dim = embed_dim

    @torch.no_grad()
    def encode(self, x):
        h = self._encode_h(x)
        return h, torch.tensor(0.0).to(h.device), (None, None, None)

    @torch.no_grad()
    def decode(self, h, force_not_quantize=False, pre_scale: float = 1.0):
        if isinstance(h, tuple):
            h = h[0]
        if force_not_quantize:
            return self._decode_quant(h, pre_scale)
        h = h.float()
        if pre_scale != 1.0:
            h = pre_scale * h
        quant, _ = self.quantize.nearest(h)
        return self._decode_quant(quant)
