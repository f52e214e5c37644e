"""Mirror of ``VAE/autoencoder.py`` — AutoEncoderKL (encode and decode on the HIP path).

``decode(z)`` = post_quant_conv (1x1) → Decoder (``autoencoder.py:126-132``).
``encode(x)`` = Encoder → quant_conv (folded into the encoder's conv_out) →
DiagonalGaussianDistribution (``autoencoder.py:114-123``); the encoder is packed on the
first encode call.
The 1x1 post_quant_conv runs as a GEMM whose output is zero-padded to 8
channels (the NHWC kernels need 8-channel granularity); the decoder's conv_in
consumes those 8 channels with zero weights on the padding.
``lossconfig`` is accepted and ignored (inference only; the reference's
``lossconfig=None`` path raises AttributeError).
"""
from __future__ import annotations

import importlib

import torch
from torch import nn

from ..Distribution.distribution import DiagonalGaussianDistribution
from ..Encoder_Decoder.encoder import Decoder, Encoder, FirstStage


class AutoEncoderKL(FirstStage):
    def __init__(self, ddconfig, embed_dim, lossconfig=None, ckpt_path=None, ignore_keys=[], colorize_nlabels=None,
                 monitor=None):
        super().__init__()
        self.encoder = Encoder(**ddconfig)
        self.decoder = Decoder(**ddconfig)
        self.learning_rate = 4.5e-06
        assert ddconfig["double_z"], "make sure `double_z: True`"
        self.quant_conv = nn.Conv2d(2 * ddconfig["z_channels"], 2 * embed_dim, kernel_size=1)
        self.post_quant_conv = nn.Conv2d(embed_dim, ddconfig["z_channels"], kernel_size=1)
        self.embed_dim = embed_dim
        self.z_channels = ddconfig["z_channels"]
        if colorize_nlabels is not None:
            self.register_buffer("colorize", torch.randn(3, colorize_nlabels, 1, 1))
        if monitor is not None:
            self.monitor = monitor
        if ckpt_path is not None:
            self.init_from_ckpt(ckpt_path, ignore_keys=ignore_keys)

    @torch.no_grad()
    def encode(self, x):
        """x: NCHW image [B, in_channels, H, W] (any float dtype) → DiagonalGaussianDistribution."""
        if not x.is_cuda:
            raise TypeError("sd_amd.AutoEncoderKL: HIP path only — move inputs to the GPU")
        return DiagonalGaussianDistribution(self.encoder.encode_packed(x, quant_conv=self.quant_conv))

    @torch.no_grad()
    def decode(self, z, pre_scale: float = 1.0):
        """z: [B, embed_dim, h, w] → [B, out_ch, 8h, 8w] fp32.  ``pre_scale`` fuses
        decode_first_stage's ``1/scale_factor * z`` into the layout conversion."""
        if not z.is_cuda:
            raise TypeError("sd_amd.AutoEncoderKL: HIP path only — move inputs to the GPU")
        return self._decode_packed(z, pre_scale)

    @torch.no_grad()
    def forward(self, input, sample_posterior=True):
        posterior = self.encode(input)
        z = posterior.sample() if sample_posterior else posterior.mode()
        return self.decode(z), posterior


def instantiate_from_config(config):
    from ..Diffusion.utils import instantiate_from_config as inst
    return inst(config)
