"""Generate the first-stage attention fixtures by importing the REFERENCE itself (build container only).

Run from the repo root:  python tests/golden/make_golden_first_stage_attn.py
Needs the reference checkout make_golden.py points at (read-only) and einops.  Uses the shims of make_golden.py
(flash_attn stand-in, fp32 ``nonlinearity``, silenced stdout).

* fsa_<case>.npz, one per entry of first_stage_attn_util.BLOCK_CASES: the output of the reference's
  ``Unet.attention.AttentionBlock`` / ``LinearAttentionBlock`` / ``LinearAttention`` / ``FlashAttentionBlock``
  (the last as the yardstick of the tolerance, made the same way at the same C, size and seeds), with the
  state_dict key list; an output above the size cap is stored for every ``cstride``-th channel.
* fsa_model_<attn_type>.npz: tiny ``Encoder`` / ``Decoder`` / ``AutoEncoderKL`` with ``attn_type="linear"``, with the
  reference's ``Encoder_Decoder.encoder.make_attention`` bound to the reference's ``AttentionBlock``
  (ours: ``attn_type="single_head"``) and with the 8-head default; one tiled decode of the single-head model,
  composed as make_golden.gen_tiled_decode.
Weights and inputs are regenerated from seeds (synth.py, first_stage_attn_util.fsa_input); only outputs are stored.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg                                    # noqa: E402
import first_stage_attn_util as fu                          # noqa: E402

OUT = HERE


def jbytes(obj):
    return np.frombuffer(json.dumps(obj).encode(), dtype=np.uint8)


def gen_blocks():
    import Unet.attention as ra
    classes = {"single": ra.AttentionBlock, "flash": ra.FlashAttentionBlock, "linear_block": ra.LinearAttentionBlock,
               "linear": ra.LinearAttention}
    for name, (kind, args, shape, seed) in fu.BLOCK_CASES.items():
        with mg.quiet():
            m = classes[kind](*args)
        mg.reinit_(m, seed)
        m.eval()
        x = torch.from_numpy(fu.block_input(name))
        with mg.quiet(), torch.no_grad():
            y = m(x).numpy()
        assert y.shape == x.shape and np.isfinite(y).all()
        cs = fu.channel_stride(y.shape)
        path = os.path.join(OUT, f"fsa_{name}.npz")
        np.savez_compressed(path, **mg.sd_keys(m), seed=np.int64(seed), out=np.ascontiguousarray(y[:, ::cs]),
                            cstride=np.int64(cs), shape=np.asarray(y.shape, dtype=np.int64))
        print(name, tuple(y.shape), "cstride", cs, os.path.getsize(path))


def reinit_scaled(module, seed, scale):
    """mg.reinit_ with synth.py's ``scale`` on the conv weights and biases."""
    from synth import synth_weights, keys_shapes_of
    new = synth_weights(keys_shapes_of(module.state_dict()), seed, scale)
    module.load_state_dict({k: torch.from_numpy(v) for k, v in new.items()})


def watch_range(module, cls, peaks):
    """Record the largest |output| of every ``cls`` block: the fp16 path cannot hold what the fp32 reference can."""
    for m in module.modules():
        if isinstance(m, cls):
            m.register_forward_hook(lambda mod, i, o: peaks.append(o.abs().max().item()))


def tiled_decode(vae, zl):
    from Diffusion.ddpm import LatentDiffusion as RefLD
    sp = fu.TILED_SP

    def delta_border(self, h, w):
        lower_right_corner = torch.tensor([h - 1, w - 1]).view(1, 1, 2)
        arr = self.meshgrid(h, w) / lower_right_corner
        dist_left_up = torch.min(arr, dim=-1, keepdim=True)[0]
        dist_right_down = torch.min(1 - arr, dim=-1, keepdim=True)[0]
        return torch.min(torch.cat([dist_left_up, dist_right_down], dim=-1), dim=-1)[0]

    class Stand:
        split_input_params = sp
        meshgrid = RefLD.meshgrid
        get_weighting = RefLD.get_weighting
        get_fold_unfold = RefLD.get_fold_unfold

    Stand.delta_border = delta_border
    st = Stand()
    z = 1.0 / fu.SCALE_FACTOR * zl
    ks, stride, uf = sp["ks"], sp["stride"], sp["vqf"]
    fold, unfold, normalization, weighting = st.get_fold_unfold(z, ks, stride, uf=uf)
    zp = unfold(z)
    zp = zp.view((zp.shape[0], -1, ks[0], ks[1], zp.shape[-1]))
    o = torch.stack([vae.decode(zp[:, :, :, :, i]) for i in range(zp.shape[-1])], axis=-1)
    o = (o * weighting).view((o.shape[0], -1, o.shape[-1]))
    return fold(o) / normalization


def gen_models():
    import Unet.unet as uu
    import Unet.attention as ra
    import Encoder_Decoder.encoder as ee
    silu = lambda x: x * torch.sigmoid(x)               # noqa: E731  (no fp16 cast)
    uu.nonlinearity = silu
    ee.nonlinearity = silu
    from VAE.autoencoder import AutoEncoderKL
    ref_make = ee.make_attention
    for attn in fu.MODEL_ATTN:
        out = {"cfg": jbytes(fu.TINY_DDCONFIG), "sp": jbytes(fu.TILED_SP), "scale_factor": np.float64(fu.SCALE_FACTOR)}
        seed = fu.MODEL_SEED[attn]
        if attn == "single_head":       # the line the reference's make_attention has commented out
            ee.make_attention = lambda in_channels, attention_type="vanilla": ra.AttentionBlock(in_channels)
            cfg = dict(fu.TINY_DDCONFIG)
        else:
            ee.make_attention = ref_make
            cfg = dict(fu.TINY_DDCONFIG, attn_type=attn)
        with mg.quiet():
            enc = ee.Encoder(**cfg)
            dec = ee.Decoder(**cfg)
            vae = AutoEncoderKL(ddconfig=cfg, embed_dim=4, lossconfig={"target": "torch.nn.Identity"})
        ee.make_attention = ref_make
        peaks = []
        for m, s in ((enc, seed), (dec, seed + 20), (vae, seed + 40)):
            reinit_scaled(m, s, fu.MODEL_WSCALE)
            m.eval()
            watch_range(m, (ra.LinearAttention, ra.AttentionBlock, ra.FlashAttentionBlock), peaks)
        want = {"linear": ra.LinearAttentionBlock, "single_head": ra.AttentionBlock, "vanilla": ra.FlashAttentionBlock}
        assert type(enc.mid.attn_1) is want[attn] and type(vae.decoder.up[1].attn[0]) is want[attn]
        x = torch.from_numpy(fu.fsa_input(seed + 1, (2, 3, 32, 32), 0.5))
        z = torch.from_numpy(fu.fsa_input(seed + 2, (2, 4, 16, 16)))
        zt = torch.from_numpy(fu.fsa_input(seed + 3, (2, 4, 16, 16)))
        with mg.quiet(), torch.no_grad():
            out[f"{attn}_enc"] = enc(x).numpy()
            out[f"{attn}_dec"] = dec(z).numpy()
            out[f"{attn}_vae_moments"] = vae.quant_conv(vae.encoder(x)).numpy()
            out[f"{attn}_vae_dec"] = vae.decode(1.0 / fu.SCALE_FACTOR * z).numpy()
            if attn == "single_head":
                out[f"{attn}_vae_tiled"] = tiled_decode(vae, zt).numpy()
        # the linear block has neither norm nor residual: with unit-gain weights its output grows by 5-50x per block
        # (1e6 after three of them), which is why the tiny models' conv weights are scaled by MODEL_WSCALE
        assert max(peaks) < 2048, (attn, max(peaks))
        print(attn, "largest attention output", max(peaks))
        for tag, m in (("enc", enc), ("dec", dec), ("vae", vae)):
            out[f"{attn}_{tag}_keys"] = mg.sd_keys(m)["keys"]
        path = os.path.join(OUT, f"fsa_model_{attn}.npz")
        np.savez_compressed(path, **out)
        print(attn, os.path.getsize(path))


def main():
    mg.install_shims()
    torch.set_num_threads(8)
    gen_blocks()
    gen_models()


if __name__ == "__main__":
    main()
