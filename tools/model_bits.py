"""Output bits of every tiny fixture model, for comparing two trees of a host-layer refactor: one line per model
with its name, the input shape and the first 32 hex digits of the SHA-256 over the output bytes (several outputs
hashed together).  Run it in each tree (each with its own build, a process of its own) and diff the listings; with
SD_AMD_UPSAMPLE_FOLD=1 / SD_AMD_UPSAMPLE_MATERIALISE=1 for the other two Upsample routes.  It uses only what the
models expose (constructors, ``load_state_dict``, ``forward`` / ``encode`` / ``decode``) and the test fixtures.
The Upsample lines run the two Upsample modules alone at 64 and 24 channels: the tiny models' Upsamples are too
narrow for the phase form."""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
DEV = "cuda"


def gpu(a):
    return torch.from_numpy(a).to(DEV)


def line(name, shape, *outs):
    h = hashlib.sha256()
    for o in outs:
        h.update(o.detach().contiguous().cpu().numpy().tobytes())
    print(f"{name:<28} {'x'.join(str(int(s)) for s in shape):<14} {h.hexdigest()[:32]}", flush=True)


def main():
    import sd_amd_loader
    sd_amd_loader.load()
    import adm_util as au
    import ca_util as ca
    import cond_util as cu
    import first_stage_attn_util as fu
    from golden_util import cfg_of, load, weights_of
    from synth import synth_weights
    from sd_amd.clip_encoder.modules import FrozenCLIPEmbedder, TransformerEmbedder
    from sd_amd.clip_encoder.x_transformer import Encoder as XEncoder, TransformerWrapper
    from sd_amd.DDPM.models.unet import UNet
    from sd_amd.Diffusion.ddpm import LatentDiffusion
    from sd_amd.Encoder_Decoder.encoder import Decoder, Encoder
    from sd_amd.openai_model import model as M
    from sd_amd.Unet import unet as V
    from sd_amd.VAE.autoencoder import AutoEncoderKL
    from sd_amd.vqvae.autoencoder import VQModel, VQModelInterface

    def unet(name):
        z = load(name)
        m = M.UNetModel(**cfg_of(z))
        m.load_state_dict(weights_of(z))
        return m, z

    with torch.no_grad():
        for name in ("unet_tiny", "unet_tiny_uncond", "unet_tiny_headch"):
            m, z = unet(name)
            ctx = gpu(z["ctx"]) if "ctx" in z.files else None
            line(name, z["x"].shape, m(gpu(z["x"]), gpu(z["t"]), ctx))
        for name in sorted(au.FIXTURES):
            m, z = unet(name)
            for shape in ((2, 4, 16, 16), au.WIDE)[:2 if name == "unet_tiny_adm_full" else 1]:
                d = {k: gpu(v) for k, v in au.inputs(shape).items()}
                kw = {"y": d["y"]} if m.num_classes is not None else {}
                ctx = d["ctx"] if cfg_of(z).get("use_spatial_transformer") else None
                line(name, shape, m(d["x"], d["t"], ctx, **kw))
        m, z = unet("unet_tiny_concat")
        d = {k: gpu(v) for k, v in ca.unet_inputs().items()}
        line("unet_tiny_concat", d["x"].shape, m(d["x"], d["t"], context=d["ctx"], concat=[d["m"], d["zi"]]))

        z = load("vae_tiny")
        vae = AutoEncoderKL(ddconfig=cfg_of(z), embed_dim=4)
        vae.load_state_dict(weights_of(z))
        line("vae_tiny decode", z["z"].shape, vae.decode(gpu(z["z"]), pre_scale=1.0 / float(z["scale_factor"])))
        line("vae_tiny encode", z["dec"].shape, vae.encode(gpu(z["dec"])).parameters)
        line("vae_tiny Encoder alone", z["dec"].shape, vae.encoder(gpu(z["dec"])))
        line("vae_tiny encode again", z["dec"].shape, vae.encode(gpu(z["dec"])).parameters)

        def tiled(vae_, sp, scale, zt):
            class LD:                      # the decode_first_stage surface of LatentDiffusion
                scale_factor = scale
                first_stage_model = vae_
                split_input_params = sp
                decode_first_stage = LatentDiffusion.decode_first_stage
                _decode_tiled = LatentDiffusion._decode_tiled
                get_weighting = LatentDiffusion.get_weighting
                delta_border = staticmethod(LatentDiffusion.delta_border)
            return LD().decode_first_stage(zt)

        z = load("vae_tiled")
        vae = AutoEncoderKL(ddconfig=cfg_of(z), embed_dim=4)
        vae.load_state_dict(weights_of(z))
        line("vae_tiled", z["z"].shape, tiled(vae, json.loads(bytes(z["sp"]).decode()), float(z["scale_factor"]),
                                              gpu(z["z"])))

        for attn in fu.MODEL_ATTN:
            z = load("fsa_model_" + attn)
            cfg = dict(json.loads(bytes(z["cfg"]).decode()), attn_type=attn)
            enc, dec, vae = Encoder(**cfg), Decoder(**cfg), AutoEncoderKL(ddconfig=cfg, embed_dim=4)
            for tag, m, s in (("enc", enc, 0), ("dec", dec, 20), ("vae", vae, 40)):
                ks = json.loads(bytes(z[f"{attn}_{tag}_keys"]).decode())
                w = synth_weights([(k, tuple(sh)) for k, sh in ks], fu.MODEL_SEED[attn] + s, fu.MODEL_WSCALE)
                m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
            seed = fu.MODEL_SEED[attn]
            x = gpu(fu.fsa_input(seed + 1, (2, 3, 32, 32), 0.5))
            zz = gpu(fu.fsa_input(seed + 2, (2, 4, 16, 16)))
            line(f"fsa_model_{attn} enc", x.shape, enc.to(DEV)(x))
            line(f"fsa_model_{attn} dec", zz.shape, dec.to(DEV)(zz))
            vae = vae.to(DEV)
            line(f"fsa_model_{attn} vae", x.shape, vae.encode(x).parameters,
                 vae.decode(zz, pre_scale=1.0 / fu.SCALE_FACTOR))
            zt = gpu(fu.fsa_input(seed + 3, (2, 4, 16, 16)))
            line(f"fsa_model_{attn} tiled", zt.shape, tiled(vae, json.loads(bytes(z["sp"]).decode()),
                                                            fu.SCALE_FACTOR, zt))

        z = load("vq_model")
        kw = dict(ddconfig=cfg_of(z), n_embed=64, embed_dim=3, lossconfig={"target": "torch.nn.Identity"})
        vqm, vqi = VQModel(**kw), VQModelInterface(**kw)
        vqm.load_state_dict(weights_of(z))
        vqi.load_state_dict(weights_of(z))
        vqm, vqi = vqm.to(DEV), vqi.to(DEV)
        quant, loss, (_, _, idx) = vqm.encode(gpu(z["x"]))
        line("vq_model VQModel", z["x"].shape, quant, loss, idx, vqm.decode(quant))
        h = gpu(z["h"])
        line("vq_model VQModelInterface", z["h"].shape, vqi.encode(gpu(z["x"]))[0], vqi.decode(h),
             vqi.decode(h, force_not_quantize=True))

        z = load("ddpm_unet")
        m = UNet(input_channels=3)
        m.load_state_dict(weights_of(z))
        line("ddpm_unet", z["x"].shape, m(gpu(z["x"]), gpu(z["t"])))

        z = load("clip_tiny")
        m = FrozenCLIPEmbedder(device=DEV, config=json.loads(bytes(z["cfg"]).decode()))
        m.transformer.load_state_dict(weights_of(z))
        line("clip_tiny", z["ids"].shape, m.encode_tokens(torch.from_numpy(z["ids"])))

        fx = load("cond_transformer_tiny")
        for name in ("te", "glu"):
            m = TransformerEmbedder(**cu.TE_CFG) if name == "te" else \
                TransformerWrapper(num_tokens=cu.VOCAB, max_seq_len=77, attn_layers=XEncoder(**cu.GLU_CFG))
            ks = [(k, tuple(s)) for k, s in json.loads(bytes(fx[name + "_keys"]).decode())]
            m.load_state_dict({k: torch.from_numpy(v) for k, v in synth_weights(ks, int(fx[name + "_seed"])).items()})
            m = m.to(DEV)
            for seq in cu.SEQ_LENS:
                ids = gpu(cu.case_ids(name, seq))
                line(f"cond_transformer_tiny {name}", ids.shape,
                     m.encode(ids) if name == "te" else m(ids, return_embeddings=True))

        for which, ch in (("unet", 64), ("vae", 64), ("unet", 24), ("vae", 24)):
            torch.manual_seed(3 + ch)
            mod = M.Upsample(ch, True) if which == "unet" else V.Upsample(ch, True)
            mod._prepare(torch.device(DEV))
            x = torch.randn(2, 8, 8, ch).half().to(DEV)
            line(f"Upsample {which}", x.shape, mod._run(x))
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
