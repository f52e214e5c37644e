"""Tiled ``LatentDiffusion.encode_first_stage`` (``split_input_params['patch_distributed_vq']``) on the GPU (run with
-m gpu): image patches encoded in chunks and blended at 1 / vqf, against the reference's ``encode_first_stage`` /
``get_fold_unfold`` (df branch) on the tiny KL and VQ first stages (tests/golden/make_golden_patch.py), and the whole
tiled chain encode -> stochastic_encode -> patch-wise decode -> tiled decode."""
import numpy as np
import pytest
import torch

import patch_util as pu
from golden_util import cfg_of, load, weights_of
from gpu_util import check_parity

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _sp(**extra):
    return pu.split_params(pu.ENC_KS, pu.ENC_STRIDE, True, patch_distributed_vq=True, vqf=pu.ENC_VQF, **extra)


def _ld(sdk, kind, sp, unet=None):
    from sd_amd.Diffusion.ddpm import DiffusionWrapper, LatentDiffusion
    from sd_amd.VAE.autoencoder import AutoEncoderKL
    from sd_amd.vqvae.autoencoder import VQModelInterface
    fx = load(f"patch_encode_{kind}")
    if kind == "kl":
        fs = AutoEncoderKL(ddconfig=cfg_of(fx), embed_dim=4)
    else:
        fs = VQModelInterface(ddconfig=cfg_of(fx), n_embed=pu.TINY_VQ_CODES, embed_dim=pu.TINY_VQ_EMBED,
                              lossconfig={"target": "torch.nn.Identity"})
    fs.load_state_dict(weights_of(fx))

    class LD(LatentDiffusion):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.parameterization, self.clip_denoised, self.v_posterior = "eps", False, 0.
            self.shorten_cond_schedule, self.log_every_t, self.scale_factor = False, 1, 0.5
            self.first_stage_model = fs
            self.cond_stage_key, self.conditioning_key = "txt", "crossattn"
            self.split_input_params = sp
            if unet is not None:
                cfg, _ = pu.MODELS[unet]
                self.model = DiffusionWrapper({"target": "openai_model.model.UNetModel", "params": dict(cfg)}, unet)
                self.model.diffusion_model.load_state_dict(weights_of(load(f"patch_unet_{unet}")))
            kw = dict(pu.SCHEDULE)
            self.register_schedule(beta_schedule=kw.pop("beta_schedule"), **kw)

    return LD().to(DEV), fx


@pytest.mark.parametrize("chunk", [16, 3], ids=["one_batch", "max_batch3"])
@pytest.mark.parametrize("kind", ["kl", "vq"])
def test_tiled_encode_vs_reference(sdk, kind, chunk):
    from sd_amd.Distribution.distribution import DiagonalGaussianDistribution
    sp = _sp(max_batch=chunk)
    ld, fx = _ld(sdk, kind, sp)
    x = torch.from_numpy(pu.encode_input()).to(DEV)
    enc = ld.encode_first_stage(x)
    assert tuple(sp["original_image_size"]) == pu.ENC_SHAPE[2:]
    if kind == "kl":
        # a posterior of the blended moments (mean | logvar) comes back, and get_first_stage_encoding takes it
        assert isinstance(enc, DiagonalGaussianDistribution)
        got = enc.parameters
        z = ld.get_first_stage_encoding(enc, noise=torch.zeros(2, 4, 12, 12, device=DEV))
        assert torch.equal(z, ld.scale_factor * enc.mode())
    else:
        assert torch.is_tensor(enc)
        got = enc
        assert torch.equal(ld.get_first_stage_encoding(enc), ld.scale_factor * enc)
    assert got.shape == fx["enc_tiled"].shape
    check_parity(f"tiled {kind} encode vs reference", got, torch.from_numpy(fx["enc_tiled"]),
                 *pu.PARITY_LIMITS[f"tiled {kind} encode vs reference"])
    # the tiled encode is not the untiled one
    del ld.split_input_params
    whole = ld.encode_first_stage(x)
    whole = whole.parameters if kind == "kl" else whole
    assert float((got - whole).abs().max()) > 1e-3 * float(whole.abs().max())


def test_single_tile_is_the_untiled_encode(sdk):
    ld, _ = _ld(sdk, "vq", pu.split_params((24, 24), (8, 8), patch_distributed_vq=True, vqf=2))
    x = torch.from_numpy(pu.encode_input()).to(DEV)
    tiled = ld.encode_first_stage(x)
    del ld.split_input_params
    assert torch.equal(tiled, ld.encode_first_stage(x))


def test_full_tiled_chain(sdk):
    """encode (tiled, 24x24 -> 12x12) -> stochastic_encode -> DDIM decode with the patch-wise UNet (8x8 latent patches
    every 4) -> tiled first-stage decode, all under one split_input_params."""
    from sd_amd.DDIM.ddim import DDIMSampler
    sp = _sp()
    ld, _ = _ld(sdk, "kl", sp, unet="crossattn")
    d = pu.unet_inputs()
    ctx = torch.from_numpy(d["ctx"]).to(DEV)
    x = torch.from_numpy(pu.encode_input()).to(DEV)
    z0 = ld.get_first_stage_encoding(ld.encode_first_stage(x), noise=torch.zeros(2, 4, 12, 12, device=DEV))
    assert z0.shape == (2, 4, 12, 12)
    # the UNet and the decode tile the latent: ks / stride there are latent sizes
    ld.split_input_params = dict(sp, ks=pu.KS, stride=pu.STRIDE)
    s = DDIMSampler(ld)
    s.make_schedule(pu.DDIM_STEPS, ddim_eta=0.0, verbose=False)
    zt = s.stochastic_encode(z0, torch.full((2,), 2, device=DEV, dtype=torch.long),
                             noise=torch.from_numpy(d["xT"]).to(DEV))
    calls = []
    real = ld.model.diffusion_model.forward
    ld.model.diffusion_model.forward = lambda *a, **kw: (calls.append(kw.get("patches")), real(*a, **kw))[1]
    zd = s.decode(zt, ctx, 2)
    assert zd.shape == z0.shape and bool(zd.isfinite().all())
    assert calls and all(p is not None and p[:4] == (8, 8, 4, 4) for p in calls)          # every step ran patch-wise
    img = ld.decode_first_stage(zd)
    assert img.shape == pu.ENC_SHAPE and bool(img.isfinite().all())
