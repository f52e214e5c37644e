"""CPU tests of the VQ first stage's drop-in boundary: config resolution, constructor kwargs and
state_dict keys against lists captured from the reference (tests/golden/make_golden_vq.py), and the
sampler's errors around ``quantize_denoised``."""
import inspect
import json

import numpy as np
import pytest
import torch

from golden_util import cfg_of, load


def _meta():
    return json.loads(bytes(load("vq_remap")["meta"]).decode())


def _sampler(first_stage):
    from sd_amd.DDIM.ddim import DDIMSampler
    from sd_amd.DDIM.diffusion_modules import register_schedule
    sch = register_schedule(1000, 0.00085, 0.012)

    class M:
        num_timesteps = 1000
        alphas_cumprod = sch["alphas_cumprod"]
        device = torch.device("cpu")
        parameterization = "eps"
        first_stage_model = first_stage

        def apply_model(self, x, t, c):
            raise AssertionError("the model must not be called")

    return DDIMSampler(M())


def test_vq_targets_resolve_through_instantiate_from_config(sdk):
    from sd_amd.Diffusion.utils import instantiate_from_config
    from sd_amd.vqvae.autoencoder import VQModel, VQModelInterface
    from sd_amd.vqvae.quantize import VectorQuantize2
    q = instantiate_from_config({"target": "vqvae.quantize.VectorQuantize2",
                                 "params": {"n_e": 16, "e_dim": 3, "beta": 0.25}})
    assert type(q) is VectorQuantize2 and tuple(q.embedding.weight.shape) == (16, 3)
    z = load("vq_model")
    m = instantiate_from_config({"target": "vqvae.autoencoder.VQModelInterface",
                                 "params": {"ddconfig": cfg_of(z), "n_embed": 64, "embed_dim": 3,
                                            "lossconfig": {"target": "torch.nn.Identity"}}})
    assert type(m) is VQModelInterface and isinstance(m, VQModel) and type(m.quantize) is VectorQuantize2
    assert m.quant_conv.weight.shape == (3, 4, 1, 1) and m.post_quant_conv.weight.shape == (4, 3, 1, 1)


def test_vq_state_dict_keys_and_kwargs_equal_the_reference(sdk, tmp_path):
    from sd_amd.vqvae.autoencoder import VQModel, VQModelInterface
    from sd_amd.vqvae.quantize import VectorQuantize2
    meta = _meta()
    names = lambda f: list(inspect.signature(f).parameters)[1:]      # noqa: E731
    assert names(VectorQuantize2.__init__) == meta["vq_kwargs"]
    assert names(VQModel.__init__) == meta["vqmodel_kwargs"]
    assert names(VQModelInterface.__init__) == meta["vqinterface_kwargs"]
    assert list(VectorQuantize2(8, 2, 0.25).state_dict().keys()) == meta["vq_keys"]
    path = str(tmp_path / "used.npy")
    np.save(path, load("vq_remap")["used"])
    q = VectorQuantize2(64, 2, 0.25, remap=path, unknown_index="extra")
    assert list(q.state_dict().keys()) == meta["vq_remap_keys"]
    assert q.re_embed == 6 and q.unknown_index == 5
    z = load("vq_model")
    ref_keys = json.loads(bytes(z["keys"]).decode())
    for cls in (VQModel, VQModelInterface):
        m = cls(ddconfig=cfg_of(z), n_embed=64, embed_dim=3, lossconfig=None)
        assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == ref_keys


def test_quantize_denoised_without_a_quantizer_raises_a_clear_error(sdk):
    class KLStage:
        pass

    s = _sampler(KLStage())
    with pytest.raises(AttributeError, match="VQ first stage"):
        s.sample(S=4, batch_size=1, shape=(4, 8, 8), quantize_x0=True, verbose=False)
    s.make_schedule(4, verbose=False)
    with pytest.raises(AttributeError, match="VQ first stage"):
        s.ddim_sampling(None, (1, 4, 8, 8), quantize_denoised=True)


def test_masking_and_friends_still_raise_not_implemented(sdk):
    s = _sampler(None)
    s.make_schedule(4, verbose=False)
    with pytest.raises(NotImplementedError):
        s.ddim_sampling(None, (1, 4, 8, 8), mask=torch.ones(1, 1, 8, 8), x0=torch.zeros(1, 4, 8, 8))
    with pytest.raises(NotImplementedError):
        s.ddim_sampling(None, (1, 4, 8, 8), score_corrector=object())
    with pytest.raises(NotImplementedError):
        s.ddim_sampling(None, (1, 4, 8, 8), noise_dropout=0.1)
    with pytest.raises(NotImplementedError):
        s.ddim_sampling(None, (1, 4, 8, 8), ddim_use_original_steps=True)
