"""The packed-weight lifecycle on the MI355X (run with -m gpu): a model that has already run picks up a checkpoint
loaded through a plain parent module.  Per model: A loads the fixture weights before its first run → ``y_ref``;
B runs once on other weights, then the fixture weights are loaded THROUGH ``nn.ModuleDict({"model": B})`` with
prefixed keys, and B runs again.  Same process, same plans: the bits are ``y_ref``'s."""
import json

import pytest
import torch
from torch import nn

import cond_util as cu
from golden_util import cfg_of, load, weights_of
from synth import synth_weights

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _gpu(a):
    return torch.from_numpy(a).to(DEV)


def _other_weights(sd, seed):
    """Seeded weights of the same layout that are not the fixture's."""
    w = synth_weights([(k, tuple(v.shape)) for k, v in sd.items()], seed)
    return {k: torch.from_numpy(v) for k, v in w.items()}


def _unet(sdk):
    from sd_amd.openai_model.model import UNetModel
    z = load("unet_tiny")
    x, t, ctx = _gpu(z["x"]), _gpu(z["t"]), _gpu(z["ctx"])
    return (lambda: UNetModel(**cfg_of(z))), weights_of(z), (lambda m: (m(x, t, ctx),))


def _vae(sdk):
    from sd_amd.VAE.autoencoder import AutoEncoderKL
    z = load("vae_tiny")
    lat, img, scale = _gpu(z["z"]), _gpu(z["dec"]), 1.0 / float(z["scale_factor"])
    return (lambda: AutoEncoderKL(ddconfig=cfg_of(z), embed_dim=4)), weights_of(z), \
        (lambda m: (m.encode(img).parameters, m.decode(lat, pre_scale=scale)))


def _vq(sdk):
    from sd_amd.vqvae.autoencoder import VQModel
    z = load("vq_model")
    kw = dict(ddconfig=cfg_of(z), n_embed=64, embed_dim=3, lossconfig={"target": "torch.nn.Identity"})
    x = _gpu(z["x"])

    def run(m):
        quant, _, (_, _, idx) = m.encode(x)
        return quant, idx, m.decode(quant)

    return (lambda: VQModel(**kw).to(DEV)), weights_of(z), run


def _ddpm(sdk):
    from sd_amd.DDPM.models.unet import UNet
    z = load("ddpm_unet")
    x, t = _gpu(z["x"]), _gpu(z["t"])
    return (lambda: UNet(input_channels=3)), weights_of(z), (lambda m: (m(x, t),))


def _clip(sdk):
    from sd_amd.clip_encoder.modules import FrozenCLIPEmbedder
    z = load("clip_tiny")
    cfg = json.loads(bytes(z["cfg"]).decode())
    # the module tree's own keys (CLIPTextModel.load_state_dict adds the prefix only when called directly)
    sd = {"transformer." + (k if k.startswith("text_model.") else "text_model." + k): v
          for k, v in weights_of(z).items() if not k.endswith("position_ids")}
    ids = torch.from_numpy(z["ids"])
    return (lambda: FrozenCLIPEmbedder(device=DEV, config=cfg)), sd, (lambda m: (m.encode_tokens(ids),))


def _wrapper(sdk):
    from sd_amd.clip_encoder.x_transformer import Encoder, TransformerWrapper
    fx = load("cond_transformer_tiny")
    ks = [(k, tuple(s)) for k, s in json.loads(bytes(fx["glu_keys"]).decode())]
    sd = {k: torch.from_numpy(v) for k, v in synth_weights(ks, int(fx["glu_seed"])).items()}
    ids = _gpu(cu.case_ids("glu", 77))
    make = lambda: TransformerWrapper(num_tokens=cu.VOCAB, max_seq_len=77, attn_layers=Encoder(**cu.GLU_CFG)).to(DEV)  # noqa: E731
    return make, sd, (lambda m: (m(ids, return_embeddings=True),))


CASES = {"UNetModel": _unet, "AutoEncoderKL": _vae, "VQModel": _vq, "DDPM_UNet": _ddpm, "FrozenCLIPEmbedder": _clip,
         "TransformerWrapper": _wrapper}


def _loaded(make, sd):
    a = make()
    a.load_state_dict(sd)
    return a


def _load_through_parent(model, sd):
    parent = nn.ModuleDict({"model": model})
    parent.load_state_dict({"model." + k: v for k, v in sd.items()})


def _same(got, ref):
    return len(got) == len(ref) and all(torch.equal(g, r) for g, r in zip(got, ref))


@pytest.mark.parametrize("name", sorted(CASES))
def test_load_through_a_parent_after_a_run_replaces_the_packs(sdk, name):
    make, sd, run = CASES[name](sdk)
    y_ref = run(_loaded(make, sd))
    b = make()
    b.load_state_dict(_other_weights(sd, 4242))
    first = run(b)
    assert not _same(first, y_ref), "the other weights must give another output"
    _load_through_parent(b, sd)
    assert _same(run(b), y_ref)


def test_graphed_unet_drops_its_graph_on_a_parent_load(sdk):
    from sd_amd.graphs import GraphedUNet
    make, sd, _ = _unet(sdk)
    z = load("unet_tiny")
    x, t, ctx = _gpu(z["x"]), _gpu(z["t"]), _gpu(z["ctx"])
    y_ref = _loaded(make, sd)(x, t, ctx)
    b = make()
    b.load_state_dict(_other_weights(sd, 4242))
    g = GraphedUNet(b)
    first = g(x, t, ctx)
    assert len(g.graphs) == 1 and not torch.equal(first, y_ref)
    _load_through_parent(b, sd)
    assert torch.equal(g(x, t, ctx), y_ref)
