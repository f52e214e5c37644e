"""The packed-weight lifecycle (sd_amd.packing.PackedOwner) on the host: when an owner's packs are dropped and
rebuilt.  The stub owner's packing code only counts calls; no GPU, no library call."""
import json

import pytest
import torch
from torch import nn

import cond_util as cu
from golden_util import cfg_of, load


@pytest.fixture(scope="module")
def Stub(sdk):
    from sd_amd.packing import PackedOwner

    class Stub(PackedOwner, nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = nn.Linear(3, 2)
            self.packs, self.dropped = [], 0

        def _pack(self, *key, **extra):
            self.packs.append((key, extra))

        def _packs_dropped(self):
            self.dropped += 1

    return Stub


def _packed(stub):
    stub.ensure_packed("dev0", 8)
    assert stub._packed_key == ("dev0", 8)
    return stub.prepare_generation, len(stub.packs), stub.dropped


def test_direct_load_invalidates(Stub):
    m = Stub()
    gen, n, dropped = _packed(m)
    m.load_state_dict(Stub().state_dict())
    assert m._packed_key is None and m.dropped == dropped + 1
    m.ensure_packed("dev0", 8)
    assert len(m.packs) == n + 1


@pytest.mark.parametrize("depth", [1, 2], ids=["parent", "grandparent"])
def test_load_through_plain_ancestors_invalidates(Stub, depth):
    m = Stub()
    root, prefix = nn.ModuleDict({"child": m}), "child."
    for _ in range(depth - 1):
        root, prefix = nn.ModuleDict({"mid": root}), "mid." + prefix
    gen, n, dropped = _packed(m)
    root.load_state_dict({prefix + k: v for k, v in Stub().state_dict().items()})
    assert m._packed_key is None and m.dropped == dropped + 1
    m.ensure_packed("dev0", 8)
    assert len(m.packs) == n + 1


def test_generation_moves_at_the_load_not_at_the_next_ensure(Stub):
    m = Stub()
    gen, n, _ = _packed(m)
    nn.ModuleDict({"child": m}).load_state_dict({"child." + k: v for k, v in Stub().state_dict().items()})
    assert m.prepare_generation > gen and len(m.packs) == n       # nothing ran in between
    at_load = m.prepare_generation
    m.ensure_packed("dev0", 8)
    assert m.prepare_generation > at_load                          # new packs are a new generation too


def test_unchanged_key_does_not_repack_a_changed_key_does(Stub):
    m = Stub()
    gen, n, _ = _packed(m)
    m.ensure_packed("dev0", 8)
    assert (m.prepare_generation, len(m.packs)) == (gen, n)
    m.ensure_packed("dev0", 16, extra=1)
    assert len(m.packs) == n + 1 and m.packs[-1] == (("dev0", 16), {"extra": 1}) and m._packed_key == ("dev0", 16)
    m.ensure_packed("dev1", 16)
    assert len(m.packs) == n + 2
    m.repack("dev1", 16)                                           # the public prepare(): unconditional
    assert len(m.packs) == n + 3 and m._packed_key == ("dev1", 16)


def test_mixin_adds_no_state(Stub):
    m, plain = Stub(), nn.Sequential()
    plain.lin = nn.Linear(3, 2)
    _packed(m)
    assert list(m.state_dict()) == list(plain.state_dict()) == ["lin.weight", "lin.bias"]
    assert [k for k, _ in m.named_parameters()] == [k for k, _ in plain.named_parameters()]
    assert [k for k, _ in m.named_modules()] == [k for k, _ in plain.named_modules()]
    assert not list(m.named_buffers())


def _owners(sdk):
    from sd_amd.clip_encoder.modules import FrozenCLIPEmbedder, TransformerEmbedder
    from sd_amd.DDPM.models.unet import UNet
    from sd_amd.openai_model.model import UNetModel
    from sd_amd.VAE.autoencoder import AutoEncoderKL
    from sd_amd.vqvae.autoencoder import VQModel, VQModelInterface
    vq = load("vq_model")
    vqkw = dict(ddconfig=cfg_of(vq), n_embed=64, embed_dim=3, lossconfig={"target": "torch.nn.Identity"})
    vae, vqm = AutoEncoderKL(ddconfig=cfg_of(load("vae_tiny")), embed_dim=4), VQModel(**vqkw)
    clip = FrozenCLIPEmbedder(device="cpu", config=json.loads(bytes(load("clip_tiny")["cfg"]).decode()))
    with torch.device("meta"):
        ddpm = UNet(input_channels=3)
    return {"UNetModel": UNetModel(**cfg_of(load("unet_tiny"))), "AutoEncoderKL": vae, "Encoder": vae.encoder,
            "Decoder": vae.decoder, "VQModel": vqm, "VQModelInterface": VQModelInterface(**vqkw),
            "VectorQuantizer": vqm.quantize, "DDPM UNet": ddpm, "CLIP text model": clip.transformer.text_model,
            "TransformerWrapper": TransformerEmbedder(**cu.TE_CFG).transformer}


def test_every_real_owner_uses_the_mixin_and_drops_its_key_on_a_parent_load(sdk):
    from sd_amd.packing import PackedOwner
    for name, m in _owners(sdk).items():
        assert isinstance(m, PackedOwner), name
        assert m._packed_key is None and "_packed_key" not in m.state_dict(), name
        if name == "DDPM UNet":                                    # built on the meta device: nothing to load
            continue
        gen = m.prepare_generation
        m._packed_key = ("stale",)
        parent = nn.ModuleDict({"model": m})
        parent.load_state_dict(parent.state_dict())
        assert m._packed_key is None and m.prepare_generation > gen, name


def test_unet_drops_its_context_cache_with_its_packs(sdk):
    from sd_amd.openai_model.model import UNetModel
    m = UNetModel(**cfg_of(load("unet_tiny")))
    m._ctx_cache = {"stale": None}
    nn.ModuleDict({"model": m}).load_state_dict({"model." + k: v for k, v in m.state_dict().items()})
    assert m._ctx_cache is None
