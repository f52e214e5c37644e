"""CPU tests of the SD-2.x boundary: open_clip's token layout (``openclip_pad``), the FrozenOpenCLIPEmbedder
state_dict against the SD-2 checkpoints' ``cond_stage_model.model.*`` table, ``hidden_act`` of the transformers-layout
tower, ``use_linear_in_transformer`` and configs/sd-v2-inference-v.yaml.  Everything is built on the meta device or at
tiny sizes; nothing runs a kernel."""
import os

import pytest
import torch

import openclip_util as ou
from golden_util import cfg_of, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOT, EOT = 49406, 49407
# 12 tensors per block; the positional and token tables, ln_final (2), text_projection, logit_scale
N_VIT_H = 24 * 12 + 6


@pytest.mark.parametrize("n", [0, 5, 75, 200])
def test_openclip_pad_layout(sdk, n):
    """An empty prompt, one that fits, one of exactly 75 tokens (fills the row) and one of 200 (truncated)."""
    from sd_amd.clip_encoder.modules import openclip_pad
    toks = [list(range(1000, 1000 + n)), [7, 8, 9]]
    ids = openclip_pad(toks, 77, SOT, EOT)
    assert ids.shape == (2, 77) and ids.dtype == torch.int64
    row = ids[0].tolist()
    kept = min(n, 75)
    assert row[0] == SOT
    assert row[1:1 + kept] == toks[0][:kept]
    assert row[1 + kept] == EOT
    assert all(v == 0 for v in row[2 + kept:]) and len(row) == 77
    if n >= 75:
        assert row[-1] == EOT and 0 not in row
    assert ids[1].tolist() == [SOT, 7, 8, 9, EOT] + [0] * 72       # padded with 0, not with EOT


def test_openclip_pad_other_context(sdk):
    from sd_amd.clip_encoder.modules import openclip_pad
    assert openclip_pad([[1, 2, 3, 4, 5, 6]], 5, 100, 101).tolist() == [[100, 1, 2, 3, 101]]
    assert openclip_pad([[]], 4, 100, 101).tolist() == [[100, 101, 0, 0]]


def test_openclip_state_dict_is_the_checkpoint_table(sdk):
    from sd_amd.clip_encoder.modules import FrozenOpenCLIPEmbedder
    with torch.device("meta"):
        m = FrozenOpenCLIPEmbedder()
    want = ou.openclip_keys(ou.VIT_H14)
    assert len(want) == N_VIT_H
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == want
    assert m.LAYERS == ["last", "penultimate"] and m.layer == "last" and m.layer_idx == 0
    assert all(not p.requires_grad for p in m.parameters())
    res = m.load_state_dict({k: torch.empty(s, device="meta") for k, s in want}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    with torch.device("meta"):
        assert FrozenOpenCLIPEmbedder(layer="penultimate").layer_idx == 1
        # all blocks are held even when one fewer runs
        assert len(FrozenOpenCLIPEmbedder(layer="penultimate").state_dict()) == N_VIT_H


def test_openclip_refusals(sdk):
    from sd_amd.clip_encoder.modules import FrozenOpenCLIPEmbedder
    with torch.device("meta"):
        with pytest.raises((AssertionError, ValueError), match="pooled"):
            FrozenOpenCLIPEmbedder(layer="pooled")
        with pytest.raises(NotImplementedError, match="ViT-bigG-14"):
            FrozenOpenCLIPEmbedder(arch="ViT-bigG-14")
        m = FrozenOpenCLIPEmbedder(arch="tiny", config=ou.TINY, layer="penultimate")
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == ou.openclip_keys(ou.TINY)
    with pytest.raises(RuntimeError, match="tokenizer"):
        m(["a prompt"])


def test_openclip_weights_helper_matches_the_table():
    w = ou.openclip_weights(ou.TINY, 5)
    assert [(k, tuple(v.shape)) for k, v in w.items()] == ou.openclip_keys(ou.TINY)
    # the bare parameters are scaled like a Linear's, not unit normals
    assert w["model.transformer.resblocks.0.attn.in_proj_weight"].abs().max() < 0.2
    ids = ou.seeded_ids(ou.TINY, 6)
    assert ids[0, 0] == ou.SOT and ids[0, 9] == ou.EOT and not ids[0, 10:].any() and ids[1, 40] == ou.EOT


@pytest.mark.parametrize("act,ok", [("quick_gelu", True), ("gelu", True), ("tanh", False)])
def test_clip_hidden_act_is_honoured_or_refused(sdk, act, ok):
    from sd_amd import ops
    from sd_amd.clip_encoder.modules import VIT_L14_TEXT, FrozenCLIPEmbedder
    cfg = dict(VIT_L14_TEXT, num_hidden_layers=1, hidden_act=act)
    with torch.device("meta"):
        if not ok:
            with pytest.raises(NotImplementedError, match="tanh"):
                FrozenCLIPEmbedder(config=cfg)
            return
        m = FrozenCLIPEmbedder(config=cfg)
    want = {"quick_gelu": ops.ACT_QUICK_GELU, "gelu": ops.ACT_GELU}[act]
    assert m.transformer.text_model.encoder.layers[0]._act == want
    assert (ops.ACT_NONE, ops.ACT_QUICK_GELU, ops.ACT_GELU) == (0, 1, 2)


def test_act_gelu_in_header_and_docs():
    header = open(os.path.join(ROOT, "include", "sdk_amd.h")).read()
    assert "SDK_ACT_QUICK_GELU = 1," in header and "SDK_ACT_GELU = 2" in header
    assert "SDK_ACT_GELU" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _shapes(m):
    return [(k, tuple(v.shape)) for k, v in m.state_dict().items()]


def test_use_linear_in_transformer_changes_only_the_projection_shapes(sdk):
    from sd_amd.openai_model.model import UNetModel
    z = load("unet_tiny")
    cfg = cfg_of(z)
    ref_keys = [(k, tuple(s)) for k, s in __import__("json").loads(bytes(z["keys"]).decode())]
    with torch.device("meta"):
        conv = _shapes(UNetModel(**cfg))
        conv_explicit = _shapes(UNetModel(**cfg, use_linear_in_transformer=False))
        lin = _shapes(UNetModel(**cfg, use_linear_in_transformer=True))
    assert conv == ref_keys == conv_explicit             # the default build is unchanged
    assert [k for k, _ in lin] == [k for k, _ in conv]
    n_proj = 0
    for (k, s_lin), (_, s_conv) in zip(lin, conv):
        if k.endswith(("proj_in.weight", "proj_out.weight")) and "transformer_blocks" not in k:
            n_proj += 1
            assert len(s_conv) == 4 and s_conv[2:] == (1, 1)
            assert s_lin == s_conv[:2], k                # 2-D, the same [out, in]
        else:
            assert s_lin == s_conv, k
    assert n_proj >= 2


def test_sd2_yaml_instantiates(sdk):
    """configs/sd-v2-inference-v.yaml: v-prediction LatentDiffusion, ViT-H OpenCLIP cond stage (penultimate), a UNet
    with 2-D projection weights, 64-channel heads and a 1024-wide context."""
    import yaml
    from sd_amd.Diffusion.utils import instantiate_from_config
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "sd-v2-inference-v.yaml")))
    with torch.device("meta"):
        ld = instantiate_from_config(cfg["model"])
    assert ld.parameterization == "v" and ld.scale_factor == 0.18215
    assert (ld.linear_start, ld.linear_end) == (0.00085, 0.0120)
    cs = ld.cond_stage_model
    assert type(cs).__name__ == "FrozenOpenCLIPEmbedder" and type(cs).__module__ == "sd_amd.clip_encoder.modules"
    assert cs.layer == "penultimate" and len(cs.state_dict()) == N_VIT_H
    unet = ld.model.diffusion_model
    proj = [(k, v) for k, v in unet.state_dict().items()
            if k.endswith(("proj_in.weight", "proj_out.weight")) and "transformer_blocks" not in k]
    assert len(proj) == 32 and all(v.dim() == 2 for _, v in proj)
    assert unet.state_dict()["input_blocks.1.1.transformer_blocks.0.attn2.to_k.weight"].shape == (320, 1024)
    assert unet.dtype == torch.float16
    # the SD-2 checkpoint layout: every key of the three stages under its prefix, loaded strictly
    full = ld.state_dict()
    assert [k for k in full if k.startswith("cond_stage_model.")] == [
        "cond_stage_model." + k for k, _ in ou.openclip_keys(ou.VIT_H14)]
    assert all(k.split(".")[0] in ("model", "first_stage_model", "cond_stage_model") or v.device.type == "cpu"
               for k, v in full.items())                 # the rest: the schedule's host buffers
    synthetic = {k: torch.zeros_like(v) for k, v in full.items()}
    res = ld.load_state_dict(synthetic, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
