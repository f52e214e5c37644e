"""CPU tests of the condition encoders' boundary (clip_encoder/modules.py, clip_encoder/x_transformer.py): the new
C ABI symbols in the header / binding / INTEGRATION.md, state_dict layouts against the reference's
(tests/golden/make_golden_cond_stage.py), YAML targets, refused options and the local BERT tokenizer."""
import json
import os
import re

import pytest
import torch

import cond_util as cu
from golden_util import cfg_of, load
from synth import synth_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sdk_embedding_rows", "sdk_resize2d")


def test_new_symbols_in_header_binding_and_integration_table(sdk):
    from sd_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "sdk_amd.h")).read()
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % sym, header), sym
        assert sym in _lib.EXPORTS, sym
        assert re.search(r"^\| `%s` \|" % sym, table, re.M), sym
    assert "sdk_resize2d_args" in header and hasattr(_lib, "Resize2dArgs")
    for fn in ("embedding_rows", "resize2d"):
        assert callable(getattr(ops, fn))
    assert set(ops.RESIZE_MODES) == {"nearest", "bilinear", "bicubic", "area"}


def _keys(fx, name):
    return [(k, tuple(s)) for k, s in json.loads(bytes(fx[name]).decode())]


def _mirrors(sdk):
    from sd_amd.clip_encoder.modules import BERTEmbedder, TransformerEmbedder
    from sd_amd.clip_encoder.x_transformer import Encoder, TransformerWrapper
    return {"te": lambda: TransformerEmbedder(**cu.TE_CFG),
            "be": lambda: BERTEmbedder(use_tokenizer=False, **cu.BE_CFG),
            "glu": lambda: TransformerWrapper(num_tokens=cu.VOCAB, max_seq_len=77, attn_layers=Encoder(**cu.GLU_CFG))}


@pytest.mark.parametrize("name", ["te", "be", "glu"])
def test_transformer_state_dict_layout_equals_the_reference(sdk, name):
    fx = load("cond_transformer_tiny")
    m = _mirrors(sdk)[name]()
    ref = _keys(fx, name + "_keys")
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == ref
    pre = "" if name == "glu" else "transformer."
    for k in ("token_emb.weight", "pos_emb.emb.weight", "attn_layers.layers.0.0.weight",
              "attn_layers.layers.0.1.to_q.weight", "attn_layers.layers.0.1.to_out.bias",
              "attn_layers.layers.1.1.net.2.bias", "norm.bias", "to_logits.weight"):
        assert pre + k in dict(ref), k
    assert (pre + "attn_layers.layers.1.1.net.0.proj.weight" in dict(ref)) == (name == "glu")
    assert (pre + "attn_layers.layers.1.1.net.0.0.weight" in dict(ref)) == (name != "glu")
    w = synth_weights(ref, int(fx[name + "_seed"]))
    res = m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys


def test_class_and_rescaler_state_dict_layouts(sdk):
    from sd_amd.clip_encoder.modules import ClassEmbedder, SpatialRescaler
    fx = load("cond_class")
    m = ClassEmbedder(**cu.CLASS_CFG)
    assert m.key == "class"
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == _keys(fx, "keys")
    for case in cu.RESCALE_CASES:
        r = SpatialRescaler(n_stages=case[3], method=case[1], multiplier=case[2], in_channels=case[0][1],
                            out_channels=cu.MAPPER_OUT, bias=cu.mapper_bias(case))
        assert [(k, tuple(v.shape)) for k, v in r.state_dict().items()] == cu.mapper_keys(case)
    assert not SpatialRescaler().state_dict() and not SpatialRescaler().remap_output


COND_CONFIGS = {
    "ClassEmbedder": ({"embed_dim": 32, "n_classes": 10, "key": "class_label"}, "class_label", "crossattn"),
    "TransformerEmbedder": (dict(cu.TE_CFG), "caption", "crossattn"),
    "BERTTokenizer": ({"vq_interface": False, "max_length": 77}, "caption", "crossattn"),
    "BERTEmbedder": (dict(use_tokenizer=False, **cu.BE_CFG), "caption", "crossattn"),
    "SpatialRescaler": ({"n_stages": 2, "in_channels": 3, "out_channels": 4}, "segmentation", "concat"),
}


@pytest.mark.parametrize("cls", list(COND_CONFIGS))
def test_targets_resolve_and_latent_diffusion_constructs(sdk, cls):
    from sd_amd.Diffusion.ddpm import LatentDiffusion
    from sd_amd.Diffusion.utils import instantiate_from_config
    params, key, ckey = COND_CONFIGS[cls]
    cfg = {"target": "clip_encoder.modules." + cls, "params": params}
    m = instantiate_from_config(cfg)
    assert type(m).__module__ == "sd_amd.clip_encoder.modules" and type(m).__name__ == cls
    u, v = load("unet_tiny_ctx1"), load("vae_tiny")
    ucfg = cfg_of(u)
    if ckey == "concat":
        ucfg["in_channels"] = 8
    ld = LatentDiffusion(
        first_stage_config={"target": "VAE.autoencoder.AutoEncoderKL",
                            "params": {"ddconfig": cfg_of(v), "embed_dim": 4,
                                       "lossconfig": {"target": "torch.nn.Identity"}}},
        cond_stage_config=cfg, cond_stage_key=key, conditioning_key=ckey,
        unet_config={"target": "openai_model.model.UNetModel", "params": ucfg}, timesteps=6)
    assert type(ld.cond_stage_model) is type(m) and not ld.cond_stage_model.training
    assert all(not p.requires_grad for p in ld.cond_stage_model.parameters())
    assert any(k.startswith("cond_stage_model.") for k in ld.state_dict()) == bool(m.state_dict())


def test_abstract_encoder_keeps_encode(sdk):
    from sd_amd.clip_encoder.modules import AbstractEncoder
    with pytest.raises(NotImplementedError):
        AbstractEncoder().encode("x")


REFUSED_LAYERS = [("causal", True), ("cross_attend", True), ("only_cross", True), ("use_scalenorm", True),
                  ("use_rmsnorm", True), ("use_rezero", True), ("position_infused_attn", True),
                  ("custom_layers", ("a", "f")), ("sandwich_coef", 1), ("par_ratio", 2), ("residual_attn", True),
                  ("cross_residual_attn", True), ("macaron", True), ("pre_norm", False), ("gate_residual", True),
                  ("attn_talking_heads", True), ("attn_num_mem_kv", 2), ("attn_on_attn", True),
                  ("attn_sparse_topk", 4), ("attn_causal", True), ("attn_use_entmax15", True),
                  ("ff_dim_out", 32), ("rotary_pos_emb", True)]


@pytest.mark.parametrize("opt,val", REFUSED_LAYERS, ids=[o for o, _ in REFUSED_LAYERS])
def test_refused_attention_layer_options_name_the_option(sdk, opt, val):
    from sd_amd.clip_encoder.x_transformer import AttentionLayers
    with pytest.raises(NotImplementedError) as e:
        AttentionLayers(dim=64, depth=1, **{opt: val})
    assert opt.replace("attn_", "").replace("ff_", "") in str(e.value)


REFUSED_WRAPPER = [("emb_dim", 32), ("tie_embedding", True), ("num_memory_tokens", 2), ("use_pos_emb", False)]


@pytest.mark.parametrize("opt,val", REFUSED_WRAPPER, ids=[o for o, _ in REFUSED_WRAPPER])
def test_refused_wrapper_options_name_the_option(sdk, opt, val):
    from sd_amd.clip_encoder.x_transformer import Encoder, TransformerWrapper
    with pytest.raises(NotImplementedError) as e:
        TransformerWrapper(num_tokens=10, max_seq_len=8, attn_layers=Encoder(dim=64, depth=1), **{opt: val})
    assert opt in str(e.value)


def test_encoder_rejects_causal_and_accepts_the_supported_kwargs(sdk):
    from sd_amd.clip_encoder.x_transformer import Encoder, TransformerWrapper
    with pytest.raises(AssertionError):
        Encoder(dim=64, depth=1, causal=False)
    enc = Encoder(dim=64, depth=2, heads=4, attn_dim_head=32, ff_mult=2, ff_glu=True, attn_dropout=0.1,
                  ff_dropout=0.1)
    assert enc.layers[0][1].to_q.weight.shape == (4 * 32, 64)            # inner width independent of dim
    assert enc.layers[1][1].net[0].proj.weight.shape == (2 * 2 * 64, 64)
    TransformerWrapper(num_tokens=10, max_seq_len=8, attn_layers=enc, emb_dropout=0.1)
    assert Encoder(dim=128, depth=1).layers[0][1].to_out.weight.shape == (128, 8 * 64)


FORWARD_REFUSED = [("mask", lambda: torch.ones(1, 4, dtype=torch.bool)), ("mems", lambda: [None]),
                   ("return_attn", lambda: True), ("return_mems", lambda: True), ("context", lambda: torch.zeros(1))]


@pytest.mark.parametrize("opt,val", FORWARD_REFUSED, ids=[o for o, _ in FORWARD_REFUSED])
def test_refused_call_options_name_the_option(sdk, opt, val):
    from sd_amd.clip_encoder.x_transformer import Encoder, TransformerWrapper
    m = TransformerWrapper(num_tokens=10, max_seq_len=8, attn_layers=Encoder(dim=64, depth=1))
    ids = torch.zeros(1, 4, dtype=torch.long)
    with pytest.raises(NotImplementedError) as e:
        m(ids, return_embeddings=True, **{opt: val()})
    assert opt in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        m(ids)
    assert "return_embeddings" in str(e.value)


def test_cpu_inputs_raise_type_error(sdk):
    from sd_amd import ops
    from sd_amd.clip_encoder.modules import BERTEmbedder, ClassEmbedder, SpatialRescaler, TransformerEmbedder
    ids = torch.zeros(1, 4, dtype=torch.long)
    for m in (BERTEmbedder(use_tokenizer=False, **cu.BE_CFG), TransformerEmbedder(device="cpu", **cu.TE_CFG)):
        with pytest.raises(TypeError, match="HIP path only"):
            m.encode(ids)
        with pytest.raises(TypeError, match="HIP path only"):
            m.transformer(ids, return_embeddings=True)
    with pytest.raises(TypeError, match="token ids"):
        BERTEmbedder(use_tokenizer=False, **cu.BE_CFG)("a prompt")
    with pytest.raises(TypeError, match="HIP path only"):
        ClassEmbedder(8, 4)({"class": torch.zeros(2, dtype=torch.long)})
    with pytest.raises(TypeError, match="HIP path only"):
        SpatialRescaler()(torch.zeros(1, 3, 4, 4))
    with pytest.raises(TypeError):
        ops.resize2d(torch.zeros(1, 3, 4, 4), 0.5)
    with pytest.raises(TypeError):
        ops.embedding_rows(torch.zeros(2, dtype=torch.long), torch.zeros(4, 8))


def test_spatial_rescaler_methods(sdk):
    from sd_amd.clip_encoder.modules import SpatialRescaler
    x = torch.zeros(1, 3, 4, 4)
    for method in ("linear", "trilinear"):
        with pytest.raises(NotImplementedError, match=method):
            SpatialRescaler(method=method)(x)
        with pytest.raises((NotImplementedError, ValueError)):      # torch refuses the same call
            torch.nn.functional.interpolate(x, scale_factor=0.5, mode=method)
    with pytest.raises(AssertionError):
        SpatialRescaler(method="lanczos")
    with pytest.raises(AssertionError):
        SpatialRescaler(n_stages=-1)
    with pytest.raises(ValueError):
        SpatialRescaler()(torch.zeros(3, 4, 4))


WORDS = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "a", "photo", "of", "cat", "the", "dog", "##s", "red", "."]


def test_bert_tokenizer_from_a_local_vocab(sdk, tmp_path):
    from transformers import BertTokenizerFast
    from sd_amd.clip_encoder.modules import BERTEmbedder, BERTTokenizer
    (tmp_path / "vocab.txt").write_text("\n".join(WORDS) + "\n")
    ref = BertTokenizerFast.from_pretrained(str(tmp_path), local_files_only=True)
    text = ["a photo of the red cats.", "the dog", "unknownword a"]
    want = ref(text, truncation=True, max_length=12, padding="max_length", return_tensors="pt")["input_ids"]
    # WordPiece by hand: [CLS] a photo of the red cat ##s . [SEP] [PAD] [PAD]
    ix = WORDS.index
    assert want[0].tolist() == [ix(w) for w in ("[CLS]", "a", "photo", "of", "the", "red", "cat", "##s", ".",
                                                  "[SEP]", "[PAD]", "[PAD]")]
    tk = BERTTokenizer(device="cpu", vq_interface=False, max_length=12, version=str(tmp_path))
    got = tk(text)
    assert got.dtype == torch.int64 and torch.equal(got, want)
    assert int(got[0, 0]) == WORDS.index("[CLS]") and WORDS.index("##s") in got[0].tolist()
    assert WORDS.index("[UNK]") in got[2].tolist() and int(got[1, -1]) == WORDS.index("[PAD]")
    assert torch.equal(tk.encode(text), want) and tk.decode("x") == "x"
    vq = BERTTokenizer(device="cpu", vq_interface=True, max_length=12, version=str(tmp_path)).encode(text)
    assert vq[0] is None and vq[1] is None and vq[2][:2] == [None, None] and torch.equal(vq[2][2], want)
    be = BERTEmbedder(n_embed=64, n_layer=1, vocab_size=len(WORDS), max_seq_len=12, device="cpu",
                      tokenizer_version=str(tmp_path))
    assert torch.equal(be.tknz_fn(text), want)


def test_bert_tokenizer_without_a_local_vocab_raises_on_text(sdk, tmp_path):
    from sd_amd.clip_encoder.modules import BERTEmbedder, BERTTokenizer
    for version in (None, "bert-base-uncased", str(tmp_path)):
        tk = BERTTokenizer(version=version)
        assert tk.tokenizer is None
        with pytest.raises(RuntimeError, match="no local tokenizer"):
            tk("a photo")
    with pytest.raises(RuntimeError, match="no local tokenizer"):
        BERTEmbedder(n_embed=64, n_layer=1)("a photo")
