"""CPU checks of the first-stage attention surface: state_dict key lists and shapes of AttentionBlock /
LinearAttention / LinearAttentionBlock against the reference's (recorded in the fixtures), the new symbols in the
header, the binding and the INTEGRATION.md table, ``make_attention``'s dispatch and the C > 512 refusal."""
import json
import os
import re

import pytest
import torch

import first_stage_attn_util as fu
from golden_util import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sdk_linear_attention", "sdk_linear_attention_workspace_bytes", "sdk_linear_attention_chunks")


def _keys(z, name="keys"):
    return [(k, tuple(s)) for k, s in json.loads(bytes(z[name]).decode())]


@pytest.mark.parametrize("name", list(fu.BLOCK_CASES))
def test_block_keys_and_shapes_equal_the_reference(sdk, name):
    from sd_amd.Unet import attention as A
    kind, args, _, _ = fu.BLOCK_CASES[name]
    cls = {"single": A.AttentionBlock, "flash": A.FlashAttentionBlock, "linear_block": A.LinearAttentionBlock,
           "linear": A.LinearAttention}[kind]
    ours = [(k, tuple(v.shape)) for k, v in cls(*args).state_dict().items()]
    assert ours == _keys(load("fsa_" + name))


def test_single_head_and_flash_share_their_keys(sdk):
    """Why a CompVis checkpoint loads into the 8-head block without complaint: the same keys; the two differ in
    eps, heads and scale only."""
    from sd_amd.Unet import attention as A
    a, f = A.AttentionBlock(64), A.FlashAttentionBlock(64)
    assert list(a.state_dict()) == list(f.state_dict())
    assert a.norm.eps == 1e-6 and f.norm.eps == 1e-5 and a.norm.num_groups == 32
    lin = A.LinearAttention(64)
    assert (lin.heads, lin.dim_head) == (4, 32) and lin.to_qkv.bias is None and lin.to_out.bias is not None
    assert tuple(lin.to_qkv.weight.shape) == (384, 64, 1, 1) and tuple(lin.to_out.weight.shape) == (64, 128, 1, 1)
    blk = A.LinearAttentionBlock(192)
    assert (blk.heads, blk.dim_head) == (1, 192) and not hasattr(blk, "norm")


@pytest.mark.parametrize("attn", fu.MODEL_ATTN)
def test_tiny_model_keys_equal_the_reference(sdk, attn):
    from sd_amd.Encoder_Decoder.encoder import Decoder, Encoder
    from sd_amd.VAE.autoencoder import AutoEncoderKL
    from sd_amd.Unet import attention as A
    z = load("fsa_model_" + attn)
    cfg = dict(json.loads(bytes(z["cfg"]).decode()), attn_type=attn)
    enc, dec, vae = Encoder(**cfg), Decoder(**cfg), AutoEncoderKL(ddconfig=cfg, embed_dim=4)
    for tag, m in (("enc", enc), ("dec", dec), ("vae", vae)):
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == _keys(z, f"{attn}_{tag}_keys"), tag
    want = {"linear": A.LinearAttentionBlock, "single_head": A.AttentionBlock, "vanilla": A.FlashAttentionBlock}[attn]
    for blk in (enc.mid.attn_1, enc.down[1].attn[0], dec.mid.attn_1, dec.up[1].attn[0], dec.up[1].attn[1],
                vae.encoder.mid.attn_1, vae.decoder.mid.attn_1):
        assert type(blk) is want
    lin = Encoder(**dict(cfg, attn_type="vanilla", use_linear_attn=True))
    assert type(lin.mid.attn_1) is A.LinearAttentionBlock


def test_make_attention_dispatch(sdk):
    from sd_amd.Unet import attention as A
    assert type(A.make_attention(64)) is A.FlashAttentionBlock
    assert type(A.make_attention(64, "vanilla")) is A.FlashAttentionBlock
    assert type(A.make_attention(64, "single_head")) is A.AttentionBlock
    assert type(A.make_attention(64, "linear")) is A.LinearAttentionBlock
    assert type(A.make_attention(64, "none")) is torch.nn.Identity
    with pytest.raises(AssertionError, match="not found"):
        A.make_attention(64, "flash")


def test_more_than_512_channels_is_refused(sdk):
    from sd_amd.Unet import attention as A
    A.AttentionBlock(512)
    with pytest.raises(NotImplementedError, match="512"):
        A.AttentionBlock(544)
    with pytest.raises(NotImplementedError, match="512"):
        A.make_attention(1024, "single_head")
    with pytest.raises(NotImplementedError, match="512"):
        A.LinearAttentionBlock(544)


def test_new_symbols_in_header_binding_and_integration_table(sdk):
    from sd_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "sdk_amd.h")).read()
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\bint(32_t|64_t)? %s\(" % sym, header), sym
        assert sym in _lib.EXPORTS, sym
        assert re.search(r"^\| `%s` \|" % sym, table, re.M), sym
    assert re.search(r"^\| `sdk_attention_form` with `SDK_ATTN_WIDE` \|", table, re.M)
    assert "sdk_linear_attention_args" in header and hasattr(_lib, "LinearAttentionArgs")
    m = re.search(r"enum \{([^}]*SDK_ATTN_WIDE[^}]*)\}", header)
    names = [n.strip().split(" ")[0] for n in m.group(1).split(",")]
    assert names.index("SDK_ATTN_WIDE") == _lib.ATTN_WIDE == ops.ATTN_FORMS["wide"]
    rows = int(re.search(r"#define SDK_ATTN_WIDE_ROWS (\d+)", header).group(1))
    kt = int(re.search(r"#define SDK_ATTN_WIDE_KT (\d+)", header).group(1))
    assert (ops.ATTN_WIDE_ROWS, ops.ATTN_WIDE_KT) == (rows, kt)
    import attn_wide_util as W
    assert (W.ROWS, W.KT) == (rows, kt)
    assert callable(ops.linear_attention)


def test_fixture_sizes():
    """No fixture of this suite outgrows the earlier suites' largest (cond_transformer_tiny.npz)."""
    g = os.path.join(ROOT, "tests", "golden")
    cap = os.path.getsize(os.path.join(g, "cond_transformer_tiny.npz"))
    files = [f for f in os.listdir(g) if f.startswith("fsa_") and f.endswith(".npz")]
    assert len(files) == len(fu.BLOCK_CASES) + len(fu.MODEL_ATTN)
    for f in files:
        assert os.path.getsize(os.path.join(g, f)) <= cap, f
