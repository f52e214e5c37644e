"""Inputs, restatements and limits of the condition-encoder tests (shared by
tests/golden/make_golden_cond_stage.py and the tests).  Inputs are regenerated from seeds (numpy PCG64), so the
fixtures hold the reference's outputs only.

Two restatements live here, each pinned against the reference's fixtures on the CPU
(tests/test_cond_stage_inputs.py):

* ``encoder_ref``: the default pre-norm encoder of ``clip_encoder/x_transformer.py`` in plain fp32 torch;
* ``resize_ref``: the four ``F.interpolate`` rules of ``SpatialRescaler`` with the tap weights computed in fp32
  as torch computes them and the sum taken in float64, together with the per-element magnitude
  ``sum_i |w_i| |p_i|`` that the error unit ``2^-24 * sum |w||p|`` refers to.
"""
import json
import math

import numpy as np
import torch
import torch.nn.functional as F

import vq_util as vu

# ------------------------------------------------------------------ transformer encoders
VOCAB = 1000
TE_CFG = dict(n_embed=128, n_layer=2, vocab_size=VOCAB)            # TransformerEmbedder
BE_CFG = dict(n_embed=128, n_layer=2, vocab_size=VOCAB)            # BERTEmbedder(use_tokenizer=False)
GLU_CFG = dict(dim=128, depth=1, ff_glu=True)                      # Encoder inside a bare TransformerWrapper
SEEDS = {"te": 9101, "be": 9102, "glu": 9103, "wide": 9104}
SEQ_LENS = (77, 10)
WIDE_CFG = dict(n_embed=1280, n_layer=2, vocab_size=VOCAB)         # the LDM text encoder's GEMM shapes, 2 layers


def token_ids(seed, batch, seq, vocab=VOCAB):
    """int64 [batch, seq]; the first and last id of the vocabulary appear."""
    ids = np.random.Generator(np.random.PCG64(seed)).integers(0, vocab, (batch, seq), dtype=np.int64)
    ids[0, 0], ids[-1, -1] = 0, vocab - 1
    return ids


def case_ids(name, seq):
    return token_ids(SEEDS[name] + 7 * seq, 2, seq)


def encoder_ref(sd, ids, heads=8, dim_head=64):
    """fp32 restatement of TransformerWrapper(Encoder(dim, depth[, ff_glu]))(ids, return_embeddings=True):
    ``sd`` the wrapper's state_dict (fp32 tensors), ids int64 [B, T]."""
    ids = torch.as_tensor(ids, dtype=torch.long)
    B, T = ids.shape
    x = sd["token_emb.weight"][ids] + sd["pos_emb.emb.weight"][:T][None]
    D = x.shape[-1]
    i = 0
    while f"attn_layers.layers.{i}.0.weight" in sd:
        p = f"attn_layers.layers.{i}."
        h = F.layer_norm(x, (D,), sd[p + "0.weight"], sd[p + "0.bias"], 1e-5)
        if p + "1.to_q.weight" in sd:
            q, k, v = (F.linear(h, sd[p + f"1.to_{n}.weight"]).view(B, T, heads, dim_head).transpose(1, 2)
                       for n in "qkv")
            a = torch.softmax(q @ k.transpose(-1, -2) * dim_head ** -0.5, -1)
            o = (a @ v).transpose(1, 2).reshape(B, T, heads * dim_head)
            x = x + F.linear(o, sd[p + "1.to_out.weight"], sd[p + "1.to_out.bias"])
        else:
            if p + "1.net.0.proj.weight" in sd:
                u, gate = F.linear(h, sd[p + "1.net.0.proj.weight"], sd[p + "1.net.0.proj.bias"]).chunk(2, -1)
                f = u * F.gelu(gate)
            else:
                f = F.gelu(F.linear(h, sd[p + "1.net.0.0.weight"], sd[p + "1.net.0.0.bias"]))
            x = x + F.linear(f, sd[p + "1.net.2.weight"], sd[p + "1.net.2.bias"])
        i += 1
    return F.layer_norm(x, (D,), sd["norm.weight"], sd["norm.bias"], 1e-5)


# ------------------------------------------------------------------ class embedder
CLASS_CFG = dict(embed_dim=32, n_classes=10)
CLASS_SEED = 9201
CLASS_SCALE = 4.0            # synth scale of the table: |entries| up to ~1.2 instead of ~0.3
CLASS_LABELS = np.asarray([3, 0, 9, 3, 7], dtype=np.int64)        # repeated ids, both ends of the table
CTX1_LABELS = np.asarray([7, 2], dtype=np.int64)                   # the labels behind unet_tiny_ctx1's context
CTX1_UNET = dict(image_size=16, in_channels=4, out_channels=4, model_channels=32, attention_resolutions=[1, 2],
                 num_res_blocks=1, channel_mult=[1, 2], num_heads=4, use_spatial_transformer=True,
                 transformer_depth=1, context_dim=32, use_checkpoint=False, legacy=False)
CTX1_SEED = 9301


def ctx1_inputs():
    return dict(x=vu.randn(CTX1_SEED + 1, 2, 4, 16, 16), t=np.asarray([981, 1], dtype=np.int64))


# ------------------------------------------------------------------ spatial rescaler
# (B, C, H, W), method, multiplier, n_stages
RESCALE_CASES = [((2, 3, 8, 8), "bilinear", 0.5, 1), ((1, 5, 7, 9), "bilinear", 0.5, 1),
                 ((1, 5, 16, 12), "bilinear", 0.5, 2), ((1, 2, 8, 8), "bilinear", 1.5, 1),
                 ((1, 3, 6, 10), "bicubic", 2.0, 1), ((1, 3, 7, 5), "bicubic", 0.5, 1),
                 ((1, 3, 5, 7), "nearest", 0.5, 1), ((1, 3, 5, 7), "nearest", 2.0, 1),
                 ((2, 4, 9, 6), "area", 0.5, 1), ((1, 3, 8, 8), "bilinear", 0.5, 0)]
MAPPER_OUT = 4
MAPPER_SEED = 9400


def rescale_tag(case):
    shape, method, mult, stages = case
    return "{}_{}_m{}_s{}".format("x".join(map(str, shape)), method, int(round(mult * 10)), stages)


def rescale_input(case):
    shape = case[0]
    return vu.randn(9401 + 13 * int(np.prod(shape)) + len(case[1]) + int(case[2] * 10), *shape)


def mapper_bias(case):
    """Cases alternate between a mapper with and without bias."""
    return RESCALE_CASES.index(case) % 2 == 1


def mapper_keys(case):
    ks = [("channel_mapper.weight", (MAPPER_OUT, case[0][1], 1, 1))]
    if mapper_bias(case):
        ks.append(("channel_mapper.bias", (MAPPER_OUT,)))
    return ks


def mapper_seed(case):
    return MAPPER_SEED + RESCALE_CASES.index(case)


f32 = np.float32


def _step(scale):
    return f32(1.0 / float(scale))          # aten compute_scales_value: the float of 1 / scale_factor


def _src_index(step, n_out, cubic):
    s = step * (np.arange(n_out).astype(f32) + f32(0.5)) - f32(0.5)
    return s if cubic else np.where(s < 0, f32(0), s)


def _index_lambda(s, n_in):
    idx = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
    lam = np.minimum(np.maximum(s - idx.astype(f32), f32(0)), f32(1))
    return idx, lam.astype(f32)


def axis_taps(n_in, scale, mode):
    """(n_out, [Wo, n_in] float64 matrix of the fp32 tap weights of one axis)."""
    n_out = int(math.floor(n_in * float(scale)))
    W = np.zeros((n_out, n_in), dtype=np.float64)
    o = np.arange(n_out)
    if mode == "nearest":
        idx = np.minimum(np.floor(o.astype(f32) * _step(scale)).astype(np.int64), n_in - 1)
        W[o, idx] = 1.0
    elif mode == "bilinear":
        if n_in == n_out:
            W[o, o] = 1.0
        else:
            i0, w1 = _index_lambda(_src_index(_step(scale), n_out, False), n_in)
            i1 = i0 + (i0 < n_in - 1)
            w0 = f32(1) - w1
            np.add.at(W, (o, i0), w0.astype(np.float64))
            np.add.at(W, (o, i1), w1.astype(np.float64))
    elif mode == "bicubic":
        i0, t = _index_lambda(_src_index(_step(scale), n_out, True), n_in)
        A = f32(-0.75)

        def c1(x):
            return ((A + f32(2)) * x - (A + f32(3))) * x * x + f32(1)

        def c2(x):
            return ((A * x - f32(5) * A) * x + f32(8) * A) * x - f32(4) * A

        u = f32(1) - t
        ws = [c2(t + f32(1)), c1(t), c1(u), c2(u + f32(1))]
        for j, w in enumerate(ws):
            assert w.dtype == np.float32
            np.add.at(W, (o, np.clip(i0 + j - 1, 0, n_in - 1)), w.astype(np.float64))
    elif mode == "area":
        for k in range(n_out):
            a, b = (k * n_in) // n_out, -((-(k + 1) * n_in) // n_out)
            W[k, a:b] = 1.0 / (b - a)
    else:
        raise ValueError(mode)
    return n_out, W


def resize_ref(x, scale, mode):
    """(float64 result, float64 magnitude sum |w||p|) of F.interpolate(x, scale_factor=scale, mode=mode) for NCHW
    ``x`` (numpy fp32).  Border taps that clamp onto one pixel add their weights, which changes neither value."""
    x64 = np.asarray(x, dtype=np.float64)
    _, Wy = axis_taps(x.shape[2], scale, mode)
    _, Wx = axis_taps(x.shape[3], scale, mode)
    out = np.einsum("oh,bchw,pw->bcop", Wy, x64, Wx)
    mag = np.einsum("oh,bchw,pw->bcop", np.abs(Wy), np.abs(x64), np.abs(Wx))
    return out, mag


def rescale_ref(case, x=None):
    """``resize_ref`` chained over the case's stages: each stage's float64 result is rounded to fp32 for the next
    one (as every implementation stores it), and the magnitude is carried through the stages,
    ``|W2| (|W1| |x|)``, so an earlier stage's rounding stays within the unit of the later one."""
    _, method, mult, stages = case
    out = np.asarray(rescale_input(case) if x is None else x, dtype=np.float64)
    mag = np.abs(out)
    for s in range(stages):
        _, Wy = axis_taps(out.shape[2], mult, method)
        _, Wx = axis_taps(out.shape[3], mult, method)
        mag = np.einsum("oh,bchw,pw->bcop", np.abs(Wy), mag, np.abs(Wx))
        out = np.einsum("oh,bchw,pw->bcop", Wy, out, Wx)
        if s + 1 < stages:
            out = out.astype(f32).astype(np.float64)
    return out, mag


def units(got, ref64, mag):
    """max over elements of |got - ref| / (2^-24 * sum |w||p|); inf where a zero-magnitude element differs."""
    d = np.abs(np.asarray(got, dtype=np.float64) - ref64)
    u = 2.0 ** -24 * mag
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(u > 0, d / u, np.where(d > 0, np.inf, 0.0))
    return float(r.max())


# torch's CPU F.interpolate (the fixtures) against resize_ref, max over the cases of a mode, in units of
# 2^-24 * sum |w||p| — measured on the CPU by tests/test_cond_stage_inputs.py, which asserts that these are the
# numbers (measured <= recorded); nearest copies a pixel and must be bit-equal.  One tap sum of n terms rounds at
# most n - 1 adds and n products per axis, so one to two units is what fp32 evaluation of the same taps gives
# (measured per case: bilinear x0.5 1.18 / 1.75 / 1.00, bicubic 2.35 / 0.82, area 2.03).  The bilinear x1.5
# case measures 7.57: torch's CPU build fuses ``step * (dst + 0.5) - 0.5`` into one multiply-add, which moves a
# source coordinate near 5 by one ulp (2^-21) and with it both tap weights; with the coordinate restated as a
# fused multiply-add the same case measures 1.70.  The restatement (and the kernel) round the product and the
# difference separately, as the expression is written.
TORCH_VS_REF_UNITS = {"nearest": 0.0, "bilinear": 7.568, "bicubic": 2.351, "area": 2.029}


def resize_limit_units(mode):
    """GPU limit against both the fixture and resize_ref: twice torch's own distance plus one unit for a
    different summation order (the kernel adds the taps in torch's order but without fused multiply-adds)."""
    return 0.0 if mode == "nearest" else 2.0 * TORCH_VS_REF_UNITS[mode] + 1.0


# ------------------------------------------------------------------ limits of the fp16-path parity checks
# (rel-L2, max |got - ref| / max |ref|), each at <= 3.5x the error measured on MI355X
# (profiles/cond_stage_parity_errors.txt); fp16 activations vs the fp32 reference
PARITY_LIMITS = {
    "SpatialRescaler + channel_mapper vs reference": (1e-3, 1.1e-3),   # measured 2.923e-4 / 3.322e-4 (worst case)
    "tiny TransformerEmbedder vs reference": (2.5e-3, 3.5e-3),   # measured 8.887e-4 / 1.009e-3
    "tiny BERTEmbedder vs reference": (2.5e-3, 3.5e-3),   # measured 8.619e-4 / 1.009e-3
    "tiny ff_glu encoder vs reference": (3e-3, 3.5e-3),   # measured 9.745e-4 / 1.100e-3
    "wide TransformerEmbedder (1280) vs restatement": (2.5e-3, 3.5e-3),   # measured 8.111e-4 / 1.122e-3
    "tiny UNet unet_tiny_ctx1 vs reference": (5e-3, 5e-3),   # measured 1.612e-3 / 1.617e-3
    # yardsticks (tests/gpu_util.py): tiny CLIP vs transformers 7.193e-4 / 1.130e-3, tiny UNet unet_tiny 1.752e-3
}


def jbytes(obj):
    return np.frombuffer(json.dumps(obj).encode(), dtype=np.uint8)
