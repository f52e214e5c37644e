"""Helpers of the OpenCLIP text-tower tests (tests/test_sd2_boundary.py on the CPU, tests/test_gpu_openclip.py on the
GPU): the open_clip key table, seeded weights and ids, a float64 CPU restatement built from torch's own
``nn.MultiheadAttention``, and the transformers -> open_clip key / shape conversion.  Nothing of the product package
is imported here."""
import json
import os

import numpy as np
import torch
from torch import nn

from synth import synth_weights

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

VIT_H14 = dict(vocab_size=49408, width=1024, heads=16, layers=24, mlp_width=4096, context_length=77)
TINY = dict(vocab_size=1000, width=128, heads=2, layers=3, mlp_width=512, context_length=77)
FULL_WIDTH_SHALLOW = dict(vocab_size=1000, width=1024, heads=16, layers=2, mlp_width=4096, context_length=77)
SOT, EOT = 998, 999          # of the tiny vocabularies


def openclip_keys(cfg, prefix="model."):
    """[(key, shape)] of an open_clip text tower in state_dict order (the table of the SD-2 checkpoints'
    ``cond_stage_model.model.*``): layers x 12 tensors + 6; a module's own parameters come first)."""
    W, M = cfg["width"], cfg["mlp_width"]
    ks = [("positional_embedding", (cfg["context_length"], W)), ("text_projection", (W, W)), ("logit_scale", ()),
          ("token_embedding.weight", (cfg["vocab_size"], W))]
    for i in range(cfg["layers"]):
        b = f"transformer.resblocks.{i}."
        ks += [(b + "ln_1.weight", (W,)), (b + "ln_1.bias", (W,)),
               (b + "attn.in_proj_weight", (3 * W, W)), (b + "attn.in_proj_bias", (3 * W,)),
               (b + "attn.out_proj.weight", (W, W)), (b + "attn.out_proj.bias", (W,)),
               (b + "ln_2.weight", (W,)), (b + "ln_2.bias", (W,)),
               (b + "mlp.c_fc.weight", (M, W)), (b + "mlp.c_fc.bias", (M,)),
               (b + "mlp.c_proj.weight", (W, M)), (b + "mlp.c_proj.bias", (W,))]
    ks += [("ln_final.weight", (W,)), ("ln_final.bias", (W,))]
    return [(prefix + k, s) for k, s in ks]


# synth_weights scales by the key's suffix: give open_clip's bare parameters the names of a Linear's
_SYNTH_NAME = {"in_proj_weight": "in_proj.weight", "in_proj_bias": "in_proj.bias",
               "positional_embedding": "positional_embedding.weight", "text_projection": "text_projection.weight"}


def openclip_weights(cfg, seed, prefix="model."):
    """Seeded fp16-representable weights under open_clip's keys (tests/golden/synth.py)."""
    ks = openclip_keys(cfg, prefix)
    alias = []
    for k, s in ks:
        head, _, leaf = k.rpartition(".")
        alias.append(((head + "." if head else "") + _SYNTH_NAME.get(leaf, leaf), s))
    w = synth_weights(alias, seed)
    return {k: torch.from_numpy(np.asarray(w[a])) for (k, _), (a, _) in zip(ks, alias)}


def seeded_ids(cfg, seed, lengths=(9, 40), sot=SOT, eot=EOT):
    """int64 [len(lengths), context_length] as open_clip.tokenize lays them out: SOT, text, EOT, zero padding."""
    g = torch.Generator().manual_seed(seed)
    T = cfg["context_length"]
    ids = torch.randint(1, sot, (len(lengths), T), generator=g)
    ids[:, 0] = sot
    for b, n in enumerate(lengths):
        ids[b, n] = eot
        ids[b, n + 1:] = 0
    return ids


class _Block(nn.Module):
    def __init__(self, width, heads, mlp_width):
        super().__init__()
        self.ln_1 = nn.LayerNorm(width, eps=1e-5)
        self.attn = nn.MultiheadAttention(width, heads)
        self.ln_2 = nn.LayerNorm(width, eps=1e-5)
        self.mlp = nn.Sequential()
        self.mlp.add_module("c_fc", nn.Linear(width, mlp_width))
        self.mlp.add_module("gelu", nn.GELU())
        self.mlp.add_module("c_proj", nn.Linear(mlp_width, width))

    def forward(self, x, mask):
        h = self.ln_1(x)
        x = x + self.attn(h, h, h, need_weights=False, attn_mask=mask)[0]
        return x + self.mlp(self.ln_2(x))


class Restatement(nn.Module):
    """open_clip's text tower restated with torch modules in float64 on the CPU: ``nn.MultiheadAttention`` reads the
    in_proj / out_proj tensors itself, so the q | k | v split is torch's reading of the layout."""

    def __init__(self, cfg):
        super().__init__()
        W = cfg["width"]
        self.cfg = cfg
        self.positional_embedding = nn.Parameter(torch.zeros(cfg["context_length"], W))
        self.token_embedding = nn.Embedding(cfg["vocab_size"], W)
        self.transformer = nn.Module()
        self.transformer.resblocks = nn.ModuleList([_Block(W, cfg["heads"], cfg["mlp_width"])
                                                    for _ in range(cfg["layers"])])
        self.ln_final = nn.LayerNorm(W, eps=1e-5)
        self.text_projection = nn.Parameter(torch.zeros(W, W))
        self.logit_scale = nn.Parameter(torch.zeros([]))

    @torch.no_grad()
    def forward(self, ids, layer_idx=0):
        T = ids.shape[1]
        x = self.token_embedding(ids) + self.positional_embedding[:T]
        mask = torch.full((T, T), float("-inf"), dtype=x.dtype).triu_(1)
        x = x.permute(1, 0, 2)                      # [T, B, W]: MultiheadAttention's default layout
        blocks = self.transformer.resblocks
        for blk in blocks[:len(blocks) - layer_idx]:
            x = blk(x, mask)
        return self.ln_final(x.permute(1, 0, 2))


def restate(cfg, weights, ids, layer_idx, prefix="model."):
    """float64 reference [B, T, W] of the tower with ``weights`` (open_clip keys under ``prefix``)."""
    m = Restatement(cfg)
    m.load_state_dict({k[len(prefix):]: v for k, v in weights.items()}, strict=True)
    return m.double()(ids, layer_idx)


def first_blocks(weights, cfg, n, prefix="model."):
    """(cfg, weights) of the tower that holds only the first ``n`` blocks of ``weights``."""
    keep = {k for k, _ in openclip_keys(dict(cfg, layers=n), prefix)}
    return dict(cfg, layers=n), {k: v for k, v in weights.items() if k in keep}


# ------------------------------------------------------------------------------ transformers <-> open_clip layouts
def load_cross_fixture():
    z = np.load(os.path.join(GOLDEN, "clip_tiny_gelu.npz"), allow_pickle=False)
    cfg = json.loads(bytes(z["cfg"]).decode())
    keys = [(k, tuple(s)) for k, s in json.loads(bytes(z["keys"]).decode())]
    w = {k: torch.from_numpy(v) for k, v in synth_weights(keys, int(z["seed"])).items()}
    return z, cfg, w


def openclip_cfg_of(tcfg):
    """The open_clip configuration of a transformers CLIP text configuration."""
    return dict(vocab_size=tcfg["vocab_size"], width=tcfg["hidden_size"], heads=tcfg["num_attention_heads"],
                layers=tcfg["num_hidden_layers"], mlp_width=tcfg["intermediate_size"],
                context_length=tcfg["max_position_embeddings"])


def transformers_to_openclip(w, tcfg, prefix="model."):
    """A transformers CLIPTextModel state_dict (``text_model.*``) under open_clip's keys and shapes: q / k / v
    concatenated into in_proj, the position table as a bare parameter; text_projection / logit_scale (absent from a
    text-only transformers model, unused by the conditioning) are filled with zeros."""
    t = "text_model."
    w = {(k if k.startswith(t) else t + k): v for k, v in w.items()}     # transformers >= 5 saves without the prefix
    W = tcfg["hidden_size"]
    out = {"positional_embedding": w[t + "embeddings.position_embedding.weight"],
           "token_embedding.weight": w[t + "embeddings.token_embedding.weight"]}
    for i in range(tcfg["num_hidden_layers"]):
        s, d = f"{t}encoder.layers.{i}.", f"transformer.resblocks.{i}."
        for n, o in (("layer_norm1", "ln_1"), ("layer_norm2", "ln_2"), ("self_attn.out_proj", "attn.out_proj"),
                     ("mlp.fc1", "mlp.c_fc"), ("mlp.fc2", "mlp.c_proj")):
            out[d + o + ".weight"], out[d + o + ".bias"] = w[s + n + ".weight"], w[s + n + ".bias"]
        out[d + "attn.in_proj_weight"] = torch.cat([w[s + f"self_attn.{p}_proj.weight"] for p in "qkv"], 0)
        out[d + "attn.in_proj_bias"] = torch.cat([w[s + f"self_attn.{p}_proj.bias"] for p in "qkv"], 0)
    out["ln_final.weight"], out["ln_final.bias"] = w[t + "final_layer_norm.weight"], w[t + "final_layer_norm.bias"]
    out["text_projection"] = torch.zeros(W, W)
    out["logit_scale"] = torch.zeros([])
    return {prefix + k: v for k, v in out.items()}
