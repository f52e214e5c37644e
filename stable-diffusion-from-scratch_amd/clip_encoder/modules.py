"""Mirror of ``clip_encoder/modules.py`` — FrozenCLIPEmbedder, HIP-backed.

The reference (``modules.py:212-257``) tokenizes a prompt batch to 77 ids and returns
``CLIPTextModel(input_ids).last_hidden_state`` (transformers, ViT-L/14 text tower: 12 pre-LN
layers, width 768, 12 heads, causal self-attention, quick_gelu MLP, final LayerNorm).  Here the
text tower runs on the library's kernels: token + position embedding (``sdk_token_embedding``),
per layer LayerNorm → one q|k|v GEMM (bias) → causal flash attention (``sdk_attention`` with
``causal``) → out_proj GEMM + residual → LayerNorm → fc1 GEMM with the activation epilogue
(``hidden_act``: ``SDK_ACT_QUICK_GELU`` or ``SDK_ACT_GELU``) → fc2 GEMM + residual, then the final
LayerNorm.  The residual stream is fp16, accumulation fp32.  The output is fp16 [B, 77, 768] — the UNet
consumes it as context directly.  ``FrozenOpenCLIPEmbedder`` (Stability's SD-2.x cond stage, not in the
reference checkout) runs the same block on open_clip's parameter layout; see the end of this file.

Weights: module names follow transformers' checkpoint layout (``transformer.text_model.…``, the
same keys an SD-1 checkpoint holds under ``cond_stage_model.``), so a local
``model.safetensors`` loads with ``load_state_dict``.  ``from_pretrained`` by hub name needs the
network, which this build never has: ``version`` may be a LOCAL directory (config.json,
model.safetensors, vocab.json + merges.txt); otherwise the ViT-L/14 text configuration is built
with uninitialised weights and ``forward(text)`` needs a local tokenizer — ``encode_tokens(ids)``
takes ids directly.

The other condition encoders of the reference's file (``modules.py:25-209``) are mirrored as well: ``ClassEmbedder``
(one ``sdk_embedding_rows`` launch → a one-token fp16 context), ``TransformerEmbedder`` / ``BERTTokenizer`` /
``BERTEmbedder`` (the HIP encoder of ``x_transformer.py``; the BERT tokenizer from a LOCAL ``vocab.txt``) and
``SpatialRescaler`` (``sdk_resize2d`` per stage, then the optional 1x1 ``channel_mapper`` on the library's conv).
The abstract method is ``encode`` (the reference spells it ``encoder``); ``FrozenClipImageEmbedder`` is not mirrored
(it needs the ``clip`` package and hub weights), so ``clip`` and ``kornia`` are not imported.
"""
from __future__ import annotations

import os

import torch
from torch import nn

from .. import ops
from ..packing import PackedOwner, f32, prep_norm

VIT_L14_TEXT = dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12,
                    num_attention_heads=12, max_position_embeddings=77, layer_norm_eps=1e-5,
                    hidden_act="quick_gelu")


class AbstractEncoder(nn.Module):
    def __init__(self):
        super().__init__()

    def encode(self, *args, **kwargs):
        raise NotImplementedError


class ClassEmbedder(nn.Module):
    """Reference ``clip_encoder/modules.py:25-45``: the class label as a one-token cross-attention context.
    ``forward(batch)`` gathers ``embedding.weight[batch[key]]`` with ``sdk_embedding_rows`` → fp16
    [B, 1, embed_dim] on the GPU (the UNet's context dtype)."""

    def __init__(self, embed_dim, n_classes=1000, key="class"):
        super().__init__()
        self.key = key
        self.embedding = nn.Embedding(n_classes, embed_dim)

    @torch.no_grad()
    def forward(self, batch, key=None):
        if key is None:
            key = self.key
        ids = batch[key]
        w = self.embedding.weight
        if not torch.is_tensor(ids) or not ids.is_cuda or not w.is_cuda:
            raise TypeError("sd_amd.ClassEmbedder: HIP path only — move the module and the labels to the GPU")
        if ids.dim() != 1 or ids.dtype not in (torch.int64, torch.int32):
            raise ValueError(f"sd_amd.ClassEmbedder: labels must be integer [B], got {ids.dtype} {tuple(ids.shape)}")
        try:
            rows = ops.embedding_rows(ids.to(torch.int64), w.detach().float())
        except ValueError as e:
            raise ValueError(f"sd_amd.ClassEmbedder: label outside [0, {w.shape[0]})") from e
        return rows[:, None, :]


class TransformerEmbedder(AbstractEncoder):
    """Some transformer encoder layers (reference ``clip_encoder/modules.py:48-73``): token ids
    [B, T <= max_seq_len] → fp16 [B, T, n_embed] on the HIP encoder of ``x_transformer.py``."""

    def __init__(self, n_embed, n_layer, vocab_size, max_seq_len=77, device="cuda"):
        super().__init__()
        from .x_transformer import Encoder, TransformerWrapper
        self.device = device
        self.transformer = TransformerWrapper(num_tokens=vocab_size, max_seq_len=max_seq_len,
                                              attn_layers=Encoder(dim=n_embed, depth=n_layer))

    def forward(self, tokens):
        tokens = tokens.to(self.device)
        return self.transformer(tokens, return_embeddings=True)

    def encode(self, x):
        return self(x)


class BERTTokenizer(AbstractEncoder):
    """Reference ``clip_encoder/modules.py:76-120``: the huggingface BERT tokenizer, padded to ``max_length``.
    The reference downloads ``bert-base-uncased``; here ``version`` may be a LOCAL directory holding
    ``vocab.txt`` (loaded with ``local_files_only=True``).  Without one the module constructs and
    ``forward(text)`` raises."""

    def __init__(self, device="cuda", vq_interface=True, max_length=77, version=None):
        super().__init__()
        self.tokenizer = None
        if isinstance(version, str) and os.path.isdir(version) and os.path.exists(os.path.join(version, "vocab.txt")):
            from transformers import BertTokenizerFast
            self.tokenizer = BertTokenizerFast.from_pretrained(version, local_files_only=True)
        self.device = device
        self.vq_interface = vq_interface
        self.max_length = max_length

    def forward(self, text):
        if self.tokenizer is None:
            raise RuntimeError("sd_amd.BERTTokenizer: no local tokenizer (a directory with vocab.txt as `version`) — "
                               "the hub download of the reference is unavailable offline; pass token ids")
        batch_encoding = self.tokenizer(text, truncation=True, max_length=self.max_length, return_length=True,
                                        return_overflowing_tokens=False, padding="max_length", return_tensors="pt")
        return batch_encoding["input_ids"].to(self.device)

    @torch.no_grad()
    def encode(self, text):
        tokens = self(text)
        if not self.vq_interface:
            return tokens
        return None, None, [None, None, tokens]

    def decode(self, text):
        return text


class BERTEmbedder(AbstractEncoder):
    """Reference ``clip_encoder/modules.py:123-165``: the BERT tokenizer followed by transformer encoder layers
    (LDM text-to-image: ``n_embed=1280, n_layer=32`` → a 77 x 1280 context).  A tensor argument is always taken
    as token ids; text goes through the tokenizer (``tokenizer_version``: its local directory)."""

    def __init__(self, n_embed, n_layer, vocab_size=30522, max_seq_len=77, device="cuda", use_tokenizer=True,
                 embedding_dropout=0.0, tokenizer_version=None):
        super().__init__()
        from .x_transformer import Encoder, TransformerWrapper
        self.use_tknz_fn = use_tokenizer
        if self.use_tknz_fn:
            self.tknz_fn = BERTTokenizer(device=device, vq_interface=False, max_length=max_seq_len,
                                         version=tokenizer_version)
        self.device = device
        self.transformer = TransformerWrapper(num_tokens=vocab_size, max_seq_len=max_seq_len,
                                              attn_layers=Encoder(dim=n_embed, depth=n_layer),
                                              emb_dropout=embedding_dropout)

    def forward(self, text):
        if torch.is_tensor(text):
            tokens = text
        elif self.use_tknz_fn:
            tokens = self.tknz_fn(text)
        else:
            raise TypeError("sd_amd.BERTEmbedder: use_tokenizer=False takes token ids (an integer tensor)")
        return self.transformer(tokens, return_embeddings=True)

    def encode(self, text):
        return self(text)


class SpatialRescaler(nn.Module):
    """Reference ``clip_encoder/modules.py:168-209``: ``n_stages`` x ``F.interpolate(x, scale_factor=multiplier,
    mode=method)``, then an optional 1x1 ``channel_mapper``.  fp32 NCHW in, fp32 NCHW out (what ``c_concat``
    takes): one ``sdk_resize2d`` launch per stage; the mapper runs as the library's 1x1 conv on the fp16 NHWC
    pack of the resized image and writes fp32 NCHW."""

    def __init__(self, n_stages=1, method="bilinear", multiplier=0.5, in_channels=3, out_channels=None, bias=False):
        super().__init__()
        self.n_stages = n_stages
        assert self.n_stages >= 0
        assert method in ["nearest", "linear", "bilinear", "trilinear", "bicubic", "area"]
        self.method = method
        self.multiplier = multiplier
        self.remap_output = out_channels is not None
        if self.remap_output:
            self.channel_mapper = nn.Conv2d(in_channels, out_channels, 1, bias=bias)
        self._pc, self._pc_key = None, None

    @torch.no_grad()
    def forward(self, x):
        if not torch.is_tensor(x) or x.dim() != 4:
            raise ValueError("sd_amd.SpatialRescaler: expected an NCHW tensor")
        if self.n_stages > 0 and self.method in ("linear", "trilinear"):
            # torch itself: "Got 4D input, but linear mode needs 3D input" / trilinear 5D
            raise NotImplementedError(f"sd_amd.SpatialRescaler: method={self.method!r} does not take a 4-D input "
                                      "(torch's F.interpolate raises for it as well)")
        if not x.is_cuda:
            raise TypeError("sd_amd.SpatialRescaler: HIP path only — move the image to the GPU")
        for _ in range(self.n_stages):
            x = ops.resize2d(x, self.multiplier, self.method)
        if self.remap_output:
            m = self.channel_mapper
            if x.dim() != 4 or x.shape[1] != m.in_channels:
                raise ValueError(f"sd_amd.SpatialRescaler: channel_mapper takes {m.in_channels} channels, got "
                                 f"{tuple(x.shape)}")
            key = (x.device, m.weight._version, None if m.bias is None else m.bias._version, m.weight.data_ptr())
            if self._pc_key != key:
                self._c_pad = (m.in_channels + 7) // 8 * 8
                self._pc = ops.PackedConv([(m.weight, self._c_pad)], m.bias, device=x.device)
                self._pc_key = key
            x = ops.conv2d(self._pc, ops.nchw_to_nhwc(x.float(), self._c_pad), out_mode=ops.OUT_NCHW_F32)
        return x

    def encode(self, x):
        return self(x)


class _Embeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.token_embedding = nn.Embedding(cfg["vocab_size"], cfg["hidden_size"])
        self.position_embedding = nn.Embedding(cfg["max_position_embeddings"], cfg["hidden_size"])


class _Attention(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        D = cfg["hidden_size"]
        self.k_proj, self.v_proj, self.q_proj, self.out_proj = (nn.Linear(D, D) for _ in range(4))


class _MLP(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.fc1 = nn.Linear(cfg["hidden_size"], cfg["intermediate_size"])
        self.fc2 = nn.Linear(cfg["intermediate_size"], cfg["hidden_size"])


_ACTS = {"quick_gelu": ops.ACT_QUICK_GELU, "gelu": ops.ACT_GELU}


def _act_of(hidden_act):
    """The fc1 epilogue of a ``hidden_act`` name (transformers' ``config.json`` key)."""
    if hidden_act not in _ACTS:
        raise NotImplementedError(f"sd_amd: CLIP text tower hidden_act={hidden_act!r} is not supported "
                                  f"(known: {sorted(_ACTS)})")
    return _ACTS[hidden_act]


class _TextBlock(nn.Module):
    """One pre-LN residual block of a CLIP text tower on the library's kernels.  The two parameter layouts
    (transformers' ``_EncoderLayer``, open_clip's ``_ResidualAttentionBlock``) name their tensors in ``_parts`` and
    share everything else: the packing (``_prepare``) and the forward (``_run``), so both produce the same bits."""

    _act = ops.ACT_QUICK_GELU

    def _parts(self):
        """(q|k|v weight [3D, D], q|k|v bias [3D], out_proj, fc1, fc2, norm1, norm2)."""
        raise NotImplementedError

    def _prepare(self, dev):
        w, b, out_proj, fc1, fc2, n1, n2 = self._parts()
        D = w.shape[1]
        self._pc_qkv = ops.PackedConv([(w, D)], b, device=dev)
        self._pc_o = ops.PackedConv([(out_proj.weight, D)], out_proj.bias, device=dev)
        self._pc_fc1 = ops.PackedConv([(fc1.weight, D)], fc1.bias, device=dev)
        self._pc_fc2 = ops.PackedConv([(fc2.weight, fc1.out_features)], fc2.bias, device=dev)
        prep_norm(n1, dev)
        prep_norm(n2, dev)
        self._norms = (n1, n2)        # a tuple: not registered as submodules

    def _run(self, x, B, T, heads):
        D = x.shape[1]
        n1, n2 = self._norms
        qkv = ops.linear(self._pc_qkv, ops.layer_norm(x, n1._g, n1._b, n1.eps))
        d = D // heads
        o = ops.attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], batch=B, heads=heads, nq=T, nk=T,
                          head_dim=d, scale=d ** -0.5, causal=True)
        x = ops.linear(self._pc_o, o, residual=x)
        f = ops.linear(self._pc_fc1, ops.layer_norm(x, n2._g, n2._b, n2.eps), act=self._act)
        return ops.linear(self._pc_fc2, f, residual=x)


def _run_tower(what, ids, tok, pos, blocks, heads, ln):
    """ids [B, T] -> token + position embedding -> ``blocks`` -> ``ln``: fp16 [B, T, D]."""
    ids = ids.to(torch.int64)
    B, T = ids.shape
    if int(ids.min()) < 0 or int(ids.max()) >= tok.shape[0]:
        raise ValueError(f"sd_amd.{what}: token id outside the vocabulary")
    x = ops.token_embedding(ids, tok, pos).view(B * T, -1)
    for blk in blocks:
        x = blk._run(x, B, T, heads)
    return ops.layer_norm(x, ln._g, ln._b, ln.eps).view(B, T, -1)


class _EncoderLayer(_TextBlock):
    def __init__(self, cfg):
        super().__init__()
        D, eps = cfg["hidden_size"], cfg["layer_norm_eps"]
        self._act = _act_of(cfg.get("hidden_act", "quick_gelu"))     # CLIP ViT-L/14's, where a config omits it
        self.self_attn = _Attention(cfg)
        self.layer_norm1 = nn.LayerNorm(D, eps=eps)
        self.mlp = _MLP(cfg)
        self.layer_norm2 = nn.LayerNorm(D, eps=eps)

    def _parts(self):
        a = self.self_attn
        w = torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight], 0)
        b = torch.cat([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias], 0)
        return w, b, a.out_proj, self.mlp.fc1, self.mlp.fc2, self.layer_norm1, self.layer_norm2


class _Encoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.layers = nn.ModuleList([_EncoderLayer(cfg) for _ in range(cfg["num_hidden_layers"])])


class CLIPTextTransformer(PackedOwner, nn.Module):
    """transformers' CLIPTextTransformer parameter layout; HIP forward (``_run``)."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = dict(cfg)
        self.embeddings = _Embeddings(cfg)
        self.encoder = _Encoder(cfg)
        self.final_layer_norm = nn.LayerNorm(cfg["hidden_size"], eps=cfg["layer_norm_eps"])

    def _pack(self, dev):
        for layer in self.encoder.layers:
            layer._prepare(dev)
        self._tok = f32(self.embeddings.token_embedding.weight, dev)
        self._pos = f32(self.embeddings.position_embedding.weight, dev)
        prep_norm(self.final_layer_norm, dev)

    @torch.no_grad()
    def _run(self, ids, n_layers=None):
        """``n_layers``: run only the first ``n_layers`` blocks (default all), then ``final_layer_norm``."""
        if not ids.is_cuda:
            raise TypeError("sd_amd.CLIPTextTransformer: HIP path only — move the ids to the GPU")
        layers = self.encoder.layers
        if n_layers is not None:
            if not 0 <= n_layers <= len(layers):
                raise ValueError(f"sd_amd.CLIPTextTransformer: n_layers={n_layers} outside [0, {len(layers)}]")
            layers = layers[:n_layers]
        self.ensure_packed(ids.device)
        return _run_tower("CLIPTextTransformer", ids, self._tok, self._pos, layers,
                          self.cfg["num_attention_heads"], self.final_layer_norm)


class CLIPTextModel(nn.Module):
    """Holder named like transformers' CLIPTextModel (``.text_model``)."""

    def __init__(self, cfg):
        super().__init__()
        self.text_model = CLIPTextTransformer(cfg)

    def load_state_dict(self, state_dict, strict=True, assign=False):
        # transformers >= 5 saves without the "text_model." prefix; older files and SD checkpoints with it
        sd = {(k if k.startswith("text_model.") else "text_model." + k): v for k, v in state_dict.items()
              if not k.endswith("position_ids")}
        return super().load_state_dict(sd, strict=strict, assign=assign)


class FrozenCLIPEmbedder(AbstractEncoder):
    """Uses the CLIP transformer encoder for text (reference ``clip_encoder/modules.py:212-257``)."""

    def __init__(self, version="openai/clip-vit-large-patch14", device="cuda", max_length=77, config=None):
        super().__init__()
        cfg = dict(VIT_L14_TEXT if config is None else config)
        local = isinstance(version, str) and os.path.isdir(version)
        if local and config is None and os.path.exists(os.path.join(version, "config.json")):
            import json
            with open(os.path.join(version, "config.json")) as f:
                c = json.load(f)
            c = c.get("text_config", c)
            cfg.update({k: c[k] for k in VIT_L14_TEXT if k in c})
        self.transformer = CLIPTextModel(cfg)
        self.tokenizer = None
        if local:
            st = os.path.join(version, "model.safetensors")
            if os.path.exists(st):
                from safetensors.torch import load_file
                sd = {k: v for k, v in load_file(st).items() if not k.startswith("vision_model.")}
                self.transformer.load_state_dict(sd, strict=False)
            if os.path.exists(os.path.join(version, "vocab.json")):
                from transformers import CLIPTokenizer
                self.tokenizer = CLIPTokenizer.from_pretrained(version, local_files_only=True)
        self.device = device
        self.max_length = max_length
        self.freeze()

    def freeze(self):
        self.transformer = self.transformer.eval()
        for param in self.parameters():
            param.requires_grad = False

    def encode_tokens(self, input_ids):
        """ids int64 [B, max_length] → last_hidden_state fp16 [B, max_length, hidden]."""
        return self.transformer.text_model._run(input_ids.to(self.device))

    def forward(self, text):
        if torch.is_tensor(text):
            return self.encode_tokens(text)
        if self.tokenizer is None:
            raise RuntimeError("sd_amd.FrozenCLIPEmbedder: no local tokenizer (vocab.json/merges.txt) — "
                               "the hub download of the reference is unavailable offline; pass token ids")
        batch_encoding = self.tokenizer(text, truncation=True, max_length=self.max_length, return_length=True,
                                        return_overflowing_tokens=False, padding="max_length", return_tensors="pt")
        return self.encode_tokens(batch_encoding["input_ids"])

    def encode(self, text):
        return self(text)


# ------------------------------------------------------------------------------------- OpenCLIP text tower (SD-2)
# Not in the reference checkout: Stability's ``ldm/modules/encoders/modules.py`` FrozenOpenCLIPEmbedder, whose
# weights an SD-2.x checkpoint holds under ``cond_stage_model.model.*`` in open_clip's layout.
VIT_H14_TEXT = dict(vocab_size=49408, width=1024, heads=16, layers=24, mlp_width=4096, context_length=77)
OPENCLIP_LN_EPS = 1e-5
OPENCLIP_SOT, OPENCLIP_EOT = 49406, 49407


def openclip_pad(id_lists, context_length=77, sot=OPENCLIP_SOT, eot=OPENCLIP_EOT):
    """Lay token id lists out as ``open_clip.tokenize`` does: ``[sot] + ids + [eot]``, truncated to
    ``context_length`` with the last id forced to ``eot``, padded with 0 (transformers pads with EOT).
    Returns int64 [len(id_lists), context_length]."""
    out = torch.zeros(len(id_lists), context_length, dtype=torch.int64)
    for i, ids in enumerate(id_lists):
        row = [sot] + [int(t) for t in ids] + [eot]
        if len(row) > context_length:
            row = row[:context_length]
            row[-1] = eot
        out[i, :len(row)] = torch.tensor(row, dtype=torch.int64)
    return out


class _InProjAttention(nn.Module):
    """The parameters of ``nn.MultiheadAttention`` as open_clip's blocks hold them: one [3D, D] in_proj (rows
    q | k | v) and ``out_proj``."""

    def __init__(self, width):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * width, width))
        self.in_proj_bias = nn.Parameter(torch.empty(3 * width))
        self.out_proj = nn.Linear(width, width)


class _OpenCLIPMLP(nn.Module):
    def __init__(self, width, mlp_width):
        super().__init__()
        self.c_fc = nn.Linear(width, mlp_width)
        self.c_proj = nn.Linear(mlp_width, width)


class _ResidualAttentionBlock(_TextBlock):
    """open_clip's ResidualAttentionBlock parameter layout; the exact (erf) GELU of ``nn.GELU()``."""

    _act = ops.ACT_GELU

    def __init__(self, width, mlp_width):
        super().__init__()
        self.ln_1 = nn.LayerNorm(width, eps=OPENCLIP_LN_EPS)
        self.attn = _InProjAttention(width)
        self.ln_2 = nn.LayerNorm(width, eps=OPENCLIP_LN_EPS)
        self.mlp = _OpenCLIPMLP(width, mlp_width)

    def _parts(self):
        a = self.attn
        return a.in_proj_weight, a.in_proj_bias, a.out_proj, self.mlp.c_fc, self.mlp.c_proj, self.ln_1, self.ln_2


class _OpenCLIPTransformer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.resblocks = nn.ModuleList([_ResidualAttentionBlock(cfg["width"], cfg["mlp_width"])
                                        for _ in range(cfg["layers"])])


class OpenCLIPTextTower(PackedOwner, nn.Module):
    """open_clip's CLIP text-side parameter layout (what Stability's class keeps after ``del model.visual``);
    HIP forward (``_run``).  ``text_projection`` and ``logit_scale`` are held so a checkpoint loads; the
    conditioning does not use them.  ``attn_mask`` is no persistent buffer in open_clip and no key here: the
    attention kernel's ``causal`` flag is the mask."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = dict(cfg)
        W = cfg["width"]
        self.positional_embedding = nn.Parameter(torch.empty(cfg["context_length"], W))
        self.token_embedding = nn.Embedding(cfg["vocab_size"], W)
        self.transformer = _OpenCLIPTransformer(cfg)
        self.ln_final = nn.LayerNorm(W, eps=OPENCLIP_LN_EPS)
        self.text_projection = nn.Parameter(torch.empty(W, W))
        self.logit_scale = nn.Parameter(torch.ones([]) * 2.659260036932778)     # ln(1 / 0.07), open_clip's init
        if self.positional_embedding.device.type != "meta":
            nn.init.normal_(self.positional_embedding, std=0.01)
            nn.init.normal_(self.text_projection, std=W ** -0.5)
            for blk in self.transformer.resblocks:
                nn.init.normal_(blk.attn.in_proj_weight, std=W ** -0.5)
                nn.init.zeros_(blk.attn.in_proj_bias)

    def _pack(self, dev):
        for blk in self.transformer.resblocks:
            blk._prepare(dev)
        self._tok = f32(self.token_embedding.weight, dev)
        self._pos = f32(self.positional_embedding, dev)
        prep_norm(self.ln_final, dev)

    @torch.no_grad()
    def _run(self, ids, n_layers=None):
        if not ids.is_cuda:
            raise TypeError("sd_amd.OpenCLIPTextTower: HIP path only — move the ids to the GPU")
        blocks = self.transformer.resblocks
        if n_layers is not None:
            if not 0 <= n_layers <= len(blocks):
                raise ValueError(f"sd_amd.OpenCLIPTextTower: n_layers={n_layers} outside [0, {len(blocks)}]")
            blocks = blocks[:n_layers]
        if ids.shape[1] > self.positional_embedding.shape[0]:
            raise ValueError("sd_amd.OpenCLIPTextTower: more tokens than context_length")
        self.ensure_packed(ids.device)
        return _run_tower("OpenCLIPTextTower", ids, self._tok, self._pos, blocks, self.cfg["heads"], self.ln_final)


class FrozenOpenCLIPEmbedder(AbstractEncoder):
    """Uses the OpenCLIP transformer encoder for text (Stability's ``FrozenOpenCLIPEmbedder``, the SD-2.x cond
    stage): ViT-H/14's text tower, width 1024, 16 heads, 24 blocks, MLP 4096 with the exact GELU.  ``layer="last"``
    runs every block, ``"penultimate"`` all but the last (what SD-2 is trained on); ``ln_final`` follows either way.

    Parameters sit under ``self.model`` with open_clip's names and shapes, so ``load_state_dict(strict=True)``
    takes the ``cond_stage_model.*`` slice of an SD-2 checkpoint.  ``open_clip`` is not imported and nothing is
    fetched: ``version`` names the pretrained tag only, unless it is a LOCAL directory with ``vocab.json`` +
    ``merges.txt``, which gives ``forward(text)`` its tokenizer (ids laid out by ``openclip_pad``).  Without one,
    pass token ids (``encode_tokens``).  ``arch`` other than ViT-H-14 needs ``config``: a dict with
    ``vocab_size, width, heads, layers, mlp_width, context_length``.

    Known difference: open_clip cleans text with ``ftfy`` before the byte-pair encoding; ``ftfy`` is not a
    dependency here, so text with mojibake or unusual unicode forms may tokenize differently.  Text is
    whitespace-collapsed and lower-cased by the tokenizer as in open_clip."""

    LAYERS = ["last", "penultimate"]

    def __init__(self, arch="ViT-H-14", version="laion2b_s32b_b79k", device="cuda", max_length=77, freeze=True,
                 layer="last", config=None):
        super().__init__()
        assert layer in self.LAYERS, f"sd_amd.FrozenOpenCLIPEmbedder: layer={layer!r} is not one of {self.LAYERS}"
        if config is None:
            if arch != "ViT-H-14":
                raise NotImplementedError(f"sd_amd.FrozenOpenCLIPEmbedder: arch={arch!r} has no built-in "
                                          "configuration (only ViT-H-14) — pass `config`")
            config = VIT_H14_TEXT
        missing = [k for k in VIT_H14_TEXT if k not in config]
        if missing:
            raise ValueError(f"sd_amd.FrozenOpenCLIPEmbedder: config lacks {missing}")
        self.model = OpenCLIPTextTower({k: config[k] for k in VIT_H14_TEXT})
        self.tokenizer = None
        if isinstance(version, str) and os.path.isdir(version) and \
                os.path.exists(os.path.join(version, "vocab.json")) and \
                os.path.exists(os.path.join(version, "merges.txt")):
            from transformers import CLIPTokenizer
            self.tokenizer = CLIPTokenizer(os.path.join(version, "vocab.json"), os.path.join(version, "merges.txt"),
                                           local_files_only=True)
        self.device = device
        self.max_length = max_length
        self.layer = layer
        self.layer_idx = self.LAYERS.index(layer)
        if freeze:
            self.freeze()

    def freeze(self):
        self.model = self.model.eval()
        for param in self.parameters():
            param.requires_grad = False

    def encode_tokens(self, input_ids):
        """ids int64 [B, context_length] → fp16 [B, context_length, width]."""
        n = len(self.model.transformer.resblocks) - self.layer_idx
        return self.model._run(input_ids.to(self.device), n_layers=n)

    def tokenize(self, text):
        if self.tokenizer is None:
            raise RuntimeError("sd_amd.FrozenOpenCLIPEmbedder: no local tokenizer (vocab.json/merges.txt in a "
                               "`version` directory) — nothing is fetched offline; pass token ids")
        if isinstance(text, str):
            text = [text]
        ids = [self.tokenizer(t, add_special_tokens=False)["input_ids"] for t in text]
        return openclip_pad(ids, self.max_length)

    def forward(self, text):
        if torch.is_tensor(text):
            return self.encode_tokens(text)
        return self.encode_tokens(self.tokenize(text))

    def encode(self, text):
        return self(text)
