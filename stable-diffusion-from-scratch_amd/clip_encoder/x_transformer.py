"""Mirror of ``clip_encoder/x_transformer.py`` — the encoder-only x-transformers subset behind
``TransformerEmbedder`` / ``BERTEmbedder`` (``clip_encoder/modules.py:48-165``), HIP-backed.

The classes carry the reference's parameter layout, so a checkpoint's ``cond_stage_model.transformer.*``
keys load with ``load_state_dict(strict=True)``::

    token_emb.weight   pos_emb.emb.weight   norm.{weight,bias}   to_logits.{weight,bias}
    attn_layers.layers.{2i}.0.{weight,bias}              pre-attention LayerNorm
    attn_layers.layers.{2i}.1.to_{q,k,v}.weight          no bias
    attn_layers.layers.{2i}.1.to_out.{weight,bias}
    attn_layers.layers.{2i+1}.0.{weight,bias}            pre-feed-forward LayerNorm
    attn_layers.layers.{2i+1}.1.net.0.0.{weight,bias}    (``net.0.proj`` with ``ff_glu``)
    attn_layers.layers.{2i+1}.1.net.2.{weight,bias}

The forward is the shape of ``CLIPTextTransformer._run``: fp16 residual stream, fp32 accumulation —
token + position embedding (``sdk_token_embedding``), per attention layer LayerNorm → one q|k|v GEMM
(no bias) → non-causal ``sdk_attention`` over the T tokens, scale ``dim_head ** -0.5`` → to_out GEMM +
residual, per feed-forward layer LayerNorm → net.0.0 GEMM → exact GELU (``sdk_gelu``) → net.2 GEMM +
residual (``ff_glu``: the GEGLU-epilogue GEMM instead of GEMM + GELU), then the final LayerNorm.  The
attention's inner width is ``heads * dim_head``, independent of ``dim``.

Every other option of the reference's ``Attention`` / ``AttentionLayers`` / ``TransformerWrapper`` raises
``NotImplementedError`` naming the option; dropouts are accepted and ignored (inference).
"""
from __future__ import annotations

import torch
from torch import nn

from .. import ops
from ..packing import PackedOwner, f32, prep_norm

DEFAULT_DIM_HEAD = 64
LN_MAX_DIM = 2048            # sdk_layer_norm: one wave per row, 4 x 64 chunks of 8 channels


def _refuse(option, where):
    raise NotImplementedError(f"sd_amd.x_transformer.{where}: option `{option}` is not supported (the HIP path "
                              "runs the default pre-norm encoder layout only)")


def _refuse_set(where, **options):
    """Each keyword is (value, the value that means "off")."""
    for name, (val, off) in options.items():
        if val != off:
            _refuse(name, where)


class AbsolutePositionalEmbedding(nn.Module):
    def __init__(self, dim, max_seq_len):
        super().__init__()
        self.emb = nn.Embedding(max_seq_len, dim)
        nn.init.normal_(self.emb.weight, std=0.02)


class Residual(nn.Module):
    """Parameter-free third entry of a layer triple (the add runs in the GEMM epilogue)."""


class GEGLU(nn.Module):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.proj = nn.Linear(dim_in, dim_out * 2)


class FeedForward(nn.Module):
    def __init__(self, dim, dim_out=None, mult=4, glu=False, dropout=0.):
        super().__init__()
        inner_dim = int(dim * mult)
        if dim_out is not None and dim_out != dim:
            _refuse("ff_dim_out", "FeedForward")
        self.glu = bool(glu)
        if self.glu and inner_dim % 32:
            raise NotImplementedError("sd_amd.x_transformer.FeedForward: `ff_glu` needs dim * ff_mult to be a "
                                      f"multiple of 32 (got {inner_dim})")
        project_in = GEGLU(dim, inner_dim) if self.glu else nn.Sequential(nn.Linear(dim, inner_dim), nn.GELU())
        self.net = nn.Sequential(project_in, nn.Dropout(dropout), nn.Linear(inner_dim, dim))

    def _prepare(self, dev):
        p = self.net[0].proj if self.glu else self.net[0][0]
        self._pc1 = ops.PackedConv([(p.weight, p.in_features)], p.bias, geglu=self.glu, device=dev)
        self._pc2 = ops.PackedConv([(self.net[2].weight, self.net[2].in_features)], self.net[2].bias, device=dev)

    def _run(self, t, residual):
        if self.glu:
            f = ops.linear(self._pc1, t, out_mode=ops.OUT_GEGLU_F16)
        else:
            f = ops.gelu(ops.linear(self._pc1, t))
        return ops.linear(self._pc2, f, residual=residual)


class Attention(nn.Module):
    def __init__(self, dim, dim_head=DEFAULT_DIM_HEAD, heads=8, causal=False, mask=None, talking_heads=False,
                 sparse_topk=None, use_entmax15=False, num_mem_kv=0, dropout=0., on_attn=False):
        super().__init__()
        _refuse_set("Attention", causal=(causal, False), mask=(mask, None), talking_heads=(talking_heads, False),
                    sparse_topk=(sparse_topk, None), use_entmax15=(use_entmax15, False),
                    num_mem_kv=(num_mem_kv, 0), on_attn=(on_attn, False))
        if dim_head % 8 or not 8 <= dim_head <= 160:
            raise NotImplementedError("sd_amd.x_transformer.Attention: `attn_dim_head` must be a multiple of 8 in "
                                      f"[8, 160] (got {dim_head})")
        self.scale = dim_head ** -0.5
        self.heads = heads
        self.dim_head = dim_head
        inner_dim = dim_head * heads
        self.to_q = nn.Linear(dim, inner_dim, bias=False)
        self.to_k = nn.Linear(dim, inner_dim, bias=False)
        self.to_v = nn.Linear(dim, inner_dim, bias=False)
        self.dropout = nn.Dropout(dropout)
        self.to_out = nn.Linear(inner_dim, dim)

    def _prepare(self, dev):
        w = torch.cat([self.to_q.weight, self.to_k.weight, self.to_v.weight], 0)
        self._pc_qkv = ops.PackedConv([(w, self.to_q.in_features)], None, device=dev)
        self._pc_o = ops.PackedConv([(self.to_out.weight, self.to_out.in_features)], self.to_out.bias, device=dev)

    def _run(self, t, residual, B, T):
        inner = self.heads * self.dim_head
        qkv = ops.linear(self._pc_qkv, t)
        o = ops.attention(qkv[:, :inner], qkv[:, inner:2 * inner], qkv[:, 2 * inner:], batch=B, heads=self.heads,
                          nq=T, nk=T, head_dim=self.dim_head, scale=self.scale)
        return ops.linear(self._pc_o, o, residual=residual)


class AttentionLayers(nn.Module):
    def __init__(self, dim, depth, heads=8, causal=False, cross_attend=False, only_cross=False, use_scalenorm=False,
                 use_rmsnorm=False, use_rezero=False, rel_pos_num_buckets=32, rel_pos_max_distance=128,
                 position_infused_attn=False, custom_layers=None, sandwich_coef=None, par_ratio=None,
                 residual_attn=False, cross_residual_attn=False, macaron=False, pre_norm=True, gate_residual=False,
                 **kwargs):
        super().__init__()
        _refuse_set("AttentionLayers", causal=(causal, False), cross_attend=(cross_attend, False),
                    only_cross=(only_cross, False), use_scalenorm=(use_scalenorm, False),
                    use_rmsnorm=(use_rmsnorm, False), use_rezero=(use_rezero, False),
                    position_infused_attn=(position_infused_attn, False), custom_layers=(custom_layers, None),
                    sandwich_coef=(sandwich_coef, None), par_ratio=(par_ratio, None),
                    residual_attn=(residual_attn, False), cross_residual_attn=(cross_residual_attn, False),
                    macaron=(macaron, False), pre_norm=(pre_norm, True), gate_residual=(gate_residual, False))
        ff_kwargs = {k[3:]: v for k, v in kwargs.items() if k.startswith("ff_")}
        attn_kwargs = {k[5:]: v for k, v in kwargs.items() if k.startswith("attn_")}
        for k in kwargs:
            if not k.startswith(("ff_", "attn_")):
                _refuse(k, "AttentionLayers")
        if dim % 8 or not 8 <= dim <= LN_MAX_DIM:
            raise NotImplementedError(f"sd_amd.x_transformer.AttentionLayers: `dim` must be a multiple of 8 in "
                                      f"[8, {LN_MAX_DIM}] (got {dim})")
        assert rel_pos_num_buckets <= rel_pos_max_distance
        self.dim = dim
        self.depth = depth
        self.has_pos_emb = False
        self.pre_norm = True
        self.layer_types = ("a", "f") * depth
        self.num_attn_layers = depth
        self.layers = nn.ModuleList([])
        for layer_type in self.layer_types:
            layer = Attention(dim, heads=heads, **attn_kwargs) if layer_type == "a" else FeedForward(dim, **ff_kwargs)
            self.layers.append(nn.ModuleList([nn.LayerNorm(dim), layer, Residual()]))

    def _prepare(self, dev):
        for norm, block, _ in self.layers:
            block._prepare(dev)
            prep_norm(norm, dev)

    def _run(self, x, B, T):
        """x fp16 [B*T, dim] → the same shape after every (LayerNorm → block → + x) pair."""
        for layer_type, (norm, block, _) in zip(self.layer_types, self.layers):
            t = ops.layer_norm(x, norm._g, norm._b, norm.eps)
            x = block._run(t, x, B, T) if layer_type == "a" else block._run(t, x)
        return x


class Encoder(AttentionLayers):
    def __init__(self, **kwargs):
        assert "causal" not in kwargs, "cannot set causality on encoder"
        super().__init__(causal=False, **kwargs)


class TransformerWrapper(PackedOwner, nn.Module):
    def __init__(self, *, num_tokens, max_seq_len, attn_layers, emb_dim=None, max_mem_len=0., emb_dropout=0.,
                 num_memory_tokens=None, tie_embedding=False, use_pos_emb=True):
        super().__init__()
        assert isinstance(attn_layers, AttentionLayers), "attention layers must be an Encoder"
        dim = attn_layers.dim
        _refuse_set("TransformerWrapper", emb_dim=(dim if emb_dim is None else emb_dim, dim),
                    num_memory_tokens=(num_memory_tokens or 0, 0), tie_embedding=(tie_embedding, False),
                    use_pos_emb=(use_pos_emb, True), max_mem_len=(max_mem_len, 0.))
        self.max_seq_len = max_seq_len
        self.max_mem_len = max_mem_len
        self.num_tokens = num_tokens
        self.num_memory_tokens = 0
        self.token_emb = nn.Embedding(num_tokens, dim)
        self.pos_emb = AbsolutePositionalEmbedding(dim, max_seq_len)
        self.emb_dropout = nn.Dropout(emb_dropout)
        self.project_emb = nn.Identity()
        self.attn_layers = attn_layers
        self.norm = nn.LayerNorm(dim)
        nn.init.normal_(self.token_emb.weight, std=0.02)
        # part of the checkpoint layout; the embeddings path (return_embeddings=True) never applies it
        self.to_logits = nn.Linear(dim, num_tokens)

    def _pack(self, dev):
        self.attn_layers._prepare(dev)
        self._tok = f32(self.token_emb.weight, dev)
        self._pos = f32(self.pos_emb.emb.weight, dev)
        prep_norm(self.norm, dev)

    @torch.no_grad()
    def forward(self, x, return_embeddings=False, mask=None, return_mems=False, return_attn=False, mems=None,
                **kwargs):
        """ids int64 [B, T <= max_seq_len] on the GPU → embeddings fp16 [B, T, dim]."""
        _refuse_set("TransformerWrapper.forward", mask=(mask is None, True), mems=(mems is None, True),
                    return_mems=(bool(return_mems), False), return_attn=(bool(return_attn), False))
        for k in kwargs:
            _refuse(k, "TransformerWrapper.forward")
        if not return_embeddings:
            _refuse("return_embeddings=False", "TransformerWrapper.forward")
        if not torch.is_tensor(x) or not x.is_cuda:
            raise TypeError("sd_amd.TransformerWrapper: HIP path only — move the ids to the GPU")
        if x.dim() != 2 or x.dtype not in (torch.int64, torch.int32):
            raise ValueError(f"sd_amd.TransformerWrapper: ids must be integer [B, T], got {x.dtype} {tuple(x.shape)}")
        B, T = x.shape
        if B < 1 or not 1 <= T <= self.max_seq_len:
            raise ValueError(f"sd_amd.TransformerWrapper: {T} tokens outside [1, max_seq_len = {self.max_seq_len}]")
        self.ensure_packed(x.device)
        ids = x.to(torch.int64)
        if int(ids.min()) < 0 or int(ids.max()) >= self.num_tokens:
            raise ValueError("sd_amd.TransformerWrapper: token id outside the vocabulary")
        h = ops.token_embedding(ids, self._tok, self._pos).view(B * T, -1)
        h = self.attn_layers._run(h, B, T)
        return ops.layer_norm(h, self.norm._g, self.norm._b, self.norm.eps).view(B, T, -1)
