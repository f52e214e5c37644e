"""The LDM condition encoders on the GPU (run with -m gpu): the ClassEmbedder row gather and SpatialRescaler's
resize kernel against the reference's fixtures (tests/golden/make_golden_cond_stage.py) and the restatements of
tests/cond_util.py, the HIP x-transformer encoder against the reference's outputs, and the three conditioning
paths end to end through LatentDiffusion (class labels with a one-token context, BERT-style text ids, concat).

Kernel limits: the row gather and nearest resize are bit-equal; the other resize modes stay within
cond_util.resize_limit_units of both the torch-written fixture and the float64 restatement.  fp16-path limits
are cond_util.PARITY_LIMITS (at most 3.5x the errors measured on MI355X,
profiles/cond_stage_parity_errors.txt)."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import cond_util as cu
import vq_util as vu
from golden_util import cfg_of, load, weights_of
from gpu_util import check_parity
from synth import keys_shapes_of, synth_weights

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _synth_into(module, seed, scale=1.0):
    w = synth_weights(keys_shapes_of(module.state_dict()), seed, scale)
    module.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    return {k: torch.from_numpy(v) for k, v in w.items()}


def _parity(tag, got, ref):
    return check_parity(tag, got, ref, *cu.PARITY_LIMITS[tag])


# ------------------------------------------------------------------ ops.embedding_rows
@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("dim", [32, 30, 1])
def test_embedding_rows_equals_index_half(sdk, dim, n):
    from sd_amd import ops
    table = _gpu(vu.randn(9500 + dim, 7, dim) * np.float32(3.0))
    ids = torch.tensor([6, 0, 3, 6, 6][:n], device=DEV)              # repeated ids, both ends of the table
    out = ops.embedding_rows(ids, table)
    assert out.dtype == torch.float16 and tuple(out.shape) == (n, dim) and out.is_contiguous()
    assert torch.equal(out.view(torch.int16), table[ids].half().view(torch.int16))


def test_embedding_rows_unaligned_table_takes_the_scalar_form(sdk):
    from sd_amd import ops
    buf = _gpu(vu.randn(9540, 1 + 7 * 32))
    table = buf[1:].view(7, 32)                                      # 4 bytes past a 16-byte boundary
    assert table.data_ptr() % 16 == 4 and table.is_contiguous()
    ids = torch.tensor([5, 1, 5], device=DEV)
    assert torch.equal(ops.embedding_rows(ids, table).view(torch.int16), table[ids].half().view(torch.int16))


def test_embedding_rows_rejects_bad_arguments(sdk):
    from sd_amd import ops
    table = torch.zeros(4, 8, device=DEV)
    for bad in ([4], [-1], [0, 7]):
        with pytest.raises(ValueError):
            ops.embedding_rows(torch.tensor(bad, device=DEV), table)
    with pytest.raises(ValueError):
        ops.embedding_rows(torch.zeros(2, 1, dtype=torch.long, device=DEV), table)
    with pytest.raises(ValueError):
        ops.embedding_rows(torch.zeros(0, dtype=torch.long, device=DEV), table)
    with pytest.raises(TypeError):
        ops.embedding_rows(torch.zeros(2, dtype=torch.int32, device=DEV), table)
    with pytest.raises(TypeError):
        ops.embedding_rows(torch.zeros(2, dtype=torch.long, device=DEV), table.half())


def _class_embedder(sdk, key="class"):
    from sd_amd.clip_encoder.modules import ClassEmbedder
    m = ClassEmbedder(key=key, **cu.CLASS_CFG)
    _synth_into(m, cu.CLASS_SEED, cu.CLASS_SCALE)
    return m.to(DEV)


def test_class_embedder_equals_the_reference(sdk):
    fx = load("cond_class")
    m = _class_embedder(sdk)
    y = m({"class": _gpu(cu.CLASS_LABELS)})
    assert y.dtype == torch.float16 and y.is_cuda and tuple(y.shape) == (len(cu.CLASS_LABELS), 1, 32)
    assert torch.equal(y.cpu().view(torch.int16), torch.from_numpy(fx["y"]).half().view(torch.int16))
    assert torch.equal(m({"other": _gpu(cu.CLASS_LABELS)}, key="other"), y)
    for bad in ([10], [-1]):
        with pytest.raises(ValueError, match="label outside"):
            m({"class": torch.tensor(bad, device=DEV)})


# ------------------------------------------------------------------ ops.resize2d
STAGED = [c for c in cu.RESCALE_CASES if c[3] > 0]
SENTINEL = 12345.0


def _guarded_resize(ops, x_np, scale, mode):
    """ops.resize2d with NaN on both sides of the input and a sentinel on both sides of the output: the result
    and proof that nothing outside the two tensors was written (sentinels) or read (no NaN came in)."""
    n, pad = x_np.size, 257
    xin = torch.full((n + 2 * pad,), float("nan"), device=DEV)
    xin[pad:pad + n] = _gpu(x_np).reshape(-1)
    x = xin[pad:pad + n].view(*x_np.shape)
    B, Cc, H, W = x_np.shape
    Ho, Wo = int(np.floor(H * scale)), int(np.floor(W * scale))
    m = B * Cc * Ho * Wo
    buf = torch.full((m + 2 * pad,), SENTINEL, device=DEV)
    out = buf[pad:pad + m].view(B, Cc, Ho, Wo)
    y = ops.resize2d(x, scale, mode, out=out)
    assert y.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert bool((buf[:pad] == SENTINEL).all()) and bool((buf[pad + m:] == SENTINEL).all()), "wrote outside the output"
    assert bool(torch.isfinite(y).all()), "read outside the input"
    assert bool(torch.isnan(xin[:pad]).all()) and bool(torch.isnan(xin[pad + n:]).all())
    return y.cpu().numpy().copy()


@pytest.mark.parametrize("case", STAGED, ids=cu.rescale_tag)
def test_resize2d_against_the_fixture_and_the_restatement(sdk, case):
    from sd_amd import ops
    _, method, mult, stages = case
    y = cu.rescale_input(case)
    for _ in range(stages):
        y = _guarded_resize(ops, y, mult, method)
    fix = load("cond_rescaler")[cu.rescale_tag(case) + "_y"]
    ref, mag = cu.rescale_ref(case)
    assert y.dtype == np.float32 and y.shape == fix.shape == ref.shape
    u_fix, u_ref = cu.units(y, fix.astype(np.float64), mag), cu.units(y, ref, mag)
    lim = cu.resize_limit_units(method)
    print(f"[resize2d] {cu.rescale_tag(case)}: {u_fix:.3f} units from torch, {u_ref:.3f} from the restatement "
          f"(<= {lim:.3f})", flush=True)
    if method == "nearest":
        assert np.array_equal(y.view(np.uint32), fix.view(np.uint32))
    assert u_fix <= lim and u_ref <= lim
    # an unguarded call (its own output allocation) gives the same bits
    x = _gpu(cu.rescale_input(case))
    for _ in range(stages):
        x = ops.resize2d(x, mult, method)
    assert np.array_equal(x.cpu().numpy().view(np.uint32), y.view(np.uint32))


def test_resize2d_anisotropic_factor_and_more_than_one_block(sdk):
    from sd_amd import ops
    x = vu.randn(9600, 2, 3, 37, 53)                                # 2*3*18*79 outputs: several workgroups
    y = _guarded_resize(ops, x, 1.0, "bilinear")                     # equal sizes copy
    assert np.array_equal(y, x)
    g = ops.resize2d(_gpu(x), (0.5, 1.5), "bilinear").cpu().numpy()
    _, Wy = cu.axis_taps(37, 0.5, "bilinear")
    _, Wx = cu.axis_taps(53, 1.5, "bilinear")
    ref = np.einsum("oh,bchw,pw->bcop", Wy, x.astype(np.float64), Wx)
    mag = np.einsum("oh,bchw,pw->bcop", np.abs(Wy), np.abs(x).astype(np.float64), np.abs(Wx))
    assert g.shape == (2, 3, 18, 79)
    u = cu.units(g, ref, mag)
    print(f"[resize2d] 2x3x37x53 bilinear (0.5, 1.5): {u:.3f} units from the restatement", flush=True)
    assert u <= cu.resize_limit_units("bilinear")


def test_resize2d_rejects_bad_arguments(sdk):
    from sd_amd import _lib, ops
    x = torch.zeros(1, 2, 4, 4, device=DEV)
    with pytest.raises(ValueError):
        ops.resize2d(x, 0.5, "lanczos")
    with pytest.raises(ValueError):
        ops.resize2d(x[0], 0.5)
    for s in (0.0, -1.0, float("inf"), 0.2):                         # 0.2: floor(4 * 0.2) = 0 rows
        with pytest.raises(ValueError):
            ops.resize2d(x, s)
    with pytest.raises(ValueError):
        ops.resize2d(x, 0.5, out=torch.zeros(1, 2, 3, 2, device=DEV))
    with pytest.raises(TypeError):
        ops.resize2d(x.half(), 0.5)
    y = torch.zeros(1, 2, 2, 2, device=DEV)

    def call(**kw):
        a = _lib.Resize2dArgs()
        a.x, a.y, a.planes, a.h, a.w, a.out_h, a.out_w = x.data_ptr(), y.data_ptr(), 2, 4, 4, 2, 2
        a.mode, a.scale_h, a.scale_w = _lib.RESIZE_BILINEAR, 0.5, 0.5
        for k, v in kw.items():
            setattr(a, k, v)
        return _lib.lib().sdk_resize2d(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))

    assert call() == 0
    for kw in (dict(mode=4), dict(mode=-1), dict(x=None), dict(y=None), dict(h=0), dict(w=-1), dict(out_h=0),
               dict(out_w=0), dict(out_h=3), dict(planes=0), dict(scale_w=0.0)):
        assert call(**kw) != 0, kw
    assert b"resize2d" in _lib.lib().sdk_last_error()
    assert _lib.lib().sdk_embedding_rows(None, None, None, 1, 1, None) != 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ SpatialRescaler with the mapper
@pytest.mark.parametrize("case", cu.RESCALE_CASES, ids=cu.rescale_tag)
def test_spatial_rescaler_with_mapper_vs_reference(sdk, case):
    from sd_amd.clip_encoder.modules import SpatialRescaler
    shape, method, mult, stages = case
    m = SpatialRescaler(n_stages=stages, method=method, multiplier=mult, in_channels=shape[1],
                        out_channels=cu.MAPPER_OUT, bias=cu.mapper_bias(case))
    w = synth_weights(cu.mapper_keys(case), cu.mapper_seed(case))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    m = m.to(DEV)
    y = m.encode(_gpu(cu.rescale_input(case)))
    ref = load("cond_rescaler")[cu.rescale_tag(case) + "_ym"]
    assert y.dtype == torch.float32 and y.is_cuda and tuple(y.shape) == ref.shape
    _parity("SpatialRescaler + channel_mapper vs reference", y, torch.from_numpy(ref))
    if stages > 0:
        plain = SpatialRescaler(n_stages=stages, method=method, multiplier=mult, in_channels=shape[1])
        got = plain(_gpu(cu.rescale_input(case))).cpu().numpy()
        fix = load("cond_rescaler")[cu.rescale_tag(case) + "_y"]
        _, mag = cu.rescale_ref(case)
        assert cu.units(got, fix.astype(np.float64), mag) <= cu.resize_limit_units(method)


# ------------------------------------------------------------------ transformer encoders
def _mirror(sdk, name):
    from sd_amd.clip_encoder.modules import BERTEmbedder, TransformerEmbedder
    from sd_amd.clip_encoder.x_transformer import Encoder, TransformerWrapper
    if name == "te":
        return TransformerEmbedder(**cu.TE_CFG)
    if name == "be":
        return BERTEmbedder(use_tokenizer=False, **cu.BE_CFG)
    return TransformerWrapper(num_tokens=cu.VOCAB, max_seq_len=77, attn_layers=Encoder(**cu.GLU_CFG))


@pytest.fixture(scope="module")
def tiny_encoders(sdk):
    fx = load("cond_transformer_tiny")
    out = {}
    for name in ("te", "be", "glu"):
        m = _mirror(sdk, name)
        ks = [(k, tuple(s)) for k, s in json.loads(bytes(fx[name + "_keys"]).decode())]
        w = synth_weights(ks, int(fx[name + "_seed"]))
        m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
        out[name] = m.to(DEV)
    return out


@pytest.mark.parametrize("seq", cu.SEQ_LENS)
@pytest.mark.parametrize("name", ["te", "be", "glu"])
def test_tiny_encoder_vs_reference(sdk, tiny_encoders, name, seq):
    m = tiny_encoders[name]
    ids = _gpu(cu.case_ids(name, seq))
    y = m(ids, return_embeddings=True) if name == "glu" else m.encode(ids)
    assert y.dtype == torch.float16 and y.is_cuda and tuple(y.shape) == (2, seq, 128)
    ref = torch.from_numpy(load("cond_transformer_tiny")[f"{name}_y{seq}"])
    tag = {"te": "tiny TransformerEmbedder vs reference", "be": "tiny BERTEmbedder vs reference",
           "glu": "tiny ff_glu encoder vs reference"}[name]
    _parity(tag, y, ref)
    assert torch.equal(y, m(ids, return_embeddings=True) if name == "glu" else m(ids))     # deterministic


def test_encoder_rejects_cpu_ids_and_ids_outside_the_vocabulary(sdk, tiny_encoders):
    be = tiny_encoders["be"]
    with pytest.raises(TypeError, match="HIP path only"):
        be.encode(torch.zeros(1, 4, dtype=torch.long))
    for bad in (cu.VOCAB, -1):
        with pytest.raises(ValueError, match="vocabulary"):
            be.encode(torch.tensor([[0, bad]], device=DEV))
    with pytest.raises(ValueError, match="max_seq_len"):
        be.encode(torch.zeros(1, 78, dtype=torch.long, device=DEV))
    y32 = be.encode(torch.tensor([[5, 7, 9]], dtype=torch.int32, device=DEV))
    assert torch.equal(y32, be.encode(torch.tensor([[5, 7, 9]], device=DEV)))


def test_reloaded_weights_replace_the_packed_copies(sdk, tiny_encoders):
    from sd_amd.clip_encoder.modules import BERTEmbedder
    m = BERTEmbedder(use_tokenizer=False, **cu.BE_CFG).to(DEV)
    ids = _gpu(cu.case_ids("be", 10))
    before = m.encode(ids)
    m.load_state_dict(tiny_encoders["be"].state_dict())
    after = m.encode(ids)
    assert not torch.equal(before, after) and torch.equal(after, tiny_encoders["be"].encode(ids))


def test_wide_encoder_vs_restatement(sdk):
    """The LDM text encoder's GEMM shapes (K = 1280 / 512 / 5120, N = 1536 / 1280 / 5120), two layers."""
    from sd_amd.clip_encoder.modules import TransformerEmbedder
    m = TransformerEmbedder(**cu.WIDE_CFG)
    w = _synth_into(m, cu.SEEDS["wide"])
    ids = cu.case_ids("wide", 77)
    ref = cu.encoder_ref({k[len("transformer."):]: v for k, v in w.items()}, ids)
    y = m.to(DEV).encode(_gpu(ids))
    assert y.dtype == torch.float16 and tuple(y.shape) == (2, 77, 1280)
    _parity("wide TransformerEmbedder (1280) vs restatement", y, ref)


# ------------------------------------------------------------------ nk = 1 at the kernel level
@pytest.mark.parametrize("d,nq", [(8, 256), (16, 64), (64, 77)])
def test_attention_with_one_key_returns_the_value_row(sdk, d, nq):
    """softmax over one key is 1: every query row of (batch, head) receives that head's value row."""
    from sd_amd import ops
    B, H = 2, 4
    q = _gpu(vu.randn(9700 + d, B * nq, H * d)).half()
    kv = _gpu(vu.randn(9701 + d, B, 2 * H * d)).half()
    o = ops.attention(q, kv[:, :H * d], kv[:, H * d:], batch=B, heads=H, nq=nq, nk=1, head_dim=d, scale=d ** -0.5)
    want = kv[:, H * d:].repeat_interleave(nq, 0)
    assert bool(torch.isfinite(o).all())
    # P = exp2(0) = 1 and the row sum is 1: the only rounding is the fp16 store of an fp16 value
    assert torch.allclose(o.float(), want.float(), rtol=2.0 ** -10, atol=0)


def test_segment_softmax_with_one_key_per_head_is_one(sdk):
    from sd_amd import ops
    s = _gpu(vu.randn(9710, 130, 8) * np.float32(20.0))
    p = ops.segment_softmax(s, 8, 1, 0.125)
    assert tuple(p.shape) == (130, 64)
    assert bool((p[:, :8] == 1).all()) and bool((p[:, 8:] == 0).all())


# ------------------------------------------------------------------ end to end through LatentDiffusion
def _ld(sdk, cond_cfg, cond_key, ckey, ucfg):
    from sd_amd.Diffusion.ddpm import LatentDiffusion
    v = load("vae_tiny")
    return LatentDiffusion(
        first_stage_config={"target": "VAE.autoencoder.AutoEncoderKL",
                            "params": {"ddconfig": cfg_of(v), "embed_dim": 4,
                                       "lossconfig": {"target": "torch.nn.Identity"}}},
        cond_stage_config=cond_cfg, cond_stage_key=cond_key, conditioning_key=ckey,
        unet_config={"target": "openai_model.model.UNetModel", "params": ucfg}, timesteps=1000,
        linear_start=0.00085, linear_end=0.012, image_size=16, channels=4)


def test_class_conditioning_end_to_end_with_a_one_token_context(sdk):
    """ClassEmbedder → get_learned_conditioning → apply_model: cross-attention with nk = 1 against the
    reference's UNet output for the same labels."""
    from sd_amd.clip_encoder.modules import ClassEmbedder
    fx = load("unet_tiny_ctx1")
    ld = _ld(sdk, {"target": "clip_encoder.modules.ClassEmbedder",
                   "params": dict(key="class_label", **cu.CLASS_CFG)}, "class_label", "crossattn", cfg_of(fx))
    assert type(ld.cond_stage_model) is ClassEmbedder
    ld.model.diffusion_model.load_state_dict(weights_of(fx))
    _synth_into(ld.cond_stage_model, cu.CLASS_SEED, cu.CLASS_SCALE)
    ld = ld.to(DEV)
    c = ld.get_learned_conditioning({ld.cond_stage_key: _gpu(cu.CTX1_LABELS)})
    assert c.dtype == torch.float16 and tuple(c.shape) == (2, 1, 32)
    assert torch.equal(c.cpu().view(torch.int16), torch.from_numpy(fx["ctx"]).half().view(torch.int16))
    y = ld.apply_model(_gpu(fx["x"]), _gpu(fx["t"]), c)
    assert y.dtype == torch.float32 and tuple(y.shape) == fx["y"].shape
    _parity("tiny UNet unet_tiny_ctx1 vs reference", y, torch.from_numpy(fx["y"]))
    # the labels matter: another class gives another output
    y2 = ld.apply_model(_gpu(fx["x"]), _gpu(fx["t"]),
                        ld.get_learned_conditioning({"class_label": _gpu(cu.CTX1_LABELS[::-1].copy())}))
    assert not torch.equal(y, y2)


def test_text_conditioning_end_to_end_with_token_ids(sdk, tiny_encoders):
    from sd_amd.DDIM.ddim import DDIMSampler
    ucfg = dict(cu.CTX1_UNET, context_dim=128)
    ld = _ld(sdk, {"target": "clip_encoder.modules.BERTEmbedder",
                   "params": dict(use_tokenizer=False, **cu.BE_CFG)}, "caption", "crossattn", ucfg)
    _synth_into(ld.model.diffusion_model, 9801)
    ld.cond_stage_model.load_state_dict(tiny_encoders["be"].state_dict())
    ld = ld.to(DEV)
    ids = _gpu(cu.case_ids("be", 77))
    c = ld.get_learned_conditioning(ids)
    assert torch.equal(c, ld.cond_stage_model(ids)) and torch.equal(c, tiny_encoders["be"].encode(ids))
    uc = ld.get_learned_conditioning(torch.zeros_like(ids))
    assert not torch.equal(c, uc)
    z, _ = DDIMSampler(ld).sample(S=2, batch_size=2, shape=(4, 16, 16), conditioning=c, eta=0.0, verbose=False,
                                  unconditional_guidance_scale=3.0, unconditional_conditioning=uc,
                                  x_T=_gpu(vu.randn(9802, 2, 4, 16, 16)))
    assert tuple(z.shape) == (2, 4, 16, 16) and bool(torch.isfinite(z).all()) and float(z.abs().max()) > 0


def test_concat_conditioning_end_to_end_through_the_rescaler(sdk):
    ucfg = dict(cfg_of(load("unet_tiny_uncond")), in_channels=8)
    ld = _ld(sdk, {"target": "clip_encoder.modules.SpatialRescaler",
                   "params": dict(n_stages=1, method="bilinear", multiplier=0.5, in_channels=3, out_channels=4,
                                  bias=True)}, "segmentation", "concat", ucfg)
    _synth_into(ld.model.diffusion_model, 9811)
    _synth_into(ld.cond_stage_model, 9812)
    ld = ld.to(DEV)
    seg = _gpu(vu.randn(9813, 2, 3, 32, 32))
    c = ld.get_learned_conditioning(seg)
    assert c.dtype == torch.float32 and tuple(c.shape) == (2, 4, 16, 16)
    assert torch.equal(c, ld.cond_stage_model(seg))
    x, t = _gpu(vu.randn(9814, 2, 4, 16, 16)), torch.tensor([981, 1], device=DEV)
    y = ld.apply_model(x, t, c)
    assert torch.equal(y, ld.model(x, t, c_concat=[c])) and bool(torch.isfinite(y).all())
    assert not torch.equal(y, ld.apply_model(x, t, torch.zeros_like(c)))
