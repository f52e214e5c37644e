"""Generate the condition-encoder fixtures by running the REFERENCE itself (build container only, CPU).

Run from the repo root:  python tests/golden/make_golden_cond_stage.py
Needs the reference checkout make_golden.py points at (read-only), einops and transformers.  Uses the shims of
make_golden.py; to import the reference's ``clip_encoder/modules.py`` its top-level ``import clip`` and
``import kornia`` (used by ``FrozenClipImageEmbedder`` only) get empty stand-in modules.

Weights come from tests/golden/synth.py, inputs from tests/cond_util.py (seeds); the fixtures hold only what the
reference computed:

* cond_transformer_tiny.npz — state_dict key / shape lists and outputs at T = 77 and T = 10 of
  ``TransformerEmbedder``, ``BERTEmbedder(use_tokenizer=False)`` and a ``TransformerWrapper`` around
  ``Encoder(ff_glu=True)``;
* cond_class.npz — ``ClassEmbedder`` keys and its output for a label batch;
* cond_rescaler.npz — ``SpatialRescaler`` outputs per case of cond_util.RESCALE_CASES, without (``y``) and with
  (``ym``) the channel mapper;
* unet_tiny_ctx1.npz — the tiny cross-attention UNet with ``context_dim=32`` on the one-token context that
  ``ClassEmbedder`` produces, written the way make_golden.py writes unet_tiny.npz.
"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg                                    # noqa: E402
import cond_util as cu                                      # noqa: E402
from synth import keys_shapes_of, synth_weights             # noqa: E402

OUT = HERE
T = torch.from_numpy


def install_shims():
    # transformers probes torchvision with find_spec, which the torchvision stand-in of make_golden.py has no
    # answer for: resolve the names the reference imports before the stand-ins go in
    from transformers import CLIPTextModel, CLIPTokenizer  # noqa: F401
    mg.install_shims()
    for name in ("clip", "kornia"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    with mg.quiet():
        from clip_encoder import modules as ref
        from clip_encoder import x_transformer as xt
    return ref, xt


def reinit(module, seed, scale=1.0):
    sd = module.state_dict()
    new = synth_weights(keys_shapes_of(sd), seed, scale)
    module.load_state_dict({k: T(v) for k, v in new.items()})
    return module.eval()


def keys_of(module):
    return cu.jbytes([[k, list(v.shape)] for k, v in module.state_dict().items()])


def gen_transformer(ref, xt):
    out = {}
    models = {
        "te": ref.TransformerEmbedder(device="cpu", **cu.TE_CFG),
        "be": ref.BERTEmbedder(device="cpu", use_tokenizer=False, **cu.BE_CFG),
        "glu": xt.TransformerWrapper(num_tokens=cu.VOCAB, max_seq_len=77, attn_layers=xt.Encoder(**cu.GLU_CFG)),
    }
    for name, m in models.items():
        reinit(m, cu.SEEDS[name])
        out[name + "_keys"] = keys_of(m)
        out[name + "_seed"] = np.int64(cu.SEEDS[name])
        for seq in cu.SEQ_LENS:
            ids = T(cu.case_ids(name, seq))
            with torch.no_grad():
                y = m(ids, return_embeddings=True) if name == "glu" else m.encode(ids)
            assert tuple(y.shape) == (2, seq, 128) and torch.isfinite(y).all()
            out[f"{name}_y{seq}"] = y.numpy()
    np.savez_compressed(os.path.join(OUT, "cond_transformer_tiny.npz"), **out)


def class_embedder(ref, key="class"):
    return reinit(ref.ClassEmbedder(key=key, **cu.CLASS_CFG), cu.CLASS_SEED, cu.CLASS_SCALE)


def gen_class(ref):
    m = class_embedder(ref)
    with torch.no_grad():
        y = m({"class": T(cu.CLASS_LABELS)})
    assert tuple(y.shape) == (len(cu.CLASS_LABELS), 1, cu.CLASS_CFG["embed_dim"])
    np.savez_compressed(os.path.join(OUT, "cond_class.npz"), keys=keys_of(m), seed=np.int64(cu.CLASS_SEED),
                        y=y.numpy())


def gen_rescaler(ref):
    out = {}
    for case in cu.RESCALE_CASES:
        shape, method, mult, stages = case
        x = T(cu.rescale_input(case))
        tag = cu.rescale_tag(case)
        with mg.quiet(), torch.no_grad():
            if stages > 0:
                out[tag + "_y"] = ref.SpatialRescaler(n_stages=stages, method=method, multiplier=mult,
                                                      in_channels=shape[1])(x).numpy()
            m = ref.SpatialRescaler(n_stages=stages, method=method, multiplier=mult, in_channels=shape[1],
                                    out_channels=cu.MAPPER_OUT, bias=cu.mapper_bias(case))
            assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == cu.mapper_keys(case)
            reinit(m, cu.mapper_seed(case))
            out[tag + "_ym"] = m.encode(x).numpy()
    np.savez_compressed(os.path.join(OUT, "cond_rescaler.npz"), **out)


def gen_unet_ctx1(ref):
    with mg.quiet():
        from openai_model.model import UNetModel
        torch.manual_seed(cu.CTX1_SEED)
        m = UNetModel(**cu.CTX1_UNET)
    mg.reinit_(m, cu.CTX1_SEED)
    m.eval()
    d = cu.ctx1_inputs()
    emb = class_embedder(ref, key="class_label")
    with mg.quiet(), torch.no_grad():
        ctx = emb({"class_label": T(cu.CTX1_LABELS)})
        assert tuple(ctx.shape) == (2, 1, 32)
        y = m(T(d["x"]), T(d["t"]), ctx)
    out = dict(mg.sd_keys(m), seed=np.int64(cu.CTX1_SEED), x=d["x"], t=d["t"], ctx=ctx.numpy(), y=y.numpy(),
               cfg=np.frombuffer(json.dumps(cu.CTX1_UNET).encode(), dtype=np.uint8))
    np.savez_compressed(os.path.join(OUT, "unet_tiny_ctx1.npz"), **out)


def main():
    ref, xt = install_shims()
    torch.set_num_threads(8)
    gen_transformer(ref, xt)
    gen_class(ref)
    gen_rescaler(ref)
    gen_unet_ctx1(ref)
    for f in ("cond_transformer_tiny.npz", "cond_class.npz", "cond_rescaler.npz", "unet_tiny_ctx1.npz"):
        print(f, os.path.getsize(os.path.join(OUT, f)))


if __name__ == "__main__":
    main()
