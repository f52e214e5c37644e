"""Golden vectors for the exact-GELU CLIP text tower and its early stop, from the installed ``transformers``
CLIPTextModel — build container only; no network, no pretrained weights: ``make_golden_clip.py``'s recipe with
``hidden_act="gelu"`` and 3 layers, the synthetic weights of tests/golden/synth.py.  Stored: ``last_hidden_state``
(what FrozenCLIPEmbedder returns) and ``final_layer_norm(hidden_states[-2])`` (what an OpenCLIP tower with
``layer="penultimate"`` returns for the same numbers).

Run from the repo root:  python tests/golden/make_golden_openclip.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)

TINY_CLIP_GELU = dict(vocab_size=1000, hidden_size=128, intermediate_size=512, num_hidden_layers=3,
                      num_attention_heads=2, max_position_embeddings=77, hidden_act="gelu",
                      layer_norm_eps=1e-5, bos_token_id=998, eos_token_id=999, pad_token_id=999)


def main():
    import transformers
    from transformers import CLIPTextConfig, CLIPTextModel
    from synth import synth_weights
    torch.manual_seed(0)
    m = CLIPTextModel(CLIPTextConfig(**TINY_CLIP_GELU)).eval()
    sd = m.state_dict()
    keys = [[k, list(v.shape)] for k, v in sd.items() if not k.endswith("position_ids")]
    w = synth_weights(keys, 33)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    g = torch.Generator().manual_seed(34)
    ids = torch.randint(0, 998, (2, 77), generator=g)
    ids[:, 0] = 998                                   # BOS, text, EOS then padding as the tokenizer emits
    ids[0, 9:] = 999
    ids[1, 40:] = 999
    with torch.no_grad():
        out = m(input_ids=ids, output_hidden_states=True)
        y = out.last_hidden_state
        tm = m.text_model if hasattr(m, "text_model") else m
        y_pen = tm.final_layer_norm(out.hidden_states[-2])
    path = os.path.join(OUT, "clip_tiny_gelu.npz")
    np.savez_compressed(path, ids=ids.numpy(), y=y.numpy(), y_penultimate=y_pen.numpy(), seed=np.int64(33),
                        keys=np.frombuffer(json.dumps(keys).encode(), dtype=np.uint8),
                        cfg=np.frombuffer(json.dumps(TINY_CLIP_GELU).encode(), dtype=np.uint8),
                        transformers_version=np.frombuffer(transformers.__version__.encode(), dtype=np.uint8))
    print("clip_tiny_gelu.npz", os.path.getsize(path), "transformers", transformers.__version__)


if __name__ == "__main__":
    main()
