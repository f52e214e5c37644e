"""FrozenOpenCLIPEmbedder on the MI355X (run with -m gpu): the OpenCLIP text tower against a float64 restatement
built from torch's own nn.MultiheadAttention (tests/openclip_util.py), against a transformers fixture in the other
parameter layout (tests/golden/clip_tiny_gelu.npz), the early stop of layer="penultimate", and the packed-weight
lifecycle.

Limits: rel-L2 and max |got - ref| / max |ref|, each at most 3.5x the error measured on the MI355X
(profiles/openclip_parity_errors.txt), the convention of tests/gpu_util.py.  The yardstick is the quick-GELU tiny tower
on the same kernels (test_tiny_clip_vs_transformers: 7.2e-4 / 1.1e-3 measured)."""
import pytest
import torch
from torch import nn

import openclip_util as ou
from gpu_util import check_parity

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (rel-L2, max-abs / max) limits per tag; measured values beside each (profiles/openclip_parity_errors.txt)
LIMITS = {
    "tiny OpenCLIP last vs float64 restatement": (2.5e-3, 3.5e-3),                  # measured 7.648e-4 / 1.007e-3
    "tiny OpenCLIP penultimate vs float64 restatement": (2.5e-3, 3.5e-3),           # measured 7.276e-4 / 1.050e-3
    "full-width OpenCLIP penultimate vs float64 restatement": (2.5e-3, 3.0e-3),     # measured 7.213e-4 / 8.697e-4
    "gelu CLIP (transformers layout) vs transformers": (2.5e-3, 3.5e-3),            # measured 7.664e-4 / 1.028e-3
    "OpenCLIP penultimate vs transformers hidden_states[-2]": (2.4e-3, 2.6e-3),     # measured 6.848e-4 / 7.529e-4
}


def _check(tag, got, ref):
    return check_parity(tag, got, ref, *LIMITS[tag])


@pytest.fixture(scope="module")
def mods(sdk):
    from sd_amd.clip_encoder import modules
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return modules


def _embedder(mods, cfg, weights, layer):
    m = mods.FrozenOpenCLIPEmbedder(arch="test", config=cfg, device=DEV, layer=layer)
    m.load_state_dict(weights, strict=True)
    return m


@pytest.fixture(scope="module")
def tiny(mods):
    """Weights, ids, the float64 references and the two outputs of the tiny tower, computed once."""
    w = ou.openclip_weights(ou.TINY, 71)
    ids = ou.seeded_ids(ou.TINY, 72)
    out = {layer: _embedder(mods, ou.TINY, w, layer).encode_tokens(ids).cpu() for layer in ("last", "penultimate")}
    ref = {layer: ou.restate(ou.TINY, w, ids, idx) for idx, layer in enumerate(("last", "penultimate"))}
    return w, ids, out, ref


@pytest.mark.parametrize("layer", ["last", "penultimate"])
def test_tiny_tower_vs_float64_restatement(tiny, layer):
    _, ids, out, ref = tiny
    y = out[layer]
    assert y.shape == (2, 77, ou.TINY["width"]) and y.dtype == torch.float16
    _check(f"tiny OpenCLIP {layer} vs float64 restatement", y, ref[layer])


def test_penultimate_differs_from_last(tiny):
    _, _, out, ref = tiny
    d = ((out["penultimate"].double() - out["last"].double()).norm() / out["last"].double().norm()).item()
    dref = ((ref["penultimate"] - ref["last"]).norm() / ref["last"].norm()).item()
    print(f"[openclip] penultimate vs last: rel-L2 {d:.3e} (float64 restatement {dref:.3e})", flush=True)
    assert d > 100 * LIMITS["tiny OpenCLIP penultimate vs float64 restatement"][0]


def test_penultimate_is_last_of_the_shorter_tower(mods, tiny):
    """Stopping one block early runs exactly the kernels of a tower that never had the block."""
    w, ids, out, _ = tiny
    cfg2, w2 = ou.first_blocks(w, ou.TINY, 2)
    y2 = _embedder(mods, cfg2, w2, "last").encode_tokens(ids).cpu()
    assert torch.equal(y2, out["penultimate"])


def test_full_width_shallow_tower(mods):
    """ViT-H's real GEMM shapes, (154, 1024, 3072 / 1024 / 4096) and (154, 4096, 1024), at one block's cost."""
    cfg = ou.FULL_WIDTH_SHALLOW
    w = ou.openclip_weights(cfg, 73)
    ids = ou.seeded_ids(cfg, 74)
    y = _embedder(mods, cfg, w, "penultimate").encode_tokens(ids)
    assert y.shape == (2, 77, 1024) and y.dtype == torch.float16
    _check("full-width OpenCLIP penultimate vs float64 restatement", y, ou.restate(cfg, w, ids, 1))


def test_cross_layout_fixture_and_bit_equality(mods):
    """The same numbers in transformers' layout (FrozenCLIPEmbedder, hidden_act="gelu") and in open_clip's: both match
    the transformers fixture, and with layer="last" they are bit-equal to each other (one block implementation)."""
    z, tcfg, w = ou.load_cross_fixture()
    ids = torch.from_numpy(z["ids"])
    hf = mods.FrozenCLIPEmbedder(device=DEV, config=tcfg)
    hf.transformer.load_state_dict(w)
    y_hf = hf.encode_tokens(ids).cpu()
    _check("gelu CLIP (transformers layout) vs transformers", y_hf, torch.from_numpy(z["y"]))
    ocfg, ow = ou.openclip_cfg_of(tcfg), ou.transformers_to_openclip(w, tcfg)
    y_pen = _embedder(mods, ocfg, ow, "penultimate").encode_tokens(ids).cpu()
    _check("OpenCLIP penultimate vs transformers hidden_states[-2]", y_pen, torch.from_numpy(z["y_penultimate"]))
    y_last = _embedder(mods, ocfg, ow, "last").encode_tokens(ids).cpu()
    assert torch.equal(y_last, y_hf)
    # the early stop of the transformers-layout tower is the same stop
    assert torch.equal(hf.transformer.text_model._run(ids.to(DEV), n_layers=2).cpu(), y_pen)


def test_weights_loaded_through_a_parent_are_picked_up(mods, tiny):
    w, ids, out, _ = tiny

    class Parent(nn.Module):
        def __init__(self, cs):
            super().__init__()
            self.cond_stage_model = cs

    m = _embedder(mods, ou.TINY, w, "penultimate")
    assert torch.equal(m.encode_tokens(ids).cpu(), out["penultimate"])
    w_new = ou.openclip_weights(ou.TINY, 75)
    Parent(m).load_state_dict({"cond_stage_model." + k: v for k, v in w_new.items()}, strict=True)
    y = m.encode_tokens(ids).cpu()
    fresh = _embedder(mods, ou.TINY, w_new, "penultimate").encode_tokens(ids).cpu()
    assert torch.equal(y, fresh)
    assert not torch.equal(y, out["penultimate"])
