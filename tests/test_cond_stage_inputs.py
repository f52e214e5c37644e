"""CPU checks of the condition-encoder fixtures against the restatements of tests/cond_util.py: the fp32 encoder
restatement reproduces what the reference's x-transformer computed, and the float64 resize restatement lies as
far from torch's own F.interpolate output as cond_util.TORCH_VS_REF_UNITS records (the GPU limits derive from
those numbers)."""
import json

import numpy as np
import pytest
import torch

import cond_util as cu
from golden_util import load
from synth import synth_weights


def _weights(fx, name):
    ks = json.loads(bytes(fx[name + "_keys"]).decode())
    w = synth_weights([(k, tuple(s)) for k, s in ks], int(fx[name + "_seed"]))
    return {k: torch.from_numpy(v) for k, v in w.items()}


@pytest.mark.parametrize("seq", cu.SEQ_LENS)
@pytest.mark.parametrize("name", ["te", "be", "glu"])
def test_encoder_restatement_matches_the_reference(name, seq):
    fx = load("cond_transformer_tiny")
    pre = "" if name == "glu" else "transformer."
    sd = {k[len(pre):]: v for k, v in _weights(fx, name).items()}
    ref = torch.from_numpy(fx[f"{name}_y{seq}"])
    got = cu.encoder_ref(sd, cu.case_ids(name, seq))
    assert got.shape == ref.shape == (2, seq, 128)
    rl2 = ((got - ref).norm() / ref.norm()).item()
    print(f"encoder_ref {name} T={seq}: rel-L2 {rl2:.3e}")
    assert rl2 <= 1e-5


def test_token_ids_cover_both_ends_of_the_vocabulary():
    for name in ("te", "be", "glu"):
        for seq in cu.SEQ_LENS:
            ids = cu.case_ids(name, seq)
            assert ids.shape == (2, seq) and ids.min() == 0 and ids.max() == cu.VOCAB - 1


STAGED = [c for c in cu.RESCALE_CASES if c[3] > 0]


@pytest.mark.parametrize("case", STAGED, ids=cu.rescale_tag)
def test_torch_lies_within_the_recorded_distance_of_the_resize_restatement(case):
    got = load("cond_rescaler")[cu.rescale_tag(case) + "_y"]
    ref, mag = cu.rescale_ref(case)
    assert got.dtype == np.float32 and got.shape == ref.shape
    h, w = case[0][2:]
    for _ in range(case[3]):
        h, w = int(np.floor(h * case[2])), int(np.floor(w * case[2]))
    assert got.shape[2:] == (h, w)
    u = cu.units(got, ref, mag)
    print(f"torch vs resize_ref {cu.rescale_tag(case)}: {u:.3f} units (recorded {cu.TORCH_VS_REF_UNITS[case[1]]})")
    if case[1] == "nearest":
        assert np.array_equal(got.view(np.uint32), ref.astype(np.float32).view(np.uint32))
    assert u <= cu.TORCH_VS_REF_UNITS[case[1]]


def test_recorded_distances_are_the_measured_maxima():
    fx = load("cond_rescaler")
    worst = {m: 0.0 for m in cu.TORCH_VS_REF_UNITS}
    for case in STAGED:
        ref, mag = cu.rescale_ref(case)
        worst[case[1]] = max(worst[case[1]], cu.units(fx[cu.rescale_tag(case) + "_y"], ref, mag))
    for mode, rec in cu.TORCH_VS_REF_UNITS.items():
        # recorded to three decimals, rounded up
        assert worst[mode] <= rec <= worst[mode] + 1e-3, (mode, worst[mode], rec)
        assert cu.resize_limit_units(mode) == (0.0 if mode == "nearest" else 2 * rec + 1)


def test_resize_restatement_edges():
    x = np.arange(2 * 5, dtype=np.float32).reshape(1, 1, 2, 5)
    # a constant image stays constant under every rule (weights sum to one up to fp32 rounding of the taps)
    for mode, s in (("nearest", 2.0), ("bilinear", 0.5), ("bilinear", 1.5), ("bicubic", 2.0), ("area", 0.5)):
        out, mag = cu.resize_ref(np.full((1, 1, 6, 7), 3.0, dtype=np.float32), s, mode)
        assert np.allclose(out, 3.0, rtol=1e-6, atol=0)
        # only bicubic has negative taps: elsewhere the magnitude is the value itself
        assert (mag >= np.abs(out) - 1e-12).all() and (mode == "bicubic" or np.allclose(mag, np.abs(out)))
    out, _ = cu.resize_ref(x, 2.0, "nearest")
    assert np.array_equal(out[0, 0, :, ::2], np.repeat(x[0, 0], 2, 0))
    out, _ = cu.resize_ref(x, 0.5, "area")          # 2 x 5 -> 1 x 2: windows [0, 3) and [2, 5) of both rows
    assert np.allclose(out[0, 0], [[(0 + 1 + 2 + 5 + 6 + 7) / 6, (2 + 3 + 4 + 7 + 8 + 9) / 6]])


def test_mapper_only_case_and_mapper_fixtures_have_the_mapped_channels():
    fx = load("cond_rescaler")
    for case in cu.RESCALE_CASES:
        tag = cu.rescale_tag(case)
        ym = fx[tag + "_ym"]
        assert ym.shape[1] == cu.MAPPER_OUT and np.isfinite(ym).all()
        assert (tag + "_y" in fx.files) == (case[3] > 0)
        if case[3] > 0:
            # the mapper is a 1x1 conv of the resized image: the reference's two outputs agree with each other
            w = synth_weights(cu.mapper_keys(case), cu.mapper_seed(case))
            m = np.einsum("oc,bchw->bohw", w["channel_mapper.weight"][:, :, 0, 0].astype(np.float64),
                          fx[tag + "_y"].astype(np.float64))
            if cu.mapper_bias(case):
                m += w["channel_mapper.bias"][None, :, None, None]
            assert np.allclose(ym, m, rtol=1e-5, atol=1e-5)


def test_class_fixtures_are_rows_of_the_table():
    fx = load("cond_class")
    ks = json.loads(bytes(fx["keys"]).decode())
    assert ks == [["embedding.weight", [cu.CLASS_CFG["n_classes"], cu.CLASS_CFG["embed_dim"]]]]
    table = synth_weights([(k, tuple(s)) for k, s in ks], int(fx["seed"]), cu.CLASS_SCALE)["embedding.weight"]
    assert np.array_equal(fx["y"], table[cu.CLASS_LABELS][:, None])
    assert np.array_equal(table.astype(np.float16).astype(np.float32), table)      # exact in fp16
    assert np.array_equal(load("unet_tiny_ctx1")["ctx"], table[cu.CTX1_LABELS][:, None])
    assert len(set(cu.CLASS_LABELS.tolist())) < len(cu.CLASS_LABELS)               # repeated ids
