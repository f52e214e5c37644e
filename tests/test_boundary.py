"""CPU tests of the drop-in boundary: the C-ABI library exports, host-side argument
validation (no kernel launch), and state_dict / constructor compatibility of the
module mirrors with the reference (key lists captured from the reference)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from golden_util import load, cfg_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    txt = open(os.path.join(ROOT, "include", "sdk_amd.h")).read()
    return sorted(set(re.findall(r"\b(sdk_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_header_symbol(sdk):
    L = sdk.library()
    syms = _header_symbols()
    assert len(syms) >= 12
    for s in syms:
        assert hasattr(L, s), s
    assert L.sdk_version() >= 1


def test_conv_plan_validates_on_host(sdk):
    from sd_amd import _lib
    L = sdk.library()
    a = _lib.ConvArgs()
    info = _lib.ConvPlanInfo()
    assert L.sdk_conv2d_plan(C.byref(a), C.byref(info)) != 0       # empty shape rejected
    assert b"nseg" in L.sdk_last_error() or b"empty" in L.sdk_last_error()
    # a well-formed 3x3 conv: 2x16x16x64 -> 128, K = 9*64
    a.batch, a.ho, a.wo, a.cout, a.nseg = 2, 16, 16, 128, 1
    s = a.seg[0]
    s.src0 = 0x1000; s.c_split = 64; s.cin = 64; s.ld0 = 64; s.h = 16; s.w = 16
    s.ksize = 3; s.stride = 1; s.pad = 1
    a.weight = 0x2000; a.out = 0x3000; a.out_ld = 128; a.k_total = 9 * 64
    assert L.sdk_conv2d_plan(C.byref(a), C.byref(info)) == 0, L.sdk_last_error()
    assert info.flops == 2.0 * 2 * 256 * 128 * 9 * 64
    a.k_total = 100
    assert L.sdk_conv2d_plan(C.byref(a), C.byref(info)) != 0
    a.k_total = 9 * 64
    s.cin = 60
    assert L.sdk_conv2d_plan(C.byref(a), C.byref(info)) != 0       # cin % 8
    s.cin = 64
    a.ho = 15
    assert L.sdk_conv2d_plan(C.byref(a), C.byref(info)) != 0       # geometry mismatch


def test_conv_plan_picks_skinny_and_names_every_variant(sdk):
    """The host planner routes <= 64-row 1x1 GEMMs (the time-embedding MLP at M = batch) to the skinny
    kernel (variant 35) and larger ones to the tiled kernels; sdk_kernel_name knows every variant id
    the autotuner may choose."""
    from sd_amd import _lib, ops
    L = sdk.library()
    L.sdk_kernel_name.restype = C.c_char_p
    for v in ops.AUTOTUNE.VARIANTS + (0,):
        assert L.sdk_kernel_name(v) != b"unknown", v
    a = _lib.ConvArgs()
    info = _lib.ConvPlanInfo()
    a.batch, a.ho, a.wo, a.cout, a.nseg = 1, 16, 1, 1280, 1
    s = a.seg[0]
    s.src0 = 0x1000; s.c_split = 320; s.cin = 320; s.ld0 = 320; s.h = 16; s.w = 1
    s.ksize = 1; s.stride = 1; s.pad = 0
    a.weight = 0x2000; a.out = 0x3000; a.out_ld = 1280; a.k_total = 320
    assert L.sdk_conv2d_plan(C.byref(a), C.byref(info)) == 0, L.sdk_last_error()
    assert info.variant == 35 and info.split_k == 1 and info.workspace_bytes == 0
    a.ho = s.h = 65                                    # 65 rows: a tiled plan
    assert L.sdk_conv2d_plan(C.byref(a), C.byref(info)) == 0, L.sdk_last_error()
    assert info.variant != 35
    a.variant_hint = 6                                 # the retired variant 5 plans as 22 (the same 256x320 tile)
    assert L.sdk_conv2d_plan(C.byref(a), C.byref(info)) == 0, L.sdk_last_error()
    assert info.variant == 22
    a.variant_hint = 36
    assert L.sdk_conv2d_plan(C.byref(a), C.byref(info)) != 0         # forced 35 on 65 rows
    a.variant_hint = 37                                # the retired halo-tile ids 36 / 37 are unknown
    assert L.sdk_conv2d_plan(C.byref(a), C.byref(info)) != 0
    assert L.sdk_kernel_name(36) == b"unknown" and L.sdk_kernel_name(37) == b"unknown"
    a.variant_hint = 42
    assert L.sdk_conv2d_plan(C.byref(a), C.byref(info)) != 0         # unknown id


def test_conv_plans_equal_the_recorded_golden(sdk):
    """The host planner decides what tests/golden/conv_plans.npz recorded, row for row: return code, variant,
    split, grid, workspace, GroupNorm chunks and FLOPs over every variant id x split request x statistics request
    of make_golden_conv_plans.CASES, and sdk_kernel_name for ids -1..48 (error text is not compared)."""
    import make_golden_conv_plans as G
    from sd_amd import _lib
    assert "SDK_CONV_VARIANT" not in os.environ
    want = np.load(G.OUT)
    got = G.sweep(sdk.library(), _lib)
    assert len(want["rc"]) == len(G.CASES) * len(G.HINTS) * len(G.SPLITS) * 2
    assert sorted(want.files) == sorted(got)
    for k in want.files:
        bad = np.flatnonzero(want[k] != got[k])
        assert bad.size == 0, (k, [(G.CASE_NAMES[got["case"][i]], int(got["hint"][i]), G.SPLITS[got["split_req"][i]],
                                    int(got["gn_req"][i]), want[k][i], got[k][i]) for i in bad[:5]]
                               if len(want[k]) == len(want["rc"]) else (want[k].tolist(), got[k].tolist()))
    G.check_coverage(got)


def _gemm_args(_lib, M, N, K, out_mode=0):
    a = _lib.ConvArgs()
    a.batch, a.ho, a.wo, a.cout, a.nseg = 1, M, 1, N, 1
    s = a.seg[0]
    s.src0 = 0x1000; s.c_split = K; s.cin = K; s.ld0 = K; s.h = M; s.w = 1
    s.ksize = 1; s.stride = 1; s.pad = 0
    a.weight = 0x2000; a.out = 0x3000; a.k_total = K
    a.out_mode, a.out_ld, a.split_k = out_mode, (N // 2 if out_mode == 2 else N), 1
    return a


def test_hand_kept_variant_lists_agree_with_the_library(sdk):
    """The lists that stay hand-kept outside csrc/conv.h's variant table fail here when they drift from it:
    the autotuner's candidates are the named ids minus the register-staged fallback and the retired 5; every
    id of the exact tests' re-declared TILE is honoured with that tile's grid, and under the GEGLU output
    exactly the ids of their GEGLU_OK are honoured."""
    import conv_exact_util as U
    from sd_amd import _lib, ops
    L = sdk.library()
    L.sdk_kernel_name.restype = C.c_char_p
    named = {v for v in range(-1, 64) if L.sdk_kernel_name(v) != b"unknown"}
    assert set(ops.AUTOTUNE.VARIANTS) == named - {0, 5}
    info = _lib.ConvPlanInfo()
    for v, (bm, bn) in U.TILE.items():
        a = _gemm_args(_lib, 600, 704, 128)
        a.variant_hint = v + 1
        assert L.sdk_conv2d_plan(C.byref(a), C.byref(info)) == 0, (v, L.sdk_last_error())
        assert info.variant == v and info.grid_tiles == -(-600 // bm) * -(-704 // bn), (v, info.variant, info.grid_tiles)
        a = _gemm_args(_lib, 600, 704, 128, out_mode=2)
        a.variant_hint = v + 1
        assert L.sdk_conv2d_plan(C.byref(a), C.byref(info)) == 0, (v, L.sdk_last_error())
        assert (info.variant == v) == (v in U.GEGLU_OK), (v, info.variant)


def test_committed_tuning_cache_matches_the_conv_source(sdk):
    """configs/conv_tuning_mi355x.json is keyed by the hash of the csrc/conv* files: a stale key loads nothing."""
    from sd_amd import ops
    assert ops._Autotune().load(os.path.join(ROOT, "configs", "conv_tuning_mi355x.json")) > 0


def test_conv_source_hash_covers_what_the_build_compiles(sdk, tmp_path, monkeypatch):
    """The tuning-cache key reads exactly the conv sources and headers the build compiles or lists as dependencies
    of the conv units, and one changed byte in any of them changes the key."""
    import shutil
    from sd_amd import build, ops
    built = set()
    for src, _stem, _defs in build._units():
        if src.startswith("conv"):
            built |= {os.path.basename(d) for d in build._deps(src, build.CSRC) if os.path.basename(d).startswith("conv")}
    hashed = [os.path.basename(f) for f in ops._conv_source_files()]
    assert len(hashed) >= 5 and set(hashed) == built and hashed == sorted(built)
    copy = tmp_path / "csrc"
    shutil.copytree(build.CSRC, copy)
    want = ops._conv_source_hash()
    monkeypatch.setenv("SD_AMD_CONV_SOURCE", str(copy))
    assert ops._conv_source_hash() == want
    monkeypatch.setenv("SD_AMD_CONV_SOURCE", str(copy / hashed[0]))   # a file inside the directory names it too
    assert ops._conv_source_hash() == want
    for name in hashed:
        data = (copy / name).read_bytes()
        (copy / name).write_bytes(data[:-1] + bytes([data[-1] ^ 1]))
        assert ops._conv_source_hash() != want, name
        (copy / name).write_bytes(data)
    assert ops._conv_source_hash() == want


def test_group_norm_workspace(sdk):
    L = sdk.library()
    assert L.sdk_group_norm_workspace(2, 4096, 320) > 0
    assert L.sdk_group_norm_workspace(0, 4096, 320) == 0


def test_ops_refuse_cpu_tensors(sdk):
    from sd_amd import ops
    with pytest.raises(TypeError):
        ops.layer_norm(torch.zeros(4, 8, dtype=torch.float16), torch.ones(8), torch.zeros(8))
    with pytest.raises(TypeError):
        ops.ddim_step(torch.zeros(8), torch.zeros(8), {})


@pytest.mark.parametrize("name", ["unet_tiny", "unet_tiny_uncond", "unet_tiny_headch"])
def test_unet_state_dict_matches_reference(sdk, name):
    from sd_amd.openai_model.model import UNetModel
    z = load(name)
    ref_keys = json.loads(bytes(z["keys"]).decode())
    m = UNetModel(**cfg_of(z))
    mine = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert mine == ref_keys


def test_vae_state_dict_matches_reference(sdk):
    from sd_amd.VAE.autoencoder import AutoEncoderKL
    z = load("vae_tiny")
    ref_keys = json.loads(bytes(z["keys"]).decode())
    m = AutoEncoderKL(ddconfig=cfg_of(z), embed_dim=4, lossconfig={"target": "torch.nn.Identity"})
    mine = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert mine == ref_keys


def test_sd1_config_instantiates_unchanged(sdk):
    """The reference's Diffusion/config.yaml (same targets/params, configs/sd-v1-txt2img.yaml)
    instantiates through the mirrored instantiate_from_config; UNet = 859.52 M params, 686 keys."""
    import yaml
    from sd_amd.Diffusion.utils import instantiate_from_config
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "sd-v1-txt2img.yaml")))
    with torch.device("meta"):
        unet = instantiate_from_config(cfg["model"]["params"]["unet_config"])
    n = sum(p.numel() for p in unet.parameters())
    assert abs(n / 1e6 - 859.52) < 0.01, n
    assert len(unet.state_dict()) == 686
    assert type(unet).__module__ == "sd_amd.openai_model.model"


REF_MODEL_JSON = os.path.join(ROOT, "tests", "golden", "reference_config_model.json")


def test_repo_yaml_equals_reference_config_model_section():
    """configs/sd-v1-txt2img.yaml holds the reference's Diffusion/config.yaml `model` section key
    for key, value for value (parsed with yaml.safe_load).  The reference's section is the golden
    fixture tests/golden/reference_config_model.json: yaml.safe_load of its file, `model` key, as JSON."""
    import yaml
    mine = yaml.safe_load(open(os.path.join(ROOT, "configs", "sd-v1-txt2img.yaml")))
    ref = json.load(open(REF_MODEL_JSON))
    assert mine["model"] == ref


def test_full_latent_diffusion_from_yaml(sdk):
    """The whole reference model config instantiates through the mirrored resolver: LatentDiffusion
    with DiffusionWrapper(UNetModel), AutoEncoderKL and the FrozenCLIPEmbedder cond stage
    (``clip_encoder`` is mirrored), schedule buffers on the host."""
    import yaml
    from sd_amd.Diffusion.utils import instantiate_from_config
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "sd-v1-txt2img.yaml")))
    with torch.device("meta"):
        ld = instantiate_from_config(cfg["model"])
    assert type(ld).__module__ == "sd_amd.Diffusion.ddpm"
    assert type(ld.model.diffusion_model).__module__ == "sd_amd.openai_model.model"
    assert type(ld.first_stage_model).__module__ == "sd_amd.VAE.autoencoder"
    assert type(ld.cond_stage_model).__module__ == "sd_amd.clip_encoder.modules"
    assert ld.model.conditioning_key == "crossattn" and ld.parameterization == "eps"
    assert ld.scale_factor == 0.18215 and ld.num_timesteps == 1000
    assert ld.alphas_cumprod.device.type == "cpu"
    assert abs(sum(p.numel() for p in ld.model.parameters()) / 1e6 - 859.52) < 0.01
