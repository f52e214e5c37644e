"""CPU tests of the chained SpatialTransformer entry's host side (sdk_proj_norm_qkv): the proj_in row permutation of
its packed weight, the routing rule, and the new C ABI symbols in the header / binding / INTEGRATION.md."""
import os

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_perm_formula_for_every_accumulator_element(sdk):
    """Accumulator (chunk c, block nb, lane group cg, q) — packed row 160 c + 16 nb + 4 cg + q of the MFMA's A
    operand — is output channel 32 (g / 2) + 8 cg + 4 (g % 2) + q with g = 10 c + nb."""
    from sd_amd import ops
    perm = ops.proj_qkv_perm()
    assert perm.shape == (320,) and sorted(perm.tolist()) == list(range(320))
    for c in range(2):
        for nb in range(10):
            g = 10 * c + nb
            for cg in range(4):
                for q in range(4):
                    assert perm[160 * c + 16 * nb + 4 * cg + q] == 32 * (g // 2) + 8 * cg + 4 * (g % 2) + q


def test_perm_makes_operand_fragments(sdk):
    """What the permutation is for: blocks 2 ks and 2 ks + 1 of lane group kq hold channels 32 ks + 8 kq + [0, 8),
    the B fragment of K-step ks; and chunk c still covers channels 160 c .. 160 c + 159."""
    from sd_amd import ops
    perm = ops.proj_qkv_perm().tolist()
    for ks in range(10):
        for kq in range(4):
            got = [perm[16 * g + 4 * kq + q] for g in (2 * ks, 2 * ks + 1) for q in range(4)]
            assert got == list(range(32 * ks + 8 * kq, 32 * ks + 8 * kq + 8))
    for c in range(2):
        assert sorted(perm[160 * c:160 * c + 160]) == list(range(160 * c, 160 * c + 160))


def test_pack_then_unpack_gives_back_weight_and_bias(sdk):
    from sd_amd import ops
    g = torch.Generator().manual_seed(1)
    w_in, b_in = torch.randn(320, 320, generator=g), torch.randn(320, generator=g)
    w_qkv = torch.randn(960, 320, generator=g)
    w, b = ops.proj_qkv_pack(w_in.reshape(320, 320, 1, 1), b_in, w_qkv)       # a 1x1 conv weight is flattened
    assert w.shape == (1280, 320) and b.shape == (1280,)
    perm = ops.proj_qkv_perm()
    for p in (0, 5, 17, 161, 319):
        assert torch.equal(w[p], w_in[perm[p]]) and b[p] == b_in[perm[p]]
    assert torch.equal(w[320:], w_qkv) and not b[320:].any()
    uw_in, ub_in, uw_qkv, ub_qkv = ops.proj_qkv_unpack(w, b)
    assert torch.equal(uw_in, w_in) and torch.equal(ub_in, b_in) and torch.equal(uw_qkv, w_qkv) and not ub_qkv.any()
    w2, b2 = ops.proj_qkv_pack(w_in, None, w_qkv, torch.arange(960.))
    assert not b2[:320].any() and torch.equal(b2[320:], torch.arange(960.))
    for bad in ((torch.zeros(640, 640), w_qkv), (w_in, torch.zeros(640, 320))):
        try:
            ops.proj_qkv_pack(bad[0], None, bad[1])
        except ValueError:
            continue
        raise AssertionError("unsupported shapes must be refused")


def test_routing_rule(sdk):
    """One round of 256-row panels, or a last round at least half full."""
    from sd_amd import ops
    fills = ops.proj_qkv_chain_fills
    assert fills(65536, 256)                       # the flagship's 64x64 level at B = 16: 256 panels
    assert fills(512, 256) and fills(16, 256)      # fewer panels than CUs: one round
    assert not fills(16 * 96 * 96, 256)            # 576 panels: two rounds and 64 left over
    assert not fills(8 * 96 * 96, 256)             # C5's 96x96 level, 288 panels: a second round of 32
    assert fills(2 * 65536, 256)                   # the CFG batch: two full rounds
    assert fills(65536 + 128 * 256, 256) and not fills(65536 + 127 * 256, 256)


def test_boundary_symbols(sdk):
    from sd_amd import _lib
    header = open(os.path.join(ROOT, "include", "sdk_amd.h")).read()
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for sym in ("sdk_proj_norm_qkv", "sdk_proj_norm_qkv_supported"):
        assert sym in _lib.EXPORTS, sym
        assert f"int {sym}(" in header, sym
        assert f"`{sym}`" in table, sym
    assert hasattr(sdk.library(), "sdk_proj_norm_qkv")
    L = sdk.library()
    assert L.sdk_proj_norm_qkv_supported(320, 320, 960) == 1 and L.sdk_proj_norm_qkv_supported(640, 640, 1920) == 0
    a = _lib.ProjNormQkvArgs()                     # rejected on the host, before any device call
    assert L.sdk_proj_norm_qkv(a, None) != 0
