"""The phase form of the Upsample convs on the MI355X (run with -m gpu): nearest-x2 + conv3x3 pad 1 as four
2x2 convs over the zero-bordered low-res image (ops.PhaseConv, ops.conv2d(phase=True),
sdk_conv_args.upsample_phase).

Exact cases in the style of tests/conv_exact_util.py: inputs and 3x3 weights in {-1, 0, 1} (the folded 2x2
weights are then integers in [-4, 4]), so every product, every partial sum in any order and every output
(|out| <= 9 * 128 + 8 < 2048) is an integer that fp32 accumulation and the fp16 store keep exactly: the output
must EQUAL the float64 reference and the folded-upsample conv, under every admitted tile variant and split."""
import pytest
import torch
import torch.nn.functional as F

import conv_exact_util as U
import gn_stats_exact_util as GS
from gpu_util import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"

# the LDS-DMA tile variants whose linear-issue kernel carries the phase form (csrc/conv.h: the GLDS family of the variant table)
ADMITTED = (2, 3, 4, 6, 7, 16, 17, 18, 19, 22, 23, 24, 25, 26, 31, 32, 33, 38, 40)
REFUSED = (0, 8, 9, 20, 21)        # register-staged and phased kernels: the planner picks an admitted one
B, H, W = 3, 7, 6                  # 126 rows per phase: ragged in every M-tile, tiles cross images


@pytest.fixture(scope="module")
def ops(sdk):
    from sd_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return o


class _Case:
    """One exact problem: CPU inputs, float64 reference [B, 2H, 2W, N], device buffers (built once)."""

    def __init__(self, ops, cin, n, b=B, h=H, w=W):
        g = torch.Generator().manual_seed(1000 * cin + n)
        self.cin, self.n, self.b, self.h, self.w_ = cin, n, b, h, w
        self.x = torch.randint(-1, 2, (b, h, w, cin), generator=g).half()
        self.w = torch.randint(-1, 2, (n, cin, 3, 3), generator=g).float()
        self.bias = torch.randint(-8, 9, (n,), generator=g).float()
        x64 = self.x.double().permute(0, 3, 1, 2)
        ref = F.conv2d(F.interpolate(x64, scale_factor=2, mode="nearest"), self.w.double(), self.bias.double(),
                       padding=1).permute(0, 2, 3, 1).contiguous()
        assert ref.abs().max().item() < U.LIMIT and torch.equal(ref, ref.round())
        self.ref = ref.float()
        self.out_shape, self.out_mode, self.name = tuple(ref.shape), U.OUT_NHWC_F16, f"phase-{cin}-{n}"
        self.cout, self.geglu = n, False
        self._fold = None
        # the conv's own source — the zero-bordered low-res image — out of a NaN-filled buffer (an image of NaN
        # before and after, NaN in the channel gap), so a read outside the image poisons an output
        xpad = F.pad(self.x.permute(0, 3, 1, 2), (1, 1, 1, 1)).permute(0, 2, 3, 1).contiguous()
        self.xpad = U.guarded_nhwc(xpad, cin + 24, DEV)
        self.xdev = U.guarded_nhwc(self.x, cin + 40, DEV)
        self.ppc = ops.PhaseConv(self.w, cin, self.bias, device=DEV)
        self.pc = ops.PackedConv([(self.w, cin)], self.bias, device=DEV)
        assert torch.equal(self.ppc.weight.float().cpu(), self.ppc.weight.float().cpu().round()), "integer fold"

    def fold(self, ops):
        """The folded-upsample 3x3 conv over the same input (the planner's own pick, unsplit), once."""
        if self._fold is None:
            self._fold = ops.conv2d(self.pc, self.xdev, upsample=True, pad=1, split_k=1).float().cpu()
        return self._fold


_CASES = {}


def _case(ops, cin, n, **kw):
    key = (cin, n, tuple(sorted(kw.items())))
    if key not in _CASES:
        _CASES[key] = _Case(ops, cin, n, **kw)
    return _CASES[key]


def _expected_split(cin, split):
    kt = 4 * cin // 64
    per = -(-kt // min(split, kt))
    return -(-kt // per)


def _run_phase(ops, c, variant, split, gn_stats=False):
    """(output tensor, logical output on the CPU, canaries clean, plan).  Statistics attach only to an output as
    wide as Cout, so the gn_stats runs write a plain tensor and the others the sentinel-filled wider buffer."""
    plan = {}
    if gn_stats:
        y = ops.conv2d(c.ppc, c.xpad, phase=True, variant=variant, split_k=split, plan_out=plan, gn_stats=True)
        torch.cuda.synchronize()
        return y, y.float().cpu(), True, plan
    buf, out = U.out_buffer(c, DEV)
    y = ops.conv2d(c.ppc, c.xpad, phase=True, out=out, variant=variant, split_k=split, plan_out=plan)
    assert y.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    got, clean = U.split_out(c, buf)
    return y, got, clean, plan


def _check_plan(c, plan, variant, split):
    if variant is not None:
        assert plan["variant"] == variant, plan
    assert plan["variant"] in ADMITTED, plan
    bm, bn = U.TILE[plan["variant"]]
    assert plan["grid_tiles"] == 4 * -(-c.b * c.h * c.w_ // bm) * -(-c.n // bn), plan      # no tile straddles phases
    if split is not None:
        assert plan["split_k"] == _expected_split(c.cin, split), plan


@pytest.mark.parametrize("split", [1, 2, 3])
@pytest.mark.parametrize("variant", ["auto"] + [str(v) for v in ADMITTED])
@pytest.mark.parametrize("cin,n", [(64, 64), (64, 328), (128, 64), (128, 328)])
def test_phase_conv_exact(ops, cin, n, variant, split):
    c = _case(ops, cin, n)
    v = None if variant == "auto" else int(variant)
    _, got, clean, plan = _run_phase(ops, c, v, split)
    _check_plan(c, plan, v, split)
    U.assert_exact(c, got, plan, ref=c.ref)
    assert clean, f"{c.name}: wrote outside the output's extent (plan {plan})"
    assert torch.equal(got, c.fold(ops)), f"{c.name}: differs from conv2d(upsample=True) (plan {plan})"


@pytest.mark.parametrize("variant", REFUSED)
def test_phase_conv_refused_variants_fall_to_an_admitted_plan(ops, variant):
    c = _case(ops, 64, 328)
    _, got, clean, plan = _run_phase(ops, c, variant, None)
    assert plan["variant"] in ADMITTED and plan["variant"] != variant, plan
    _check_plan(c, plan, None, None)
    U.assert_exact(c, got, plan, ref=c.ref)
    assert clean


def test_phase_conv_rejects_what_it_cannot_do(ops):
    c = _case(ops, 64, 64)
    with pytest.raises(RuntimeError, match="phase form"):
        ops.conv2d(c.ppc, c.xpad, phase=True, split_k=-2)                      # in-launch split-K
    with pytest.raises(RuntimeError, match="phase form"):
        ops.conv2d(c.ppc, c.xpad, phase=True, residual=torch.zeros(c.out_shape, dtype=torch.float16, device=DEV))


def _check_partials(ops, c, y, plan):
    part = getattr(y, ops.GN_ATTR, None)
    assert part is not None and plan["gn_chunks"] > 0, f"plan {plan} should emit GroupNorm statistics"
    pp, nch, _ = part
    rows = 4 * c.h * c.w_
    assert pp.shape == (c.b, nch, c.n, 2) and nch == plan["gn_chunks"] and rows % nch == 0
    # every (image, chunk, channel) pair against the float64 statistics of exactly that chunk's stored rows, phase
    # major (a swapped chunk leaves every merged statistic unchanged), under the operation-count bound of the route
    # that emitted (tests/gn_stats_exact_util.py): the split-K reduce's 32 row lanes, else the tile's row blocks
    s = GS.REDUCE_S if plan["split_k"] > 1 else GS.tile_s(U.TILE[plan["variant"]][0])
    GS.check_chunk_stats(pp, y, s, phase=True, what=f"{c.name} plan {plan}")
    # the tolerances of test_conv_emits_group_norm_statistics stay: at these magnitudes (|y| up to 100) they are the
    # tighter ones for the mean
    t = GS.phase_major(y).double().reshape(c.b, nch, rows // nch, c.n)
    mean = t.mean(2)
    m2 = ((t - mean[:, :, None]) ** 2).sum(2)
    assert torch.allclose(pp[..., 0].double().cpu(), mean.cpu(), rtol=1e-5, atol=1e-4)
    assert rel_l2(pp[..., 1].double().cpu(), m2.cpu()) < 1e-4
    if c.n % 32 == 0:      # finalized: GroupNorm from the partials == GroupNorm from its own statistics pass
        g = torch.Generator().manual_seed(7)
        gamma = torch.rand(c.n, generator=g) + 0.5
        beta = torch.randn(c.n, generator=g) * 0.1
        s1 = ops.group_norm_scale_shift(y, gamma.to(DEV), beta.to(DEV), 1e-5, 32)
        s0 = ops.group_norm_scale_shift(y.clone(), gamma.to(DEV), beta.to(DEV), 1e-5, 32)
        assert rel_l2(s1[0], s0[0]) < 1e-3 and rel_l2(s1[1], s0[1]) < 1e-3
        # ... and within the three-rounding bounds of the float64 merge of the same fp32 partials
        ref = GS.Affine(*GS.merge_partials([pp.cpu()], rows, 32), 1e-5, gamma, beta, c.n // 32,
                        amax=y.abs().max().item())
        rs, rh = ref.ratios(*s1)
        assert rs <= 1.0 and rh <= 1.0, f"{c.name}: finalize of the emitted partials off by {rs:.3g} / {rh:.3g} of the bound"


@pytest.mark.parametrize("split", [2, 3])
@pytest.mark.parametrize("cin,n", [(64, 64), (128, 328)])
def test_phase_conv_split_reduce_emits_group_norm_statistics(ops, cin, n, split):
    """The split-K reduce applies the row -> pixel map and emits the image's statistics (one chunk of 168 rows)."""
    c = _case(ops, cin, n)
    y, got, clean, plan = _run_phase(ops, c, None, split, gn_stats=True)
    U.assert_exact(c, got, plan, ref=c.ref)
    assert clean
    _check_partials(ops, c, y, plan)


@pytest.mark.parametrize("variant", ADMITTED)
def test_phase_conv_tile_epilogue_emits_group_norm_statistics(ops, variant):
    """16x16 -> 32x32: 256 rows per (image, phase), whole 128- and 256-row tiles: the tile epilogue emits one chunk
    per (phase, M-tile), equal counts, phase major inside the image."""
    c = _case(ops, 64, 64, b=2, h=16, w=16)
    y, got, clean, plan = _run_phase(ops, c, variant, 1, gn_stats=True)
    _check_plan(c, plan, variant, 1)
    assert plan["gn_chunks"] == 4 * 256 // U.TILE[variant][0]
    U.assert_exact(c, got, plan, ref=c.ref)
    assert clean
    _check_partials(ops, c, y, plan)


def test_zero_border_exact(ops):
    c = _case(ops, 64, 64)
    y = ops.zero_border(c.xdev, 1)
    want = F.pad(c.x.permute(0, 3, 1, 2), (1, 1, 1, 1)).permute(0, 2, 3, 1)
    assert y.shape == want.shape and y.is_contiguous()
    assert torch.equal(y.cpu(), want)


def test_phase_conv_random_data_error_within_twice_the_fold_form(ops):
    """N(0, 1) activations, 0.02 N(0, 1) weights.  Against the float64 conv on the same fp16 inputs and fp16 3x3
    weights the fold form's error is the fp16 rounding of the output; the phase form adds one fp16 rounding of each
    summed weight, an independent error of the same relative size: sqrt(2) x.  Limit 2 x (summation order)."""
    g = torch.Generator().manual_seed(5)
    b, h, w, cin, n = 2, 8, 8, 128, 128
    x = torch.randn(b, h, w, cin, generator=g).half()
    wt = (0.02 * torch.randn(n, cin, 3, 3, generator=g)).half().float()
    bias = torch.randn(n, generator=g) * 0.1
    ref = F.conv2d(F.interpolate(x.double().permute(0, 3, 1, 2), scale_factor=2, mode="nearest"), wt.double(),
                   bias.double(), padding=1).permute(0, 2, 3, 1)
    xd = x.to(DEV)
    fold = ops.conv2d(ops.PackedConv([(wt, cin)], bias, device=DEV), xd, upsample=True, pad=1)
    phase = ops.conv2d(ops.PhaseConv(wt, cin, bias, device=DEV), ops.zero_border(xd, 1), phase=True)
    e_fold = ((fold.double().cpu() - ref).norm() / ref.norm()).item()
    e_phase = ((phase.double().cpu() - ref).norm() / ref.norm()).item()
    print(f"[parity] upsample conv rel-L2 vs float64: fold {e_fold:.3e}  phase {e_phase:.3e}  "
          f"ratio {e_phase / e_fold:.3f} (<= 2)", flush=True)
    assert e_phase <= 2.0 * e_fold


@pytest.mark.parametrize("which", ["unet", "vae"])
def test_upsample_modules_both_routes_vs_oracle(ops, sdk, which, monkeypatch):
    """A tiny UNet Upsample and a tiny VAE Upsample under the phase route (default) and the materialised route
    (the A/B switch), each against the oracle's interpolate + conv, at the conv parity limit of
    tests/test_gpu_kernels.py (rel-L2 2e-3)."""
    from oracle import unet_ref, vae_ref
    from sd_amd import packing as P
    from sd_amd.openai_model import model as M
    from sd_amd.Unet import unet as V
    torch.manual_seed(3)
    ch = 64
    mod = M.Upsample(ch, True) if which == "unet" else V.Upsample(ch, True)
    with torch.no_grad():
        mod.conv.weight.mul_(0.5)
    mod._prepare(DEV)
    assert mod._ppc is not None
    x = torch.randn(2, 8, 8, ch).half()
    sd = {"conv.weight": mod.conv.weight.detach().half().float(), "conv.bias": mod.conv.bias.detach().float()}
    up = F.interpolate(x.float().permute(0, 3, 1, 2), scale_factor=2, mode="nearest")
    ref = (unet_ref._conv(up, sd, "conv") if which == "unet" else vae_ref._conv(up, sd, "conv")).permute(0, 2, 3, 1)
    seen = []
    real = ops.conv2d

    def spy(pc, *a, **kw):
        seen.append(bool(kw.get("phase")))
        return real(pc, *a, **kw)

    monkeypatch.setattr(ops, "conv2d", spy)
    for materialise in (False, True):
        monkeypatch.setattr(P, "UPSAMPLE_MATERIALISE", materialise)
        y = mod._run(x.to(DEV))
        assert seen[-1] == (not materialise), "the switch selects the route"
        assert y.shape == ref.shape
        e = rel_l2(y, ref)
        print(f"[parity] {which} Upsample {'materialised' if materialise else 'phase'} vs oracle: rel-L2 {e:.3e}",
              flush=True)
        assert e < 2e-3
