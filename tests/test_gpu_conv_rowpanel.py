"""Exact per-element tests of the row-panel-stationary conv kernel (csrc/conv_rowpanel.hip, variant 49) on the
MI355X (run with -m gpu).

The helpers of tests/conv_exact_util.py make every case exact: integer-valued fp16 inputs, a float64 CPU reference,
sources and residual read out of NaN-filled buffers with a channel gap, the output written into a sentinel-filled
buffer wider than Cout.  Every case asserts that the plan reports variant 49 with split_k 1, that the output EQUALS
the reference element for element, that nothing outside the output's extent was written, and that the whole output
buffer has the bits of the same problem forced to variant 22 (the 256x320 tile on the same MFMA shape and K order).

Shapes, the smallest at which the kernel takes another path:
  M in {256, 257, 511, 768}: one exact 256-row panel, one ragged row in a second panel, a ragged last panel, three
  panels;  N in {160, 200, 320, 480}: one 160-column chunk, a partial last chunk, a chunk seam, three chunks (with
  K = 320 that is 15 slots through the 6-slot W ring: it wraps across chunks);  K in {32, 96, 320}: one slot per chunk
  (fewer K-steps than ring slots, only the lower K-step of the slot), an odd K-step count, the flagship's five slots.
Epilogues: none, bias, residual (row stride wider than N), bias + residual.
K = 352 and a 3x3 conv are outside the kernel's reach: forced to 49 they must plan another variant and stay exact."""
import pytest
import torch

import conv_exact_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROWPANEL, TILE22 = 49, 22
MS, NS, KS = (256, 257, 511, 768), (160, 200, 320, 480), (32, 96, 320)
EPILOGUES = {"none": (False, False, False), "bias": (True, False, False), "res": (False, False, True),
             "bias_res": (True, False, True)}


@pytest.fixture(scope="module")
def ops(sdk):
    from sd_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return o


_CASES = {}


def _case(M, N, K, epi, ksize=1):
    """The case (inputs seeded by its name) with its reference, built once."""
    name = f"rowpanel-m{M}-n{N}-k{K}-{epi}-ks{ksize}"
    if name not in _CASES:
        hw = (M, 1) if ksize == 1 else (M // 8, 8)
        _, kw = U._conv_case(name, hw, [K], cout=N, k=ksize, pad=ksize // 2, epi=EPILOGUES[epi], B=1)
        _CASES[name] = U.Case(name, **kw)
    return _CASES[name]


def _run(ops, c, variant):
    """Launch the case forced to ``variant``; returns (output buffer, logical output, canaries clean, plan)."""
    cin = c.srcs[0].shape[-1]
    x = U.guarded_nhwc(c.srcs[0], cin + 24, DEV)
    pc = ops.PackedConv([(c.w, cin)], c.bias, geglu=False, device=DEV)
    res = None if c.residual is None else U.guarded_residual(c.residual, c.nout + 16, DEV)
    buf, out = U.out_buffer(c, DEV)
    plan = {}
    y = ops.conv2d(pc, x, ksize=c.ksize, stride=1, pad=c.pad, residual=res, out=out, variant=variant, plan_out=plan)
    assert y.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    got, clean = U.split_out(c, buf)
    return buf.cpu(), got, clean, plan


@pytest.mark.parametrize("epi", list(EPILOGUES))
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", MS)
def test_rowpanel_exact(ops, M, N, K, epi):
    c = _case(M, N, K, epi)
    buf, got, clean, plan = _run(ops, c, ROWPANEL)
    assert plan["variant"] == ROWPANEL and plan["split_k"] == 1, plan
    assert plan["grid_tiles"] == -(-M // 256) * -(-N // 160), plan
    U.assert_exact(c, got, plan)
    assert clean, f"{c.name}: wrote outside the output's extent; plan {plan}"
    buf22, got22, clean22, plan22 = _run(ops, c, TILE22)
    assert plan22["variant"] == TILE22 and plan22["split_k"] == 1, plan22
    U.assert_exact(c, got22, plan22)
    assert torch.equal(buf.view(torch.int16), buf22.view(torch.int16)), f"{c.name}: bits differ from variant 22"


@pytest.mark.parametrize("M,N,K,ksize", [(256, 160, 352, 1), (256, 160, 64, 3)], ids=["k352", "ksize3"])
def test_rowpanel_not_honoured(ops, M, N, K, ksize):
    """The honoured-variant rule: a conv the kernel cannot run plans another variant when 49 is forced."""
    c = _case(M, N, K, "bias", ksize)
    _, got, clean, plan = _run(ops, c, ROWPANEL)
    assert plan["variant"] != ROWPANEL and plan["variant"] in U.TILE, plan
    U.assert_exact(c, got, plan)
    assert clean, f"{c.name}: wrote outside the output's extent; plan {plan}"
