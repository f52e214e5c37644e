"""Exact-input tests of sdk_layer_norm on the MI355X, all five instantiations (run with -m gpu).

The test ids carry the column count that selects the kernel (tests/ln_exact_util.py KERNEL_OF).  Rows are small
integers, so the kernels' pivot-shifted sums are exact and what remains is a fixed sequence of fp32 operations:
every element must be within one fp16 ulp of the float64 value rounded once, and at most 0.5 % of the elements may
differ from it at all — a condition tests/test_gn_stats_inputs.py shows correct fp32 row math to meet on these
inputs with room (it measures under 0.2 %).  ``x`` and ``out`` are strided views into NaN- and sentinel-filled
buffers; nothing may be written outside the view."""
import pytest
import torch

import ln_exact_util as L

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops(sdk):
    from sd_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return o


_PARAMS = {}


def _params(cols):
    if cols not in _PARAMS:
        gamma, beta = L.params(cols)
        _PARAMS[cols] = (gamma.to(DEV), beta.to(DEV))
    return _PARAMS[cols]


def _check(ops, family, rows, cols, x_dev, ref_dev, what):
    """Run on the rows ``x_dev`` [rows, cols] (fp16, on the device) against ``ref_dev``."""
    xbuf, xv = L.guarded_rows(x_dev, cols + 8, DEV)
    obuf, ov = L.out_rows(rows, cols, cols + 24, DEV)
    gamma, beta = _params(cols)
    y = ops.layer_norm(xv, gamma, beta, L.EPS, out=ov)
    torch.cuda.synchronize()
    assert y.data_ptr() == ov.data_ptr()
    assert L.guards_hit(obuf, rows, cols) == 0, f"{what}: wrote outside the output view"
    ulp, share = L.compare(ov, ref_dev)
    print(f"[ln-exact] {what} ({L.KERNEL_OF[cols]}): largest distance {ulp} fp16 ulp, {100 * share:.4f} % differ",
          flush=True)
    assert ulp <= 1, f"{what}: {ulp} fp16 ulp from the float64 value"
    assert share <= L.MAX_DIFFER, f"{what}: {100 * share:.3f} % of the elements differ"


@pytest.mark.parametrize("rows", L.ROWS)
@pytest.mark.parametrize("cols", L.COLS, ids=[f"cols{c}" for c in L.COLS])
@pytest.mark.parametrize("family", L.FAMILIES)
def test_layer_norm_exact(ops, family, cols, rows):
    x, _, _, ref = L.case(family, max(L.ROWS), cols)             # one reference per (family, cols); rows truncate it
    _check(ops, family, rows, cols, x[:rows].half().to(DEV), ref[:rows].to(DEV), f"{family} {rows} x {cols}")


@pytest.mark.parametrize("cols", sorted(L.WALK), ids=[f"cols{c}" for c in sorted(L.WALK)])
def test_layer_norm_walking_waves_exact(ops, cols):
    """More rows than the capped grid holds (2048 blocks of 4 rows; of 64 in the quad form): every wave walks, and
    its last step prefetches the row past the end.  Row r repeats base row r % 4099."""
    rows = L.WALK[cols]
    x, _, _, ref = L.case("hashed", rows, cols)
    idx = (torch.arange(rows, device=DEV) % L.WALK_PERIOD)
    _check(ops, "hashed", rows, cols, x.half().to(DEV)[idx], ref.to(DEV)[idx], f"walking {rows} x {cols}")
