"""The phase form of nearest-x2 + conv3x3 (ops.fold_upsample_weight) is the reference math regrouped:
four 2x2 convs over the zero-bordered low-res image, one per output parity, against float64
F.interpolate + F.conv2d.  Integer weights and inputs, so every sum is exact and the results must be EQUAL,
borders included."""
import pytest
import torch
import torch.nn.functional as F

import sd_amd_loader

sd_amd_loader.load()
from sd_amd.ops import fold_upsample_weight  # noqa: E402


def phase_conv_reference(x, w, bias=None):
    """x [B, C, H, W], w [N, C, 3, 3] -> [B, N, 2H, 2W] through the four phase kernels."""
    ph = fold_upsample_weight(w)
    xp = F.pad(x, (1, 1, 1, 1))
    B, _, H, W = x.shape
    y = x.new_zeros(B, w.shape[0], 2 * H, 2 * W)
    for a in range(2):
        for b in range(2):
            # window origin (i + a, j + b) of the zero-bordered image, 2x2 taps
            y[:, :, a::2, b::2] = F.conv2d(xp[:, :, a:a + H + 1, b:b + W + 1], ph[2 * a + b])
    return y if bias is None else y + bias[None, :, None, None]


@pytest.mark.parametrize("H,W", [(5, 4), (1, 1)])
def test_fold_equals_interpolate_conv_float64(H, W):
    g = torch.Generator().manual_seed(11 * H + W)
    x = torch.randint(-3, 4, (2, 6, H, W), generator=g).double()
    w = torch.randint(-2, 3, (5, 6, 3, 3), generator=g).double()
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1)
    got = phase_conv_reference(x, w)
    assert got.shape == ref.shape
    assert torch.equal(got, ref)


def test_fold_keeps_dtype_and_sums_taps():
    w = torch.arange(9, dtype=torch.float32).reshape(1, 1, 3, 3)
    ph = fold_upsample_weight(w)
    assert ph.dtype == torch.float32 and ph.shape == (4, 1, 1, 2, 2)
    # every phase redistributes all nine taps
    assert all(float(ph[q].sum()) == 36.0 for q in range(4))
    # phase (0, 0): rows {w0, w1 + w2}, columns alike
    assert ph[0, 0, 0].tolist() == [[0.0, 1.0 + 2.0], [3.0 + 6.0, 4.0 + 5.0 + 7.0 + 8.0]]
    # phase (1, 1): rows {w0 + w1, w2}
    assert ph[3, 0, 0].tolist() == [[0.0 + 1.0 + 3.0 + 4.0, 2.0 + 5.0], [6.0 + 7.0, 8.0]]
