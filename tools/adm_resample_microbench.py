"""GroupNorm + SiLU + 2x resample with two outputs (csrc/norm.hip: sdk_group_norm_resample, the resampling
ResBlock's in_layers norm) vs (1) the composition it replaces on this code base: ``ops.group_norm`` (+ SiLU),
then one resample pass for h and one for x; (2) the reference's torch expressions on the same GPU
(openai_model/model.py:233-238: GroupNorm32 in fp32 cast back, nn.SiLU, avg_pool2d / interpolate nearest of h
and of x, NCHW fp16).

All three start from the raw tensor and include the GroupNorm statistics pass; ``kernel`` is the fused launch
alone (statistics given) and its GB/s is over the algorithmic bytes: one read of x, two writes (the zero border
of the activated output included).  Device time per call from a HIP graph of ``PER`` back-to-back calls
(tools/sweep_shape.graph_us), the lower of two alternated medians of 7 windows after a warm-up.  The tensors of
one call (42-105 MB) fit in the 256 MB last-level cache, so the GB/s is not an HBM rate."""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.sweep_shape import graph_us  # noqa: E402

CASES = [((16, 64, 64, 320), "down"), ((16, 32, 32, 640), "up")]
PER = 100
EPS = 1e-5


def main():
    import sd_amd_loader
    sd_amd_loader.load()
    from sd_amd import ops
    dev = torch.device("cuda")
    torch.manual_seed(0)
    print("shape               mode  torch_us  composed_us  fused_us  kernel_us  kernel_GB/s  fused/composed  act rel-L2")
    for shape, mode in CASES:
        B, H, W, C = shape
        x = (torch.randn(shape, device=dev) * 1.5 + 0.5).half()
        xn = x.permute(0, 3, 1, 2).contiguous()                  # the reference's layout
        gamma, beta = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.1
        Ho, Wo = (H // 2, W // 2) if mode == "down" else (2 * H, 2 * W)
        nbytes = 2 * C * B * (H * W + (Ho + 2) * (Wo + 2) + Ho * Wo)

        def torch_ref():
            h = F.silu(F.group_norm(xn.float(), 32, gamma, beta, EPS).type(xn.dtype))
            if mode == "down":
                return F.avg_pool2d(h, 2), F.avg_pool2d(xn, 2)
            return F.interpolate(h, scale_factor=2, mode="nearest"), F.interpolate(xn, scale_factor=2, mode="nearest")

        def composed():
            h = ops.group_norm(x, gamma, beta, EPS, silu=True)
            if mode == "down":                                   # the conv then pads by masking (pad 1)
                return ops.group_norm_resample(h, None, "down")[1], ops.group_norm_resample(x, None, "down")[1]
            return ops.upsample_nearest2x_padded(h, 1), ops.upsample_nearest2x_padded(x, 0)

        def fused():
            return ops.group_norm_resample(x, ops.group_norm_scale_shift(x, gamma, beta, EPS), mode, silu=True, pad=1)

        gn = ops.group_norm_scale_shift(x, gamma, beta, EPS)

        def kernel():
            return ops.group_norm_resample(x, gn, mode, silu=True, pad=1)

        ref = torch_ref()[0].permute(0, 2, 3, 1).float()
        got = fused()[0][:, 1:-1, 1:-1].float()
        err = float((got - ref).norm() / ref.norm())
        ts = {}
        for rnd in range(2):                                     # alternated repeat
            for name, fn in (("torch", torch_ref), ("composed", composed), ("fused", fused), ("kernel", kernel)):
                t = graph_us(fn, per=PER)
                ts[name] = min(ts.get(name, t), t)
        print(f"{str(shape):<20s}{mode:<5s}{ts['torch']:9.1f}  {ts['composed']:11.1f}  {ts['fused']:8.1f}  "
              f"{ts['kernel']:9.1f}  {nbytes / ts['kernel'] * 1e-3:11.0f}  {ts['fused'] / ts['composed']:13.2f}x  "
              f"{err:.2e}", flush=True)


if __name__ == "__main__":
    main()
