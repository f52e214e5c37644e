"""Fused nearest-code search (csrc/vq.hip, ops.vq_nearest) vs a restatement of the reference's three
torch expressions run as torch ops on the same GPU (vqvae/quantize.py:132-163): the b c h w → b h w c
copy, the [M, n_e] fp32 distance matrix, ``argmin``, the embedding gather and z + (e − z), back to
NCHW.  The restatement is the baseline; it shares no code with the kernel under test.
Device time per call from a HIP graph of back-to-back calls (tools/sweep_shape.graph_us: warm-up,
20 calls per replay, median of 7 replays)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.sweep_shape import graph_us  # noqa: E402

# (n_e, e_dim, B, H, W): VQ-f4 at 256² B=8; f8 at M = 8192; the D = 256 codebook at M = 256 and 4096
SHAPES = [(8192, 3, 8, 64, 64), (16384, 4, 8, 32, 32), (1024, 256, 1, 16, 16), (1024, 256, 4, 32, 32)]


def restatement(z, w):
    zp = z.permute(0, 2, 3, 1).contiguous()
    zf = zp.view(-1, w.shape[1])
    d = torch.sum(zf ** 2, dim=1, keepdim=True) + torch.sum(w ** 2, dim=1) - 2 * torch.einsum("bd,dn->bn", zf, w.t())
    idx = torch.argmin(d, dim=1)
    zq = torch.nn.functional.embedding(idx, w).view(zp.shape)
    zq = zp + (zq - zp)
    return zq.permute(0, 3, 1, 2).contiguous(), idx


def main():
    import sd_amd_loader
    sd_amd_loader.load()
    from sd_amd import ops
    dev = torch.device("cuda")
    torch.manual_seed(0)
    print("n_e    e_dim  M      splits  torch_us   fused_us  speedup  fused TFLOP/s (2·M·n_e·e_dim)  idx equal")
    for n, d, b, h, w in SHAPES:
        cb = torch.randn(n, d, device=dev)
        z = torch.randn(b, d, h, w, device=dev)
        norms = ops.vq_code_norms(cb)
        M = b * h * w
        zq1, i1 = ops.vq_nearest(z, cb, norms)
        zq0, i0 = restatement(z, cb)
        same = float((i0 == i1).float().mean())
        t0 = graph_us(lambda: restatement(z, cb))
        t1 = graph_us(lambda: ops.vq_nearest(z, cb, norms))
        sp = ops.lib().sdk_vq_nearest_splits(M, n, d)
        print(f"{n:<7d}{d:<7d}{M:<7d}{sp:<8d}{t0:8.1f}  {t1:9.1f}  {t0 / t1:6.2f}x  {2.0 * M * n * d / t1 / 1e6:8.2f}"
              f"{'':22s}{same:.5f}", flush=True)


if __name__ == "__main__":
    main()
