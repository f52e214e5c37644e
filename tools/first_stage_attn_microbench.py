"""Microbenchmark of the first-stage attention kernels on the MI355X.

  python tools/first_stage_attn_microbench.py [--rounds 7] [--out profiles/first_stage_attn_microbench.txt]

(a) the wide kernel: ops.attention at (B, 1, 4096, 4096, 512), B in {1, 16};
(b) the existing 8 x 64 form at the same B, n, bytes and FLOPs (the yardstick of what the wide head costs);
(c) the reference's expressions for AttentionBlock (bmm, scale, softmax, bmm in fp16) on the same device tensors;
and ops.linear_attention against the reference's two einsums (softmax over the tokens, fp16) at (16, 1, 4096, 512).

The arms of a group run alternated in one process, ``--rounds`` rounds of ``--iters`` launches each, timed with
device events; per arm the median, minimum and maximum round are reported (the spread), the achieved FLOP/s from
the algorithm's 4 B n^2 d, and the peak device memory of one call above the inputs (torch's allocator; the
kernels' own workspaces come from it too).  Inputs are seeded normal data (zeros would flatter the softmax)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sd_amd_loader                                    # noqa: E402

sd_amd_loader.load()
from sd_amd import ops                                  # noqa: E402

DEV = "cuda"


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    y = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del y
    return peak


def group(title, arms, flops, rounds, iters, lines):
    """arms: [(name, fn)]; alternated rounds."""
    for _, fn in arms:                                   # warm-up: code objects, allocator, dynamic-LDS attribute
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {n: [] for n, _ in arms}
    for _ in range(rounds):
        for n, fn in arms:
            ms[n].append(timed(fn, iters))
    lines.append(title)
    for n, fn in arms:
        v = ms[n]
        med = statistics.median(v)
        lines.append(f"  {n:<34} median {med:9.3f} ms  min {min(v):9.3f}  max {max(v):9.3f}  "
                     f"{flops / (med * 1e-3) / 1e12:7.1f} TFLOP/s  peak memory {peak_bytes(fn) / 2 ** 20:9.1f} MiB")
    print("\n".join(lines[-len(arms) - 1:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, C = a.n, 512
    lines = [f"first-stage attention microbench: n = {n}, C = {C}, {a.rounds} alternated rounds x {a.iters} launches, "
             f"device {torch.cuda.get_device_name(0)}"]
    for B in (1, 16):
        g = torch.Generator().manual_seed(B)
        q, k, v = (torch.randn(B * n, C, generator=g).half().to(DEV) for _ in range(3))
        scale = C ** -0.5

        def wide():
            return ops.attention(q, k, v, batch=B, heads=1, nq=n, nk=n, head_dim=C, scale=scale)

        def heads8():
            return ops.attention(q, k, v, batch=B, heads=8, nq=n, nk=n, head_dim=C // 8, scale=(C // 8) ** -0.5)

        def reference():
            qq, kk, vv = q.view(B, n, C), k.view(B, n, C), v.view(B, n, C)
            w = torch.bmm(qq, kk.transpose(1, 2)) * scale
            w = torch.nn.functional.softmax(w, dim=2)
            return torch.bmm(w, vv).view(B * n, C)

        rel = ((wide().float() - reference().float()).norm() / reference().float().norm()).item()
        lines.append(f"B = {B}: wide vs the fp16 reference expressions rel-L2 {rel:.2e}")
        group(f"attention (B, 1, {n}, {n}, {C}), B = {B}",
              [("(a) wide, 1 x 512", wide), ("(b) 8 x 64 form", heads8), ("(c) bmm/softmax/bmm fp16", reference)],
              4.0 * B * n * n * C, a.rounds, a.iters, lines)
        del q, k, v
    B = 16
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(B * n, C, generator=g).half().to(DEV) for _ in range(3))

    def lin():
        return ops.linear_attention(q, k, v, batch=B, heads=1, n=n, dim_head=C)

    def lin_ref():
        q4, k4, v4 = (t.view(B, n, 1, C).permute(0, 2, 3, 1) for t in (q, k, v))        # b h c n
        ctx = torch.einsum("bhdn,bhen->bhde", k4.softmax(dim=-1), v4)
        return torch.einsum("bhde,bhdn->bhen", ctx, q4)

    group(f"linear attention ({B}, 1, {n}, {C})", [("sdk_linear_attention", lin), ("softmax + two einsums fp16", lin_ref)],
          4.0 * B * n * C * C, a.rounds, a.iters, lines)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
