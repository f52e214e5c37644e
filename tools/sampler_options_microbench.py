"""Does fusing the next iteration's known-region blend into the DDIM step pay?  One masked DDIM iteration at
(16, 4, 64, 64), eta = 1, three ways on the same device tensors:

* (a) fused:  ``ops.ddim_step(..., blend_*)`` — one launch of ``sdk_ddim_step_ex``;
* (b) split:  ``ops.ddim_step`` then ``ops.masked_q_sample`` — the two launches the loop would otherwise make;
* (c) torch:  the reference's expressions (``ddim.py:146-147,195-203``) with torch on the device.

Each time is one window of 200 calls between two device events after a warm-up, host launches included (at this
size the kernels are bound by launch cost, not bandwidth).  The three arms alternate, 7 repetitions in one run;
the table gives every repetition, and per arm the median and the spread (max - min).  The fused blend is kept
only if median(a) < median(b) - spread(b)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPE = (16, 4, 64, 64)
CALLS, REPS, WARM = 200, 7, 50


def window_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / CALLS


def main():
    import sd_amd_loader
    sd_amd_loader.load()
    from sd_amd import ops
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(0)
    x, e, nz, x0, qn = (torch.randn(SHAPE, generator=g).to(dev) for _ in range(5))
    mask = (torch.rand(SHAPE[0], 1, *SHAPE[2:], generator=g) > 0.5).float().to(dev)
    f32 = np.float32
    a_t, a_prev, sigma = f32(0.5), f32(0.6), f32(0.3)
    sc = {"sqrt_one_minus_at": float(np.sqrt(f32(1) - a_t)), "sqrt_at": float(np.sqrt(a_t)),
          "dir_coef": float(np.sqrt(f32(f32(1) - a_prev) - sigma * sigma)), "sqrt_a_prev": float(np.sqrt(a_prev)),
          "sigma": float(sigma)}
    sa, s1m = np.asarray([np.sqrt(a_prev)], dtype=f32), np.asarray([np.sqrt(f32(1) - a_prev)], dtype=f32)
    xp, p0, xn = (torch.empty_like(x) for _ in range(3))

    def fused():
        return ops.ddim_step(x, e, sc, noise=nz, x_prev=xp, pred_x0=p0, blend_x0=x0, blend_noise=qn, blend_mask=mask,
                             blend_sqrt_acp=float(sa[0]), blend_sqrt_1m_acp=float(s1m[0]), x_next=xn)[2]

    def split():
        ops.ddim_step(x, e, sc, noise=nz, x_prev=xp, pred_x0=p0)
        return ops.masked_q_sample(x0, qn, mask, xp, 0, sa, s1m, out=xn)

    full = lambda v: torch.full((SHAPE[0], 1, 1, 1), float(v), device=dev)          # noqa: E731

    def torch_ref():
        at, ap, sg, s1 = full(a_t), full(a_prev), full(sigma), full(sc["sqrt_one_minus_at"])
        pred = (x - s1 * e) / at.sqrt()
        dir_xt = (1. - ap - sg ** 2).sqrt() * e
        x_prev = ap.sqrt() * pred + dir_xt + sg * nz * 1.0
        img_orig = float(sa[0]) * x0 + float(s1m[0]) * qn
        return img_orig * mask + (1. - mask) * x_prev

    ra, rb, rc = fused().clone(), split().clone(), torch_ref()
    print(f"one masked DDIM iteration at {SHAPE}, eta > 0; {CALLS} calls per window, {REPS} alternated repetitions")
    print(f"fused == split bit for bit: {torch.equal(ra, rb)}; max |fused - torch| {float((ra - rc).abs().max()):.1e}")
    arms = (("fused", fused), ("split", split), ("torch", torch_ref))
    for _, fn in arms:
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k, _ in arms}
    print("repeat   fused_us  split_us  torch_us")
    for rep in range(REPS):
        for k, fn in arms:
            times[k].append(window_us(fn))
        print(f"{rep:<8d} {times['fused'][-1]:8.2f}  {times['split'][-1]:8.2f}  {times['torch'][-1]:8.2f}", flush=True)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    spread = {k: max(v) - min(v) for k, v in times.items()}
    print("median   " + "  ".join(f"{med[k]:8.2f}" for k in ("fused", "split", "torch")))
    print("spread   " + "  ".join(f"{spread[k]:8.2f}" for k in ("fused", "split", "torch")))
    keep = med["fused"] < med["split"] - spread["split"]
    print(f"median(fused) < median(split) - spread(split): {keep} "
          f"({med['fused']:.2f} vs {med['split'] - spread['split']:.2f}) -> the fused blend {'stays' if keep else 'goes'}")


if __name__ == "__main__":
    main()
