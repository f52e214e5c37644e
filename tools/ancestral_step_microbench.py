"""Fused ancestral step + known-region blend (csrc/sampler.hip: sdk_posterior_step, sdk_masked_q_sample)
vs a restatement of the reference's torch expressions run as torch ops on the same GPU
(ldm/diffusion/ddpm.py: predict_start_from_noise :314-322, clamp_ :1565, q_posterior :325-338, the
noise term of p_sample :1621-1636, q_sample + blend of p_sample_loop :1783-1784).  The restatement is
the baseline; it shares no code with the kernels under test.

Two times per shape, each the lower of two alternated medians of 7 windows after a warm-up:
* eager: 200 steps between two device events, host launches included — what a sampler loop pays;
* graph: device time per step from a HIP graph of 20 back-to-back steps (tools/sweep_shape.graph_us).
Both paths are also compared on the same inputs (max |difference|; 0 means bit-equal up to the last
bit of exp(0.5 logvar), which torch evaluates on the device here and the fused path takes from the host)."""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.sweep_shape import graph_us  # noqa: E402

SHAPES = [(16, 4, 64, 64), (1, 4, 64, 64)]
T_STEP = 417
TEMPERATURE = 1.0


def eager_us(fn, per=200, reps=7, warm=50):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(per):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / per)
    return sorted(ts)[len(ts) // 2]


def main():
    import sd_amd_loader
    sd_amd_loader.load()
    from sd_amd import ops
    from sd_amd.DDIM.diffusion_modules import register_schedule
    dev = torch.device("cuda")
    torch.manual_seed(0)
    sch = register_schedule(1000, 0.00085, 0.012)
    host = {k: v.numpy() for k, v in sch.items() if torch.is_tensor(v)}
    tab = {"c_recip": host["sqrt_recip_alphas_cumprod"], "c_recipm1": host["sqrt_recipm1_alphas_cumprod"],
           "coef1": host["posterior_mean_coef1"], "coef2": host["posterior_mean_coef2"],
           "sigma": np.asarray([math.exp(0.5 * float(v)) for v in host["posterior_log_variance_clipped"]],
                               dtype=np.float32)}
    buf = {k: v.to(dev) for k, v in sch.items() if torch.is_tensor(v)}
    print("shape            path    torch_us  fused_us  speedup   max|diff|")
    for shape in SHAPES:
        b = shape[0]
        x, eps, nz, x0, qn = (torch.randn(shape, device=dev) for _ in range(5))
        mask = (torch.rand(b, 1, *shape[2:], device=dev) > 0.5).float()
        t = torch.full((b,), T_STEP, device=dev, dtype=torch.long)
        ext = lambda a: a[t].reshape(b, 1, 1, 1)                                      # noqa: E731

        def torch_step():
            x_recon = ext(buf["sqrt_recip_alphas_cumprod"]) * x - ext(buf["sqrt_recipm1_alphas_cumprod"]) * eps
            x_recon.clamp_(-1., 1.)
            mean = ext(buf["posterior_mean_coef1"]) * x_recon + ext(buf["posterior_mean_coef2"]) * x
            logvar = ext(buf["posterior_log_variance_clipped"])
            noise = nz * TEMPERATURE
            nonzero = (1 - (t == 0).float()).reshape(b, 1, 1, 1)
            img = mean + nonzero * (0.5 * logvar).exp() * noise
            img_orig = ext(buf["sqrt_alphas_cumprod"]) * x0 + ext(buf["sqrt_one_minus_alphas_cumprod"]) * qn
            return img_orig * mask + (1. - mask) * img

        def fused_step():
            img, _ = ops.posterior_step(x, eps, T_STEP, tab, noise=nz, clip=True, temperature=TEMPERATURE)
            return ops.masked_q_sample(x0, qn, mask, img, T_STEP, host["sqrt_alphas_cumprod"],
                                       host["sqrt_one_minus_alphas_cumprod"], out=img)

        diff = float((torch_step() - fused_step()).abs().max())
        for path, timer in (("eager", eager_us), ("graph", graph_us)):
            t0, t1 = timer(torch_step), timer(fused_step)
            t0b, t1b = timer(torch_step), timer(fused_step)                           # alternated repeat
            t0, t1 = min(t0, t0b), min(t1, t1b)
            print(f"{str(shape):<17s}{path:<8s}{t0:8.1f}  {t1:8.1f}  {t0 / t1:6.2f}x   {diff:.1e}", flush=True)


if __name__ == "__main__":
    main()
