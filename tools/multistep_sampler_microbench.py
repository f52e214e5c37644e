"""What does the fused multistep update cost against the same expressions written as torch ops?  One sampler update
at (16, 4, 64, 64) on the same device tensors, for four forms — PLMS with three history entries and DPM-Solver++
second order, each with and without the classifier-free-guidance combine:

* fused:  ``ops.multistep_step`` — one launch of ``sdk_multistep_step`` (outputs preallocated);
* torch:  the formulas of DESIGN.md §3.2 with torch on the device, the history entry written with ``copy_``.

Both arms run eager and as a captured linear graph (``torch.cuda.graph``, one update per replay).  Each time is one
window of 200 calls between two device events after a warm-up, host launches included: at this size (1 MiB per
tensor) the update is bound by launch cost, not bandwidth.  The arms alternate, 7 repetitions in one run; the table
gives every repetition, and per arm the median and the spread (max - min).

``--models``: also build the SD-1 512² B = 16 benchmark model (bench.py's ``c3`` configuration, seeded weights) and
report img/s of DDIM at S = 50, DPM-Solver++ at S = 20 and PLMS at S = 25, sampling + decode, graphs on."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = (16, 4, 64, 64)
CALLS, REPS, WARM = 200, 7, 50
GUIDANCE = 7.5


def window_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / CALLS


def graphed(fn):
    """``fn`` captured once on a side stream's warm-up, replayed per call."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def update_arms(ops, dev):
    """{form: (fused, torch_ref, outputs of each)} on one set of device tensors."""
    gen = torch.Generator(device="cpu").manual_seed(0)
    x, e, eu, h1, h2, h3 = (torch.randn(SHAPE, generator=gen).to(dev) for _ in range(6))
    f32 = np.float32
    a_t, a_prev = f32(0.5), f32(0.6)
    sc = {"sqrt_one_minus_at": float(np.sqrt(f32(1) - a_t)), "sqrt_at": float(np.sqrt(a_t)),
          "dir_coef": float(np.sqrt(f32(1) - a_prev)), "sqrt_a_prev": float(np.sqrt(a_prev)), "sigma": 0.0}
    coefs = (float(f32(1.1)), float(f32(0.45)), float(f32(-0.12)))
    s1m, sa, dirc, sap = sc["sqrt_one_minus_at"], sc["sqrt_at"], sc["dir_coef"], sc["sqrt_a_prev"]
    arms = {}
    for cfg in (False, True):
        xp, p0, ho, tp, tq, th = (torch.empty_like(x) for _ in range(6))
        gkw = dict(e_uncond=eu, guidance=GUIDANCE) if cfg else {}

        def plms(xp=xp, p0=p0, ho=ho, gkw=gkw):
            return ops.multistep_step(x, e, sc, "plms", history=[h1, h2, h3], x_prev=xp, pred_x0=p0, hist_out=ho, **gkw)

        def plms_torch(cfg=cfg, th=th):
            eg = eu + GUIDANCE * (e - eu) if cfg else e
            th.copy_(eg)
            ep = (55 * eg - 59 * h1 + 37 * h2 - 9 * h3) / 24
            pred = (x - s1m * ep) / sa
            return sap * pred + dirc * ep, pred

        def dpm(xp=xp, p0=p0, ho=ho, gkw=gkw):
            return ops.multistep_step(x, e, sc, "dpm", history=[h1], coefs=coefs, x_prev=xp, pred_x0=p0, hist_out=ho,
                                      **gkw)

        def dpm_torch(cfg=cfg, th=th):
            eg = eu + GUIDANCE * (e - eu) if cfg else e
            d = (x - s1m * eg) / sa
            th.copy_(d)
            return coefs[0] * x + coefs[1] * d + coefs[2] * h1, d

        tag = "+cfg" if cfg else ""
        arms["plms3" + tag] = (plms, plms_torch)
        arms["dpm2" + tag] = (dpm, dpm_torch)
    return arms


def run_updates(ops, dev):
    arms = update_arms(ops, dev)
    print(f"one multistep update at {SHAPE}; {CALLS} calls per window, {REPS} alternated repetitions, times in us")
    for name, (fused, ref) in arms.items():
        a, b = fused()[0].clone(), ref()[0]
        print(f"{name}: max |fused - torch| {float((a - b).abs().max()):.1e}")
        cols = (("fused", fused), ("torch", ref), ("fused_graph", graphed(fused)), ("torch_graph", graphed(ref)))
        for _, fn in cols:
            for _ in range(WARM):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k, _ in cols}
        print("repeat   " + "  ".join(f"{k:>11s}" for k, _ in cols))
        for rep in range(REPS):
            for k, fn in cols:
                times[k].append(window_us(fn))
            print(f"{rep:<8d} " + "  ".join(f"{times[k][-1]:11.2f}" for k, _ in cols), flush=True)
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        spread = {k: max(v) - min(v) for k, v in times.items()}
        print("median   " + "  ".join(f"{med[k]:11.2f}" for k, _ in cols))
        print("spread   " + "  ".join(f"{spread[k]:11.2f}" for k, _ in cols))
        for f, t in (("fused", "torch"), ("fused_graph", "torch_graph")):
            faster = med[f] + spread[f] < med[t] - spread[t]
            print(f"{name}: {f} {med[f]:.2f} us vs {t} {med[t]:.2f} us ({med[t] / med[f]:.2f}x): "
                  f"{'faster beyond the spread' if faster else 'NOT faster beyond the spread'}")


def run_models(dev, rounds):
    """img/s of whole runs (sampling + decode) of the three samplers on the c3 benchmark model, alternated."""
    import bench
    from sd_amd import ops
    from sd_amd.DDIM.ddim import DDIMSampler
    from sd_amd.DDIM.dpm_solver import DPMSolverSampler
    from sd_amd.DDIM.plms import PLMSSampler
    cfg = bench.CONFIGS["c3"]
    ops.AUTOTUNE.table.clear()
    ops.AUTOTUNE.load(os.path.join(ROOT, "configs", "conv_tuning_mi355x.json"))
    ops.AUTOTUNE.enable(False)
    unet, vae, ld = bench.build_models(cfg, dev, graph=True)
    B, L = cfg["batch"], cfg["latent"]
    xT, ctx = bench.rank_inputs(2024, 1, 0, B, (4, L, L), cfg["ctx"], dev)
    ld.use_graphs(True)
    runs = (("DDIM S=50", DDIMSampler(ld), 50, dict(eta=0.0)), ("DPM++ 2M S=20", DPMSolverSampler(ld), 20, {}),
            ("PLMS S=25", PLMSSampler(ld), 25, {}))

    def one(s, S, kw):
        z, _ = s.sample(S, B, (4, L, L), conditioning=ctx, x_T=xT, verbose=False, log_every_t=10 ** 9, **kw)
        return ld.decode_first_stage(z)

    for _, s, S, kw in runs:
        one(s, S, kw)
    torch.cuda.synchronize()
    print(f"c3 (SD-1 512x512, B = {B}, no CFG), sampling + decode, graphs on; {rounds} alternated rounds")
    rates = {name: [] for name, *_ in runs}
    for _ in range(rounds):
        for name, s, S, kw in runs:
            t0 = time.perf_counter()
            one(s, S, kw)
            torch.cuda.synchronize()
            rates[name].append(B / (time.perf_counter() - t0))
    for name, v in rates.items():
        print(f"{name:14s} img/s per round: " + " ".join(f"{r:6.2f}" for r in v) +
              f"   median {sorted(v)[len(v) // 2]:.2f}  spread {max(v) - min(v):.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", action="store_true", help="also time whole runs on the c3 benchmark model")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import sd_amd_loader
    sd_amd_loader.load()
    from sd_amd import ops
    dev = torch.device("cuda")
    run_updates(ops, dev)
    if args.models:
        run_models(dev, args.rounds)


if __name__ == "__main__":
    main()
