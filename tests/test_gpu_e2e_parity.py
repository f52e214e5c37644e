"""End-to-end parity of the benchmarked configurations vs the fp32 CPU oracle chain (run with -m gpu).

* C3 (the headline): the bench's own ``one_step`` — B = 16, the committed conv tuning table, HIP-graph
  replay, 50 DDIM steps through LatentDiffusion.apply_model, then the 64² → 512² decode — and image 0
  of it against ``oracle.sampler_ref.ddim_sample`` → ``oracle.unet_ref.unet_forward`` (50 fp32 UNet
  evaluations) → ``oracle.vae_ref.decode_first_stage`` on the same seeded weights and inputs.
  Reference path: ``ldm/diffusion/ddim.py:114-206`` (sampling loop), ``ldm/diffusion/ddpm.py:1095``
  (decode_first_stage).
* C2 (uncond 256², B = 8): the same 50-step chain on samples 0 and 7 of the bench batch.
* C5 (SD-2 shape 768², v-prediction, B = 8): one UNet evaluation at the bench batch (tuning table,
  graph replay) on samples 0 and 7, and the B = 8 decode of images 0 and 7; then the bench's own 50-step
  v-prediction chain (graph replay) teacher-forced at 3 of its states + the decode of its final latent,
  and a free-running 10-step v-prediction chain + decode vs the oracle's (a 50-step fp32 chain at 96²
  would take ~6 min of CPU).
Every comparison prints and asserts rel-L2 AND max-abs error (relative to the oracle's max-abs); the
thresholds are ~3x the errors measured on MI355X (profiles/r5_parity_errors.txt, r6_parity_errors.txt)."""
import os
import sys
import time

import numpy as np
import pytest
import torch

from gpu_util import rel_l2

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS = 16


def max_abs_rel(a, b):
    """max |a - b| over max |b| (the oracle's range)."""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _report(tag, got, ref, rl2_max, mabs_max):
    rl2, mab = rel_l2(got, ref), max_abs_rel(got, ref)
    print(f"[parity] {tag}: rel-L2 {rl2:.3e} (<= {rl2_max:.1e})  max-abs/max {mab:.3e} (<= {mabs_max:.1e})",
          flush=True)
    assert rl2 <= rl2_max, f"{tag}: rel-L2 {rl2:.3e}"
    assert mab <= mabs_max, f"{tag}: max-abs {mab:.3e}"


def _bench_models(name):
    sys.path.insert(0, ROOT)
    import bench
    from sd_amd import ops
    cfg = bench.CONFIGS[name]
    ops.AUTOTUNE.table.clear()
    loaded = ops.AUTOTUNE.load(os.path.join(ROOT, "configs", "conv_tuning_mi355x.json"))
    assert loaded > 0, "the committed tuning table is stale for the csrc/conv* sources"
    ops.AUTOTUNE.enable(False)
    unet, vae, ld = bench.build_models(cfg, DEV, graph=True)
    B, L = cfg["batch"], cfg["latent"]
    xT, ctx = bench.rank_inputs(2024, 1, 0, B, (4, L, L), cfg["ctx"], DEV)
    return bench, cfg, unet, vae, ld, xT, ctx


def _oracle_chain(cfg, usd, vsd, x_T, ctx, scale_factor, v=False):
    from oracle.sampler_ref import ddim_sample
    from oracle.unet_ref import unet_forward
    from oracle.vae_ref import decode_first_stage
    import bench
    torch.set_num_threads(THREADS)
    fn = lambda x, t: unet_forward(usd, cfg["unet"], x, t, ctx)   # noqa: E731
    z, _ = ddim_sample(fn, x_T, 50, 0.0, parameterization="v" if v else "eps")
    return decode_first_stage(vsd, bench.SD_VAE, z, scale_factor), z


def _cpu_sd(m):
    return {k: v.detach().float().cpu() for k, v in m.state_dict().items()}


def test_c3_bench_step_vs_oracle_chain(sdk):
    """The exact C3 bench step (B=16, tuning table, graphs, 50 DDIM steps + decode) — image 0 vs the fp32
    oracle chain (~2 min of CPU at 16 threads), plus the pins that separate the kernels' error from the
    trajectory's sensitivity:
    * free-running: GPU chain vs oracle chain end to end (both integrate their own trajectory);
    * teacher-forced: at 5 states of the GPU's own trajectory, the GPU's eps vs the oracle UNet's eps at
      that same state, and the GPU decode of the GPU's final latent vs the oracle decode of that latent;
    * amplification: the same GPU chain from x_T perturbed by 1e-3 (relative) — how much the 50-step
      DDIM map magnifies a small input difference with these seeded weights."""
    from oracle.unet_ref import unet_forward
    from oracle.vae_ref import decode_first_stage
    from sd_amd.DDIM.ddim import DDIMSampler
    bench, cfg, unet, vae, ld, xT, ctx = _bench_models("c3")
    assert xT.shape[0] == 16
    ld.use_graphs(True)
    sampler = DDIMSampler(ld)
    step = bench.make_one_step(sampler, ld, xT, ctx, 50, 1, None)
    img = step().float().cpu()
    assert img.shape == (16, 3, 512, 512) and torch.isfinite(img).all()
    # the same sampling with every intermediate kept (the same graph replays: the same bits)
    z, inter = sampler.sample(S=50, batch_size=16, shape=(4, 64, 64), conditioning=ctx, eta=0.0, x_T=xT,
                              verbose=False, log_every_t=1)
    xs = [x.float().cpu().clone() for x in inter["x_inter"]]
    assert len(xs) == 51
    assert torch.equal(ld.decode_first_stage(z).float().cpu(), img), "the bench step is deterministic"
    # amplification of a 1e-3 input perturbation through the GPU chain
    g = torch.Generator().manual_seed(5)
    xT_p = xT + 1e-3 * xT.norm() / xT.numel() ** 0.5 * torch.randn(xT.shape, generator=g).to(DEV)
    zp, _ = sampler.sample(S=50, batch_size=16, shape=(4, 64, 64), conditioning=ctx, eta=0.0, x_T=xT_p,
                           verbose=False, log_every_t=10 ** 9)
    img_p = ld.decode_first_stage(zp).float().cpu()
    amp = rel_l2(img_p[0:1], img[0:1]) / rel_l2(xT_p[0:1], xT[0:1])
    print(f"[parity] C3 chain amplification of an x_T perturbation: {amp:.1f}x", flush=True)
    usd, vsd = _cpu_sd(unet), _cpu_sd(vae)
    torch.set_num_threads(THREADS)
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from oracle import schedule as sch
    ts = np.flip(sch.ddim_tables(50, 0.0)["ddim_timesteps"])
    for i in (0, 12, 25, 37, 49):
        t = torch.full((16,), int(ts[i]), dtype=torch.long, device=DEV)
        e_gpu = ld.apply_model(xs[i].to(DEV), t, ctx)[0:1].float().cpu()
        e_ref = unet_forward(usd, cfg["unet"], xs[i][0:1], t[0:1].cpu(), ctx[0:1].cpu())
        _report(f"C3 teacher-forced eps at DDIM step {i} (t={int(ts[i])})", e_gpu, e_ref, 5e-3, 7e-3)   # <= 2.04e-3 / 2.29e-3
    dref = decode_first_stage(vsd, bench.SD_VAE, xs[-1][0:1], ld.scale_factor)
    _report("C3 decode of the GPU's final latent (image 0)", img[0:1], dref, 5e-3, 9e-3)   # 2.15e-3 / 2.75e-3
    t0 = time.time()
    ref, _ = _oracle_chain(cfg, usd, vsd, xT[0:1].cpu(), ctx[0:1].cpu(), ld.scale_factor)
    print(f"[parity] C3 oracle chain: {time.time() - t0:.0f} s", flush=True)
    # free-running: the GPU's per-step error (~2e-3, teacher-forced above) integrated over 50 steps and
    # magnified by the chain (amplification above): measured 2.39e-3 / 3.17e-3 (profiles/r5_parity_errors.txt)
    # -> limits ~3.3x / 3.2x
    _report("C3 image 0 free-running (50 DDIM steps + decode, B=16 bench step)", img[0:1], ref, 8e-3, 1e-2)   # 2.39e-3 / 3.17e-3


def test_c2_bench_batch_vs_oracle_chain(sdk):
    """C2 (unconditional 256², B=8): 50 DDIM steps + decode through the bench's step, samples 0 and 7."""
    from sd_amd.DDIM.ddim import DDIMSampler
    bench, cfg, unet, vae, ld, xT, ctx = _bench_models("c2")
    assert xT.shape[0] == 8 and ctx is None
    ld.use_graphs(True)
    step = bench.make_one_step(DDIMSampler(ld), ld, xT, ctx, 50, 1, None)
    img = step().float().cpu()
    usd, vsd = _cpu_sd(unet), _cpu_sd(vae)
    for i in (0, 7):
        ref, _ = _oracle_chain(cfg, usd, vsd, xT[i:i + 1].cpu(), None, ld.scale_factor)
        _report(f"C2 image {i} (50 DDIM steps + decode, B=8 bench step)", img[i:i + 1], ref, 5e-3, 8e-3)   # 2.38e-3 / 2.64e-3


def test_c5_bench_batch_unet_and_decode_vs_oracle(sdk):
    """C5 (SD-2 shape, 96² latent, v-prediction, B=8): the UNet at the bench batch with the tuning table
    and graph replay, and the B=8 decode, samples 0 and 7 vs the fp32 oracle."""
    from oracle.unet_ref import unet_forward
    from oracle.vae_ref import decode_first_stage
    bench, cfg, unet, vae, ld, xT, ctx = _bench_models("c5")
    assert xT.shape[0] == 8
    t = torch.full((8,), 641, dtype=torch.long, device=DEV)
    ld.use_graphs(True)
    ld.apply_model(xT, t, ctx)                               # capture
    y = ld.apply_model(xT, t, ctx).float().cpu()
    z = torch.randn(8, 4, 96, 96, generator=torch.Generator().manual_seed(31)).to(DEV)
    dec = ld.decode_first_stage(z).float().cpu()
    usd, vsd = _cpu_sd(unet), _cpu_sd(vae)
    torch.set_num_threads(THREADS)
    for i in (0, 7):
        ref = unet_forward(usd, cfg["unet"], xT[i:i + 1].cpu(), torch.tensor([641]), ctx[i:i + 1].cpu())
        _report(f"C5 UNet sample {i} (B=8 bench batch, graph)", y[i:i + 1], ref, 5e-3, 7e-3)   # 2.01e-3 / 2.17e-3
        dref = decode_first_stage(vsd, bench.SD_VAE, z[i:i + 1].cpu(), ld.scale_factor)
        _report(f"C5 decode image {i} (B=8 96->768)", dec[i:i + 1], dref, 5e-3, 8e-3)   # 2.18e-3 / 2.66e-3


def test_c5_vpred_chain_vs_oracle(sdk):
    """C5's v-prediction DDIM chain on the GPU (B=8, tuning table, graph replay at the 96² latent):
    * the bench step itself (50 steps + decode) is finite and bitwise reproducible, and at 3 states of its
      own trajectory the GPU's model output (v) matches the oracle UNet's for samples 0 and 7; the decode of
      its final latent matches the oracle decode;
    * free-running: a 10-step chain + decode from the same x_T, sample 0, vs the oracle's 10-step chain
      (``oracle.sampler_ref.ddim_sample(parameterization="v")``; v-pred is parity-unpinned: the reference
      has no v-prediction)."""
    from oracle.sampler_ref import ddim_sample
    from oracle.unet_ref import unet_forward
    from oracle.vae_ref import decode_first_stage
    from sd_amd.DDIM.ddim import DDIMSampler
    bench, cfg, unet, vae, ld, xT, ctx = _bench_models("c5")
    assert xT.shape[0] == 8 and ld.parameterization == "v"
    ld.use_graphs(True)
    sampler = DDIMSampler(ld)
    step = bench.make_one_step(sampler, ld, xT, ctx, 50, 1, None)
    img = step().float().cpu()
    assert img.shape == (8, 3, 768, 768) and torch.isfinite(img).all()
    z, inter = sampler.sample(S=50, batch_size=8, shape=(4, 96, 96), conditioning=ctx, eta=0.0, x_T=xT,
                              verbose=False, log_every_t=1)
    xs = [x.float().cpu().clone() for x in inter["x_inter"]]
    assert len(xs) == 51
    assert torch.equal(ld.decode_first_stage(z).float().cpu(), img), "the C5 bench step is deterministic"
    usd, vsd = _cpu_sd(unet), _cpu_sd(vae)
    torch.set_num_threads(THREADS)
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from oracle import schedule as sch
    ts = np.flip(sch.ddim_tables(50, 0.0)["ddim_timesteps"])
    for i in (0, 25, 49):
        t = torch.full((8,), int(ts[i]), dtype=torch.long, device=DEV)
        v_gpu = ld.apply_model(xs[i].to(DEV), t, ctx).float().cpu()
        for b in (0, 7):
            v_ref = unet_forward(usd, cfg["unet"], xs[i][b:b + 1], t[b:b + 1].cpu(), ctx[b:b + 1].cpu())
            _report(f"C5 teacher-forced v at DDIM step {i} (t={int(ts[i])}), sample {b}", v_gpu[b:b + 1], v_ref,
                    5e-3, 9e-3)   # <= 2.08e-3 / 2.78e-3
    dref = decode_first_stage(vsd, bench.SD_VAE, xs[-1][0:1], ld.scale_factor)
    _report("C5 decode of the GPU's final latent (image 0)", img[0:1], dref, 5e-3, 1.1e-2)   # 2.27e-3 / 3.51e-3
    z10, _ = sampler.sample(S=10, batch_size=8, shape=(4, 96, 96), conditioning=ctx, eta=0.0, x_T=xT,
                            verbose=False, log_every_t=10 ** 9)
    img10 = ld.decode_first_stage(z10)[0:1].float().cpu()
    t0 = time.time()
    fn = lambda x, t: unet_forward(usd, cfg["unet"], x, t, ctx[0:1].cpu())   # noqa: E731
    zr, _ = ddim_sample(fn, xT[0:1].cpu(), 10, 0.0, parameterization="v")
    ref10 = decode_first_stage(vsd, bench.SD_VAE, zr, ld.scale_factor)
    print(f"[parity] C5 10-step oracle chain: {time.time() - t0:.0f} s", flush=True)
    _report("C5 image 0 free-running (10 v-pred DDIM steps + decode, B=8)", img10, ref10, 8e-3, 1.4e-2)   # 2.90e-3 / 4.22e-3
