"""Two measurements of the patch-wise UNet (``split_input_params``) on the GPU; device events around windows of
calls after a warm-up, the arms alternated, every repetition printed, then per arm the median and the spread
(max - min).

1. The input pack.  ``sdk_patch_pack`` against the composition it replaces (``sdk_extract_patches`` per source, then
   ``sdk_concat_nchw_to_nhwc``) on a latent of (B, 4 + 5, 128, 128), patches of 64 every 32 (L = 9), c_pad 16, at
   B = 1 and B = 4.  Bytes the fused kernel has to move: 4 per source element read, 2 per output element written.
   The fused kernel stays if median(fused) <= median(composition) + spread(composition).

2. One UNet step at a 128x128 latent with the SD-shape UNet (9 input channels, context (77, 768), B = 1), three ways:
   (a) patch-wise, the project's path (``LatentDiffusion.apply_model``, all 9 patches in one UNet call, and in
   chunks of ``max_batch`` = 3); (b) a loop of L separate UNet calls on the patches, one per patch — the reference's
   structure, the yardstick; (c) the untiled 128x128 call.  Time per step and peak allocated memory above the
   resident weights, which is what the feature bounds.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KS, STRIDE, LATENT = 64, 32, 128
SD_UNET9 = dict(image_size=32, in_channels=9, out_channels=4, model_channels=320, attention_resolutions=[4, 2, 1],
                num_res_blocks=2, channel_mult=[1, 2, 4, 4], num_heads=8, use_spatial_transformer=True,
                transformer_depth=1, context_dim=768, use_checkpoint=False, legacy=False)


def window_us(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def run_arms(arms, calls, reps, warm, unit=1.0, fmt="{:10.2f}"):
    for _, fn in arms:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k, _ in arms}
    print("repeat   " + "  ".join(f"{k:>10s}" for k, _ in arms))
    for rep in range(reps):
        for k, fn in arms:
            times[k].append(window_us(fn, calls) * unit)
        print(f"{rep:<8d} " + "  ".join(fmt.format(times[k][-1]) for k, _ in arms), flush=True)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    spread = {k: max(v) - min(v) for k, v in times.items()}
    print("median   " + "  ".join(fmt.format(med[k]) for k, _ in arms))
    print("spread   " + "  ".join(fmt.format(spread[k]) for k, _ in arms))
    return med, spread


def pack_bench(ops, dev):
    for B in (1, 4):
        g = torch.Generator().manual_seed(B)
        srcs = [torch.randn(B, c, LATENT, LATENT, generator=g).to(dev) for c in (4, 1, 4)]

        def fused():
            return ops.patch_pack(srcs, 16, KS, KS, STRIDE, STRIDE)

        def composed():
            return ops.concat_nchw_to_nhwc([ops.extract_patches(s, KS, KS, STRIDE, STRIDE).view(-1, s.shape[1], KS, KS)
                                            for s in srcs], 16)

        same = torch.equal(fused().view(torch.int16), composed().view(torch.int16))
        rows = 9 * B * KS * KS
        nbytes = rows * (9 * 4 + 16 * 2)
        print(f"\n[pack] B = {B}: (B, 4+1+4, {LATENT}, {LATENT}) -> [{9 * B}, {KS}, {KS}, 16] fp16; fused == composition "
              f"bit for bit: {same}; the fused kernel moves {nbytes / 1e6:.2f} MB; microseconds per call, 200 calls "
              "per window")
        med, spread = run_arms((("fused", fused), ("composed", composed)), 200, 7, 50)
        keep = med["fused"] <= med["composed"] + spread["composed"]
        print(f"fused at its median: {nbytes / med['fused'] / 1e3:.1f} GB/s of required traffic (launch-bound at this "
              f"size); median(fused) <= median(composed) + spread(composed): {keep} -> the fused kernel "
              f"{'stays' if keep else 'must be looked at'}")


def unet_bench(ops, dev):
    from sd_amd.Diffusion.ddpm import DiffusionWrapper, LatentDiffusion

    class LD(LatentDiffusion):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.cond_stage_key, self.conditioning_key = "image", "hybrid"
            self.model = DiffusionWrapper({"target": "openai_model.model.UNetModel", "params": dict(SD_UNET9)}, "hybrid")

    torch.manual_seed(0)
    ld = LD()
    for p in ld.parameters():                  # the zero-initialised convs would make every output zero
        if float(p.detach().abs().max()) == 0.0:
            torch.nn.init.normal_(p, std=0.02)
    ld = ld.to(dev)
    unet = ld.model.diffusion_model
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1, 4, LATENT, LATENT, generator=g).to(dev)
    cc = [torch.randn(1, c, LATENT, LATENT, generator=g).to(dev) for c in (1, 4)]
    ctx = torch.randn(1, 77, 768, generator=g).to(dev)
    t = torch.tensor([500], device=dev)
    cond = {"c_concat": cc, "c_crossattn": [ctx]}
    sp = {"ks": (KS, KS), "stride": (STRIDE, STRIDE), "clip_min_weight": 0.01, "clip_max_weight": 0.5,
          "tie_braker": False}
    Ly = Lx = (LATENT - KS) // STRIDE + 1
    pix, _ = ld.get_weighting(KS, KS, Ly, Lx, sp)
    pix = torch.from_numpy(pix).to(dev)

    def patched(max_batch):
        def fn():
            ld.split_input_params = dict(sp, max_batch=max_batch)
            return ld.apply_model(x, t, cond)
        return fn

    def loop():
        # the reference's structure (Diffusion/ddpm.py:1170-1266): unfold x and the conditioning, one model call per patch
        cut = lambda z: ops.extract_patches(z, KS, KS, STRIDE, STRIDE)                       # noqa: E731
        xp, cp = cut(x), [cut(c) for c in cc]
        outs = [unet(xp[l], t, context=ctx, concat=[c[l] for c in cp]) for l in range(Ly * Lx)]
        return ops.fold_patches(torch.stack(outs, 0), pix, None, LATENT, LATENT, STRIDE, STRIDE, Ly, Lx)

    def untiled():
        ld.__dict__.pop("split_input_params", None)
        return ld.apply_model(x, t, cond)

    arms = (("patch_mb16", patched(16)), ("patch_mb3", patched(3)), ("loop_of_L", loop), ("untiled", untiled))
    torch.cuda.synchronize()
    resident = torch.cuda.memory_allocated()
    print(f"\n[unet] SD-shape UNet (9 input channels), latent (1, 4+5, {LATENT}, {LATENT}), patches of {KS} every "
          f"{STRIDE} (L = {Ly * Lx}); resident after loading {resident / 2**20:.0f} MiB")
    peaks = {}
    for k, fn in arms:
        fn()                                   # first call: packs weights, sizes the workspaces
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        peaks[k] = (torch.cuda.max_memory_allocated() - base, bool(out.isfinite().all()))
        del out
    same = torch.equal(patched(16)(), loop())
    print(f"patch-wise (one batch of 9) == loop of 9 calls bit for bit: {same} (batch 9 and batch 1 may pick "
          "different conv plans)")
    print("milliseconds per UNet step, 3 steps per window")
    med, spread = run_arms(arms, 3, 5, 1, unit=1e-3, fmt="{:10.3f}")
    print("peak MiB " + "  ".join(f"{peaks[k][0] / 2**20:10.1f}" for k, _ in arms) +
          "   (allocated above what is resident before the call)")
    print("finite   " + "  ".join(f"{str(peaks[k][1]):>10s}" for k, _ in arms))


def main():
    import sd_amd_loader
    sd_amd_loader.load()
    from sd_amd import ops
    dev = torch.device("cuda")
    print(torch.cuda.get_device_name(0))
    which = sys.argv[1:] or ["pack", "unet"]
    if "pack" in which:
        pack_bench(ops, dev)
    if "unet" in which:
        with torch.no_grad():
            unet_bench(ops, dev)


if __name__ == "__main__":
    main()
