"""OpenCLIP ViT-H/14 text-tower encode timings (the encode runs once per prompt batch, not per sampling step, so these
are records, not gates): ``FrozenOpenCLIPEmbedder(layer="penultimate")`` with seeded weights at B = 2, 8 and 16 prompts
of 77 ids, warm and eager (host launches included), next to the same 23 blocks written as torch fp16 ops on the same
device tensors (F.layer_norm, F.linear, scaled_dot_product_attention with is_causal, F.gelu), and the weight-stream
floor: the fp16 bytes of the 23 blocks' matrices over the HBM copy rate measured by ``sdk_probe_copy``.

Each time is the median of 9 windows between two device events after a warm-up; min and max show the spread; the two
sides alternate and every measurement is repeated once.  The encode is not measured inside a captured graph: it checks
the token ids against the vocabulary on the host before it launches anything, which a capture cannot contain."""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BATCHES = (2, 8, 16)
SEED = 1234


def window_ms(fn, per, reps=9, warm=3):
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
        ts.append(e0.elapsed_time(e1) / per)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def seeded_fill(model, dev):
    """Seeded weights generated on the device: matrices N(0, 1 / fan_in), norm scales 1 + 0.1 N, biases 0.02 N."""
    g = torch.Generator(device=dev).manual_seed(SEED)
    for name, p in model.named_parameters():
        if p.dim() == 2:
            p.data.normal_(0.0, p.shape[1] ** -0.5, generator=g)
        elif name.endswith(("ln_1.weight", "ln_2.weight", "ln_final.weight")):
            p.data.normal_(0.0, 0.1, generator=g).add_(1.0)
        elif p.dim() == 1:
            p.data.normal_(0.0, 0.02, generator=g)
        else:
            p.data.fill_(1.0)


def torch_tower(tower, n_blocks, heads):
    """The same blocks as torch fp16 ops on fp16 copies of the same weights."""
    h = lambda t: t.detach().half()                                                      # noqa: E731
    tok, pos = h(tower.token_embedding.weight), h(tower.positional_embedding)
    blocks = [dict(l1=(h(b.ln_1.weight), h(b.ln_1.bias)), l2=(h(b.ln_2.weight), h(b.ln_2.bias)),
                   wi=h(b.attn.in_proj_weight), bi=h(b.attn.in_proj_bias),
                   wo=h(b.attn.out_proj.weight), bo=h(b.attn.out_proj.bias),
                   w1=h(b.mlp.c_fc.weight), b1=h(b.mlp.c_fc.bias), w2=h(b.mlp.c_proj.weight), b2=h(b.mlp.c_proj.bias))
              for b in tower.transformer.resblocks[:n_blocks]]
    lf = (h(tower.ln_final.weight), h(tower.ln_final.bias))

    @torch.no_grad()
    def run(ids):
        B, T = ids.shape
        x = tok[ids] + pos[:T]
        W = x.shape[-1]
        for p in blocks:
            qkv = F.linear(F.layer_norm(x, (W,), *p["l1"], 1e-5), p["wi"], p["bi"])
            q, k, v = qkv.view(B, T, 3, heads, -1).permute(2, 0, 3, 1, 4)
            o = F.scaled_dot_product_attention(q, k, v, is_causal=True).transpose(1, 2).reshape(B, T, W)
            x = x + F.linear(o, p["wo"], p["bo"])
            f = F.gelu(F.linear(F.layer_norm(x, (W,), *p["l2"], 1e-5), p["w1"], p["b1"]))
            x = x + F.linear(f, p["w2"], p["b2"])
        return F.layer_norm(x, (W,), *lf, 1e-5)
    return run


def main():
    import sd_amd_loader
    sd_amd_loader.load()
    from sd_amd import ops
    from sd_amd.clip_encoder.modules import FrozenOpenCLIPEmbedder
    if not torch.cuda.is_available():
        raise SystemExit("openclip_microbench: needs the GPU (nothing is measured without one)")
    dev = torch.device("cuda")
    with torch.device("meta"):
        m = FrozenOpenCLIPEmbedder(layer="penultimate")
    m = m.to_empty(device=dev)
    seeded_fill(m, dev)
    tower = m.model
    cfg = tower.cfg
    n_blocks = cfg["layers"] - m.layer_idx
    ref = torch_tower(tower, n_blocks, cfg["heads"])

    W, M = cfg["width"], cfg["mlp_width"]
    wbytes = n_blocks * 2 * (3 * W * W + W * W + 2 * W * M)
    hbm = ops.probe_peaks(reps=3)["hbm_copy_gbs"]
    floor_ms = wbytes / (hbm * 1e9) * 1e3
    print(f"ViT-H/14 text tower, layer=penultimate: {n_blocks} blocks, {wbytes / 1e6:.1f} MB of fp16 block matrices")
    print(f"measured HBM copy rate {hbm:.0f} GB/s -> weight-stream floor {floor_ms:.3f} ms per encode")
    g = torch.Generator().manual_seed(SEED + 1)
    print("B   repeat  sd_amd_ms (min..max)        torch_fp16_ms (min..max)    sd_amd/floor  rel-L2(sd_amd, torch)")
    for B in BATCHES:
        ids = torch.randint(1, 49406, (B, 77), generator=g)
        ids[:, 0] = 49406
        for b in range(B):
            n = 5 + (7 * b) % 60
            ids[b, n] = 49407
            ids[b, n + 1:] = 0
        ids = ids.to(dev)
        y, r = m.encode_tokens(ids).float(), ref(ids).float()
        rl2 = float((y - r).norm() / r.norm())
        assert tuple(y.shape) == (B, 77, W) and bool(torch.isfinite(y).all())
        for rep in range(2):
            t_ref = window_ms(lambda: ref(ids), 5)
            t_own = window_ms(lambda: m.encode_tokens(ids), 5)
            print(f"{B:<3d} {rep:<7d} {t_own[0]:7.3f} ({t_own[1]:.3f}..{t_own[2]:.3f})     "
                  f"{t_ref[0]:7.3f} ({t_ref[1]:.3f}..{t_ref[2]:.3f})     {t_own[0] / floor_ms:8.1f}x    "
                  f"{rl2:.2e}", flush=True)


if __name__ == "__main__":
    main()
