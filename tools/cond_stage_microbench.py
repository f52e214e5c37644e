"""Condition-encoder timings (nothing here runs once per sampling step, so these are records, not gates):

* the encode time of the LDM text encoder's layout, ``BERTEmbedder(n_embed=1280, n_layer=32)`` on 32 rows of 77
  token ids (a classifier-free-guidance pair at B = 16), random weights;
* ``ops.resize2d`` (csrc/cond.hip: sdk_resize2d) at (4, 182, 256, 512), bilinear x0.5 — a COCO-stuff one-hot
  layout map halved, ``SpatialRescaler``'s per-stage launch — with the achieved bytes/s from the algorithmic
  bytes (input read once + output written once), next to ``F.interpolate`` on the same device tensor.

Each time is the median of 7 windows between two device events after a warm-up, host launches included; the two
sides of a comparison alternate and every measurement is repeated once so the spread shows."""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RESIZE_SHAPE = (4, 182, 256, 512)
ENCODE_ROWS, ENCODE_SEQ = 32, 77


def window_us(fn, per, reps=7, warm=3):
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
    from sd_amd.clip_encoder.modules import BERTEmbedder
    dev = torch.device("cuda")
    torch.manual_seed(0)

    x = torch.randn(RESIZE_SHAPE, device=dev)
    nbytes = 4 * (x.numel() + x.numel() // 4)
    out = torch.empty(RESIZE_SHAPE[0], RESIZE_SHAPE[1], RESIZE_SHAPE[2] // 2, RESIZE_SHAPE[3] // 2, device=dev)
    ours = lambda: ops.resize2d(x, 0.5, "bilinear", out=out)                            # noqa: E731
    ref = lambda: F.interpolate(x, scale_factor=0.5, mode="bilinear")                   # noqa: E731
    diff = float((ours() - ref()).abs().max())
    print(f"resize2d {RESIZE_SHAPE} bilinear x0.5, {nbytes / 1e6:.1f} MB algorithmic; max |ours - F.interpolate| "
          f"{diff:.2e}")
    print("repeat   F.interpolate_us  resize2d_us  resize2d_GB/s")
    for rep in range(2):
        t_ref, t_ours = window_us(ref, 20), window_us(ours, 20)
        print(f"{rep:<8d} {t_ref:15.1f}  {t_ours:11.1f}  {nbytes / t_ours / 1e3:13.1f}", flush=True)
    del x, out

    m = BERTEmbedder(n_embed=1280, n_layer=32, use_tokenizer=False).to(dev)
    ids = torch.randint(0, 30522, (ENCODE_ROWS, ENCODE_SEQ), device=dev)
    y = m.encode(ids)
    assert tuple(y.shape) == (ENCODE_ROWS, ENCODE_SEQ, 1280) and bool(torch.isfinite(y).all())
    print(f"BERTEmbedder(n_embed=1280, n_layer=32) encode of {ENCODE_ROWS} x {ENCODE_SEQ} ids (fp16 out)")
    print("repeat   encode_ms")
    for rep in range(2):
        print(f"{rep:<8d} {window_us(lambda: m.encode(ids), 3) / 1e3:9.2f}", flush=True)


if __name__ == "__main__":
    main()
