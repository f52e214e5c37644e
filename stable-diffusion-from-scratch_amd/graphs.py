"""HIP-graph replay of the UNet forward (one sampler step's ~600 kernel launches).

``GraphedUNet(unet)(x, timesteps, context, concat, y)`` captures ``unet.forward`` once per
(input shapes, context tensor, concat shapes, label shape) and afterwards replays it: the inputs (x, timesteps,
the class labels ``y`` of an 'adm' model and the concat tensors of a 'concat' / 'hybrid' model) are copied into the graph's static
buffers, the whole step is one ``hipGraphLaunch``.  Everything the
forward launches goes through the C ABI on the current stream, so it is captured like
any torch op.

Soundness rules (each one is what a replay reads from memory it does not own):
* the graph key holds the context tensor ITSELF (identity + ``_version``), never its
  address — a new conditioning that the caching allocator places at an old one's address
  gets its own capture;
* an entry keeps strong references to the context and to the cross-attention K/V it
  was captured with, so model-side cache eviction cannot free memory a replay reads;
* workspaces (split-K slabs, GroupNorm partials) are never freed while graphs may hold
  their pointers (``ops._Workspace`` retires, never releases, a grown buffer);
* loading parameters into the model (directly or through any parent module) or re-packing them
  (``UNetModel.prepare``) moves the model's ``prepare_generation`` (``packing.PackedOwner``) and
  the next call drops every graph.
Preconditions: run one eager step first so the conv autotuner, the workspaces and the
context K/V cache are settled.  The result is a fresh tensor per call, as the eager forward
returns (a copy of the graph's static output, 1 MiB at the C3 batch: a caller may keep eps
across calls — PLMS-style samplers, separate cond / uncond calls); ``alias_output=True`` returns
the static buffer itself, overwritten by the next replay, for a caller that consumes it at once.
Every new conditioning tensor (a new prompt) is a new key: one eager warm-up plus one capture,
and each kept graph owns a private memory pool of one forward's activations, so at most
``MAX_GRAPHS`` (4) are kept, least recently used first out.
The reference has no counterpart (eager PyTorch, ``ldm/diffusion/ddim.py`` calls
``apply_model`` per step); this is the MI355X launch-overhead remedy."""
from __future__ import annotations

from collections import OrderedDict

import torch


class GraphedUNet:
    MAX_GRAPHS = 4

    def __init__(self, unet, alias_output=False):
        self.unet = unet
        self.alias_output = alias_output
        self.graphs = OrderedDict()
        self._gen = getattr(unet, "prepare_generation", None)

    @staticmethod
    def _key(x, timesteps, context, concat=(), y=None, patches=None):
        ctx = None if context is None else (id(context), tuple(context.shape), context.dtype)
        return (tuple(x.shape), x.dtype, tuple(timesteps.shape), ctx, tuple(tuple(c.shape) for c in concat),
                None if y is None else tuple(y.shape), None if patches is None else tuple(patches))

    def _valid(self, ent, context):
        if context is None:
            return ent["ctx"] is None
        return ent["ctx"] is context and ent["ctx_version"] == context._version

    @torch.no_grad()
    def __call__(self, x, timesteps, context=None, concat=None, y=None, patches=None):
        # concat tensors (UNetModel.forward's extension) are inputs like x: shapes in the key, contents
        # copied into static fp32 buffers on every replay (no identity cache, they change per call)
        concat = [] if concat is None else [c.to(device=x.device, dtype=torch.float32) for c in concat]
        # class labels (y) are one more static input: int64 on the device, copied on every replay like timesteps
        # (a device y is never range-checked on the host: an id out of range gives NaN rows, not a fault)
        if y is not None:
            y = torch.as_tensor(y).to(device=x.device, dtype=torch.int64)
        # a patch window (UNetModel.forward's ``patches``) is baked into the captured pack kernel's arguments: it
        # is part of the key, so a graph is never replayed for another window
        pk = {} if patches is None else {"patches": tuple(int(v) for v in patches)}
        kw = lambda cc, yy=None: dict({"concat": cc} if cc else {}, **({} if yy is None else {"y": yy}), **pk)  # noqa: E731
        gen = getattr(self.unet, "prepare_generation", None)
        if gen != self._gen:
            self.reset()
            self._gen = gen
        key = self._key(x, timesteps, context, concat, y, pk.get("patches"))
        ent = self.graphs.get(key)
        if ent is not None and not self._valid(ent, context):
            del self.graphs[key]
            ent = None
        if ent is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("GraphedUNet: nested capture")
            sx, st = x.clone(), timesteps.clone()
            sc = [c.clone() for c in concat]
            sy = None if y is None else y.clone()
            side = torch.cuda.Stream(device=x.device)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):          # settle caches/attributes outside the capture
                self.unet(sx, st, context=context, **kw(sc, sy))
            torch.cuda.current_stream().wait_stream(side)
            kv = None
            if context is not None and hasattr(self.unet, "_context_kv"):
                kv = self.unet._context_kv(context)[0]     # the K/V the capture will read (cache hit)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = self.unet(sx, st, context=context, **kw(sc, sy))
            ent = {"graph": g, "x": sx, "t": st, "concat": sc, "y": sy, "out": out, "ctx": context,
                   "ctx_version": None if context is None else context._version, "kv": kv}
            self.graphs[key] = ent
            while len(self.graphs) > self.MAX_GRAPHS:
                self.graphs.popitem(last=False)
        self.graphs.move_to_end(key)
        ent["x"].copy_(x)
        ent["t"].copy_(timesteps)
        for dst, src in zip(ent["concat"], concat):
            dst.copy_(src)
        if y is not None:
            ent["y"].copy_(y)
        ent["graph"].replay()
        return ent["out"] if self.alias_output else ent["out"].clone()

    def reset(self):
        self.graphs.clear()
