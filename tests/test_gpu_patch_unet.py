"""``LatentDiffusion.apply_model`` under ``split_input_params`` on the GPU (run with -m gpu): the UNet on overlapping
latent patches, gathered by ``sdk_patch_pack`` and blended by ``sdk_fold_patches``.

* Against the pieces, bit-equal: ``ops.fold_patches`` of ``UNetModel.forward`` on ``ops.extract_patches`` of x and
  of every concat source, run as one batch L·B (or in the same chunks) through the public ``concat=`` path.  The two
  run the same kernels at the same shapes; only the input pack differs, and the pack is exact.
* Against the reference's fixtures (tests/golden/make_golden_patch.py) under patch_util.PARITY_LIMITS.
* Graph replay, the identity of the repeated contexts, and the cases that must not change anything."""
import numpy as np
import pytest
import torch

import patch_util as pu
from golden_util import load, weights_of
from gpu_util import check_parity
from synth import keys_shapes_of, synth_weights

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
COND_STAGE_KEY = {"concat": "image", "crossattn": "txt", "adm": "class_label", "hybrid": "image"}


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ld(sdk, name, sp=None):
    """A LatentDiffusion around the tiny UNet ``name`` (patch_util.MODELS) without first / cond stage: apply_model and
    the DDIM sampler are under test.  Weights: the fixture's key order where the reference wrote one."""
    from sd_amd.Diffusion.ddpm import DiffusionWrapper, LatentDiffusion
    cfg, seed = pu.MODELS[name]

    class LD(LatentDiffusion):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.parameterization, self.clip_denoised, self.v_posterior = "eps", False, 0.
            self.shorten_cond_schedule, self.log_every_t = False, 1
            self.channels, self.image_size = pu.X_SHAPE[1], pu.X_SHAPE[2]
            self.cond_stage_key, self.conditioning_key = COND_STAGE_KEY[name], name
            self.model = DiffusionWrapper({"target": "openai_model.model.UNetModel", "params": dict(cfg)}, name)
            kw = dict(pu.SCHEDULE)
            self.register_schedule(beta_schedule=kw.pop("beta_schedule"), **kw)

    ld = LD()
    unet = ld.model.diffusion_model
    if name == "hybrid":
        sd = {k: torch.from_numpy(v) for k, v in synth_weights(keys_shapes_of(unet.state_dict()), seed).items()}
    else:
        sd = weights_of(load(f"patch_unet_{name}"))
    unet.load_state_dict(sd)
    if sp is not None:
        ld.split_input_params = sp
    return ld.to(DEV)


@pytest.fixture(scope="module")
def inputs():
    return {k: _gpu(v) for k, v in pu.unet_inputs().items()}


def _cond(name, d):
    """The conditioning as apply_model takes it (by key)."""
    return {"concat": {"c_concat": [d["m"], d["zi"]]}, "crossattn": d["ctx"], "adm": [d["y"]],
            "hybrid": {"c_concat": [d["m"], d["zi"]], "c_crossattn": [d["ctx"]]}}[name]


def _composition(sdk, ld, name, d, sp, chunk=None):
    """fold_patches of UNetModel.forward on extract_patches(x) and of each concat source, through ``concat=``."""
    from sd_amd import ops
    unet = ld.model.diffusion_model
    x = d["x"]
    B, _, h, w = x.shape
    ks, stride, Ly, Lx = ops.patch_grid(h, w, sp["ks"], sp["stride"])
    total = Ly * Lx * B
    chunk = chunk or total
    cut = lambda z: ops.extract_patches(z, ks[0], ks[1], stride[0], stride[1]).view(total, z.shape[1], *ks)  # noqa: E731
    xp = cut(x)
    cps = [cut(d["m"]), cut(d["zi"])] if name in ("concat", "hybrid") else []
    tt = d["t"].repeat(Ly * Lx)
    ctx = d["ctx"].repeat(Ly * Lx, 1, 1) if name in ("crossattn", "hybrid") else None
    y = d["y"].repeat(Ly * Lx) if name == "adm" else None
    outs = []
    for p0 in range(0, total, chunk):
        s = slice(p0, p0 + chunk)
        kw = {}
        if cps:
            kw["concat"] = [c[s] for c in cps]
        if y is not None:
            kw["y"] = y[s]
        outs.append(unet(xp[s], tt[s], context=None if ctx is None else ctx[s].contiguous(), **kw))
    eps = torch.cat(outs, 0).view(Ly * Lx, B, -1, *ks)
    pix, lw = ld.get_weighting(ks[0], ks[1], Ly, Lx, sp)
    return ops.fold_patches(eps, _gpu(pix), None if lw is None else _gpu(lw), h, w, stride[0], stride[1], Ly, Lx)


# ------------------------------------------------------------------ against the pieces, bit-equal
@pytest.mark.parametrize("chunk", [None, 3], ids=["one_batch", "max_batch3"])
@pytest.mark.parametrize("tie", [True, False], ids=["tie", "notie"])
@pytest.mark.parametrize("name", ["concat", "crossattn", "hybrid", "adm"])
def test_apply_model_equals_fold_of_unet_on_patches(sdk, inputs, name, tie, chunk):
    sp = pu.split_params(pu.KS, pu.STRIDE, tie, **({} if chunk is None else {"max_batch": chunk}))
    ld = _ld(sdk, name, sp)
    got = ld.apply_model(inputs["x"], inputs["t"], _cond(name, inputs))
    want = _composition(sdk, ld, name, inputs, sp, chunk)
    assert got.shape == pu.X_SHAPE and got.dtype == torch.float32 and bool(got.isfinite().all())
    assert torch.equal(got, want)
    # ... and it is not the untiled call
    del ld.split_input_params
    whole = ld.apply_model(inputs["x"], inputs["t"], _cond(name, inputs))
    assert float((got - whole).abs().max()) > 1e-2 * float(whole.abs().max())


# ------------------------------------------------------------------ against the reference's fixtures
def _check(tag, got, ref):
    return check_parity(tag, got, torch.from_numpy(np.asarray(ref)), *pu.PARITY_LIMITS[tag])


@pytest.mark.parametrize("name,tie", [("concat", True), ("concat", False), ("crossattn", True), ("crossattn", False),
                                      ("adm", True)])
def test_apply_model_vs_reference(sdk, inputs, name, tie):
    fx = load(f"patch_unet_{name}")
    ld = _ld(sdk, name, pu.split_params(pu.KS, pu.STRIDE, tie))
    got = ld.apply_model(inputs["x"], inputs["t"], _cond(name, inputs))
    _check(f"patch-wise {name} UNet vs reference", got, fx[f"y_tie{int(tie)}"])


@pytest.mark.parametrize("name", ["concat", "crossattn"])
def test_ddim_loop_vs_reference(sdk, inputs, name):
    """3 DDIM steps, eta = 0, every apply_model call patch-wise; CFG (scale 7.5, batch doubled) on the crossattn model."""
    from sd_amd.DDIM.ddim import DDIMSampler
    fx = load(f"patch_unet_{name}")
    ld = _ld(sdk, name, pu.split_params(pu.KS, pu.STRIDE, True))
    kw = {}
    if name == "crossattn":
        kw = dict(unconditional_guidance_scale=pu.CFG_SCALE, unconditional_conditioning=inputs["uc"])
    out, _ = DDIMSampler(ld).sample(S=pu.DDIM_STEPS, batch_size=2, shape=pu.X_SHAPE[1:],
                                    conditioning=_cond(name, inputs), eta=0.0, x_T=inputs["xT"], verbose=False, **kw)
    _check(f"patch-wise {name} DDIM loop vs reference", out, fx["ddim_samples"])


# ------------------------------------------------------------------ graphs
@pytest.mark.parametrize("name", ["concat", "crossattn"])
def test_graphs_equal_eager(sdk, inputs, name):
    """Two calls with different x: a replay reads the new x through the captured pack, one graph per window."""
    ld = _ld(sdk, name, pu.split_params(pu.KS, pu.STRIDE, True, max_batch=3))
    cond = _cond(name, inputs)
    xs = [inputs["x"], inputs["xT"]]
    eager = [ld.apply_model(x, inputs["t"], cond) for x in xs]
    ld.use_graphs(True)
    graphed = [ld.apply_model(x, inputs["t"], cond) for x in xs]
    assert len(ld.model._graphed.graphs) == 3                   # windows [0, 3), [3, 6), [6, 8)
    assert len({k[-1] for k in ld.model._graphed.graphs}) == 3
    for e, g in zip(eager, graphed):
        assert torch.equal(e, g)
    assert not torch.equal(graphed[0], graphed[1])


# ------------------------------------------------------------------ context identity
def test_repeated_contexts_keep_their_identity(sdk, inputs):
    """Three calls with one conditioning tensor: the UNet's context K/V cache holds the same chunk contexts and the
    same K/V objects throughout (nothing is re-projected per step), and a new conditioning gets its own."""
    ld = _ld(sdk, "crossattn", pu.split_params(pu.KS, pu.STRIDE, True, max_batch=3))
    unet = ld.model.diffusion_model
    ld.apply_model(inputs["x"], inputs["t"], inputs["ctx"])
    first = [(e[0], e[2]) for e in unet._ctx_cache.values()]
    assert [tuple(c.shape) for c, _ in first] == [(3, 7, 48), (3, 7, 48), (2, 7, 48)]
    for x in (inputs["xT"], inputs["x"]):
        ld.apply_model(x, inputs["t"], inputs["ctx"])
        now = [(e[0], e[2]) for e in unet._ctx_cache.values()]
        assert len(now) == len(first) and all(a[0] is b[0] and a[1] is b[1] for a, b in zip(first, now))
    # the chunk contexts are patch p = l*B + b -> ctx[b]
    rep = torch.cat([c for c, _ in first], 0)
    assert torch.equal(rep, inputs["ctx"].repeat(4, 1, 1))
    ld.apply_model(inputs["x"], inputs["t"], inputs["uc"])
    assert len(unet._ctx_cache) == 6 and all(a[0] is b[0] for a, b in zip(first, unet._ctx_cache.values()))
    # the LatentDiffusion's own cache is bounded: the oldest conditioning leaves
    for i in range(ld.PATCH_CONTEXT_CACHE_SIZE):
        ld._patch_contexts(torch.zeros(2, 7, 48, device=DEV) + i, 4, 3)
    assert len(ld._patch_ctx) == ld.PATCH_CONTEXT_CACHE_SIZE
    assert all(ent[0] is not inputs["ctx"] for ent in ld._patch_ctx.values())


# ------------------------------------------------------------------ cases that change nothing
@pytest.mark.parametrize("name", ["concat", "crossattn"])
def test_single_patch_escape_hatch_and_no_attribute(sdk, inputs, name):
    ld = _ld(sdk, name)
    cond = _cond(name, inputs)
    plain = ld.apply_model(inputs["x"], inputs["t"], cond)
    # without the attribute apply_model returns what self.model(...) returns
    kw = cond if isinstance(cond, dict) else {"c_crossattn": [cond]}
    assert torch.equal(plain, ld.model(inputs["x"], inputs["t"], **kw))
    for sp in (pu.split_params((12, 12), pu.STRIDE), pu.split_params((64, 64), (32, 32)),       # L == 1
               pu.split_params(pu.KS, pu.STRIDE, patch_unet=False)):
        ld.split_input_params = sp
        assert torch.equal(ld.apply_model(inputs["x"], inputs["t"], cond), plain)
    ld.split_input_params = pu.split_params(pu.KS, pu.STRIDE)
    assert not torch.equal(ld.apply_model(inputs["x"], inputs["t"], cond), plain)
