"""Concat / hybrid conditioning and LatentDiffusion's ancestral sampler on the GPU (run with -m gpu).

Kernel and loop tests compare with fixtures written by the reference's own functions
(tests/golden/make_golden_concat_ancestral.py) bit for bit: the kernels evaluate the reference's fp32
expressions operation by operation without contraction, so no tolerance applies.  The model-level parity
test compares the fp16-activation UNet with the reference's fp32 output under the limits of
ca_util.PARITY_LIMITS (at most 3.5x the errors measured on MI355X,
profiles/concat_ancestral_parity_errors.txt)."""
import numpy as np
import pytest
import torch

import ca_util as cu
import vq_util as vu
from golden_util import cfg_of, load, weights_of
from gpu_util import check_parity

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _same(got, ref, what=""):
    """fp32 equality as np.array_equal sees it (the reference fixture as the yardstick)."""
    assert np.array_equal(got.detach().cpu().numpy(), np.asarray(ref)), what


# ------------------------------------------------------------------ pack kernel
# (B, channels of x and of each concat tensor, H, W, c_pad)
PACK_CASES = [(2, [4, 1, 4], 8, 8, 16), (1, [3, 3], 5, 7, 8), (2, [4, 4, 1, 3], 4, 4, 16),
              (1, [3, 3], 5, 7, 7), (3, [2, 5], 9, 11, 12)]     # the last two: c_pad % 8 != 0 (scalar stores)


def _pack_ref(srcs, c_pad):
    y = torch.cat(srcs, 1).permute(0, 2, 3, 1).half()
    out = torch.zeros(*y.shape[:3], c_pad, dtype=torch.float16, device=y.device)
    out[..., :y.shape[3]] = y
    return out


@pytest.mark.parametrize("case", PACK_CASES, ids=lambda c: "b{}_c{}_{}x{}_p{}".format(c[0], "+".join(map(str, c[1])), *c[2:]))
def test_concat_pack_equals_cat_permute_half(sdk, case):
    from sd_amd import ops
    b, chans, h, w, c_pad = case
    srcs = [_gpu(vu.randn(8000 + 31 * i + sum(case[2:]), b, c, h, w) * np.float32(3.0)) for i, c in enumerate(chans)]
    y = ops.concat_nchw_to_nhwc(srcs, c_pad)
    assert y.dtype == torch.float16 and tuple(y.shape) == (b, h, w, c_pad) and y.is_contiguous()
    assert torch.equal(y, _pack_ref(srcs, c_pad))


@pytest.mark.parametrize("shape,c_pad", [((2, 4, 8, 8), 8), ((1, 3, 5, 7), 8), ((2, 9, 16, 16), 16), ((1, 5, 3, 3), 6)])
def test_concat_pack_single_source_equals_nchw_to_nhwc(sdk, shape, c_pad):
    from sd_amd import ops
    x = _gpu(vu.randn(8100 + sum(shape), *shape))
    assert torch.equal(ops.concat_nchw_to_nhwc([x], c_pad).view(torch.int16), ops.nchw_to_nhwc(x, c_pad).view(torch.int16))


def test_concat_pack_rejects_bad_arguments(sdk):
    from sd_amd import ops
    x = torch.zeros(1, 4, 4, 4, device=DEV)
    with pytest.raises(ValueError):
        ops.concat_nchw_to_nhwc([x] * 5, 24)
    with pytest.raises(ValueError):
        ops.concat_nchw_to_nhwc([x, torch.zeros(1, 1, 4, 2, device=DEV)], 8)
    with pytest.raises(ValueError):
        ops.concat_nchw_to_nhwc([x, x], 4)
    with pytest.raises(TypeError):
        ops.concat_nchw_to_nhwc([x.cpu()], 8)


# ------------------------------------------------------------------ stand-in model
def _stub_ld(sdk, schedule, parameterization="eps", clip_denoised=False, outputs=None, codebook=None):
    """A LatentDiffusion whose apply_model returns recorded tensors (``outputs[t]``), built without a
    UNet / first stage: only the schedule and the sampler methods are under test."""
    from sd_amd.Diffusion.ddpm import LatentDiffusion

    class StubLD(LatentDiffusion):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.parameterization, self.clip_denoised, self.v_posterior = parameterization, clip_denoised, 0.
            self.shorten_cond_schedule, self.log_every_t = False, 1
            self.channels, self.image_size = cu.LOOP_SHAPE[1], cu.LOOP_SHAPE[2]
            kw = dict(schedule)
            self.register_schedule(beta_schedule=kw.pop("beta_schedule"), **kw)
            self.calls = 0

        def apply_model(self, x_noisy, t, cond, return_ids=False):
            self.calls += 1
            return outputs if outputs.dim() == 4 else outputs[int(t[0])]        # one tensor, or one per timestep

    ld = StubLD()
    if codebook is not None:
        from sd_amd.vqvae.quantize import VectorQuantize2
        q = VectorQuantize2(codebook.shape[0], codebook.shape[1], 0.25)
        q.load_state_dict({"embedding.weight": torch.from_numpy(codebook)}, strict=False)
        ld.first_stage_model = torch.nn.Module()
        ld.first_stage_model.quantize = q
    return ld.to(DEV)


# ------------------------------------------------------------------ posterior step
STEP_IDS = ["x".join(map(str, s)) for s, _ in cu.STEP_CASES]


@pytest.mark.parametrize("temp", cu.STEP_TEMPS, ids=lambda v: f"T{v}")
@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("param", cu.STEP_PARAMS)
@pytest.mark.parametrize("case", cu.STEP_CASES, ids=STEP_IDS)
def test_posterior_step_bitexact_vs_reference(sdk, case, param, clip, temp):
    from sd_amd import ops
    shape, t = case
    fx = load("ca_step")
    tag = cu.step_tag(shape, param, clip, temp)
    x, mo, nz = (_gpu(a) for a in cu.step_inputs(shape))
    ld = _stub_ld(sdk, cu.STEP_SCHEDULE, param, outputs=mo)
    tt = torch.tensor(t, device=DEV)
    # one call, with and without x_recon; the reference's spelling of the temperature
    xp, xr = ld.p_sample(x, None, tt, clip_denoised=clip, return_x0=True, temperture=temp, noise=nz)
    _same(xp, fx[tag + "_xprev"], "x_prev")
    _same(xr, fx[tag + "_xrecon"], "x_recon")
    xp1 = ld.p_sample(x, None, tt, clip_denoised=clip, temperature=temp, noise=nz)
    assert np.array_equal(_bits(xp1), _bits(xp))
    # the two halves, fed their own x_recon, give the one-call x_prev bit for bit
    tab = ld._host_tables()
    _, xr2 = ops.posterior_step(x, mo, t, tab, stage=1, clip=clip, x0_param=param == "x0")
    xp2, _ = ops.posterior_step(x, None, t, tab, noise=nz, stage=2, x_recon_in=xr2, temperature=temp)
    assert np.array_equal(_bits(xr2), _bits(xr)) and np.array_equal(_bits(xp2), _bits(xp))
    # p_mean_variance: the same x_recon; its mean is the step without noise; table entries broadcast
    mean, var, logvar, xr3 = ld.p_mean_variance(x, None, tt, clip_denoised=clip, return_x0=True)
    assert np.array_equal(_bits(xr3), _bits(xr))
    _same(mean, ld.p_sample(x, None, tt, clip_denoised=clip, noise=torch.zeros_like(x)).cpu().numpy())
    assert var.shape == logvar.shape == (shape[0], 1, 1, 1)
    assert torch.equal(var.reshape(-1).cpu(), ld.posterior_variance.cpu()[t])
    if param == "eps" and not clip:
        assert np.array_equal(_bits(ld.predict_start_from_noise(x, tt, mo)), _bits(xr))
        assert np.array_equal(_bits(ld.q_posterior(xr, x, tt)[0]), _bits(mean))


def test_posterior_step_in_place_unaligned_and_rejects(sdk):
    """x_prev written over x, on a view that is not 16-byte aligned (scalar path), equals the aligned result."""
    from sd_amd import ops
    shape, t = cu.STEP_CASES[0]
    x, mo, nz = (_gpu(a) for a in cu.step_inputs(shape))
    ld = _stub_ld(sdk, cu.STEP_SCHEDULE, outputs=mo)
    tab = ld._host_tables()
    ref, _ = ops.posterior_step(x, mo, t, tab, noise=nz)
    n = x.numel()
    buf = torch.zeros(3, n + 1, device=DEV)
    xs, ms, ns = (buf[i, 1:].view(shape) for i in range(3))     # 4 bytes past a 16-byte boundary
    xs.copy_(x), ms.copy_(mo), ns.copy_(nz)
    assert xs.data_ptr() % 16 == 4
    out, _ = ops.posterior_step(xs, ms, t, tab, noise=ns, x_prev=xs)
    assert out.data_ptr() == xs.data_ptr() and torch.equal(xs, ref)
    with pytest.raises(ValueError):
        ops.posterior_step(x, mo[:1], t, tab, noise=nz)
    with pytest.raises(ValueError):
        ops.posterior_step(x, mo, [1, 2, 3], tab, noise=nz)


# ------------------------------------------------------------------ masked blend
@pytest.mark.parametrize("binary", [True, False], ids=["bin", "frac"])
@pytest.mark.parametrize("kind", cu.BLEND_MASKS)
def test_masked_q_sample_bitexact_vs_reference(sdk, kind, binary):
    from sd_amd import ops
    fx = load("ca_blend")[f"{kind}_{'bin' if binary else 'frac'}"]
    x0, qn, imgs = (_gpu(a) for a in cu.blend_inputs())
    mask = _gpu(cu.blend_mask(kind, binary))
    ld = _stub_ld(sdk, cu.LOOP_SCHEDULE)
    tab = ld._host_tables()
    for i in range(cu.LOOP_T):
        img = imgs[i].clone()
        out = ops.masked_q_sample(x0, qn[i], mask, img, i, tab["sqrt_acp"], tab["sqrt_1m_acp"])
        assert out.data_ptr() != img.data_ptr() and torch.equal(img, imgs[i])
        _same(out, fx[i], f"t={i} out of place")
        same = ops.masked_q_sample(x0, qn[i], mask, img, i, tab["sqrt_acp"], tab["sqrt_1m_acp"], out=img)
        assert same.data_ptr() == img.data_ptr()
        _same(img, fx[i], f"t={i} in place")
    # per-sample timesteps: sample b at t_b is row b of that timestep's fixture
    ts = [4, 1]
    mixed_n = torch.stack([qn[ts[b]][b] for b in range(2)])
    mixed_i = torch.stack([imgs[ts[b]][b] for b in range(2)])
    out = ops.masked_q_sample(x0, mixed_n, mask, mixed_i, ts, tab["sqrt_acp"], tab["sqrt_1m_acp"])
    _same(out, np.stack([fx[ts[b]][b] for b in range(2)]), "per-sample t")
    # q_sample alone: mask of ones
    ones = torch.ones(cu.BLEND_SHAPE, device=DEV)
    q = ld.q_sample(x0, torch.tensor(ts, device=DEV), noise=mixed_n)
    assert torch.equal(q, ops.masked_q_sample(x0, mixed_n, ones, mixed_i, ts, tab["sqrt_acp"], tab["sqrt_1m_acp"]))


def test_masked_q_sample_rejects_bad_masks(sdk):
    from sd_amd import ops
    x = torch.zeros(cu.BLEND_SHAPE, device=DEV)
    tab = _stub_ld(sdk, cu.LOOP_SCHEDULE)._host_tables()
    for bad in ((2, 1, 5, 1), (1, 3, 5, 5), (2, 2, 5, 5)):
        with pytest.raises(ValueError):
            ops.masked_q_sample(x, x, torch.zeros(bad, device=DEV), x, 0, tab["sqrt_acp"], tab["sqrt_1m_acp"])


# ------------------------------------------------------------------ loops
@pytest.mark.parametrize("mode", cu.LOOP_MODES)
def test_p_sample_loop_bitexact_vs_reference(sdk, mode):
    fx = load("ca_loop")[mode]
    d = {k: _gpu(v) for k, v in cu.loop_inputs().items()}
    cb = vu.case_data(cu.LOOP_VQ_CASE)[0] if mode == "quantize" else None
    ld = _stub_ld(sdk, cu.LOOP_SCHEDULE, clip_denoised=(mode == "clip"), outputs=d["es"], codebook=cb)
    kw = dict(x_T=d["xT"], verbose=False, quantize_denoised=(mode == "quantize"))
    hooks = dict(noise_fn=lambda i, shape: d["nz"][i], q_noise_fn=lambda i, shape: d["qn"][i])
    if mode == "mask":
        kw.update(mask=d["mask"], x0=d["x0"])
    seen = []
    img, inter = ld.p_sample_loop(None, cu.LOOP_SHAPE, return_intermediates=True, log_every_t=1,
                                  img_callback=lambda im, i: seen.append(i), **kw, **hooks)
    assert ld.calls == cu.LOOP_T and seen == list(range(cu.LOOP_T - 1, -1, -1))
    assert len(inter) == cu.LOOP_T + 1 and inter[0].data_ptr() == d["xT"].data_ptr()
    for k in range(cu.LOOP_T):
        _same(inter[k + 1], fx[k], f"{mode}: after timestep {cu.LOOP_T - 1 - k}")
    assert torch.equal(img, inter[-1])
    _same(d["xT"], cu.loop_inputs()["xT"], "x_T was written")
    # sample(...) reaches the same result (its shape / cond handling in front of the same loop)
    out = ld.sample(None, batch_size=cu.LOOP_SHAPE[0], **kw, **hooks)
    assert tuple(out.shape) == cu.LOOP_SHAPE and np.array_equal(_bits(out), _bits(img))
    out2, inter2 = ld.sample(None, batch_size=2, shape=cu.LOOP_SHAPE, return_intermediates=True, **kw, **hooks)
    assert np.array_equal(_bits(out2), _bits(img)) and len(inter2) == cu.LOOP_T + 1


def test_p_sample_loop_under_graph_capture(sdk):
    """The three kernels take the stream and neither allocate nor synchronise: a whole masked loop
    captured in a HIP graph replays to the eager result."""
    d = {k: _gpu(v) for k, v in cu.loop_inputs().items()}
    ld = _stub_ld(sdk, cu.LOOP_SCHEDULE, clip_denoised=True, outputs=d["es"])
    ld.apply_model = lambda x, t, c, return_ids=False: d["es"][ld._cur]      # no device read while capturing
    orig = ld.p_sample

    def p_sample(x, c, t, **kw):
        ld._cur = kw["t_host"]
        return orig(x, c, t, **kw)

    ld.p_sample = p_sample
    run = lambda: ld.p_sample_loop(None, cu.LOOP_SHAPE, x_T=d["xT"], verbose=False, mask=d["mask"], x0=d["x0"],     # noqa: E731
                                   noise_fn=lambda i, s: d["nz"][i], q_noise_fn=lambda i, s: d["qn"][i])
    eager = run().clone()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = run()
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


# ------------------------------------------------------------------ model level
PLAIN9 = dict(image_size=16, in_channels=9, out_channels=4, model_channels=32, attention_resolutions=[2],
              num_res_blocks=1, channel_mult=[1, 2], num_heads=2, use_spatial_transformer=False,
              use_checkpoint=False, legacy=False)


def _wrapper(sdk, unet, key):
    from sd_amd.Diffusion.ddpm import DiffusionWrapper
    dw = DiffusionWrapper.__new__(DiffusionWrapper)
    torch.nn.Module.__init__(dw)
    dw.diffusion_model, dw.conditioning_key, dw._graphed, dw._graphs_on = unet, key, None, False
    return dw


def _concat_unet(sdk):
    from sd_amd.openai_model.model import UNetModel
    z = load("unet_tiny_concat")
    assert cfg_of(z) == cu.TINY_UNET_CONCAT
    m = UNetModel(**cfg_of(z))
    m.load_state_dict(weights_of(z))
    return m.to(DEV), z, {k: _gpu(v) for k, v in cu.unet_inputs().items()}


def test_hybrid_and_concat_equal_the_unet_on_the_concatenated_input(sdk):
    from sd_amd.openai_model.model import UNetModel
    m, _, d = _concat_unet(sdk)
    dw = _wrapper(sdk, m, "hybrid")
    y = dw(d["x"], d["t"], c_concat=[d["m"], d["zi"]], c_crossattn=[d["ctx"]])
    ref = m(torch.cat([d["x"], d["m"], d["zi"]], 1), d["t"], context=d["ctx"])
    assert y.shape == (2, 4, 16, 16) and torch.equal(y, ref)
    assert not torch.equal(y, dw(d["x"], d["t"], c_concat=[1 - d["m"], d["zi"]], c_crossattn=[d["ctx"]]))
    with pytest.raises(ValueError, match="in_channels"):
        dw(d["x"], d["t"], c_concat=[d["zi"]], c_crossattn=[d["ctx"]])
    # 'concat' without a context, on a UNet without cross-attention
    from synth import keys_shapes_of, synth_weights
    p = UNetModel(**PLAIN9)
    p.load_state_dict({k: torch.from_numpy(v) for k, v in synth_weights(keys_shapes_of(p.state_dict()), 73).items()})
    p = p.to(DEV)
    y = _wrapper(sdk, p, "concat")(d["x"], d["t"], c_concat=[d["m"], d["zi"]])
    assert torch.equal(y, p(torch.cat([d["x"], d["m"], d["zi"]], 1), d["t"])) and float(y.abs().max()) > 0


def test_hybrid_unet_vs_reference(sdk):
    m, z, d = _concat_unet(sdk)
    y = _wrapper(sdk, m, "hybrid")(d["x"], d["t"], c_concat=[d["m"], d["zi"]], c_crossattn=[d["ctx"]])
    tag = "tiny 9-channel hybrid UNet vs reference"
    check_parity(tag, y, torch.from_numpy(z["y_hybrid"]), *cu.PARITY_LIMITS[tag])


def test_hybrid_graph_replay_equals_eager_with_new_concat_contents(sdk):
    m, _, d = _concat_unet(sdk)
    dw = _wrapper(sdk, m, "hybrid")
    calls = [(d["x"], [d["m"], d["zi"]]),
             (d["x"] * 0.5 + 0.25, [1 - d["m"], d["zi"].flip(0) * 1.5])]      # same shapes, other contents
    eager = [dw(x, d["t"], c_concat=cc, c_crossattn=[d["ctx"]]).clone() for x, cc in calls]
    assert not torch.equal(eager[0], eager[1])
    dw.use_graphs(True)
    for rnd in range(2):                     # the second round replays only
        for (x, cc), ref in zip(calls, eager):
            assert torch.equal(dw(x, d["t"], c_concat=cc, c_crossattn=[d["ctx"]]), ref), f"round {rnd}"
    assert len(dw._graphed.graphs) == 1


def test_ddim_sample_with_concat_conditioning_end_to_end(sdk):
    """The existing DDIMSampler through apply_model with conditioning_key='concat' and the conditioning
    passed as {'c_concat': [c]}: completes and equals a hand-rolled loop over the same wrapper."""
    from sd_amd import ops
    from sd_amd.DDIM.ddim import DDIMSampler
    from sd_amd.Diffusion.ddpm import LatentDiffusion
    from sd_amd.openai_model.model import UNetModel
    from synth import keys_shapes_of, synth_weights
    cfg = dict(PLAIN9, in_channels=8)
    p = UNetModel(**cfg)
    p.load_state_dict({k: torch.from_numpy(v) for k, v in synth_weights(keys_shapes_of(p.state_dict()), 79).items()})

    class LD(LatentDiffusion):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.parameterization, self.v_posterior = "eps", 0.
            self.model = _wrapper(sdk, p, "concat")
            self.register_schedule(beta_schedule="linear", timesteps=1000, linear_start=0.00085, linear_end=0.012)

    ld = LD().to(DEV)
    xT, c = _gpu(vu.randn(8300, 2, 4, 16, 16)), _gpu(vu.randn(8301, 2, 4, 16, 16))
    cond = {"c_concat": [c]}
    s = DDIMSampler(ld)
    out, _ = s.sample(S=4, batch_size=2, shape=(4, 16, 16), conditioning=cond, eta=0.0, x_T=xT, verbose=False,
                      unconditional_guidance_scale=1.)
    assert out.shape == xT.shape and bool(torch.isfinite(out).all()) and not torch.equal(out, xT)
    x = xT
    for index in range(3, -1, -1):
        ts = torch.full((2,), int(s.ddim_timesteps[index]), device=DEV, dtype=torch.long)
        e = ld.model(x, ts, c_concat=[c])
        x, _ = ops.ddim_step(x, e.float().contiguous(), s.step_scalars(index))
    assert torch.equal(out, x)
