"""Mirror of the inference surface of ``Diffusion/ddpm.py`` — DiffusionWrapper and LatentDiffusion.

Kept: ``register_schedule`` buffers (``ddpm.py:195-253``), ``apply_model``
conditioning wrapping (``ddpm.py:1139-1147,1269-1272`` → ``{'c_crossattn': [c]}``),
``DiffusionWrapper.forward`` dispatch (``ddpm.py:46-73``: None, 'crossattn', 'concat' and 'hybrid' — the
channel concat is folded into the UNet's input pack; 'adm' passes ``y = c_crossattn[0]`` to a UNet with a
class head, ``num_classes``, and raises for one without),
LatentDiffusion's ancestral sampler (``ldm/diffusion/ddpm.py:1528-1811``: ``q_sample`` …
``p_sample_loop`` / ``sample`` with ``clip_denoised``, ``quantize_denoised``, ``mask`` / ``x0``), ``decode_first_stage``
with the CompVis scaling ``z / scale_factor`` (``ldm/diffusion/ddpm.py:1095``;
``Diffusion/ddpm.py:728`` drops z — SURVEY Q8), ``parameterization``.
``cond_stage_config`` is instantiated as the reference does (``ddpm.py:568-587``:
``__is_first_stage__`` / ``__is_unconditional__`` / a target, frozen), so the reference YAML's
``clip_encoder.modules.FrozenCLIPEmbedder`` resolves to the HIP-backed text tower;
``get_learned_conditioning`` (``ddpm.py:1031-1051``) encodes through it.
``use_graphs(True)`` makes ``DiffusionWrapper.forward`` replay one HIP graph per UNet call
(``graphs.GraphedUNet``) — same chain apply_model → DiffusionWrapper.forward → UNetModel,
one hipGraphLaunch per step instead of ~600 kernel launches.
``score_corrector`` / ``noise_dropout`` (``ldm/diffusion/ddpm.py:1544-1546,1623-1624``; the keep mask is drawn
with torch and multiplied in by ``sdk_posterior_step_ex``), ``progressive_denoising`` (``:1641-1739``),
``shorten_cond_schedule`` (``make_cond_schedule`` ``:676-681`` and the ``q_sample`` of the conditioning in both
loops, Gaussian noise) and ``sample_log`` (``:1814-1826``) follow the reference; the hooks ``noise_fn``,
``q_noise_fn``, ``dropout_fn`` and ``cond_noise_fn`` supply recorded draws.
``split_input_params`` (the large-image path) is read in the reference's three places: ``decode_first_stage``
(``ddpm.py:731``, tiled decode), ``encode_first_stage`` (``:808-846``, tiled encode with ``patch_distributed_vq``; a KL
posterior is blended as its moments) and ``apply_model`` (``:1151-1266``: the UNet on overlapping
latent patches gathered by ``sdk_patch_pack`` and blended by ``sdk_fold_patches``, conditioning by key, chunks of
``max_batch``; ``sp['patch_unet'] = False``, an extension, keeps the UNet untiled).  Refused there: ``return_ids``
(ValueError, the reference asserts), ``cond_stage_key == 'coordinates_bbox'`` (NotImplementedError) and a patch
geometry that leaves pixels uncovered (ValueError; the reference divides 0 by 0).
Refused (NotImplementedError): ``return_codebook_ids`` (the reference itself raises on it), and the four options
above on a model that is not on the GPU (HIP kernels, no CPU fallback).
Out of scope (training / Lightning): losses, EMA, optimisers, data, logging.
"""
from __future__ import annotations

import math

import numpy as np
import torch
from torch import nn

from .. import ops
from ..DDIM.diffusion_modules import register_schedule
from .utils import instantiate_from_config


class DiffusionWrapper(nn.Module):
    def __init__(self, diff_model_config, conditioning_key):
        super().__init__()
        self.diffusion_model = instantiate_from_config(diff_model_config)
        self.conditioning_key = conditioning_key
        assert self.conditioning_key in [None, "concat", "crossattn", "hybrid", "adm"]
        self._graphed = None
        self._graphs_on = False

    def use_graphs(self, on=True):
        """Route the UNet call through one captured HIP graph per (shape, context) key (the
        captured graphs are kept while switched off, e.g. for an eager profiling pass)."""
        from ..graphs import GraphedUNet
        if on and self._graphed is None:
            self._graphed = GraphedUNet(self.diffusion_model)
        self._graphs_on = bool(on)

    @staticmethod
    def _int_timesteps(t, device):
        """Timesteps as int64 on the device, the same check on both paths: fractional values raise
        (the UNet's sinusoidal table is indexed by integer steps); only a floating-point t is
        checked, so the sampler's int64 timesteps never cost a host sync."""
        if not torch.is_tensor(t):
            t = torch.as_tensor(t)
        if t.is_floating_point():
            if not bool((t == t.round()).all()):
                raise ValueError("sd_amd: timesteps must be integral")
        return t.to(device=device, dtype=torch.long)

    def _unet(self, x, t, context=None, concat=None, y=None, patches=None):
        t = self._int_timesteps(t, x.device)
        kw = {"concat": list(concat)} if concat else {}
        if y is not None:
            kw["y"] = y
        if patches is not None:
            kw["patches"] = tuple(int(v) for v in patches)
        if self._graphs_on:
            return self._graphed(x, t.reshape(-1).expand(x.shape[0] if patches is None else kw["patches"][5]),
                                 context, **kw)
        return self.diffusion_model(x, t, context=context, **kw)

    def forward(self, x, t, c_concat: list = None, c_crossattn: list = None, patches=None):
        """``patches`` (extension): ``UNetModel.forward``'s patch window; ``x`` and ``c_concat`` are then the
        full-size tensors, ``t`` and ``c_crossattn`` are per patch."""
        if self.conditioning_key is None:
            return self._unet(x, t, patches=patches)
        if self.conditioning_key == "crossattn":
            cc = c_crossattn[0] if len(c_crossattn) == 1 else torch.cat(c_crossattn, 1)
            return self._unet(x, t, context=cc, patches=patches)
        if self.conditioning_key in ("concat", "hybrid"):
            # Diffusion/ddpm.py:51-63: torch.cat([x] + c_concat, 1) — done inside the UNet's input pack
            if not c_concat:
                raise ValueError(f"sd_amd: conditioning_key={self.conditioning_key} needs c_concat")
            cc = None
            if self.conditioning_key == "hybrid":
                if not c_crossattn:
                    raise ValueError("sd_amd: conditioning_key=hybrid needs c_crossattn")
                cc = c_crossattn[0] if len(c_crossattn) == 1 else torch.cat(c_crossattn, 1)
            return self._unet(x, t, context=cc, concat=c_concat, patches=patches)
        if getattr(self.diffusion_model, "num_classes", None) is None:
            raise NotImplementedError(f"sd_amd: conditioning_key={self.conditioning_key} needs a class-conditional "
                                      "UNet (this one has no class head: num_classes is None)")
        # Diffusion/ddpm.py:65-67: the class labels travel as c_crossattn[0]
        if not c_crossattn:
            raise ValueError("sd_amd: conditioning_key=adm needs c_crossattn=[y]")
        return self._unet(x, t, y=c_crossattn[0], patches=patches)


def _is_vq(first_stage):
    from ..vqvae.autoencoder import VQModelInterface
    return isinstance(first_stage, VQModelInterface)


def _first_stage_decode(first_stage, z, pre_scale, force_not_quantize=False):
    """One first-stage decode of ``pre_scale * z``; a ``VQModelInterface`` quantises first unless
    ``force_not_quantize`` (``Diffusion/ddpm.py:756-798``)."""
    if _is_vq(first_stage):
        return first_stage.decode(z, force_not_quantize=force_not_quantize, pre_scale=pre_scale)
    return first_stage.decode(z, pre_scale=pre_scale)


class LatentDiffusion(nn.Module):
    def __init__(self, first_stage_config, cond_stage_config=None, unet_config=None, num_timesteps_cond=None,
                 cond_stage_key="txt", cond_stage_trainable=False, concat_mode=True, cond_stage_forward=None,
                 conditioning_key=None, scale_factor=1.0, scale_by_std=False, timesteps=1000,
                 beta_schedule="linear", linear_start=1e-4, linear_end=2e-2, cosine_s=8e-3, given_betas=None,
                 parameterization="eps", image_size=256, channels=3, first_stage_key="image", log_every_t=100,
                 clip_denoised=True, v_posterior=0., **ignored):
        super().__init__()
        assert parameterization in ["eps", "x0", "v"], "eps / x0 (reference) or v (extension, SURVEY Q9)"
        # x0 runs through the ancestral sampler (p_sample_loop); DDIMSampler.p_sample_ddim refuses it
        self.parameterization = parameterization
        self.clip_denoised = clip_denoised
        self.v_posterior = v_posterior
        self.num_timesteps_cond = 1 if num_timesteps_cond is None else num_timesteps_cond
        self.shorten_cond_schedule = self.num_timesteps_cond > 1
        if conditioning_key is None:
            conditioning_key = "concat" if concat_mode else "crossattn"
        if cond_stage_config == "__is_unconditional__":
            conditioning_key = None
        self.conditioning_key = conditioning_key
        self.model = DiffusionWrapper(unet_config, conditioning_key)
        self.first_stage_model = instantiate_from_config(first_stage_config)
        self.cond_stage_trainable = cond_stage_trainable
        self.cond_stage_key = cond_stage_key
        self.cond_stage_forward = cond_stage_forward
        self.instantiate_cond_stage(cond_stage_config)
        self.scale_factor = scale_factor
        self.image_size = image_size
        self.channels = channels
        self.log_every_t = log_every_t
        self.register_schedule(given_betas=given_betas, beta_schedule=beta_schedule, timesteps=timesteps,
                               linear_start=linear_start, linear_end=linear_end, cosine_s=cosine_s)
        if self.shorten_cond_schedule:
            self.make_cond_schedule()

    def make_cond_schedule(self):
        """``ldm/diffusion/ddpm.py:676-681``: the conditioning's timestep per sampler timestep, the same torch
        CPU calls (a host table: the loops index it with host ints)."""
        with torch.device("cpu"):
            self.cond_ids = torch.full(size=(self.num_timesteps,), fill_value=self.num_timesteps - 1, dtype=torch.long)
            ids = torch.round(torch.linspace(0, self.num_timesteps - 1, self.num_timesteps_cond)).long()
            self.cond_ids[:self.num_timesteps_cond] = ids

    def register_schedule(self, given_betas=None, beta_schedule="linear", timesteps=1000, linear_start=1e-4,
                          linear_end=2e-2, cosine_s=8e-3):
        """``DDPM.register_schedule`` (``Diffusion/ddpm.py:195-253``): the twelve fp32 buffers, with
        ``self.v_posterior`` in the posterior variance (the training-only ``lvlb_weights`` is left out)."""
        sch = register_schedule(timesteps, linear_start, linear_end, beta_schedule, given_betas, cosine_s,
                                v_posterior=getattr(self, "v_posterior", 0.))
        self.num_timesteps = sch.pop("num_timesteps")
        self.linear_start, self.linear_end = linear_start, linear_end
        for k, v in sch.items():
            self.register_buffer(k, v)
        self._post_cache = None

    @property
    def device(self):
        return next(self.model.parameters()).device

    def use_graphs(self, on=True):
        self.model.use_graphs(on)

    def instantiate_cond_stage(self, config):
        """Reference ``Diffusion/ddpm.py:568-587`` (inference: the stage is always frozen)."""
        if config is None or config == "__is_unconditional__":
            self.cond_stage_model = None
        elif config == "__is_first_stage__":
            self.cond_stage_model = self.first_stage_model
        else:
            model = instantiate_from_config(config)
            self.cond_stage_model = model.eval()
            for param in self.cond_stage_model.parameters():
                param.requires_grad = False

    @torch.no_grad()
    def get_learned_conditioning(self, c):
        """Reference ``Diffusion/ddpm.py:1031-1051``: encode prompts (or token ids) with the cond stage."""
        if self.cond_stage_forward is None:
            if hasattr(self.cond_stage_model, "encode") and callable(self.cond_stage_model.encode):
                c = self.cond_stage_model.encode(c)
                from ..Distribution.distribution import DiagonalGaussianDistribution
                if isinstance(c, DiagonalGaussianDistribution):
                    c = c.mode()
            else:
                c = self.cond_stage_model(c)
        else:
            assert hasattr(self.cond_stage_model, self.cond_stage_forward)
            c = getattr(self.cond_stage_model, self.cond_stage_forward)(c)
        return c

    def apply_model(self, x_noisy, t, cond, return_ids=False):
        if isinstance(cond, dict):
            pass
        else:
            if not isinstance(cond, list):
                cond = [cond]
            key = "c_concat" if self.model.conditioning_key == "concat" else "c_crossattn"
            cond = {key: cond}
        sp = getattr(self, "split_input_params", None)
        if sp is not None and sp.get("patch_unet", True):
            # Diffusion/ddpm.py:1151: the attribute's presence is the trigger (sp['patch_unet'] = False, an
            # extension, keeps the UNet untiled); None: the latent is one patch, the untiled call below
            out = self._apply_model_patched(x_noisy, t, cond, sp, return_ids)
            if out is not None:
                return out
        if self.model.conditioning_key is None:
            return self.model(x_noisy, t)
        return self.model(x_noisy, t, **cond)

    # ------------------------------------------------------------------ patch-wise UNet
    PATCH_CONTEXT_CACHE_SIZE = 4     # repeated conditionings kept: cond, uncond, their CFG concat, one spare

    @staticmethod
    def _check_coverage(h, w, ks, stride, what):
        """Patches of ``ks`` every ``stride`` must reach the last row and column and leave no gap between them: a
        pixel that no patch covers has normalisation 0, and the reference's ``fold(o) / normalization`` is 0 / 0
        there."""
        if (h - ks[0]) % stride[0] or (w - ks[1]) % stride[1] or stride[0] > ks[0] or stride[1] > ks[1]:
            raise ValueError(f"sd_amd: {what} with split_input_params: patches of ks {tuple(ks)} every stride "
                             f"{tuple(stride)} leave part of the {h}x{w} tensor uncovered ((h - ks) % stride must "
                             "be 0 and stride <= ks in both dimensions); the blend would be 0 / 0 = NaN there")

    def _patch_weights(self, slot, h, w, Ly, Lx, sp, device):
        """``get_weighting`` on the device, cached per ``slot`` ('apply' / 'encode') as ``_decode_tiled`` caches
        its own in ``_tile_w``, so the three tiled paths of one sampling run do not evict each other."""
        key = (h, w, Ly, Lx, device, sp["clip_min_weight"], sp["clip_max_weight"], bool(sp.get("tie_braker", False)))
        cache = self.__dict__.setdefault("_patch_w", {})
        ent = cache.get(slot)
        if ent is None or ent[0] != key:
            pix, lw = self.get_weighting(h, w, Ly, Lx, sp)
            ent = (key, torch.from_numpy(pix).to(device), torch.from_numpy(lw).to(device) if lw is not None else None)
            cache[slot] = ent
        return ent[1], ent[2]

    def _patch_contexts(self, c, L, chunk):
        """``c`` repeated for the L patches (patch ``p = l*B + b`` takes ``c[b]``) and cut into the chunks the UNet
        is called with, the SAME tensor objects on every call: ``UNetModel._context_kv`` (and a captured graph)
        recognise a conditioning by identity, so a repeat made afresh per step would re-project K/V for L·B rows at
        every step.  Keyed on ``(id, _version, L, chunk)`` with a strong reference to ``c``; oldest entry out."""
        from collections import OrderedDict
        cache = self.__dict__.setdefault("_patch_ctx", OrderedDict())
        key = (id(c), c._version, L, chunk)
        ent = cache.get(key)
        if ent is None or ent[0] is not c:
            rep = c.repeat(L, *([1] * (c.dim() - 1)))
            ent = (c, [rep[i:i + chunk] for i in range(0, rep.shape[0], chunk)])
            cache[key] = ent
            while len(cache) > self.PATCH_CONTEXT_CACHE_SIZE:
                cache.popitem(last=False)
        cache.move_to_end(key)
        return ent[1]

    def _apply_model_patched(self, x, t, cond, sp, return_ids):
        """``Diffusion/ddpm.py:1151-1266``: the UNet on overlapping latent patches of ``ks`` every ``stride``,
        blended by ``get_weighting``.  The patches are never materialised in fp32: ``UNetModel.forward(patches=)``
        gathers each chunk of ``sp.get('max_batch', 16)`` patches straight into its input layout
        (``sdk_patch_pack``), every chunk's output lands in one ``[L, B, C, kh, kw]`` buffer, one
        ``sdk_fold_patches`` blends it.  Conditioning goes by key: ``c_concat`` entries are spatial and gathered
        with ``x``, ``c_crossattn`` entries (class labels of 'adm' included) are repeated for the L patches.
        Returns None when the latent is a single patch."""
        if return_ids:
            raise ValueError("sd_amd: return_ids is not supported with split_input_params (Diffusion/ddpm.py:1157)")
        if self.cond_stage_key == "coordinates_bbox":
            raise NotImplementedError("sd_amd: split_input_params with cond_stage_key='coordinates_bbox' is not "
                                      "implemented (the reference has no bbox_tokenizer)")
        B, _, h, w = x.shape
        ks, stride, Ly, Lx = ops.patch_grid(h, w, sp["ks"], sp["stride"])
        self._check_coverage(h, w, ks, stride, "apply_model")
        L = Ly * Lx
        if L == 1:
            return None
        wrapper = self.model
        ckey = wrapper.conditioning_key
        concat = list(cond.get("c_concat") or []) if ckey in ("concat", "hybrid") else []
        cross = list(cond.get("c_crossattn") or []) if ckey in ("crossattn", "hybrid", "adm") else []
        for c in concat:
            if not torch.is_tensor(c) or c.dim() != 4 or c.shape[0] != B or c.shape[2:] != x.shape[2:]:
                raise ValueError(f"sd_amd: c_concat entries must be NCHW of x's batch and spatial size "
                                 f"{tuple(x.shape)} to be cut into patches, got {tuple(getattr(c, 'shape', ()))}")
        chunk = max(1, int(sp.get("max_batch", 16)))
        total = L * B
        nchunks = -(-total // chunk)
        cross = [self._patch_contexts(c if torch.is_tensor(c) else torch.as_tensor(c), L, chunk) for c in cross]
        unet = wrapper.diffusion_model
        if cross and ckey != "adm" and 2 * nchunks > unet.CONTEXT_CACHE_SIZE:
            # K/V of every chunk context of one cond / uncond pair stay resident across the sampler's steps
            unet.CONTEXT_CACHE_SIZE = 2 * nchunks
        pix_w, l_w = self._patch_weights("apply", ks[0], ks[1], Ly, Lx, sp, x.device)
        tt = torch.as_tensor(t).reshape(-1)
        tt = (tt.expand(B) if tt.numel() == 1 else tt).repeat(L)
        dtype, x = x.dtype, self._f32(x)
        buf = None
        for k, p0 in enumerate(range(0, total, chunk)):
            n = min(chunk, total - p0)
            kw = {}
            if concat:
                kw["c_concat"] = concat
            if cross:
                kw["c_crossattn"] = [c[k] for c in cross]
            out = wrapper(x, tt[p0:p0 + n], patches=(ks[0], ks[1], stride[0], stride[1], p0, n), **kw)
            if buf is None:
                buf = torch.empty(L, B, out.shape[1], ks[0], ks[1], dtype=torch.float32, device=x.device)
            buf.view(total, out.shape[1], ks[0], ks[1])[p0:p0 + n].copy_(out)
        out = ops.fold_patches(buf, pix_w, l_w, h, w, stride[0], stride[1], Ly, Lx)
        return out if dtype == torch.float32 else out.to(dtype)

    # ------------------------------------------------------------------ ancestral sampler
    # LatentDiffusion's own sampler (``ldm/diffusion/ddpm.py:1528-1811``; the reference's
    # ``sample_log(ddim=False)`` path) on three fused HIP kernels: ``sdk_posterior_step`` (predict x0 →
    # clamp → posterior mean → + σ·noise, one launch; two with the nearest-code search of
    # ``quantize_denoised`` in between), ``sdk_masked_q_sample`` (known-region blend) and
    # ``sdk_stochastic_encode`` (q_sample).  fp32, no contraction: bit-identical to the reference's
    # expressions on the same inputs.  Reference quirks resolved as CompVis does:
    # q_sample draws Gaussian noise (ldm's copy draws ``rand_like``), ``p_sample(return_x0=True)`` ADDS
    # the noise term (ldm ``:1633`` multiplies), ``posterior_variance`` is spelt correctly, nothing is
    # forced onto ``cuda:0``.
    def _host_tables(self):
        """Host fp32 copies of the per-timestep scalars the kernels take, and
        σ_t = exp(0.5·posterior_log_variance_clipped[t]), the reference's ``(0.5 * model_log_variance).exp()``,
        as the correctly rounded fp32 value (libm's fp64 exp, rounded once).  torch's own CPU fp32 ``exp`` is
        within 1 ulp of it but depends on the host (its AVX2 and AVX-512 paths differ in the last bit for
        some entries), which would make a run irreproducible across machines; rebuilt when the buffers change."""
        lv = self.posterior_log_variance_clipped
        key = (lv.data_ptr(), lv._version, self.posterior_mean_coef1.data_ptr(), self.sqrt_alphas_cumprod.data_ptr())
        ent = getattr(self, "_post_cache", None)
        if ent is not None and ent[0] == key:
            return ent[1]
        host = lambda b: b.detach().to("cpu", torch.float32)      # noqa: E731
        tab = {"c_recip": host(self.sqrt_recip_alphas_cumprod).numpy(),
               "c_recipm1": host(self.sqrt_recipm1_alphas_cumprod).numpy(),
               "coef1": host(self.posterior_mean_coef1).numpy(), "coef2": host(self.posterior_mean_coef2).numpy(),
               "sigma": np.asarray([math.exp(0.5 * float(v)) for v in host(lv).tolist()], dtype=np.float32),
               "sqrt_acp": host(self.sqrt_alphas_cumprod).numpy(),
               "sqrt_1m_acp": host(self.sqrt_one_minus_alphas_cumprod).numpy()}
        self._post_cache = (key, tab)
        return tab

    def _host_t(self, t, b):
        """Timesteps as a list of ``b`` host ints, range-checked (a device ``t`` costs one sync; the
        sampler loop passes host ints)."""
        if torch.is_tensor(t):
            t = t.reshape(-1).tolist()
        elif not isinstance(t, (list, tuple)):
            t = [t]
        t = [int(v) for v in t]
        if len(t) == 1:
            t = t * b
        if len(t) != b or not all(0 <= v < self.num_timesteps for v in t):
            raise ValueError(f"sd_amd: timesteps {t} for a batch of {b} and {self.num_timesteps} steps")
        return t

    @staticmethod
    def _f32(x):
        return x.float().contiguous()

    def _bcast(self, buf, t, x):
        tt = torch.as_tensor(t, device=buf.device, dtype=torch.long)
        return buf[tt].reshape(len(t), *((1,) * (x.dim() - 1))).to(x.device)

    @torch.no_grad()
    def q_sample(self, x_start, t, noise=None):
        """q(x_t | x_0) = sqrt_alphas_cumprod[t]·x_start + sqrt_one_minus_alphas_cumprod[t]·noise with
        Gaussian noise (``Diffusion/ddpm.py:326-342``), per-sample ``t``."""
        x_start = self._f32(x_start)
        if noise is None:
            noise = torch.randn_like(x_start)
        noise = noise.to(device=x_start.device, dtype=torch.float32).contiguous()
        tab = self._host_tables()
        out = torch.empty_like(x_start)
        for b0, b1, ti in ops._t_runs(self._host_t(t, x_start.shape[0]), x_start.shape[0]):
            ops.stochastic_encode(x_start[b0:b1], noise[b0:b1], float(tab["sqrt_acp"][ti]),
                                  float(tab["sqrt_1m_acp"][ti]), out=out[b0:b1])
        return out

    @torch.no_grad()
    def predict_start_from_noise(self, x_t, t, noise):
        x_t = self._f32(x_t)
        return ops.posterior_step(x_t, self._f32(noise), self._host_t(t, x_t.shape[0]), self._host_tables(),
                                  stage=1)[1]

    @torch.no_grad()
    def q_posterior(self, x_start, x_t, t):
        """(posterior mean, variance, clipped log-variance) of q(x_{t-1} | x_t, x_0); the last two are
        the ``[b, 1, 1, 1]`` table entries as the reference's ``extract_into_tensor`` returns them."""
        x_t = self._f32(x_t)
        th = self._host_t(t, x_t.shape[0])
        mean = self._posterior_mean(self._f32(x_start), x_t, th)
        return mean, self._bcast(self.posterior_variance, th, x_t), \
            self._bcast(self.posterior_log_variance_clipped, th, x_t)

    def _posterior_mean(self, x_recon, x, th):
        # stage 2 without noise: the noise term is (0·σ)·(0·T) = 0, x_prev = mean + 0
        return ops.posterior_step(x, None, th, self._host_tables(), stage=2, x_recon_in=x_recon)[0]

    def _refuse(self, return_codebook_ids=False):
        if return_codebook_ids:
            raise NotImplementedError("sd_amd: return_codebook_ids is not implemented (the reference dropped it)")

    @staticmethod
    def _need_gpu(device, noise_dropout=0., score_corrector=None, **flags):
        """Off the GPU these options stay NotImplementedError, as before they had kernels."""
        for on, option in [(noise_dropout > 0, "noise_dropout"), (score_corrector is not None, "score_corrector")] + \
                [(on, name) for name, on in flags.items()]:
            if on:
                ops.need_gpu_sampler(option, device)

    def _model_out(self, x, c, t, score_corrector=None, corrector_kwargs=None):
        """``apply_model`` and the optional ``score_corrector.modify_score`` (``ldm/diffusion/ddpm.py:1542-1546``)."""
        model_out = self._f32(self.apply_model(x, t, c))
        if score_corrector is None:
            return model_out
        if self.parameterization != "eps":
            raise AssertionError(f"sd_amd: score_corrector needs an eps model (ddpm.py:1545), this one is "
                                 f"'{self.parameterization}'")
        out = score_corrector.modify_score(self, model_out, x, t, c, **(corrector_kwargs or {}))
        if not torch.is_tensor(out) or not out.is_cuda or out.dtype != torch.float32 or out.shape != x.shape:
            raise ValueError("sd_amd: score_corrector.modify_score must return a CUDA fp32 tensor of x's shape "
                             f"{tuple(x.shape)}")
        return out.contiguous()

    def _quantizer(self):
        q = getattr(getattr(self, "first_stage_model", None), "quantize", None)
        if q is None or not hasattr(q, "nearest"):
            raise AttributeError("sd_amd.LatentDiffusion: quantize_denoised needs a VQ first stage "
                                 "(first_stage_model.quantize); this model's first stage has no quantizer")
        return q

    def _x_recon(self, x, model_out, th, clip_denoised, quantize_denoised):
        if self.parameterization not in ("eps", "x0"):
            raise NotImplementedError(f"sd_amd: the ancestral sampler takes eps / x0 models, not "
                                      f"'{self.parameterization}'")
        x_recon = ops.posterior_step(x, model_out, th, self._host_tables(), stage=1, clip=clip_denoised,
                                     x0_param=self.parameterization == "x0")[1]
        if quantize_denoised:
            x_recon, _ = self._quantizer().nearest(x_recon)
        return x_recon

    @torch.no_grad()
    def p_mean_variance(self, x, c, t, clip_denoised: bool, return_codebook_ids=False, quantize_denoised=False,
                        return_x0=False, score_corrector=None, corrector_kwargs=None):
        self._refuse(return_codebook_ids)
        self._need_gpu(x.device, score_corrector=score_corrector)
        x = self._f32(x)
        th = self._host_t(t, x.shape[0])
        model_out = self._model_out(x, c, t, score_corrector, corrector_kwargs)
        x_recon = self._x_recon(x, model_out, th, clip_denoised, quantize_denoised)
        out = (self._posterior_mean(x_recon, x, th), self._bcast(self.posterior_variance, th, x),
               self._bcast(self.posterior_log_variance_clipped, th, x))
        return out + (x_recon,) if return_x0 else out

    @torch.no_grad()
    def p_sample(self, x, c, t, clip_denoised=False, repeat_noise=False, return_codebook_ids=False,
                 quantize_denoised=False, return_x0=False, temperture=1., noise_dropout=0., score_corrector=None,
                 corrector_kwargs=None, temperature=None, noise=None, t_host=None, keep=None):
        """One ancestral step x_t → x_{t-1}.  ``temperture`` is the reference's spelling; ``temperature``
        (when given) overrides it.  Extensions: ``noise`` (recorded noise instead of a fresh draw), ``keep`` (the
        keep mask of ``noise_dropout``, one byte per element, instead of a Bernoulli(1 − p) draw) and
        ``t_host`` (``t`` as host ints, saving the device read of ``t``)."""
        self._refuse(return_codebook_ids)
        if self.parameterization not in ("eps", "x0"):
            raise NotImplementedError(f"sd_amd: the ancestral sampler takes eps / x0 models, not "
                                      f"'{self.parameterization}'")
        if not 0.0 <= float(noise_dropout) <= 1.0:
            raise ValueError(f"sd_amd: noise_dropout must be in [0, 1], got {noise_dropout}")
        self._need_gpu(x.device, noise_dropout, score_corrector)
        temp = float(temperture if temperature is None else temperature)
        x = self._f32(x)
        th = self._host_t(t if t_host is None else t_host, x.shape[0])
        model_out = self._model_out(x, c, t, score_corrector, corrector_kwargs)
        if noise is None:
            from ..DDIM.diffusion_modules import noise_like
            noise = noise_like(x.shape, x.device, repeat_noise)
        noise = noise.to(device=x.device, dtype=torch.float32).contiguous()
        tab = self._host_tables()
        kw = dict(temperature=temp)
        if noise_dropout > 0:
            # ldm/diffusion/ddpm.py:1623-1624: F.dropout of noise·temperature
            kw["keep"] = keep if keep is not None else \
                torch.empty(x.shape, dtype=torch.uint8, device=x.device).bernoulli_(1.0 - float(noise_dropout))
            kw["drop_p"] = float(noise_dropout)
        if not quantize_denoised:
            x_prev, x0 = ops.posterior_step(x, model_out, th, tab, noise=noise, clip=clip_denoised,
                                            x0_param=self.parameterization == "x0", want_x_recon=return_x0, **kw)
        else:
            x0 = self._x_recon(x, model_out, th, clip_denoised, True)
            x_prev, _ = ops.posterior_step(x, None, th, tab, noise=noise, stage=2, x_recon_in=x0, **kw)
        return (x_prev, x0) if return_x0 else x_prev

    def _ancestral_loop(self, cond, shape, x_T, timesteps, temps, progressive, quantize_denoised, mask, x0,
                        log_every_t, callback, img_callback, noise_dropout, score_corrector, corrector_kwargs,
                        noise_fn, q_noise_fn, dropout_fn, cond_noise_fn):
        """The loop of ``p_sample_loop`` (``ldm/diffusion/ddpm.py:1772-1789``) and ``progressive_denoising``
        (``:1704-1737``): ``temps`` is a float or a list indexed by timestep; ``progressive`` collects the
        ``x0_partial``s instead of the images."""
        if not log_every_t:
            log_every_t = self.log_every_t
        device = self.betas.device
        shorten = getattr(self, "shorten_cond_schedule", False)
        self._need_gpu(device, noise_dropout, score_corrector, progressive_denoising=progressive,
                       shorten_cond_schedule=shorten)
        b = shape[0]
        img = torch.randn(tuple(shape), device=device) if x_T is None else x_T.to(device=device, dtype=torch.float32)
        img = img.contiguous()
        intermediates = [] if progressive else [img]
        if mask is not None:
            if x0 is None:
                raise ValueError("sd_amd: mask needs x0 (the known region's latent)")
            if x0.shape[2:] != mask.shape[2:]:
                raise ValueError(f"sd_amd: mask {tuple(mask.shape)} and x0 {tuple(x0.shape)} differ in spatial size")
            mask = mask.to(device=device, dtype=torch.float32)
            x0 = x0.to(device=device, dtype=torch.float32)
        if quantize_denoised:
            self._quantizer()
        if shorten:
            if self.model.conditioning_key == "hybrid":
                raise AssertionError("sd_amd: shorten_cond_schedule does not take hybrid conditioning "
                                     "(ldm/diffusion/ddpm.py:1775)")
            if not torch.is_tensor(cond):
                raise ValueError("sd_amd: shorten_cond_schedule needs the conditioning as one tensor, got "
                                 f"{type(cond).__name__}")
        tab = self._host_tables()
        for i in reversed(range(0, timesteps)):
            ts = torch.full((b,), i, device=device, dtype=torch.long)
            if shorten:
                # reassigned every iteration, exactly as the reference does (:1776-1777)
                cn = cond_noise_fn(i, cond.shape) if cond_noise_fn is not None else torch.randn_like(cond)
                cond = self.q_sample(cond, int(self.cond_ids[i]), noise=cn)
            out = self.p_sample(img, cond, ts, clip_denoised=self.clip_denoised, quantize_denoised=quantize_denoised,
                                return_x0=progressive, t_host=i, noise_dropout=noise_dropout,
                                temperature=temps[i] if isinstance(temps, (list, tuple)) else temps,
                                score_corrector=score_corrector, corrector_kwargs=corrector_kwargs,
                                noise=noise_fn(i, img.shape) if noise_fn is not None else None,
                                keep=dropout_fn(i, img.shape) if dropout_fn is not None else None)
            img, x0_partial = out if progressive else (out, None)
            if mask is not None:
                qn = q_noise_fn(i, img.shape) if q_noise_fn is not None else torch.randn_like(x0)
                img = ops.masked_q_sample(x0, qn.to(device=device, dtype=torch.float32), mask, img, i,
                                          tab["sqrt_acp"], tab["sqrt_1m_acp"], out=img)
            if i % log_every_t == 0 or i == timesteps - 1:
                intermediates.append(x0_partial if progressive else img)
            if callback:
                callback(i)
            if img_callback:
                img_callback(img, i)
        return img, intermediates

    @staticmethod
    def _trim_cond(cond, batch_size):
        if cond is None:
            return None
        if isinstance(cond, dict):
            return {key: cond[key][:batch_size] if not isinstance(cond[key], list) else
                    list(map(lambda x: x[:batch_size], cond[key])) for key in cond}
        return [c[:batch_size] for c in cond] if isinstance(cond, list) else cond[:batch_size]

    @torch.no_grad()
    def progressive_denoising(self, cond, shape, verbose=True, callback=None, quantize_denoised=False,
                              img_callback=None, mask=None, x0=None, temperture=1., noise_dropout=0.,
                              score_corrector=None, corrector_kwargs=None, batch_size=None, x_T=None, start_T=None,
                              log_every_t=None, noise_fn=None, q_noise_fn=None, dropout_fn=None, cond_noise_fn=None):
        """``ldm/diffusion/ddpm.py:1641-1739``: the ancestral loop that returns the ``x0_partial`` of the logged
        steps.  ``batch_size`` prepends to ``shape``; ``temperture`` is a float or a list indexed by timestep.
        The hooks are those of ``p_sample_loop``."""
        if batch_size is not None:
            shape = [batch_size] + list(shape)
        else:
            batch_size = shape[0]
        cond = self._trim_cond(cond, batch_size)
        timesteps = self.num_timesteps
        if start_T is not None:
            timesteps = min(timesteps, start_T)
        temps = list(temperture) if isinstance(temperture, (list, tuple)) else float(temperture)
        return self._ancestral_loop(cond, shape, x_T, timesteps, temps, True, quantize_denoised, mask, x0, log_every_t,
                                    callback, img_callback, noise_dropout, score_corrector, corrector_kwargs,
                                    noise_fn, q_noise_fn, dropout_fn, cond_noise_fn)

    @torch.no_grad()
    def p_sample_loop(self, cond, shape, return_intermediates=False, x_T=None, verbose=True, callback=None,
                      timesteps=None, quantize_denoised=False, mask=None, x0=None, img_callback=None, start_T=None,
                      log_every_t=None, temperature=1., noise_fn=None, q_noise_fn=None, noise_dropout=0.,
                      score_corrector=None, corrector_kwargs=None, dropout_fn=None, cond_noise_fn=None):
        """``ldm/diffusion/ddpm.py:1745-1793``.  Extensions: ``temperature``, ``noise_dropout`` /
        ``score_corrector`` / ``corrector_kwargs`` (passed to ``p_sample``), and the hooks ``noise_fn(i, shape)`` /
        ``q_noise_fn(i, shape)`` / ``dropout_fn(i, shape)`` / ``cond_noise_fn(i, shape)`` that supply the step
        noise, the q_sample noise of the mask blend, the dropout keep mask and the q_sample noise of the
        shortened conditioning schedule at timestep ``i`` (reproducible runs, as DDIMSampler's ``noise_fn``)."""
        if timesteps is None:
            timesteps = self.num_timesteps
        if start_T is not None:
            timesteps = min(timesteps, start_T)
        img, intermediates = self._ancestral_loop(cond, shape, x_T, timesteps, temperature, False, quantize_denoised,
                                                  mask, x0, log_every_t, callback, img_callback, noise_dropout,
                                                  score_corrector, corrector_kwargs, noise_fn, q_noise_fn,
                                                  dropout_fn, cond_noise_fn)
        if return_intermediates:
            return img, intermediates
        return img

    @torch.no_grad()
    def sample(self, cond, batch_size=16, return_intermediates=False, x_T=None, verbose=True, timesteps=None,
               quantize_denoised=False, mask=None, x0=None, shape=None, **kwargs):
        """``ldm/diffusion/ddpm.py:1796-1811``; of ``kwargs`` the p_sample_loop extensions are passed on
        (the reference drops them all)."""
        if shape is None:
            shape = (batch_size, self.channels, self.image_size, self.image_size)
        cond = self._trim_cond(cond, batch_size)
        if "temperture" in kwargs:
            kwargs.setdefault("temperature", kwargs.pop("temperture"))
        self._refuse(kwargs.pop("return_codebook_ids", False))
        extra = {k: kwargs[k] for k in ("temperature", "noise_fn", "q_noise_fn", "callback", "img_callback",
                                        "start_T", "log_every_t", "noise_dropout", "score_corrector",
                                        "corrector_kwargs", "dropout_fn", "cond_noise_fn") if k in kwargs}
        return self.p_sample_loop(cond, shape, return_intermediates=return_intermediates, x_T=x_T, verbose=verbose,
                                  timesteps=timesteps, quantize_denoised=quantize_denoised, mask=mask, x0=x0, **extra)

    @torch.no_grad()
    def sample_log(self, cond, batch_size, ddim, ddim_steps, **kwargs):
        """``ldm/diffusion/ddpm.py:1814-1826``: (samples, intermediates) of the DDIM sampler or of ``sample``."""
        if ddim:
            from ..DDIM.ddim import DDIMSampler
            shape = (self.channels, self.image_size, self.image_size)
            return DDIMSampler(self).sample(ddim_steps, batch_size, shape, cond, verbose=False, **kwargs)
        return self.sample(cond=cond, batch_size=batch_size, return_intermediates=True, **kwargs)

    @torch.no_grad()
    def encode_first_stage(self, x):
        """``ldm/diffusion/ddpm.py:1237-1279``: the first stage's posterior; for a ``VQModelInterface`` the
        pre-quantisation latent ``h`` of its ``(h, 0, info)`` tuple.  With
        ``split_input_params['patch_distributed_vq']`` the tiled (patch) encode (``Diffusion/ddpm.py:808-846``)."""
        sp = getattr(self, "split_input_params", None)
        if sp and sp.get("patch_distributed_vq"):
            enc = self._encode_tiled(x, sp)
            if enc is not None:
                return enc
        enc = self.first_stage_model.encode(x)
        if _is_vq(self.first_stage_model):
            return enc[0]
        return enc

    def _encode_tiled(self, x, sp):
        """Patch encode (``Diffusion/ddpm.py:808-846`` + ``get_fold_unfold`` df branch ``:908-919``): image patches
        of ``ks`` every ``stride`` are encoded in chunks of ``sp.get('max_batch', 16)`` patches·images, weighted and
        overlap-added at 1 / df (df = vqf) on the device.  A VQ first stage blends its pre-quantisation ``h``; a KL
        first stage blends the moments (mean | logvar) and returns their ``DiagonalGaussianDistribution`` (the
        reference stacks distribution objects and cannot run — DESIGN.md Q27).  Returns None for a single tile."""
        from ..Distribution.distribution import DiagonalGaussianDistribution
        df = int(sp["vqf"])
        sp["original_image_size"] = x.shape[-2:]
        B, _, h, w = x.shape
        ks, stride, Ly, Lx = ops.patch_grid(h, w, sp["ks"], sp["stride"])
        if df < 1 or any(v % df for v in ks + stride):
            raise ValueError(f"sd_amd: encode_first_stage with split_input_params: ks {ks} and stride {stride} must "
                             f"be divisible by vqf = {df} (the latent patch grid is theirs over vqf)")
        self._check_coverage(h, w, ks, stride, "encode_first_stage")
        L = Ly * Lx
        if L == 1:
            return None
        vq = _is_vq(self.first_stage_model)
        flat = ops.extract_patches(self._f32(x), ks[0], ks[1], stride[0], stride[1]).view(L * B, -1, ks[0], ks[1])
        chunk = max(1, int(sp.get("max_batch", 16)))
        enc = []
        for i in range(0, L * B, chunk):
            e = self.first_stage_model.encode(flat[i:i + chunk])
            enc.append(e[0] if vq else e.parameters)
        enc = torch.cat(enc, 0) if len(enc) > 1 else enc[0]
        kh, kw = ks[0] // df, ks[1] // df
        if enc.shape[2:] != (kh, kw):
            raise ValueError(f"sd_amd: the first stage maps a {ks[0]}x{ks[1]} patch to {tuple(enc.shape[2:])}, "
                             f"split_input_params['vqf'] = {df} says {kh}x{kw}")
        pix_w, l_w = self._patch_weights("encode", kh, kw, Ly, Lx, sp, x.device)
        out = ops.fold_patches(enc.float().view(L, B, enc.shape[1], kh, kw), pix_w, l_w, h // df, w // df,
                               stride[0] // df, stride[1] // df, Ly, Lx)
        return out if vq else DiagonalGaussianDistribution(out)

    def get_first_stage_encoding(self, encoder_posterior, noise=None):
        """``ldm/diffusion/ddpm.py:795-806``: scale_factor * posterior sample (fused on the device)."""
        from ..Distribution.distribution import DiagonalGaussianDistribution
        if isinstance(encoder_posterior, DiagonalGaussianDistribution):
            return encoder_posterior.sample_scaled(self.scale_factor, noise=noise)
        if isinstance(encoder_posterior, torch.Tensor):
            return self.scale_factor * encoder_posterior
        raise NotImplementedError(f"encoder_posterior of type '{type(encoder_posterior)}' not yet implemented")

    @torch.no_grad()
    def decode_first_stage(self, z, predict_cids=False, force_not_quantize=False):
        """``ldm/diffusion/ddpm.py:1083-1156``: z / scale_factor → first-stage decode; with
        ``split_input_params['patch_distributed_vq']`` the tiled (patch) decode.  ``predict_cids``
        (``:1086-1095``): z holds codebook indices, or 4-D per-class scores whose argmax over the
        channels gives them; the codebook entries are decoded without quantising again."""
        if predict_cids:
            if z.dim() == 4:
                z = torch.argmax(z.exp(), dim=1).long()
            z = self.first_stage_model.quantize.get_codebook_entry(z, shape=None)
            z = z.permute(0, 3, 1, 2).contiguous()
        fnq = bool(predict_cids or force_not_quantize)
        sp = getattr(self, "split_input_params", None)
        if sp and sp.get("patch_distributed_vq"):
            return self._decode_tiled(z, sp, fnq)
        return _first_stage_decode(self.first_stage_model, z, 1.0 / self.scale_factor, fnq)

    # ------------------------------------------------------------------ tiled decode
    @staticmethod
    def delta_border(h, w):
        """Normalised distance of each pixel to the nearest border (0 at the border, 0.5 at the
        centre): min(y/(h-1), x/(w-1), 1-y/(h-1), 1-x/(w-1)) in fp32 — the CompVis semantics of
        ``ldm/diffusion/ddpm.py:838-859``; the reference takes its first min over dim=1 and then
        fails in torch.cat for any w > 1."""
        f32 = np.float32
        y = np.arange(h, dtype=np.int64)[:, None].astype(f32) / f32(h - 1)
        x = np.arange(w, dtype=np.int64)[None, :].astype(f32) / f32(w - 1)
        y, x = np.broadcast_to(y, (h, w)), np.broadcast_to(x, (h, w))
        lu = np.minimum(y, x)
        rd = np.minimum(f32(1.0) - y, f32(1.0) - x)
        return np.minimum(lu, rd).astype(f32)

    def get_weighting(self, h, w, Ly, Lx, sp):
        """Pixel weights [h, w] and (tie-breaker) patch weights [Ly*Lx] or None
        (``ldm/diffusion/ddpm.py:862-891``; weighting = pixel ⊗ patch, kept separable)."""
        pix = np.clip(self.delta_border(h, w), sp["clip_min_weight"], sp["clip_max_weight"]).astype(np.float32)
        lw = None
        if sp.get("tie_braker", False):
            lo = sp.get("clip_min_tie_weight", sp.get("clip_min_the_weight"))
            hi = sp.get("clip_max_tie_weight", sp.get("clip_max_the_weight"))
            lw = np.clip(self.delta_border(Ly, Lx), lo, hi).astype(np.float32).reshape(-1)
        return pix, lw

    def _decode_tiled(self, z, sp, force_not_quantize=False):
        """Patch decode (``ldm/diffusion/ddpm.py:1097-1139`` + ``get_fold_unfold`` uf branch
        ``:894-960``): latent patches of ``ks`` every ``stride`` are decoded as one batch
        (chunks of ``sp.get('max_batch', 16)`` patches·images), weighted and overlap-added at
        uf = vqf on the device (``sdk_extract_patches`` / ``sdk_fold_patches``)."""
        ks, stride, uf = tuple(sp["ks"]), tuple(sp["stride"]), int(sp["vqf"])
        B, Cz, h, w = z.shape
        ks = (min(ks[0], h), min(ks[1], w))
        stride = (min(stride[0], h), min(stride[1], w))
        Ly, Lx = (h - ks[0]) // stride[0] + 1, (w - ks[1]) // stride[1] + 1
        key = (ks, stride, uf, Ly, Lx, z.device)
        cache = getattr(self, "_tile_w", None)
        if cache is None or cache[0] != key:
            pix, lw = self.get_weighting(ks[0] * uf, ks[1] * uf, Ly, Lx, sp)
            cache = (key, torch.from_numpy(pix).to(z.device),
                     torch.from_numpy(lw).to(z.device) if lw is not None else None)
            self._tile_w = cache
        _, pix_w, l_w = cache
        patches = ops.extract_patches(z.float(), ks[0], ks[1], stride[0], stride[1])   # [L, B, C, kh, kw]
        flat = patches.view(Ly * Lx * B, Cz, ks[0], ks[1])
        chunk = int(sp.get("max_batch", 16))
        dec = [_first_stage_decode(self.first_stage_model, flat[i:i + chunk], 1.0 / self.scale_factor,
                                   force_not_quantize) for i in range(0, flat.shape[0], chunk)]
        dec = torch.cat(dec, 0) if len(dec) > 1 else dec[0]
        dec = dec.view(Ly * Lx, B, dec.shape[1], dec.shape[2], dec.shape[3])
        return ops.fold_patches(dec, pix_w, l_w, h * uf, w * uf, stride[0] * uf, stride[1] * uf, Ly, Lx)
