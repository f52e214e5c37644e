"""PLMSSampler — pseudo linear multistep sampling (Liu et al., "Pseudo Numerical Methods for Diffusion Models on
Manifolds") with the names, signatures and arithmetic of CompVis' ``ldm/models/diffusion/plms.py``.  The reference
this package mirrors has no such class: this is an extension on ``DDIMSampler``'s schedule, scalars, CFG context
cache and q-tables.

Per step the model call and ONE fused HIP launch (``sdk_multistep_step``): guidance combine, v→ε conversion, the
Adams-Bashforth combination of ε with the last one to three guided ε (``e_t_prime``), the eta = 0 DDIM update
with the combined ε (``get_x_prev_and_pred_x0``), the store of the guided ε into the history and, with ``mask`` / ``x0``, the
known-region blend that opens the next iteration.  The history is a ring of three preallocated buffers; the launch
overwrites the oldest entry while it reads it.  The first step has no history: a tentative ``x_prev`` from ε alone,
a second model call at ``(x_prev, t_next)``, then ``e' = (e_t + e_t_next) / 2`` from the original ``x`` — S + 1
model calls per run.

What differs from CompVis: fp32 scalars on the host as ``DDIMSampler.step_scalars`` (CompVis holds the same fp32
tables on the device); every product, sum and quotient rounded on its own in the order of the formulas above;
``quantize_x0``, ``noise_dropout``, ``score_corrector`` and original-steps sampling are refused (NotImplementedError)
instead of implemented; ``parameterization == "v"`` and the ``q_noise_fn(i, shape)`` hook are added.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import ops
from .ddim import DDIMSampler


def refuse_options(name, model, **options):
    """The options the multistep samplers do not implement: NotImplementedError naming the option."""
    for option, on in options.items():
        if on:
            raise NotImplementedError(f"sd_amd.{name}: {option} is not implemented (DDIMSampler has it)")
    if getattr(model, "parameterization", "eps") == "x0":
        raise NotImplementedError(f"sd_amd.{name}: x0-parameterised models are not implemented (the ancestral "
                                  "sampler, LatentDiffusion.p_sample_loop, takes x0 models)")


def model_outputs(sampler, x, c, t, scale, uc):
    """(e, e_uncond or None): the model at (x, t), both halves of classifier-free guidance in one batched call
    (``ddim.py:171-177``), fp32 and contiguous."""
    if uc is None or scale == 1.:
        return sampler.model.apply_model(x, t, c).float().contiguous(), None
    b = x.shape[0]
    both = sampler.model.apply_model(torch.cat([x] * 2), torch.cat([t] * 2), sampler._cfg_context(uc, c))
    return both[b:].float().contiguous(), both[:b].float().contiguous()


def open_loop(sampler, shape, x_T, mask, x0, q_noise_fn, time_range):
    """The start of a sampling loop: (img, x_in, blend_of).  ``img`` is x_T or a draw; with a mask ``x_in``
    is its first known-region blend (``sdk_masked_q_sample``) and ``blend_of(i)`` gives the blend keywords of the
    step at loop counter ``i``; otherwise ``x_in`` is ``img`` and ``blend_of`` None."""
    device = sampler.model.device
    img = torch.randn(shape, device=device) if x_T is None else x_T.to(device=device, dtype=torch.float32)
    img = img.contiguous()
    if mask is None:
        return img, img, None
    mask = mask.to(device=device, dtype=torch.float32).contiguous()
    x0 = x0.to(device=device, dtype=torch.float32).contiguous()
    sa_tab, s1m_tab = sampler._q_tables()
    q_noise = lambda k: (q_noise_fn(k, img.shape) if q_noise_fn is not None else          # noqa: E731
                         torch.randn_like(x0)).to(device=device, dtype=torch.float32)
    x_in = ops.masked_q_sample(x0, q_noise(0), mask, img, time_range[0], sa_tab, s1m_tab)

    def blend_of(i):
        """The ``blend_*`` keywords of the step at loop counter ``i``: the blend at the NEXT timestep."""
        nxt = time_range[i + 1]
        return dict(blend_x0=x0, blend_noise=q_noise(i + 1), blend_mask=mask, blend_sqrt_acp=float(sa_tab[nxt]),
                    blend_sqrt_1m_acp=float(s1m_tab[nxt]))

    return img, x_in, blend_of


def check_mask(mask, x0):
    if mask is not None:
        if x0 is None:
            raise ValueError("sd_amd: mask needs x0 (the known region's latent)")
        if x0.shape[2:] != mask.shape[2:]:
            raise ValueError(f"sd_amd: mask {tuple(mask.shape)} and x0 {tuple(x0.shape)} differ in spatial size")


class PLMSSampler(DDIMSampler):
    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        if ddim_eta != 0:
            raise ValueError("ddim_eta must be 0 for PLMS")
        super().make_schedule(ddim_num_steps, ddim_discretize=ddim_discretize, ddim_eta=ddim_eta, verbose=verbose)

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, q_noise_fn=None, **kwargs):
        """CompVis' ``PLMSSampler.sample``; ``temperature`` has nothing to scale (eta = 0)."""
        if conditioning is not None:
            ctmp = conditioning[list(conditioning.keys())[0]] if isinstance(conditioning, dict) else conditioning
            while isinstance(ctmp, list):
                ctmp = ctmp[0]
            cbs = ctmp.shape[0]
            if cbs != batch_size:
                print(f"Warning: Got {cbs} conditionings but batch-size is {batch_size}")
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        C, H, W = shape
        size = (batch_size, C, H, W)
        if verbose:
            print(f"Data shape for PLMS sampling is {size}")
        return self.plms_sampling(conditioning, size, callback=callback, img_callback=img_callback,
                                  quantize_denoised=quantize_x0, mask=mask, x0=x0, noise_dropout=noise_dropout,
                                  temperature=temperature, score_corrector=score_corrector,
                                  corrector_kwargs=corrector_kwargs, x_T=x_T, log_every_t=log_every_t,
                                  unconditional_guidance_scale=unconditional_guidance_scale,
                                  unconditional_conditioning=unconditional_conditioning, q_noise_fn=q_noise_fn)

    @torch.no_grad()
    def plms_sampling(self, cond, shape, x_T=None, ddim_use_original_steps=False, callback=None, timesteps=None,
                      quantize_denoised=False, mask=None, x0=None, img_callback=None, log_every_t=100,
                      temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None,
                      unconditional_guidance_scale=1., unconditional_conditioning=None, q_noise_fn=None):
        """CompVis' ``plms_sampling``.  Extension: the hook ``q_noise_fn(i, shape)`` (q_sample noise of the mask blend,
        ``i`` the loop counter).  With a mask the first blend is ``sdk_masked_q_sample``; every later one is
        written by the step before it (``x_inter`` and the result stay unblended, as in ``DDIMSampler``)."""
        refuse_options("PLMSSampler", self.model, quantize_x0=quantize_denoised, noise_dropout=noise_dropout > 0,
                       score_corrector=score_corrector is not None, ddim_use_original_steps=ddim_use_original_steps)
        check_mask(mask, x0)
        ops.need_gpu_sampler("PLMS sampling", self.model.device)
        b = shape[0]
        ts_all = self.ddim_timesteps if timesteps is None else \
            self.ddim_timesteps[:int(min(timesteps / self.ddim_timesteps.shape[0], 1) * self.ddim_timesteps.shape[0]) - 1]
        time_range = [int(v) for v in np.flip(ts_all)]
        total_steps = ts_all.shape[0]
        img, x_in, blend_of = open_loop(self, shape, x_T, mask, x0, q_noise_fn, time_range)
        device = img.device
        intermediates = {"x_inter": [img], "pred_x0": [img]}
        ring = [torch.empty_like(img) for _ in range(3)]
        old_eps = []
        for i, step in enumerate(time_range):
            index = total_steps - i - 1
            ts = torch.full((b,), step, device=device, dtype=torch.long)
            ts_next = torch.full((b,), time_range[min(i + 1, total_steps - 1)], device=device, dtype=torch.long)
            blend = blend_of(i) if blend_of is not None and i + 1 < total_steps else None
            # the ring's free buffer, or its oldest entry (old_eps[0]: read and overwritten by the same launch)
            free = [r for r in ring if all(r is not o for o in old_eps)]
            outs = self.p_sample_plms(x_in, cond, ts, index=index,
                                      unconditional_guidance_scale=unconditional_guidance_scale,
                                      unconditional_conditioning=unconditional_conditioning, old_eps=old_eps,
                                      t_next=ts_next, blend=blend, hist_out=free[0] if free else old_eps[0])
            img, pred_x0, e_t = outs[0], outs[1], outs[2]
            x_in = outs[3] if blend is not None else img
            old_eps.append(e_t)
            if len(old_eps) >= 4:
                old_eps.pop(0)
            if callback:
                callback(i)
            if img_callback:
                img_callback(pred_x0, i)
            if index % log_every_t == 0 or index == total_steps - 1:
                intermediates["x_inter"].append(img)
                intermediates["pred_x0"].append(pred_x0)
        return img, intermediates

    @torch.no_grad()
    def p_sample_plms(self, x, c, t, index, repeat_noise=False, use_original_steps=False, quantize_denoised=False,
                      temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None,
                      unconditional_guidance_scale=1., unconditional_conditioning=None, old_eps=None, t_next=None,
                      blend=None, hist_out=None):
        """CompVis' ``p_sample_plms``: returns (x_prev, pred_x0, e_t), ``e_t`` the guided ε of this step (what the next
        steps take as history; ``old_eps`` is oldest first, as CompVis keeps it).  Extensions: ``blend`` (the
        ``blend_*`` keywords of ``ops.multistep_step``: the next iteration's known-region blend, returned fourth)
        and ``hist_out`` (the buffer ``e_t`` is written to; it may be ``old_eps[-3]``)."""
        refuse_options("PLMSSampler", self.model, quantize_x0=quantize_denoised, noise_dropout=noise_dropout > 0,
                       score_corrector=score_corrector is not None, use_original_steps=use_original_steps)
        ops.need_gpu_sampler("PLMS sampling", x.device)
        is_v = getattr(self.model, "parameterization", "eps") == "v"
        sc = self.step_scalars(index)
        v_of = lambda s: (s["v_sqrt_a"], s["v_sqrt_1ma"]) if is_v else None           # noqa: E731
        g, uc = unconditional_guidance_scale, unconditional_conditioning
        hist = list(old_eps or [])[::-1][:3]                  # most recent first
        x = x.float().contiguous()
        e_t = hist_out if hist_out is not None else torch.empty_like(x)
        e_c, e_u = model_outputs(self, x, c, t, g, uc)
        if hist:
            outs = ops.multistep_step(x, e_c, sc, "plms", history=hist, e_uncond=e_u, guidance=g, v_param=v_of(sc),
                                      hist_out=e_t, **(blend or {}))
            return (outs[0], outs[1], e_t) + tuple(outs[2:])
        # no history yet (CompVis' ``len(old_eps) == 0`` branch).  A tentative x_prev from e_t alone, the model again at (x_prev, t_next),
        # then the update from the original x with the mean of the two ε
        if t_next is None:
            raise ValueError("sd_amd.PLMSSampler: the first step (no old_eps) needs t_next")
        x_tent, _ = ops.multistep_step(x, e_c, sc, "plms", e_uncond=e_u, guidance=g, v_param=v_of(sc), hist_out=e_t)
        n_c, n_u = model_outputs(self, x_tent, c, t_next, g, uc)
        if is_v:
            # the second output becomes ε with t_next's scalars and the tentative x_prev (its x_prev is not used)
            e_next = torch.empty_like(x)
            ops.multistep_step(x_tent, n_c, self.step_scalars(max(index - 1, 0)), "plms", e_uncond=n_u, guidance=g,
                               v_param=v_of(self.step_scalars(max(index - 1, 0))), hist_out=e_next)
        elif n_u is not None:
            e_next = ops.cfg_combine(n_u, n_c, g)
        else:
            e_next = n_c
        outs = ops.multistep_step(x, e_t, sc, "plms_warmup", e_next=e_next, **(blend or {}))
        return (outs[0], outs[1], e_t) + tuple(outs[2:])
