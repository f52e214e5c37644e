"""DPMSolverSampler — DPM-Solver++(2M) (Lu et al., "DPM-Solver++: Fast Solver for Guided Sampling of Diffusion
Probabilistic Models", the multistep second-order data-prediction solver) on ``DDIMSampler``'s timestep grid.  The
reference this package mirrors has no such class: this is an extension on ``DDIMSampler``'s schedule, scalars, CFG
context cache and q-tables.

This is NOT CompVis' ``ldm/models/diffusion/dpm_solver`` wrapper: that one runs a continuous-time ``DPM_Solver``
on its own ``time_uniform`` grid; this one is multistep order 2 on the S discrete DDIM timesteps, so an S-step run
evaluates the model at exactly the timesteps an S-step DDIM run does.

At DDIM index i, with a = ddim_alphas[i], a' = ddim_alphas_prev[i], α = √a, σ = √(1 − a), λ = ½ ln(a / (1 − a))
(α', σ', λ' from a'), h = λ' − λ and φ = expm1(−h):

    D      = (x − σ·ε) / α                                  the data prediction, DDIM's pred_x0
    x_prev = (σ'/σ)·x − α'φ·D                                first order (this is the eta = 0 DDIM step)
    x_prev = (σ'/σ)·x − α'φ(1 + 1/(2 r0))·D + α'φ/(2 r0)·D_prev        second order, r0 = h_prev / h

The three coefficients are evaluated in float64 on the host and rounded once to fp32 (``step_coefficients``); the
update is ONE fused HIP launch per step (``sdk_multistep_step``, form DPM: guidance combine, v→ε conversion, D, the
update, the store of D for the next step and, with ``mask`` / ``x0``, the known-region blend that opens the next
iteration).  First order is used at the first step, and at the last one when ``lower_order_final`` and S < 15.
One model call per step.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import ops
from .ddim import DDIMSampler
from .plms import check_mask, model_outputs, open_loop, refuse_options


class DPMSolverSampler(DDIMSampler):
    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        if ddim_eta != 0:
            raise ValueError("ddim_eta must be 0 for DPM-Solver++ (a deterministic solver)")
        super().make_schedule(ddim_num_steps, ddim_discretize=ddim_discretize, ddim_eta=ddim_eta, verbose=verbose)

    def _log_snr(self, index):
        """float64 (a, a', h = λ' − λ) at DDIM index ``index``."""
        a, ap = float(self.ddim_alphas[index]), float(self.ddim_alphas_prev[index])
        lam = lambda v: 0.5 * np.log(v / (1.0 - v))          # noqa: E731
        return a, ap, lam(ap) - lam(a)

    def step_order(self, index, lower_order_final=True):
        """1 or 2: first order at the first step (index S − 1), and at the last (index 0) when
        ``lower_order_final`` and S < 15; S is the number of timesteps of the schedule."""
        S = int(self.ddim_timesteps.shape[0])
        return 1 if index == S - 1 or (index == 0 and lower_order_final and S < 15) else 2

    def step_coefficients(self, index, prev_index=None):
        """(c_x, c_0, c_1) of the step at DDIM index ``index`` as Python floats holding fp32 values: float64 on
        the host, rounded once.  ``prev_index`` None: first order (c_1 = 0); otherwise the index of the step
        before (index + 1 in a sampling loop), whose h gives r0."""
        a, ap, h = self._log_snr(index)
        phi = np.expm1(-h)
        alpha_p = np.sqrt(ap)
        c_x = np.sqrt(1.0 - ap) / np.sqrt(1.0 - a)
        if prev_index is None:
            c_0, c_1 = -alpha_p * phi, 0.0
        else:
            r0 = self._log_snr(prev_index)[2] / h
            c_0 = -alpha_p * phi * (1.0 + 1.0 / (2.0 * r0))
            c_1 = alpha_p * phi / (2.0 * r0)
        return tuple(float(np.float32(c)) for c in (c_x, c_0, c_1))

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, x_T=None, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, mask=None, x0=None, callback=None, img_callback=None, log_every_t=100,
               lower_order_final=True, verbose=True, **kwargs):
        """Returns (samples, intermediates), ``intermediates`` as ``DDIMSampler``'s.  Multistep order 2 on the
        DDIM grid, not CompVis' continuous-time wrapper (module docstring).  ``kwargs``: ``q_noise_fn(i, shape)``
        (q_sample noise of the mask blend); ``eta`` must be 0; ``quantize_x0``, ``noise_dropout`` and
        ``score_corrector`` are refused; the rest of ``DDIMSampler.sample``'s keywords has nothing to act on."""
        refuse_options("DPMSolverSampler", self.model, quantize_x0=kwargs.get("quantize_x0", False),
                       noise_dropout=kwargs.get("noise_dropout", 0.) > 0,
                       score_corrector=kwargs.get("score_corrector") is not None)
        check_mask(mask, x0)
        if conditioning is not None:
            ctmp = conditioning[list(conditioning.keys())[0]] if isinstance(conditioning, dict) else conditioning
            while isinstance(ctmp, list):
                ctmp = ctmp[0]
            cbs = ctmp.shape[0]
            if cbs != batch_size:
                print(f"Warning: Got {cbs} conditionings but batch-size is {batch_size}")
        self.make_schedule(ddim_num_steps=S, ddim_eta=kwargs.get("eta", 0.), verbose=verbose)
        C, H, W = shape
        size = (batch_size, C, H, W)
        if verbose:
            print(f"Data shape for DPM-Solver++ sampling is {size}")
        return self.dpm_sampling(conditioning, size, x_T=x_T, callback=callback, mask=mask, x0=x0,
                                 img_callback=img_callback, log_every_t=log_every_t,
                                 unconditional_guidance_scale=unconditional_guidance_scale,
                                 unconditional_conditioning=unconditional_conditioning,
                                 lower_order_final=lower_order_final, q_noise_fn=kwargs.get("q_noise_fn"))

    @torch.no_grad()
    def dpm_sampling(self, cond, shape, x_T=None, callback=None, mask=None, x0=None, img_callback=None,
                     log_every_t=100, unconditional_guidance_scale=1., unconditional_conditioning=None,
                     lower_order_final=True, q_noise_fn=None):
        """The loop over ``np.flip(ddim_timesteps)`` of the schedule ``make_schedule`` built (as
        ``DDIMSampler.ddim_sampling``): the number of steps is the number of timesteps of that grid, which the
        uniform discretisation makes larger than the S asked for when S does not divide the model's steps.  With a
        mask the first blend is ``sdk_masked_q_sample``; every later one is written by the step before it."""
        refuse_options("DPMSolverSampler", self.model)
        check_mask(mask, x0)
        ops.need_gpu_sampler("DPM-Solver++ sampling", self.model.device)
        b = shape[0]
        time_range = [int(v) for v in np.flip(self.ddim_timesteps)]
        total_steps = len(time_range)
        img, x_in, blend_of = open_loop(self, shape, x_T, mask, x0, q_noise_fn, time_range)
        intermediates = {"x_inter": [img], "pred_x0": [img]}
        ring = [torch.empty_like(img) for _ in range(2)]
        old_d = None
        for i, step in enumerate(time_range):
            index = total_steps - i - 1
            ts = torch.full((b,), step, device=img.device, dtype=torch.long)
            blend = blend_of(i) if blend_of is not None and i + 1 < total_steps else None
            second = old_d is not None and self.step_order(index, lower_order_final) == 2
            outs = self.p_sample_dpm(x_in, cond, ts, index=index, prev_index=index + 1 if second else None,
                                     unconditional_guidance_scale=unconditional_guidance_scale,
                                     unconditional_conditioning=unconditional_conditioning,
                                     old_d=old_d if second else None, blend=blend, hist_out=ring[i % 2])
            img, pred_x0, old_d = outs[0], outs[1], outs[2]
            x_in = outs[3] if blend is not None else img
            if callback:
                callback(i)
            if img_callback:
                img_callback(pred_x0, i)
            if index % log_every_t == 0 or index == total_steps - 1:
                intermediates["x_inter"].append(img)
                intermediates["pred_x0"].append(pred_x0)
        return img, intermediates

    @torch.no_grad()
    def p_sample_dpm(self, x, c, t, index, prev_index=None, unconditional_guidance_scale=1.,
                     unconditional_conditioning=None, old_d=None, blend=None, hist_out=None):
        """One step: returns (x_prev, pred_x0, d), ``d`` the data prediction the next step takes as ``old_d``
        (written to ``hist_out`` when given), and the blended next input fourth with ``blend`` (the ``blend_*``
        keywords of ``ops.multistep_step``).  Second order needs both ``prev_index`` and ``old_d``."""
        refuse_options("DPMSolverSampler", self.model)
        ops.need_gpu_sampler("DPM-Solver++ sampling", x.device)
        if (prev_index is None) != (old_d is None):
            raise ValueError("sd_amd.DPMSolverSampler: second order needs prev_index and old_d, first order neither")
        sc = self.step_scalars(index)
        v = (sc["v_sqrt_a"], sc["v_sqrt_1ma"]) if getattr(self.model, "parameterization", "eps") == "v" else None
        x = x.float().contiguous()
        d = hist_out if hist_out is not None else torch.empty_like(x)
        e_c, e_u = model_outputs(self, x, c, t, unconditional_guidance_scale, unconditional_conditioning)
        outs = ops.multistep_step(x, e_c, sc, "dpm", history=[] if old_d is None else [old_d],
                                  coefs=self.step_coefficients(index, prev_index), e_uncond=e_u,
                                  guidance=unconditional_guidance_scale, v_param=v, hist_out=d, **(blend or {}))
        return (outs[0], outs[1], d) + tuple(outs[2:])
