"""Restatement of the multistep samplers (PLMS, DPM-Solver++ 2M on the DDIM grid) for the tests, written from the
formulas below and never from the product code: numpy, one rounded operation per
product / sum / quotient, in the dtype of ``x`` (fp32 for the bit-exact comparisons, float64 for the accuracy
scenario).  The schedule tables are the oracle's (``oracle/schedule.py``), which the older tests pin to the
reference bit for bit.

e  = e_u + g (e_c − e_u), then with v-prediction e = √a·v + √(1 − a)·x
PLMS      e' = e | (3e − h1)/2 | ((23e − 16h1) + 5h2)/12 | (((55e − 59h1) + 37h2) − 9h3)/24 | warm-up (e + e_next)/2
          pred_x0 = (x − √(1 − a)·e')/√a,  x_prev = (√a'·pred_x0 + √(1 − a')·e') + 0
DPM++ 2M  D = (x − √(1 − a)·e)/√a,  x_prev = c_x·x + c_0·D (+ c_1·D_prev)
          λ = ½ ln(a/(1 − a)), h = λ' − λ, φ = expm1(−h), c_x = σ'/σ, c_0 = −α'φ(1 + 1/(2 r0)), c_1 = α'φ/(2 r0),
          r0 = h_prev/h; first order: c_0 = −α'φ, no c_1.
"""
import numpy as np

from oracle import schedule as sch

F32, F64 = np.float32, np.float64
GUIDANCE = 2.5
KERNEL_SHAPES = [(2, 3, 5, 5), (1, 3, 5, 5), (2, 4, 8, 8)]     # n = 150 (a tail of 2), 75 (a tail of 3), 512 (aligned)
PLMS_STEPS = (1, 2, 3, 4, 5, 8)          # history shorter than, equal to and longer than the ring of three
DPM_STEPS = (1, 2, 3, 14, 15)            # 14 / 15: the lower_order_final threshold
COEF_STEPS = (1, 2, 3, 14, 15, 20)
LOOP_SHAPE = (2, 4, 8, 8)

# ---- the accuracy scenario: data N(0, s^2), the ideal model, the exact solution of the probability-flow ODE
SCENARIO_S = 2.0
SCENARIO_XT = (1.3, -0.7, 0.2, 2.1)
# max |x − exact| over SCENARIO_XT in float64 (to four digits): S -> (DDIM, PLMS, DPM++ 2M)
SCENARIO_ERRORS = {10: (3.879e-1, 6.295e-3, 1.677e-1), 20: (2.072e-1, 1.217e-3, 5.396e-2)}


def randn(seed, *shape):
    return np.random.Generator(np.random.PCG64(seed)).standard_normal(shape, dtype=F32)


NUM_TIMESTEPS = 1000


def discretize(S):
    """The DDIM discretisation that gives exactly S timesteps on the 1000-step schedule: "uniform" where it does
    (S = 1, 2, 4, 5, 8, 10, 20 ...).  Where it does not (S = 3 steps past the schedule's end, as the reference;
    S = 14 / 15 give 15 / 16 timesteps) "quad", which gives S timesteps for every S > 1."""
    ts = range(0, NUM_TIMESTEPS, NUM_TIMESTEPS // S)
    return "uniform" if len(ts) == S and ts[-1] + 1 < NUM_TIMESTEPS else "quad"


def tables(S):
    """The SD schedule (linear in sqrt(beta), 0.00085-0.012, 1000 steps) and its S-step DDIM tables, eta = 0."""
    schedule = sch.register_schedule()
    assert schedule["num_timesteps"] == NUM_TIMESTEPS
    ts = sch.make_ddim_timesteps(discretize(S), S, NUM_TIMESTEPS)
    assert len(ts) == S and len(set(ts.tolist())) == S
    out = sch.make_ddim_sampling_parameters(schedule["alphas_cumprod"], ts, 0.0)
    out["schedule"] = schedule
    return out


def time_range(tab):
    return [int(t) for t in np.flip(tab["ddim_timesteps"])]


def scalars(tab, index, T=F32):
    """The scalars of one step in dtype ``T``: fp32 as the oracle's ``ddim_step_scalars`` (the fp32 table entries
    and the fp32 roots torch forms from them) plus the v-conversion pair; float64 from the same table entries."""
    if T is F32:
        sc = dict(sch.ddim_step_scalars(tab, index))
        a = sc["a_t"]
        sc["v_sqrt_a"], sc["v_sqrt_1ma"] = np.sqrt(a, dtype=F32), np.sqrt(F32(F32(1.0) - a), dtype=F32)
        return sc
    a, ap = F64(tab["ddim_alphas"][index]), F64(tab["ddim_alphas_prev"][index])
    return dict(a_t=a, a_prev=ap, sigma=F64(0), sqrt_one_minus_at=np.sqrt(1.0 - a), sqrt_at=np.sqrt(a),
                dir_coef=np.sqrt(1.0 - ap), sqrt_a_prev=np.sqrt(ap), v_sqrt_a=np.sqrt(a), v_sqrt_1ma=np.sqrt(1.0 - a))


def guided_eps(x, e, eu=None, g=1.0, v=None):
    T = x.dtype.type
    if eu is not None:
        d = e - eu
        e = eu + T(g) * d
    if v is not None:
        e = T(v[0]) * e + T(v[1]) * x
    return e


def plms_eprime(e, hist, e_next=None):
    """``hist``: the guided ε of the previous steps, most recent first."""
    T = e.dtype.type
    if e_next is not None:
        return (e + e_next) / T(2)
    if len(hist) == 0:
        return e
    if len(hist) == 1:
        return (T(3) * e - hist[0]) / T(2)
    if len(hist) == 2:
        return ((T(23) * e - T(16) * hist[0]) + T(5) * hist[1]) / T(12)
    return (((T(55) * e - T(59) * hist[0]) + T(37) * hist[1]) - T(9) * hist[2]) / T(24)


def ddim0(x, e, sc):
    """The DDIM update at sigma = 0 (its noise term is +0): (x_prev, pred_x0)."""
    T = x.dtype.type
    p0 = (x - T(sc["sqrt_one_minus_at"]) * e) / T(sc["sqrt_at"])
    return (T(sc["sqrt_a_prev"]) * p0 + T(sc["dir_coef"]) * e) + T(0), p0


def dpm_step(x, e, sc, coefs, d_prev=None):
    """(x_prev, D); ``coefs`` already in the dtype of x."""
    T = x.dtype.type
    d = (x - T(sc["sqrt_one_minus_at"]) * e) / T(sc["sqrt_at"])
    xp = T(coefs[0]) * x + T(coefs[1]) * d
    if d_prev is not None:
        xp = xp + T(coefs[2]) * d_prev
    return xp, d


def dpm_order(S, index, lower_order_final=True):
    return 1 if index == S - 1 or (index == 0 and lower_order_final and S < 15) else 2


def dpm_coefficients64(tab, index, prev_index=None):
    """(c_x, c_0, c_1) in float64 from the fp32 table entries; ``prev_index`` None: first order."""
    def alpha_sigma_lambda(a):
        a = F64(a)
        return np.sqrt(a), np.sqrt(1.0 - a), 0.5 * np.log(a / (1.0 - a))

    def h_of(i):
        return alpha_sigma_lambda(tab["ddim_alphas_prev"][i])[2] - alpha_sigma_lambda(tab["ddim_alphas"][i])[2]

    _, sigma, _ = alpha_sigma_lambda(tab["ddim_alphas"][index])
    alpha_p, sigma_p, _ = alpha_sigma_lambda(tab["ddim_alphas_prev"][index])
    h = h_of(index)
    phi = np.expm1(-h)
    if prev_index is None:
        return sigma_p / sigma, -alpha_p * phi, F64(0)
    r0 = h_of(prev_index) / h
    return sigma_p / sigma, -alpha_p * phi * (1.0 + 1.0 / (2.0 * r0)), alpha_p * phi / (2.0 * r0)


def blend(x0, qn, mask, img, tab, t):
    """The known-region blend at timestep ``t``: (√acp·x0 + √(1 − acp)·noise)·mask + (1 − mask)·img."""
    T = img.dtype.type
    sa, s1m = tab["schedule"]["sqrt_alphas_cumprod"][t], tab["schedule"]["sqrt_one_minus_alphas_cumprod"][t]
    return (T(sa) * x0 + T(s1m) * qn) * mask + (T(1) - mask) * img


def blend_mask(kind, binary, shape, seed=8100):
    b, c, h, w = shape
    ms = {"b1hw": (b, 1, h, w), "11hw": (1, 1, h, w), "bchw": (b, c, h, w)}[kind]
    u = np.random.Generator(np.random.PCG64(seed + len(kind) + 17 * sum(ms))).random(ms, dtype=F32)
    return (u > 0.5).astype(F32) if binary else u


# ---------------------------------------------------------------- loops
def run_loop(kind, model, xT, S, g=None, v=False, mask=None, x0=None, qn=None, lower_order_final=True):
    """``kind`` "ddim" | "plms" | "dpm" in the dtype of ``xT``.  ``model(x, t) -> (out, out_uncond or None)``; ``g``
    None: unguided (the unconditional output is not asked for).  ``qn[i]``: the q-noise of the blend that opens
    loop iteration i.  Returns dict(calls=[(x, t)], x, x_inter, pred_x0): every model call's input, the result,
    and the unblended x_prev / pred_x0 of every step."""
    T = xT.dtype.type
    tab = tables(S)
    tr = time_range(tab)
    calls, x_inter, pred = [], [], []

    def ev(x, t, sc):
        calls.append((x.copy(), t))
        e, eu = model(x, t)
        return guided_eps(x, e, eu if g is not None else None, g, (sc["v_sqrt_a"], sc["v_sqrt_1ma"]) if v else None)

    x_in = xT if mask is None else blend(x0, qn[0], mask, xT, tab, tr[0])
    hist, d_prev = [], None
    for i, t in enumerate(tr):
        index = S - 1 - i
        sc = scalars(tab, index, T)
        e = ev(x_in, t, sc)
        if kind == "ddim":
            img, p0 = ddim0(x_in, e, sc)
        elif kind == "plms":
            if i == 0:
                x_tent, _ = ddim0(x_in, e, sc)
                i_next = min(i + 1, S - 1)
                e_next = ev(x_tent, tr[i_next], scalars(tab, S - 1 - i_next, T))
                ep = plms_eprime(e, [], e_next)
            else:
                ep = plms_eprime(e, hist)
            img, p0 = ddim0(x_in, ep, sc)
            hist = [e] + hist[:2]
        else:
            second = dpm_order(S, index, lower_order_final) == 2
            coefs = [T(c) for c in dpm_coefficients64(tab, index, index + 1 if second else None)]
            img, p0 = dpm_step(x_in, e, sc, coefs, d_prev if second else None)
            d_prev = p0
        x_inter.append(img)
        pred.append(p0)
        x_in = img if mask is None or i + 1 >= S else blend(x0, qn[i + 1], mask, img, tab, tr[i + 1])
    return dict(calls=calls, x=x_inter[-1], x_inter=x_inter, pred_x0=pred)


def stub_bias(seed=8200):
    """b[8, *LOOP_SHAPE] and the unconditional one of the loops' stand-in model e = 0.25·x + b[t % 8]."""
    return randn(seed, 8, *LOOP_SHAPE) * F32(0.5), randn(seed + 1, 8, *LOOP_SHAPE) * F32(0.5)


def stub_model(b, bu):
    """0.25·x is exact, so each output is one rounded add: a wrong x or t reaching the model shows."""
    return lambda x, t: (F32(0.25) * x + b[t % 8], F32(0.25) * x + bu[t % 8])


def loop_inputs(seed=8300):
    return dict(xT=randn(seed, *LOOP_SHAPE), x0=randn(seed + 1, *LOOP_SHAPE), qn=randn(seed + 2, 16, *LOOP_SHAPE))


# ---------------------------------------------------------------- accuracy scenario
def scenario_variance(a):
    return a * SCENARIO_S ** 2 + 1.0 - a


def scenario_model64(tab):
    """The ideal model of N(0, s²) data: ε*(x, t) = σ_t·x / (a_t s² + 1 − a_t)."""
    ac = tab["schedule"]["alphas_cumprod"].astype(F64)
    return lambda x, t: (np.sqrt(1.0 - ac[t]) * x / scenario_variance(ac[t]), None)


def scenario_exact(S):
    tab = tables(S)
    ac = tab["schedule"]["alphas_cumprod"].astype(F64)
    xT = np.asarray(SCENARIO_XT, dtype=F64)
    return xT * np.sqrt(scenario_variance(ac[0]) / scenario_variance(ac[time_range(tab)[0]]))


def scenario_errors64(S):
    """(DDIM, PLMS, DPM++ 2M) max-abs errors of the float64 restatement."""
    tab = tables(S)
    xT = np.asarray(SCENARIO_XT, dtype=F64)
    exact = scenario_exact(S)
    return tuple(float(np.abs(run_loop(k, scenario_model64(tab), xT, S)["x"] - exact).max())
                 for k in ("ddim", "plms", "dpm"))


# ---------------------------------------------------------------- tiny real model
MODEL_STEPS = 4
MODEL_SCALE = 5.0
# (latent rel-L2, image rel-L2) of the sample and of decode_first_stage(sample) against the fp32 CPU loop of this
# restatement driving oracle/unet_ref.py and oracle/vae_ref.py: at most 3.5x the errors measured on MI355X
# (profiles/multistep_parity_errors.txt; DDIM at the same S: 2.619e-3 / 2.590e-3)
PARITY_LIMITS = {
    "plms": (7.9e-3, 7.8e-3),   # measured 2.285e-3 / 2.254e-3
    "dpm": (8.6e-3, 8.6e-3),   # measured 2.478e-3 / 2.485e-3
}
