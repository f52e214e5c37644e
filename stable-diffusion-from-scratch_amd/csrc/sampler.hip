// Sampler-side elementwise kernels (HBM-bound, fp32) and layout glue, plus the
// library's error/introspection entry points.
//
// The DDIM / DDPM updates are compiled with floating-point contraction OFF
// (see the pragma) so each a*b+c is two correctly-rounded operations, exactly
// as torch's CPU kernels evaluate the reference expression; fed the same
// inputs the result is bit-identical to the oracle.
#include <cmath>
#include <cstdio>

#include "common.h"

#pragma clang fp contract(off)

namespace sdk {

static thread_local std::string g_last_error;

void set_error(const std::string& msg) { g_last_error = msg; }

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(SDK_EHIP, std::string(what) + ": " + hipGetErrorString(e));
  return SDK_OK;
}

namespace {

// e = e_u + g (e_c - e_u)  (ddim.py:178): the two operations of the fused combine and of sdk_cfg_combine
__device__ __forceinline__ float cfg_combine_elem(float u, float e, float g) {
  const float d = e - u;
  return u + g * d;
}

// keep (0 / 1, one byte per element) times fp32(1 / (1 - p)): the factor F.dropout multiplies by
__device__ __forceinline__ float dropout_factor(unsigned char keep, float drop_scale) {
  return (float)keep * drop_scale;
}

// img = (sa x0 + s1m noise) mask + (1 - mask) img  (ldm/diffusion/ddpm.py:1783-1784), the mask read by
// index: mask_mode 0 [B,1,H,W], 1 [1,1,H,W], 2 [B,C,H,W]
__device__ __forceinline__ float masked_q_elem(const sdk_masked_q_args& a, int64_t i, float x0, float nz, float im) {
  int64_t mi = i;
  if (a.mask_mode == 0) mi = (i / a.per_sample) * a.hw + i % a.hw;
  else if (a.mask_mode == 1) mi = i % a.hw;
  const float mk = a.mask[mi];
  const float t0 = a.sqrt_acp * x0;
  const float t1 = a.sqrt_1m_acp * nz;
  const float q = t0 + t1;
  const float t2 = q * mk;
  const float om = 1.f - mk;
  const float t3 = om * im;
  return t2 + t3;
}

// One element of p_sample_ddim (ddim.py:171-204).  e: the model output (ε, or v with v_param); u: the
// unconditional output (read when e_uncond); p0: pred_x0, an INPUT with pred_x0_in (the quantize_denoised
// path quantises it between the two halves) and otherwise computed here.  Returns x_prev.
__device__ __forceinline__ float ddim_elem(const sdk_ddim_ex_args& ex, float x, float e, float u, float nz,
                                           float kf, float& p0) {
  const sdk_ddim_args& a = ex.step;
  if (a.e_uncond) e = cfg_combine_elem(u, e, a.guidance);
  if (a.v_param) {
    const float t0 = a.v_sqrt_a * e;
    const float t1 = a.v_sqrt_1ma * x;
    e = t0 + t1;
  }
  if (!ex.pred_x0_in) {
    const float t1 = a.sqrt_one_minus_at * e;
    const float t2 = x - t1;
    p0 = t2 / a.sqrt_at;
  }
  const float dir = a.dir_coef * e;
  const float t3 = a.sqrt_a_prev * p0;
  const float t4 = t3 + dir;
  float nn = (a.sigma * nz) * a.temperature;
  if (ex.keep) nn = nn * kf;
  return t4 + nn;
}

// n4 16-byte groups (0 when a pointer is not aligned for them), then the scalar tail [4 n4, n).  With
// blend.mask the next iteration's known-region blend (ddim.py:146-147) of x_prev is written to blend.out.
__global__ void __launch_bounds__(256) ddim_step_kernel(sdk_ddim_ex_args ex, int64_t n4) {
  const sdk_ddim_args& a = ex.step;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const bool need_x = !ex.pred_x0_in || a.v_param, blend = ex.blend.mask != nullptr;
  for (int64_t i = tid; i < n4; i += stride) {
    const f4 z = {0.f, 0.f, 0.f, 0.f};
    f4 x = z, u = z, nz = z, p0 = z, kf = z, xp;
    if (need_x) x = reinterpret_cast<const f4*>(a.x)[i];
    const f4 e = reinterpret_cast<const f4*>(a.e)[i];
    if (a.e_uncond) u = reinterpret_cast<const f4*>(a.e_uncond)[i];
    if (a.noise) nz = reinterpret_cast<const f4*>(a.noise)[i];
    if (ex.pred_x0_in) p0 = reinterpret_cast<const f4*>(a.pred_x0)[i];
    if (ex.keep) {
      const uchar4 k = reinterpret_cast<const uchar4*>(ex.keep)[i];
      kf[0] = dropout_factor(k.x, ex.drop_scale), kf[1] = dropout_factor(k.y, ex.drop_scale);
      kf[2] = dropout_factor(k.z, ex.drop_scale), kf[3] = dropout_factor(k.w, ex.drop_scale);
    }
    for (int j = 0; j < 4; ++j) {
      float p = p0[j];
      xp[j] = ddim_elem(ex, x[j], e[j], u[j], nz[j], kf[j], p);
      p0[j] = p;
    }
    reinterpret_cast<f4*>(a.x_prev)[i] = xp;
    if (a.pred_x0 && !ex.pred_x0_in) reinterpret_cast<f4*>(a.pred_x0)[i] = p0;
    if (blend) {
      const f4 b0 = reinterpret_cast<const f4*>(ex.blend.x0)[i];
      const f4 bn = reinterpret_cast<const f4*>(ex.blend.noise)[i];
      f4 o;
      for (int j = 0; j < 4; ++j) o[j] = masked_q_elem(ex.blend, 4 * i + j, b0[j], bn[j], xp[j]);
      reinterpret_cast<f4*>(ex.blend.out)[i] = o;
    }
  }
  for (int64_t i = 4 * n4 + tid; i < a.n; i += stride) {
    float p0 = ex.pred_x0_in ? a.pred_x0[i] : 0.f;
    const float kf = ex.keep ? dropout_factor(ex.keep[i], ex.drop_scale) : 0.f;
    const float xp = ddim_elem(ex, need_x ? a.x[i] : 0.f, a.e[i], a.e_uncond ? a.e_uncond[i] : 0.f,
                               a.noise ? a.noise[i] : 0.f, kf, p0);
    a.x_prev[i] = xp;
    if (a.pred_x0 && !ex.pred_x0_in) a.pred_x0[i] = p0;
    if (blend) ex.blend.out[i] = masked_q_elem(ex.blend, i, ex.blend.x0[i], ex.blend.noise[i], xp);
  }
}

// One element of the multistep update (sdk_multistep_step).  e / u: the model output and the unconditional one;
// h1..h3: the history (PLMS: earlier guided ε, DPM: the previous data prediction in h1); en: the warm-up form's
// second ε.  p0 = pred_x0, ho = the value the history receives.  Returns x_prev.
__device__ __forceinline__ float multistep_elem(const sdk_multistep_args& m, float x, float e, float u, float h1,
                                                float h2, float h3, float en, float& p0, float& ho) {
  const sdk_ddim_args& a = m.step;
  if (a.e_uncond) e = cfg_combine_elem(u, e, a.guidance);
  if (a.v_param) {
    const float t0 = a.v_sqrt_a * e;
    const float t1 = a.v_sqrt_1ma * x;
    e = t0 + t1;
  }
  if (m.form == SDK_MULTISTEP_DPM) {
    const float t1 = a.sqrt_one_minus_at * e;
    const float t2 = x - t1;
    const float d = t2 / a.sqrt_at;
    p0 = d, ho = d;
    const float t3 = m.c_x * x;
    const float t4 = m.c_0 * d;
    float r = t3 + t4;
    if (m.nhist) {
      const float t5 = m.c_1 * h1;
      r = r + t5;
    }
    return r;
  }
  ho = e;
  float ep = e;                                   // e_t_prime of CompVis' p_sample_plms
  if (m.form == SDK_MULTISTEP_PLMS_WARMUP) {
    const float s = e + en;
    ep = s / 2.f;
  } else if (m.nhist == 1) {
    const float t0 = 3.f * e;
    const float t1 = t0 - h1;
    ep = t1 / 2.f;
  } else if (m.nhist == 2) {
    const float t0 = 23.f * e;
    const float t1 = 16.f * h1;
    const float t2 = t0 - t1;
    const float t3 = 5.f * h2;
    const float t4 = t2 + t3;
    ep = t4 / 12.f;
  } else if (m.nhist == 3) {
    const float t0 = 55.f * e;
    const float t1 = 59.f * h1;
    const float t2 = t0 - t1;
    const float t3 = 37.f * h2;
    const float t4 = t2 + t3;
    const float t5 = 9.f * h3;
    const float t6 = t4 - t5;
    ep = t6 / 24.f;
  }
  // ddim_elem at sigma = 0 (its noise term is then +0)
  const float t1 = a.sqrt_one_minus_at * ep;
  const float t2 = x - t1;
  p0 = t2 / a.sqrt_at;
  const float dir = a.dir_coef * ep;
  const float t3 = a.sqrt_a_prev * p0;
  const float t4 = t3 + dir;
  return t4 + 0.f;
}

// n4 16-byte groups (0 when a pointer is not aligned for them), then the scalar tail [4 n4, n).  Every input of
// an element is read before any output of it is written, so hist_out may alias a history pointer and blend.out x.
__global__ void __launch_bounds__(256) multistep_step_kernel(sdk_multistep_args m, int64_t n4) {
  const sdk_ddim_args& a = m.step;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const bool blend = m.blend.mask != nullptr, warm = m.form == SDK_MULTISTEP_PLMS_WARMUP;
  const int nh = warm ? 0 : m.nhist;
  for (int64_t i = tid; i < n4; i += stride) {
    const f4 z = {0.f, 0.f, 0.f, 0.f};
    f4 u = z, h1 = z, h2 = z, h3 = z, en = z, b0 = z, bn = z, xp, p0, ho;
    const f4 x = reinterpret_cast<const f4*>(a.x)[i];
    const f4 e = reinterpret_cast<const f4*>(a.e)[i];
    if (a.e_uncond) u = reinterpret_cast<const f4*>(a.e_uncond)[i];
    if (nh > 0) h1 = reinterpret_cast<const f4*>(m.hist[0])[i];
    if (nh > 1) h2 = reinterpret_cast<const f4*>(m.hist[1])[i];
    if (nh > 2) h3 = reinterpret_cast<const f4*>(m.hist[2])[i];
    if (warm) en = reinterpret_cast<const f4*>(m.e_next)[i];
    if (blend) {
      b0 = reinterpret_cast<const f4*>(m.blend.x0)[i];
      bn = reinterpret_cast<const f4*>(m.blend.noise)[i];
    }
    for (int j = 0; j < 4; ++j) {
      float p, h;
      xp[j] = multistep_elem(m, x[j], e[j], u[j], h1[j], h2[j], h3[j], en[j], p, h);
      p0[j] = p, ho[j] = h;
    }
    reinterpret_cast<f4*>(a.x_prev)[i] = xp;
    if (a.pred_x0) reinterpret_cast<f4*>(a.pred_x0)[i] = p0;
    if (m.hist_out) reinterpret_cast<f4*>(m.hist_out)[i] = ho;
    if (blend) {
      f4 o;
      for (int j = 0; j < 4; ++j) o[j] = masked_q_elem(m.blend, 4 * i + j, b0[j], bn[j], xp[j]);
      reinterpret_cast<f4*>(m.blend.out)[i] = o;
    }
  }
  for (int64_t i = 4 * n4 + tid; i < a.n; i += stride) {
    const float h1 = nh > 0 ? m.hist[0][i] : 0.f, h2 = nh > 1 ? m.hist[1][i] : 0.f, h3 = nh > 2 ? m.hist[2][i] : 0.f;
    const float b0 = blend ? m.blend.x0[i] : 0.f, bn = blend ? m.blend.noise[i] : 0.f;
    float p0, ho;
    const float xp = multistep_elem(m, a.x[i], a.e[i], a.e_uncond ? a.e_uncond[i] : 0.f, h1, h2, h3,
                                    warm ? m.e_next[i] : 0.f, p0, ho);
    a.x_prev[i] = xp;
    if (a.pred_x0) a.pred_x0[i] = p0;
    if (m.hist_out) m.hist_out[i] = ho;
    if (blend) m.blend.out[i] = masked_q_elem(m.blend, i, b0, bn, xp);
  }
}

__global__ void __launch_bounds__(256) cfg_combine_kernel(const float* e_u, const float* e_c, float* out, int64_t n,
                                                          int64_t n4, float g) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  for (int64_t i = tid; i < n4; i += stride) {
    const f4 u = reinterpret_cast<const f4*>(e_u)[i];
    const f4 c = reinterpret_cast<const f4*>(e_c)[i];
    f4 o;
    for (int j = 0; j < 4; ++j) o[j] = cfg_combine_elem(u[j], c[j], g);
    reinterpret_cast<f4*>(out)[i] = o;
  }
  for (int64_t i = 4 * n4 + tid; i < n; i += stride) out[i] = cfg_combine_elem(e_u[i], e_c[i], g);
}

__global__ void __launch_bounds__(256) ddpm_step_kernel(const float* x, const float* eps, const float* noise,
                                                        float* out, int64_t n, float inv_sqrt_alpha, float coef,
                                                        float sigma) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) {
    const float t = coef * eps[i];
    float v = inv_sqrt_alpha * (x[i] - t);
    if (noise) v = v + sigma * noise[i];
    out[i] = v;
  }
}

// ---- ancestral (posterior) sampler, LatentDiffusion.p_sample (ldm/diffusion/ddpm.py:1528-1636).
// One element of the update; every product and sum is rounded on its own (contraction is off), in the
// order torch evaluates predict_start_from_noise -> clamp_ -> q_posterior -> mean + mask*std*(noise*T).
// `xr` carries x_recon: computed here for stage 0 / 1, the caller's (quantised) value for stage 2.
__device__ __forceinline__ float posterior_recon(const sdk_posterior_args& a, float x, float m) {
  float xr = m;
  if (!a.x0_param) {
    const float t0 = a.c_recip * x;
    const float t1 = a.c_recipm1 * m;
    xr = t0 - t1;
  }
  if (a.clip) xr = fminf(fmaxf(xr, -1.f), 1.f);
  return xr;
}

// kf: the dropout factor of the noise (ddpm.py:1621-1624: noise*temperature, then F.dropout), read with ex.keep
__device__ __forceinline__ float posterior_xprev(const sdk_posterior_ex_args& ex, float x, float xr, float nz,
                                                 float kf) {
  const sdk_posterior_args& a = ex.step;
  const float t2 = a.coef1 * xr;
  const float t3 = a.coef2 * x;
  const float mean = t2 + t3;
  const float s = a.nonzero * a.sigma;
  float nt = nz * a.temperature;
  if (ex.keep) nt = nt * kf;
  const float sn = s * nt;
  return mean + sn;
}

// n4 16-byte groups (0 when a pointer is not 16-byte aligned), then the scalar tail [4 n4, n)
__global__ void __launch_bounds__(256) posterior_step_kernel(sdk_posterior_ex_args ex, int64_t n4) {
  const sdk_posterior_args& a = ex.step;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const bool need_m = a.stage != 2, need_x = a.stage != 1 || !a.x0_param;
  for (int64_t i = tid; i < n4; i += stride) {
    f4 x = {0.f, 0.f, 0.f, 0.f}, m = x, nz = x, kf = x, xr, xp;
    if (need_x) x = reinterpret_cast<const f4*>(a.x)[i];
    if (need_m) m = reinterpret_cast<const f4*>(a.model_out)[i];
    if (a.stage == 2) xr = reinterpret_cast<const f4*>(a.x_recon_in)[i];
    else
      for (int j = 0; j < 4; ++j) xr[j] = posterior_recon(a, x[j], m[j]);
    if (a.x_recon) reinterpret_cast<f4*>(a.x_recon)[i] = xr;
    if (a.stage == 1) continue;
    if (a.noise) nz = reinterpret_cast<const f4*>(a.noise)[i];
    if (ex.keep) {
      const uchar4 k = reinterpret_cast<const uchar4*>(ex.keep)[i];
      kf[0] = dropout_factor(k.x, ex.drop_scale), kf[1] = dropout_factor(k.y, ex.drop_scale);
      kf[2] = dropout_factor(k.z, ex.drop_scale), kf[3] = dropout_factor(k.w, ex.drop_scale);
    }
    for (int j = 0; j < 4; ++j) xp[j] = posterior_xprev(ex, x[j], xr[j], nz[j], kf[j]);
    reinterpret_cast<f4*>(a.x_prev)[i] = xp;
  }
  for (int64_t i = 4 * n4 + tid; i < a.n; i += stride) {
    const float x = need_x ? a.x[i] : 0.f;
    const float xr = a.stage == 2 ? a.x_recon_in[i] : posterior_recon(a, x, need_m ? a.model_out[i] : 0.f);
    if (a.x_recon) a.x_recon[i] = xr;
    if (a.stage == 1) continue;
    a.x_prev[i] = posterior_xprev(ex, x, xr, a.noise ? a.noise[i] : 0.f,
                                  ex.keep ? dropout_factor(ex.keep[i], ex.drop_scale) : 0.f);
  }
}

__global__ void __launch_bounds__(256) masked_q_sample_kernel(sdk_masked_q_args a, int64_t n4) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  for (int64_t i = tid; i < n4; i += stride) {
    const f4 x0 = reinterpret_cast<const f4*>(a.x0)[i];
    const f4 nz = reinterpret_cast<const f4*>(a.noise)[i];
    const f4 im = reinterpret_cast<const f4*>(a.img)[i];
    f4 o;
    for (int j = 0; j < 4; ++j) o[j] = masked_q_elem(a, 4 * i + j, x0[j], nz[j], im[j]);
    reinterpret_cast<f4*>(a.out)[i] = o;
  }
  for (int64_t i = 4 * n4 + tid; i < a.n; i += stride) a.out[i] = masked_q_elem(a, i, a.x0[i], a.noise[i], a.img[i]);
}

// channel c of the concat of the sources (planes of hw floats) at (b, pix); zero from the channel sum up to
// c_pad.  Args: sdk_concat_args or sdk_patch_pack_args (the same src / channels / nsrc)
template <class Args>
__device__ __forceinline__ float concat_fetch(const Args& a, int64_t hw, int64_t b, int64_t pix, int c) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {   // constant trip count: src[] / channels[] stay in scalar registers
    if (s >= a.nsrc) break;
    if (c < a.channels[s]) return a.src[s][(b * a.channels[s] + c) * hw + pix];
    c -= a.channels[s];
  }
  return 0.f;
}

// items [0, nvec): one 8-channel group of one pixel, a 16-byte store (consecutive lanes take consecutive
// pixels, so the NCHW reads coalesce); items [nvec, nvec + nscal): one channel past the last full group
__global__ void __launch_bounds__(256) concat_nchw_to_nhwc_kernel(sdk_concat_args a, int ngrp, int64_t nvec,
                                                                  int64_t nscal) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t bhw = (int64_t)a.batch * a.hw;
  half_t* y = reinterpret_cast<half_t*>(a.y);
  for (int64_t e = tid; e < nvec; e += stride) {
    const int g = (int)(e / bhw);
    const int64_t r = e - g * bhw, b = r / a.hw, pix = r - b * a.hw;
    h8 o;
    for (int j = 0; j < 8; ++j) o[j] = (half_t)concat_fetch(a, a.hw, b, pix, 8 * g + j);
    *reinterpret_cast<h8*>(y + r * a.c_pad + 8 * g) = o;
  }
  const int c0 = 8 * ngrp;
  for (int64_t e = tid; e < nscal; e += stride) {
    const int c = c0 + (int)(e / bhw);
    const int64_t r = e % bhw, b = r / a.hw, pix = r - b * a.hw;
    y[r * a.c_pad + c] = (half_t)concat_fetch(a, a.hw, b, pix, c);
  }
}

// row r of the patch window -> (image b, offset of its pixel in an h x w plane): r = (pl*kh + i)*kw + j, patch
// p = p0 + pl = l*batch + b, l = ly*Lx + lx (torch.nn.Unfold order, as extract_patches_kernel)
__device__ __forceinline__ void patch_row(const sdk_patch_pack_args& a, int Lx, int64_t r, int64_t& b, int64_t& pix) {
  const int khw = a.kh * a.kw;
  const int64_t p = a.p0 + r / khw;
  const int q = (int)(r % khw), i = q / a.kw, j = q - i * a.kw;
  const int64_t l = p / a.batch;
  b = p - l * a.batch;
  const int ly = (int)(l / Lx), lx = (int)(l - (int64_t)ly * Lx);
  pix = (int64_t)(ly * a.sy + i) * a.w + lx * a.sx + j;
}

// concat_nchw_to_nhwc_kernel over the rows of np patches gathered from the full-size sources: items
// [0, nvec) one 8-channel group of one patch pixel (a 16-byte store; consecutive lanes take consecutive
// pixels of one patch row, so the reads are runs of kw floats), items [nvec, nvec + nscal) one channel
// past the last full group
__global__ void __launch_bounds__(256) patch_pack_kernel(sdk_patch_pack_args a, int Lx, int ngrp, int64_t nvec,
                                                         int64_t nscal) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t rows = (int64_t)a.np * a.kh * a.kw, hw = (int64_t)a.h * a.w;
  half_t* y = reinterpret_cast<half_t*>(a.y);
  for (int64_t e = tid; e < nvec; e += stride) {
    const int g = (int)(e / rows);
    const int64_t r = e - g * rows;
    int64_t b, pix;
    patch_row(a, Lx, r, b, pix);
    h8 o;
    for (int j = 0; j < 8; ++j) o[j] = (half_t)concat_fetch(a, hw, b, pix, 8 * g + j);
    *reinterpret_cast<h8*>(y + r * a.c_pad + 8 * g) = o;
  }
  const int c0 = 8 * ngrp;
  for (int64_t e = tid; e < nscal; e += stride) {
    const int c = c0 + (int)(e / rows);
    const int64_t r = e % rows;
    int64_t b, pix;
    patch_row(a, Lx, r, b, pix);
    y[r * a.c_pad + c] = (half_t)concat_fetch(a, hw, b, pix, c);
  }
}

__global__ void temb_kernel(const int64_t* t, const float* freqs, half_t* out, int batch, int dim) {
  const int half = dim / 2;
  const int b = blockIdx.x;
  const float tf = (float)t[b];
  for (int k = threadIdx.x; k < dim; k += blockDim.x) {
    float v = 0.f;
    if (k < half) v = cosf(tf * freqs[k]);
    else if (k < 2 * half) v = sinf(tf * freqs[k - half]);
    out[(size_t)b * dim + k] = (half_t)v;
  }
}

__global__ void __launch_bounds__(256) nchw_to_nhwc_kernel(const float* x, half_t* y, int C, int HW, int Cp,
                                                           float scale) {
  // grid (ceil(HW/64), B); tile 64 pixels x C through LDS so both sides are coalesced
  __shared__ float tile[64][33];
  const int b = blockIdx.y, p0 = blockIdx.x * 64;
  for (int c0 = 0; c0 < Cp; c0 += 32) {
    for (int e = threadIdx.x; e < 32 * 64; e += 256) {
      const int cc = e / 64, pp = e % 64;
      const int c = c0 + cc, pix = p0 + pp;
      float v = 0.f;
      if (c < C && pix < HW) v = x[((size_t)b * C + c) * HW + pix] * scale;
      tile[pp][cc] = v;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 32 * 64; e += 256) {
      const int pp = e / 32, cc = e % 32;
      const int c = c0 + cc, pix = p0 + pp;
      if (c < Cp && pix < HW) y[((size_t)b * HW + pix) * Cp + c] = (half_t)tile[pp][cc];
    }
    __syncthreads();
  }
}

// grid-stride over the latent elements; moments = [mean | logvar] along channels (NCHW)
__global__ void __launch_bounds__(256) diag_gauss_kernel(const float* moments, const float* noise, float* z,
                                                         int channels, int hw, int64_t n, float scale) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t per_img = (int64_t)channels * hw;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t b = i / per_img, r = i - b * per_img;
    const float mean = moments[b * 2 * per_img + r];
    float v = mean;
    if (noise) {
      const float lv = fminf(fmaxf(moments[b * 2 * per_img + per_img + r], -30.f), 20.f);
      const float sd = expf(0.5f * lv);
      v = mean + sd * noise[i];
    }
    z[i] = scale * v;
  }
}

__global__ void __launch_bounds__(256) stochastic_encode_kernel(const float* x0, const float* noise, float* out,
                                                                int64_t n, float sa, float s1ma) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) {
    const float t0 = sa * x0[i];
    const float t1 = s1ma * noise[i];
    out[i] = t0 + t1;
  }
}

// one block per token row: 8 channels per thread, fp32 sum rounded once to fp16
__global__ void __launch_bounds__(128) token_embedding_kernel(const int64_t* ids, const float* tok, const float* pos,
                                                              half_t* out, int seq, int dim) {
  const int row = blockIdx.x, t = row % seq;
  const int64_t id = ids[row];
  for (int c = threadIdx.x * 4; c < dim; c += blockDim.x * 4) {
    const f4 a = *reinterpret_cast<const f4*>(tok + id * dim + c);
    const f4 b = *reinterpret_cast<const f4*>(pos + (int64_t)t * dim + c);
    h4 o;
    for (int j = 0; j < 4; ++j) o[j] = (half_t)(a[j] + b[j]);
    *reinterpret_cast<h4*>(out + (int64_t)row * dim + c) = o;
  }
}

// F.interpolate(scale_factor=2, mode="bilinear", align_corners=True) on NHWC fp16, 8 channels per
// thread: source coordinate = dst * (in - 1) / (out - 1), fp32 weights as torch computes them
__global__ void __launch_bounds__(256) upsample_bilinear2x_kernel(const half_t* x, half_t* y, int h, int w, int c,
                                                                  int64_t nvec) {
  const int c8 = c / 8, ho = 2 * h, wo = 2 * w;
  const float ry = ho > 1 ? (float)(h - 1) / (float)(ho - 1) : 0.f;
  const float rx = wo > 1 ? (float)(w - 1) / (float)(wo - 1) : 0.f;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < nvec; e += stride) {
    const int cc = (int)(e % c8) * 8;
    int64_t r = e / c8;
    const int ox = (int)(r % wo); r /= wo;
    const int oy = (int)(r % ho);
    const int b = (int)(r / ho);
    const float sy = ry * oy, sx = rx * ox;
    const int y0 = (int)sy, x0 = (int)sx;
    const int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
    const float ly = sy - y0, lx = sx - x0, hy = 1.f - ly, hx = 1.f - lx;
    const half_t* base = x + (size_t)b * h * w * c + cc;
    const h8 a = *reinterpret_cast<const h8*>(base + ((size_t)y0 * w + x0) * c);
    const h8 bb = *reinterpret_cast<const h8*>(base + ((size_t)y0 * w + x1) * c);
    const h8 cq = *reinterpret_cast<const h8*>(base + ((size_t)y1 * w + x0) * c);
    const h8 d = *reinterpret_cast<const h8*>(base + ((size_t)y1 * w + x1) * c);
    h8 o;
    for (int j = 0; j < 8; ++j)
      o[j] = (half_t)(hy * (hx * (float)a[j] + lx * (float)bb[j]) + ly * (hx * (float)cq[j] + lx * (float)d[j]));
    *reinterpret_cast<h8*>(y + ((size_t)(b * ho + oy) * wo + ox) * c + cc) = o;
  }
}

// exact (erf) GELU, nn.GELU(): fp16 in / out, fp32 math
__global__ void __launch_bounds__(256) gelu_kernel(const half_t* x, half_t* y, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) {
    const float v = (float)x[i];
    y[i] = (half_t)(0.5f * v * (1.0f + erff(v * 0.70710678118654752f)));
  }
}

// patch p = ((ly*Lx + lx)*B + b): out[p][c][i][j] = z[b][c][ly*sy + i][lx*sx + j] (torch.nn.Unfold order)
__global__ void __launch_bounds__(256) extract_patches_kernel(const float* z, float* out, int B, int C, int H, int W,
                                                              int kh, int kw, int sy, int sx, int Lx, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += stride) {
    const int j = (int)(e % kw);
    int64_t r = e / kw;
    const int i = (int)(r % kh); r /= kh;
    const int c = (int)(r % C); r /= C;
    const int b = (int)(r % B);
    const int l = (int)(r / B);
    const int ly = l / Lx, lx = l - ly * Lx;
    out[e] = z[(((int64_t)b * C + c) * H + ly * sy + i) * W + lx * sx + j];
  }
}

// overlap-add of weighted decoded patches, normalised per pixel:
// out = sum_l w(l, y, x) * patch_l / sum_l w(l, y, x), w = pix_w[i][j] * (l_w ? l_w[l] : 1)
// (torch.nn.Fold of o*weighting divided by Fold(weighting)); one thread per output element
// gathers the <= ceil(ph/sy) x ceil(pw/sx) covering patches — no atomics, deterministic
__global__ void __launch_bounds__(256) fold_patches_kernel(const float* patches, const float* pix_w, const float* l_w,
                                                           float* out, int B, int C, int H, int W, int ph, int pw,
                                                           int sy, int sx, int Ly, int Lx, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += stride) {
    const int x = (int)(e % W);
    int64_t r = e / W;
    const int y = (int)(r % H); r /= H;
    const int c = (int)(r % C);
    const int b = (int)(r / C);
    const int ly0 = y >= ph ? (y - ph) / sy + 1 : 0, ly1 = min(Ly - 1, y / sy);
    const int lx0 = x >= pw ? (x - pw) / sx + 1 : 0, lx1 = min(Lx - 1, x / sx);
    float num = 0.f, den = 0.f;
    for (int ly = ly0; ly <= ly1; ++ly)
      for (int lx = lx0; lx <= lx1; ++lx) {
        const int l = ly * Lx + lx, i = y - ly * sy, j = x - lx * sx;
        float w = pix_w[i * pw + j];
        if (l_w) w = w * l_w[l];
        const float v = patches[((((int64_t)l * B + b) * C + c) * ph + i) * pw + j];
        num = num + v * w;
        den = den + w;
      }
    out[e] = num / den;   // 0/0 = NaN where no patch covers the pixel, as Fold / normalization
  }
}

}  // namespace
}  // namespace sdk

using namespace sdk;

extern "C" int sdk_upsample_bilinear2x(const void* x, void* y, int32_t batch, int32_t h, int32_t w,
                                       int32_t channels, sdk_stream_t stream) {
  if (!x || !y || batch <= 0 || h <= 0 || w <= 0 || channels <= 0 || channels % 8)
    return fail(SDK_EINVAL, "upsample_bilinear2x: bad args (channels % 8)");
  const int64_t nvec = (int64_t)batch * 4 * h * w * (channels / 8);
  const int blocks = (int)std::min<int64_t>((nvec + 255) / 256, 8192);
  hipLaunchKernelGGL(upsample_bilinear2x_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const half_t*)x,
                     (half_t*)y, h, w, channels, nvec);
  return check_launch("upsample_bilinear2x");
}

extern "C" int sdk_gelu(const void* x, void* y, int64_t n, sdk_stream_t stream) {
  if (!x || !y || n <= 0) return fail(SDK_EINVAL, "gelu: bad args");
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(gelu_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const half_t*)x, (half_t*)y, n);
  return check_launch("gelu");
}

extern "C" int sdk_extract_patches(const float* z, float* out, int32_t batch, int32_t channels, int32_t h, int32_t w,
                                   int32_t kh, int32_t kw, int32_t sy, int32_t sx, sdk_stream_t stream) {
  if (!z || !out || batch <= 0 || channels <= 0 || kh <= 0 || kw <= 0 || sy <= 0 || sx <= 0 || kh > h || kw > w)
    return fail(SDK_EINVAL, "extract_patches: bad geometry");
  const int Ly = (h - kh) / sy + 1, Lx = (w - kw) / sx + 1;
  const int64_t n = (int64_t)Ly * Lx * batch * channels * kh * kw;
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(extract_patches_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, z, out, batch, channels,
                     h, w, kh, kw, sy, sx, Lx, n);
  return check_launch("extract_patches");
}

extern "C" int sdk_fold_patches(const float* patches, const float* pix_w, const float* l_w, float* out, int32_t batch,
                                int32_t channels, int32_t h, int32_t w, int32_t ph, int32_t pw, int32_t sy, int32_t sx,
                                int32_t ly, int32_t lx, sdk_stream_t stream) {
  if (!patches || !pix_w || !out || batch <= 0 || channels <= 0 || ph <= 0 || pw <= 0 || sy <= 0 || sx <= 0 ||
      ly <= 0 || lx <= 0 || (ly - 1) * sy + ph > h || (lx - 1) * sx + pw > w)
    return fail(SDK_EINVAL, "fold_patches: bad geometry");
  const int64_t n = (int64_t)batch * channels * h * w;
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(fold_patches_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, patches, pix_w, l_w, out,
                     batch, channels, h, w, ph, pw, sy, sx, ly, lx, n);
  return check_launch("fold_patches");
}

extern "C" int sdk_token_embedding(const int64_t* ids, const float* tok, const float* pos, void* out, int32_t batch,
                                   int32_t seq, int32_t dim, sdk_stream_t stream) {
  if (!ids || !tok || !pos || !out || batch <= 0 || seq <= 0 || dim <= 0 || dim % 4)
    return fail(SDK_EINVAL, "token_embedding: bad args (dim must be a multiple of 4)");
  hipLaunchKernelGGL(token_embedding_kernel, dim3(batch * seq), dim3(128), 0, (hipStream_t)stream, ids, tok, pos,
                     (half_t*)out, seq, dim);
  return check_launch("token_embedding");
}

extern "C" int sdk_diag_gaussian_sample(const float* moments, const float* noise, float* z, int32_t batch,
                                        int32_t channels, int32_t hw, float scale, sdk_stream_t stream) {
  if (!moments || !z || batch <= 0 || channels <= 0 || hw <= 0) return fail(SDK_EINVAL, "diag_gaussian_sample: bad args");
  const int64_t n = (int64_t)batch * channels * hw;
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 2048);
  hipLaunchKernelGGL(diag_gauss_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, moments, noise, z, channels,
                     hw, n, scale);
  return check_launch("diag_gaussian_sample");
}

extern "C" int sdk_stochastic_encode(const float* x0, const float* noise, float* out, int64_t n, float sqrt_a,
                                     float sqrt_1ma, sdk_stream_t stream) {
  if (!x0 || !noise || !out || n <= 0) return fail(SDK_EINVAL, "stochastic_encode: bad args");
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 2048);
  hipLaunchKernelGGL(stochastic_encode_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x0, noise, out, n,
                     sqrt_a, sqrt_1ma);
  return check_launch("stochastic_encode");
}

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the one launch of the DDIM family; the entry points below have checked their own arguments
static int launch_ddim(const sdk_ddim_ex_args& ex, const char* what, sdk_stream_t stream) {
  const sdk_ddim_args& a = ex.step;
  const bool vec = aligned16(a.x) && aligned16(a.e) && aligned16(a.e_uncond) && aligned16(a.noise) &&
                   aligned16(a.x_prev) && aligned16(a.pred_x0) && aligned16(ex.blend.x0) &&
                   aligned16(ex.blend.noise) && aligned16(ex.blend.out) &&
                   (reinterpret_cast<uintptr_t>(ex.keep) & 3) == 0;
  const int64_t n4 = vec ? a.n / 4 : 0;
  const int64_t items = std::max<int64_t>(n4, a.n - 4 * n4);
  const int blocks = (int)std::min<int64_t>((items + 255) / 256, 2048);
  hipLaunchKernelGGL(ddim_step_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, ex, n4);
  return check_launch(what);
}

extern "C" int sdk_ddim_step_ex(const sdk_ddim_ex_args* ex, sdk_stream_t stream) {
  if (!ex) return fail(SDK_EINVAL, "ddim_step_ex: null pointer");
  const sdk_ddim_args& a = ex->step;
  const sdk_masked_q_args& m = ex->blend;
  const bool blend = m.mask != nullptr;
  if (!a.e || !a.x_prev || (ex->pred_x0_in ? (!a.pred_x0 || (a.v_param && !a.x)) : !a.x))
    return fail(SDK_EINVAL, "ddim_step_ex: null pointer");
  if (a.n <= 0) return fail(SDK_EINVAL, "ddim_step_ex: n must be positive");
  if (ex->keep && !a.noise) return fail(SDK_EINVAL, "ddim_step_ex: keep needs noise");
  if (blend) {
    if (!m.x0 || !m.noise || !m.out) return fail(SDK_EINVAL, "ddim_step_ex: blend needs x0, noise and out");
    if (m.hw <= 0 || m.per_sample <= 0 || m.per_sample % m.hw || a.n % m.per_sample || m.mask_mode < 0 ||
        m.mask_mode > 2)
      return fail(SDK_EINVAL, "ddim_step_ex: bad blend geometry (n = batch * per_sample, per_sample = channels * hw)");
  }
  return launch_ddim(*ex, "ddim_step_ex", stream);
}

extern "C" int sdk_ddim_step(const sdk_ddim_args* a, sdk_stream_t stream) {
  if (!a || !a->x || !a->e || !a->x_prev) return fail(SDK_EINVAL, "ddim_step: null pointer");
  if (a->n <= 0 || a->n % 4) return fail(SDK_EINVAL, "ddim_step: n must be a positive multiple of 4");
  sdk_ddim_ex_args ex = {};
  ex.step = *a;
  return launch_ddim(ex, "ddim_step", stream);
}

extern "C" int sdk_ddim_xprev(const sdk_ddim_args* a, sdk_stream_t stream) {
  if (!a || !a->e || !a->x_prev || !a->pred_x0 || (a->v_param && !a->x))
    return fail(SDK_EINVAL, "ddim_xprev: null pointer");
  if (a->n <= 0 || a->n % 4) return fail(SDK_EINVAL, "ddim_xprev: n must be a positive multiple of 4");
  sdk_ddim_ex_args ex = {};
  ex.step = *a;
  ex.pred_x0_in = 1;
  if (!a->v_param) ex.step.x = nullptr;          // read only for the v conversion
  return launch_ddim(ex, "ddim_xprev", stream);
}

extern "C" int sdk_multistep_step(const sdk_multistep_args* m, sdk_stream_t stream) {
  if (!m) return fail(SDK_EINVAL, "multistep_step: null pointer");
  const sdk_ddim_args& a = m->step;
  const sdk_masked_q_args& b = m->blend;
  if (!a.x || !a.e || !a.x_prev) return fail(SDK_EINVAL, "multistep_step: null pointer");
  if (a.n <= 0) return fail(SDK_EINVAL, "multistep_step: n must be positive");
  if (a.noise || a.sigma != 0.f) return fail(SDK_EINVAL, "multistep_step: deterministic only (noise NULL, sigma 0)");
  if (m->form < SDK_MULTISTEP_PLMS || m->form > SDK_MULTISTEP_DPM) return fail(SDK_EINVAL, "multistep_step: bad form");
  const bool warm = m->form == SDK_MULTISTEP_PLMS_WARMUP;
  const int max_hist = m->form == SDK_MULTISTEP_PLMS ? 3 : m->form == SDK_MULTISTEP_DPM ? 1 : 0;
  if (m->nhist < 0 || m->nhist > max_hist)
    return fail(SDK_EINVAL, "multistep_step: nhist must be 0..3 (PLMS), 0 (warm-up) or 0..1 (DPM)");
  for (int k = 0; k < m->nhist; ++k)
    if (!m->hist[k]) return fail(SDK_EINVAL, "multistep_step: nhist history pointers must be set");
  if (warm && !m->e_next) return fail(SDK_EINVAL, "multistep_step: the warm-up form needs e_next");
  bool vec = aligned16(a.x) && aligned16(a.e) && aligned16(a.e_uncond) && aligned16(a.x_prev) &&
             aligned16(a.pred_x0) && aligned16(m->hist_out) && (!warm || aligned16(m->e_next));
  for (int k = 0; k < m->nhist; ++k) vec = vec && aligned16(m->hist[k]);
  if (b.mask) {
    if (!b.x0 || !b.noise || !b.out) return fail(SDK_EINVAL, "multistep_step: blend needs x0, noise and out");
    if (b.hw <= 0 || b.per_sample <= 0 || b.per_sample % b.hw || a.n % b.per_sample || b.mask_mode < 0 ||
        b.mask_mode > 2)
      return fail(SDK_EINVAL, "multistep_step: bad blend geometry (n = batch * per_sample, per_sample = channels * hw)");
    vec = vec && aligned16(b.x0) && aligned16(b.noise) && aligned16(b.out);
  }
  const int64_t n4 = vec ? a.n / 4 : 0;
  const int64_t items = std::max<int64_t>(n4, a.n - 4 * n4);
  const int blocks = (int)std::min<int64_t>((items + 255) / 256, 2048);
  hipLaunchKernelGGL(multistep_step_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, *m, n4);
  return check_launch("multistep_step");
}

extern "C" int sdk_cfg_combine(const float* e_uncond, const float* e_cond, float* out, int64_t n, float guidance,
                               sdk_stream_t stream) {
  if (!e_uncond || !e_cond || !out || n <= 0) return fail(SDK_EINVAL, "cfg_combine: bad args");
  const int64_t n4 = aligned16(e_uncond) && aligned16(e_cond) && aligned16(out) ? n / 4 : 0;
  const int64_t items = std::max<int64_t>(n4, n - 4 * n4);
  const int blocks = (int)std::min<int64_t>((items + 255) / 256, 2048);
  hipLaunchKernelGGL(cfg_combine_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, e_uncond, e_cond, out, n,
                     n4, guidance);
  return check_launch("cfg_combine");
}

extern "C" int sdk_ddpm_step(const float* x, const float* eps, const float* noise, float* out, int64_t n,
                             float inv_sqrt_alpha, float coef, float sigma, sdk_stream_t stream) {
  if (!x || !eps || !out || n <= 0) return fail(SDK_EINVAL, "ddpm_step: bad args");
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 2048);
  hipLaunchKernelGGL(ddpm_step_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, eps, noise, out, n,
                     inv_sqrt_alpha, coef, sigma);
  return check_launch("ddpm_step");
}

extern "C" int sdk_timestep_embedding(const int64_t* t, const float* freqs, void* out, int32_t batch, int32_t dim,
                                      sdk_stream_t stream) {
  if (!t || !freqs || !out || batch <= 0 || dim <= 0) return fail(SDK_EINVAL, "timestep_embedding: bad args");
  hipLaunchKernelGGL(temb_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, t, freqs, (half_t*)out, batch,
                     dim);
  return check_launch("timestep_embedding");
}

extern "C" int sdk_nchw_to_nhwc(const float* x, void* y, int32_t batch, int32_t channels, int32_t hw, int32_t c_pad,
                                float scale, sdk_stream_t stream) {
  if (!x || !y || batch <= 0 || channels <= 0 || hw <= 0 || c_pad < channels)
    return fail(SDK_EINVAL, "nchw_to_nhwc: bad args");
  hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3((hw + 63) / 64, batch), dim3(256), 0, (hipStream_t)stream, x,
                     (half_t*)y, channels, hw, c_pad, scale);
  return check_launch("nchw_to_nhwc");
}

static int posterior_launch(const sdk_posterior_ex_args& ex, const char* what, sdk_stream_t stream);

extern "C" int sdk_posterior_step(const sdk_posterior_args* a, sdk_stream_t stream) {
  if (!a) return fail(SDK_EINVAL, "posterior_step: bad n / stage");
  sdk_posterior_ex_args ex = {};
  ex.step = *a;
  return posterior_launch(ex, "posterior_step", stream);
}

extern "C" int sdk_posterior_step_ex(const sdk_posterior_ex_args* ex, sdk_stream_t stream) {
  if (!ex) return fail(SDK_EINVAL, "posterior_step_ex: bad n / stage");
  if (ex->keep && (ex->step.stage == 1 || !ex->step.noise))
    return fail(SDK_EINVAL, "posterior_step_ex: keep needs noise and a stage that writes x_prev");
  return posterior_launch(*ex, "posterior_step_ex", stream);
}

// the argument checks and the launch shared by the two entry points
static int posterior_launch(const sdk_posterior_ex_args& ex, const char* what, sdk_stream_t stream) {
  const sdk_posterior_args* a = &ex.step;
  const std::string w(what);
  if (a->n <= 0 || a->stage < 0 || a->stage > 2) return fail(SDK_EINVAL, w + ": bad n / stage");
  const bool need_m = a->stage != 2, need_x = a->stage != 1 || !a->x0_param;
  if ((need_x && !a->x) || (need_m && !a->model_out) || (a->stage == 2 && !a->x_recon_in) ||
      (a->stage != 1 && !a->x_prev) || (a->stage == 1 && !a->x_recon))
    return fail(SDK_EINVAL, w + ": null pointer");
  if (a->stage != 1 && !a->noise && a->nonzero != 0.f)
    return fail(SDK_EINVAL, w + ": noise may be NULL only where nonzero == 0");
  const bool vec = aligned16(a->x) && aligned16(a->model_out) && aligned16(a->noise) && aligned16(a->x_recon_in) &&
                   aligned16(a->x_prev) && aligned16(a->x_recon) && (reinterpret_cast<uintptr_t>(ex.keep) & 3) == 0;
  const int64_t n4 = vec ? a->n / 4 : 0;
  const int64_t items = std::max<int64_t>(n4, a->n - 4 * n4);
  const int blocks = (int)std::min<int64_t>((items + 255) / 256, 2048);
  hipLaunchKernelGGL(posterior_step_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, ex, n4);
  return check_launch(what);
}

extern "C" int sdk_masked_q_sample(const sdk_masked_q_args* a, sdk_stream_t stream) {
  if (!a || !a->x0 || !a->noise || !a->mask || !a->img || !a->out) return fail(SDK_EINVAL, "masked_q_sample: null pointer");
  if (a->n <= 0 || a->hw <= 0 || a->per_sample <= 0 || a->per_sample % a->hw || a->n % a->per_sample ||
      a->mask_mode < 0 || a->mask_mode > 2)
    return fail(SDK_EINVAL, "masked_q_sample: bad geometry (n = batch * per_sample, per_sample = channels * hw)");
  const bool vec = aligned16(a->x0) && aligned16(a->noise) && aligned16(a->img) && aligned16(a->out);
  const int64_t n4 = vec ? a->n / 4 : 0;
  const int64_t items = std::max<int64_t>(n4, a->n - 4 * n4);
  const int blocks = (int)std::min<int64_t>((items + 255) / 256, 2048);
  hipLaunchKernelGGL(masked_q_sample_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, *a, n4);
  return check_launch("masked_q_sample");
}

extern "C" int sdk_concat_nchw_to_nhwc(const sdk_concat_args* a, sdk_stream_t stream) {
  if (!a || !a->y || a->nsrc < 1 || a->nsrc > 4 || a->batch <= 0 || a->hw <= 0)
    return fail(SDK_EINVAL, "concat_nchw_to_nhwc: bad args (1..4 sources)");
  int64_t csum = 0;
  for (int s = 0; s < a->nsrc; ++s) {
    if (!a->src[s] || a->channels[s] <= 0) return fail(SDK_EINVAL, "concat_nchw_to_nhwc: null source / channels <= 0");
    csum += a->channels[s];
  }
  if (a->c_pad < csum) return fail(SDK_EINVAL, "concat_nchw_to_nhwc: c_pad below the channel sum");
  const int ngrp = (a->c_pad % 8 == 0 && aligned16(a->y)) ? a->c_pad / 8 : 0;
  const int64_t bhw = (int64_t)a->batch * a->hw;
  const int64_t nvec = ngrp * bhw, nscal = (a->c_pad - 8 * ngrp) * bhw;
  const int blocks = (int)std::min<int64_t>((std::max(nvec, nscal) + 255) / 256, 2048);
  hipLaunchKernelGGL(concat_nchw_to_nhwc_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, *a, ngrp, nvec,
                     nscal);
  return check_launch("concat_nchw_to_nhwc");
}

extern "C" int sdk_patch_pack(const sdk_patch_pack_args* a, sdk_stream_t stream) {
  if (!a || !a->y || a->nsrc < 1 || a->nsrc > 4 || a->batch <= 0 || a->h <= 0 || a->w <= 0)
    return fail(SDK_EINVAL, "patch_pack: bad args (1..4 sources)");
  int64_t csum = 0;
  for (int s = 0; s < a->nsrc; ++s) {
    if (!a->src[s] || a->channels[s] <= 0) return fail(SDK_EINVAL, "patch_pack: null source / channels <= 0");
    csum += a->channels[s];
  }
  if (a->c_pad < csum) return fail(SDK_EINVAL, "patch_pack: c_pad below the channel sum");
  if (a->kh <= 0 || a->kw <= 0 || a->sy <= 0 || a->sx <= 0 || a->kh > a->h || a->kw > a->w)
    return fail(SDK_EINVAL, "patch_pack: bad geometry (0 < kh <= h, 0 < kw <= w, strides > 0)");
  const int Ly = (a->h - a->kh) / a->sy + 1, Lx = (a->w - a->kw) / a->sx + 1;
  const int64_t total = (int64_t)Ly * Lx * a->batch;
  if (a->p0 < 0 || a->np < 1 || (int64_t)a->p0 + a->np > total)
    return fail(SDK_EINVAL, "patch_pack: patch window [p0, p0 + np) outside the " + std::to_string(total) +
                                " patches");
  const int ngrp = (a->c_pad % 8 == 0 && aligned16(a->y)) ? a->c_pad / 8 : 0;
  const int64_t rows = (int64_t)a->np * a->kh * a->kw;
  const int64_t nvec = ngrp * rows, nscal = (a->c_pad - 8 * ngrp) * rows;
  const int blocks = (int)std::min<int64_t>((std::max(nvec, nscal) + 255) / 256, 2048);
  hipLaunchKernelGGL(patch_pack_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, *a, Lx, ngrp, nvec, nscal);
  return check_launch("patch_pack");
}

extern "C" const char* sdk_last_error(void) { return g_last_error.c_str(); }

extern "C" int sdk_version(void) { return 1; }
