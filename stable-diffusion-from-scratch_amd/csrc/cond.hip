// Condition-encoder kernels (clip_encoder/modules.py): the ClassEmbedder row gather and SpatialRescaler's
// F.interpolate.  Both are HBM-bound elementwise kernels: no LDS, one output element (or one 16-byte
// group) per thread, consecutive lanes on consecutive addresses.
//
// The resize evaluates torch's CPU expressions (aten UpSampleKernel.cpp / AdaptiveAvgPoolKernel.cpp) in
// fp32, operation by operation, with floating-point contraction OFF as in sampler.hip.
#include <cmath>

#include "common.h"

#pragma clang fp contract(off)

namespace sdk {
namespace {

// items [0, nvec): 8 columns of one row (two 16-byte loads, one 16-byte store); nvec == 0 selects the
// scalar form, one element per thread
__global__ void __launch_bounds__(256) embedding_rows_kernel(const int64_t* ids, const float* table, half_t* out,
                                                             int dim, int64_t nvec, int64_t nscal) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (nvec > 0) {
    if (e >= nvec) return;
    const int d8 = dim / 8;
    const int64_t i = e / d8;
    const int c = (int)(e - i * d8) * 8;
    const float* src = table + ids[i] * dim + c;
    const f4 a = *reinterpret_cast<const f4*>(src), b = *reinterpret_cast<const f4*>(src + 4);
    h8 o;
    for (int j = 0; j < 4; ++j) {
      o[j] = (half_t)a[j];
      o[4 + j] = (half_t)b[j];
    }
    *reinterpret_cast<h8*>(out + i * dim + c) = o;
    return;
  }
  if (e >= nscal) return;
  const int64_t i = e / dim;
  const int c = (int)(e - i * dim);
  out[e] = (half_t)table[ids[i] * dim + c];
}

// ---- source coordinates, aten/src/ATen/native/UpSample.h
// area_pixel_compute_source_index(align_corners = false): the linear form clamps at zero, the cubic does not
__device__ __forceinline__ float src_index(float step, int dst, bool cubic) {
  const float t0 = (float)dst + 0.5f;
  const float t1 = step * t0;
  const float s = t1 - 0.5f;
  return (!cubic && s < 0.f) ? 0.f : s;
}

// guard_index_and_lambda: index = min(floor(s), in - 1), lambda = clamp(s - index, 0, 1)
__device__ __forceinline__ void index_lambda(float s, int in, int& idx, float& lam) {
  idx = min((int)floorf(s), in - 1);
  lam = fminf(fmaxf(s - (float)idx, 0.f), 1.f);
}

// compute_source_index_and_lambda: equal sizes copy; the upper tap stays inside the image
__device__ __forceinline__ void linear_taps(float step, int dst, int in, int out, int& i0, int& i1, float& w0,
                                            float& w1) {
  if (in == out) {
    i0 = i1 = dst;
    w0 = 1.f;
    w1 = 0.f;
    return;
  }
  index_lambda(src_index(step, dst, false), in, i0, w1);
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  w0 = 1.f - w1;
}

__device__ __forceinline__ float cubic1(float x, float A) { return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f; }
__device__ __forceinline__ float cubic2(float x, float A) { return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A; }

// get_cubic_upsample_coefficients (A = -0.75) with the four taps clamped into the image
__device__ __forceinline__ void cubic_taps(float step, int dst, int in, int (&idx)[4], float (&w)[4]) {
  int i0;
  float t;
  index_lambda(src_index(step, dst, true), in, i0, t);
  const float A = -0.75f;
  w[0] = cubic2(t + 1.f, A);
  w[1] = cubic1(t, A);
  const float u = 1.f - t;
  w[2] = cubic1(u, A);
  w[3] = cubic2(u + 1.f, A);
#pragma unroll
  for (int j = 0; j < 4; ++j) idx[j] = max(min(i0 + j - 1, in - 1), 0);
}

// one thread per output element; e runs over [plane][oy][ox], ox fastest
template <int MODE>
__global__ void __launch_bounds__(256) resize2d_kernel(const float* __restrict__ x, float* __restrict__ y, int h, int w,
                                                       int ho, int wo, float step_h, float step_w, int64_t n) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= n) return;
  const int ox = (int)(e % wo);
  const int64_t r = e / wo;
  const int oy = (int)(r % ho);
  const float* p = x + (r / ho) * ((int64_t)h * w);
  float v;
  if (MODE == SDK_RESIZE_NEAREST) {
    // nearest_neighbor_compute_source_index: min(floor(dst * step), in - 1)
    const int iy = min((int)floorf((float)oy * step_h), h - 1);
    const int ix = min((int)floorf((float)ox * step_w), w - 1);
    v = p[(int64_t)iy * w + ix];
  } else if (MODE == SDK_RESIZE_BILINEAR) {
    int y0, y1, x0, x1;
    float wy0, wy1, wx0, wx1;
    linear_taps(step_h, oy, h, ho, y0, y1, wy0, wy1);
    linear_taps(step_w, ox, w, wo, x0, x1, wx0, wx1);
    const float* r0 = p + (int64_t)y0 * w;
    const float* r1 = p + (int64_t)y1 * w;
    float a = r0[x0] * wx0;
    a = a + r0[x1] * wx1;
    float b = r1[x0] * wx0;
    b = b + r1[x1] * wx1;
    v = a * wy0;
    v = v + b * wy1;
  } else if (MODE == SDK_RESIZE_BICUBIC) {
    int iy[4], ix[4];
    float wy[4], wx[4];
    cubic_taps(step_h, oy, h, iy, wy);
    cubic_taps(step_w, ox, w, ix, wx);
    v = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float* row = p + (int64_t)iy[i] * w;
      float a = row[ix[0]] * wx[0];
#pragma unroll
      for (int j = 1; j < 4; ++j) a = a + row[ix[j]] * wx[j];
      v = i == 0 ? a * wy[0] : v + a * wy[i];
    }
  } else {
    // adaptive average pooling: rows [floor(o*in/out), ceil((o+1)*in/out)), summed row by row
    const int y0 = (int)(((int64_t)oy * h) / ho), y1 = (int)(((int64_t)(oy + 1) * h + ho - 1) / ho);
    const int x0 = (int)(((int64_t)ox * w) / wo), x1 = (int)(((int64_t)(ox + 1) * w + wo - 1) / wo);
    float s = 0.f;
    for (int iy = y0; iy < y1; ++iy)
      for (int ix = x0; ix < x1; ++ix) s = s + p[(int64_t)iy * w + ix];
    v = s / (float)(y1 - y0) / (float)(x1 - x0);
  }
  y[e] = v;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace sdk

using namespace sdk;

extern "C" int sdk_embedding_rows(const int64_t* ids, const float* table, void* out, int32_t n, int32_t dim,
                                  sdk_stream_t stream) {
  if (!ids || !table || !out || n <= 0 || dim <= 0) return fail(SDK_EINVAL, "embedding_rows: bad args");
  const bool vec = dim % 8 == 0 && aligned16(table) && aligned16(out);
  const int64_t nvec = vec ? (int64_t)n * (dim / 8) : 0, nscal = (int64_t)n * dim;
  const int64_t blocks = ((vec ? nvec : nscal) + 255) / 256;
  if (blocks > 0x7fffffffLL) return fail(SDK_EINVAL, "embedding_rows: grid too large");
  hipLaunchKernelGGL(embedding_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, ids, table,
                     (half_t*)out, dim, nvec, nscal);
  return check_launch("embedding_rows");
}

extern "C" int sdk_resize2d(const sdk_resize2d_args* a, sdk_stream_t stream) {
  if (!a || !a->x || !a->y) return fail(SDK_EINVAL, "resize2d: null pointer");
  if (a->planes <= 0 || a->h <= 0 || a->w <= 0 || a->out_h <= 0 || a->out_w <= 0)
    return fail(SDK_EINVAL, "resize2d: planes, h, w, out_h and out_w must be positive");
  if (a->mode < SDK_RESIZE_NEAREST || a->mode > SDK_RESIZE_AREA) return fail(SDK_EINVAL, "resize2d: unknown mode");
  if (!(a->scale_h > 0.0) || !(a->scale_w > 0.0) || !std::isfinite(a->scale_h) || !std::isfinite(a->scale_w))
    return fail(SDK_EINVAL, "resize2d: scale factors must be positive and finite");
  if ((double)a->out_h != std::floor((double)a->h * a->scale_h) ||
      (double)a->out_w != std::floor((double)a->w * a->scale_w))
    return fail(SDK_EINVAL, "resize2d: out_h / out_w must be floor(in * scale_factor)");
  const int64_t n = (int64_t)a->planes * a->out_h * a->out_w;
  const int64_t blocks = (n + 255) / 256;
  if (blocks > 0x7fffffffLL) return fail(SDK_EINVAL, "resize2d: grid too large");
  // compute_scales_value: the step between source samples is the float of 1 / scale_factor
  const float sh = (float)(1.0 / a->scale_h), sw = (float)(1.0 / a->scale_w);
  const dim3 g((unsigned)blocks), b(256);
  hipStream_t s = (hipStream_t)stream;
  switch (a->mode) {
    case SDK_RESIZE_NEAREST:
      hipLaunchKernelGGL(resize2d_kernel<SDK_RESIZE_NEAREST>, g, b, 0, s, a->x, a->y, a->h, a->w, a->out_h, a->out_w,
                         sh, sw, n);
      break;
    case SDK_RESIZE_BILINEAR:
      hipLaunchKernelGGL(resize2d_kernel<SDK_RESIZE_BILINEAR>, g, b, 0, s, a->x, a->y, a->h, a->w, a->out_h,
                         a->out_w, sh, sw, n);
      break;
    case SDK_RESIZE_BICUBIC:
      hipLaunchKernelGGL(resize2d_kernel<SDK_RESIZE_BICUBIC>, g, b, 0, s, a->x, a->y, a->h, a->w, a->out_h, a->out_w,
                         sh, sw, n);
      break;
    default:
      hipLaunchKernelGGL(resize2d_kernel<SDK_RESIZE_AREA>, g, b, 0, s, a->x, a->y, a->h, a->w, a->out_h, a->out_w, sh,
                         sw, n);
  }
  return check_launch("resize2d");
}
