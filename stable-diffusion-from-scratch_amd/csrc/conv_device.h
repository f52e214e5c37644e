// Device helpers shared by the conv tile kernels (conv_tile.h) and the small kernels (conv_small.hip).
#pragma once
#include "conv.h"

namespace sdk {
namespace {

// Phase form: output row (pixel index of the 2ho x 2wo NHWC output) of GEMM row m, or -1 for a padding row
__device__ __forceinline__ int phase_out_row(const Params& p, int m) {
  const int ph = m / p.ph_rows_pad, rp = m - ph * p.ph_rows_pad;
  if (ph > 3 || rp >= p.ph_rows) return -1;
  const int img = rp / p.hw_out, rem = rp - img * p.hw_out;
  const int i = rem / p.wo, j = rem - i * p.wo;
  return (img * 2 * p.ho + 2 * i + (ph >> 1)) * (2 * p.wo) + 2 * j + (ph & 1);
}

// the output row an epilogue stores GEMM row m to (-1: none).  PH: compiled with the phase form (only the
// linear-issue conv_glds_kernel and the split-K reduces; everything else keeps its code)
template <bool PH>
__device__ __forceinline__ int out_row(const Params& p, int m) {
  if (PH && p.phase) return phase_out_row(p, m);
  return m < p.M ? m : -1;
}

// diagnostics build: s_memtime at kernel entry / after the prologue / after the K loop / at the end (+ after
// epilogue groups 0-3 at 4-7), by
// thread 0 of every workgroup (sdk_diag_conv_stamps copies them out); compiled out of the product library
// SDK_CONV_STAMPS=2: slots 6 / 7 hold s_memrealtime (100 MHz) at entry / end instead of epilogue groups 2 / 3, so the
// shader clock the workgroup ran at is (memtime end - entry) / (realtime end - entry) x 100 MHz (MI355X_MICROARCH.md
// 'DVFS give-back' item 6)
__device__ __forceinline__ void ph_stamp(const Params& p, int i) {
#ifdef SDK_CONV_DIAGNOSTICS
  if (p.stamps && threadIdx.x == 0) {
    const size_t wg = ((size_t)blockIdx.x + (size_t)blockIdx.y * gridDim.x) * 8;
    if (p.stamps_rt && i >= 6) return;
    p.stamps[wg + i] = __builtin_amdgcn_s_memtime();
    if (p.stamps_rt && (i == 0 || i == 3)) p.stamps[wg + (i == 0 ? 6 : 7)] = __builtin_amdgcn_s_memrealtime();
  }
#endif
}

// epilogue activation: CLIP's quick_gelu x*sigmoid(1.702x) (transformers activations.py QuickGELUActivation) or the
// exact GELU of nn.GELU() (OpenCLIP's MLP) through gelu_erf, the library's one erf (common.h).  ERF = false compiles
// the erf branch out, for a kernel whose launcher sends SDK_ACT_GELU to an instantiation of its own
template <bool ERF = true>
__device__ __forceinline__ float act_fn(int act, float x) {
  if (act == SDK_ACT_QUICK_GELU) return x * __builtin_amdgcn_rcpf(1.0f + __expf(-1.702f * x));
  if (ERF && act == SDK_ACT_GELU) return gelu_erf(x);
  return x;
}

__device__ __forceinline__ int swz(int row, int chunk) {   // element offset inside a [128][64] tile
  return row * BK + ((chunk ^ ((row >> 1) & 7)) << 3);
}

__device__ __forceinline__ h8 ldg16(const half_t* p) { return *reinterpret_cast<const h8*>(p); }

// fp16 output row stores of the epilogues (SDK_STORE_HINT=1: non-temporal; 2: no store — A/B builds only)
__device__ __forceinline__ void st_out16(half_t* p, const h8& v) {
#if defined(SDK_STORE_HINT) && SDK_STORE_HINT == 1
  __builtin_nontemporal_store(v, reinterpret_cast<h8*>(p));
#elif defined(SDK_STORE_HINT) && SDK_STORE_HINT == 2
  asm volatile("" ::"v"(v), "v"(p));   // A/B build only: the whole epilogue but its global stores
#else
  *reinterpret_cast<h8*>(p) = v;
#endif
}

}  // namespace
}  // namespace sdk
