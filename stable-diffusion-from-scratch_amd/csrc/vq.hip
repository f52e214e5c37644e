// Vector-quantiser kernels (vqvae/quantize.py VectorQuantize2): fused nearest-code search, codebook
// lookup and index remap.  All fp32.
//
// Nearest code: the reference builds d = |z|^2 + |e|^2 - 2 z.e as an [M, N] fp32 matrix and takes its
// argmin.  Here a row's scores s_j = |e_j|^2 - 2 z.e_j (the per-row constant |z|^2 dropped: same
// argmin, smaller magnitude) are produced tile by tile and folded into a running (min, index) that
// never leaves registers.  z is read in place from NCHW: row m = (b, y, x), element c at stride H*W.
//   D <= 8: one row per thread, z row in registers, the codebook streamed through LDS pre-scaled by -2
//           with |e|^2 in the slot after it, D FMAs + compare per code (every lane reads the same LDS
//           address: a broadcast).
//   D  > 8: v_mfma_f32_32x32x2_f32 (exact fp32, k-ordered fma chain).  A wave owns 32 rows whose z
//           fragments stay in registers for the whole search (D <= 256); code tiles go through LDS in
//           the instruction's operand order; each lane keeps (min, index) for its 16 rows x its
//           code column, reduced over the 32 columns at the very end.
// Ties: codes are visited in ascending order with a strict "<", and every cross-lane / cross-workgroup
// combine is a min over the 64-bit key (order-preserving score bits << 32 | index), so the lowest
// index wins among equal scores (torch.argmin's rule) and the result does not depend on launch
// geometry or timing.  A NaN score never replaces the running minimum, so a NaN row still yields an
// index in [0, N).
// Small M: the codebook is split over blockIdx.y, the partial winners meet in a global atomicMin on
// the key, and a second tiny pass decodes the key and writes z_q.
// z_q = z + (e - z), two roundings (the reference's straight-through line), contraction off.
#include <cmath>

#include "common.h"

#pragma clang fp contract(off)

namespace sdk {
namespace {

constexpr int VQ_VALU_CH = 512;      // codes per LDS chunk, VALU form
constexpr int VQ_MFMA_LDS = 8192;    // floats of code tile, MFMA form (32 KB)
constexpr int VQ_MFMA_MAXCT = 256;

__device__ __forceinline__ unsigned long long vq_key(float s, int idx) {
  s = s + 0.0f;                      // -0 -> +0: equal scores must have equal keys
  unsigned u = __float_as_uint(s);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)u << 32) | (unsigned)idx;
}

__global__ void __launch_bounds__(256) vq_code_norms_kernel(const float* cb, float* norms, int N, int D) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= N) return;
  float s = 0.f;
  for (int c = 0; c < D; ++c) {
    const float v = cb[(int64_t)j * D + c];
    s = __builtin_fmaf(v, v, s);
  }
  norms[j] = s;
}

template <int D>
__global__ void __launch_bounds__(256) vq_nearest_valu_kernel(const float* __restrict__ z,
                                                              const float* __restrict__ cb,
                                                              const float* __restrict__ norms,
                                                              int64_t* __restrict__ idx, float* __restrict__ zq,
                                                              unsigned long long* __restrict__ keys, int64_t M, int N,
                                                              int HW, int cps) {
  constexpr int DP = (D + 1 + 3) / 4 * 4;
  __shared__ float tile[VQ_VALU_CH * DP];
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = m < M;
  const int64_t mm = live ? m : M - 1;          // dead lanes load a valid row and store nothing
  const int64_t b = mm / HW;
  const int64_t off = b * D * HW + (mm - b * HW);
  float zr[D];
#pragma unroll
  for (int c = 0; c < D; ++c) zr[c] = z[off + (int64_t)c * HW];
  const int c0 = blockIdx.y * cps, c1 = min(N, c0 + cps);
  float best = INFINITY;
  int bi = c0;
  for (int base = c0; base < c1; base += VQ_VALU_CH) {
    const int cnt = min(VQ_VALU_CH, c1 - base);
    __syncthreads();
    for (int t = threadIdx.x; t < cnt * DP; t += blockDim.x) {
      const int j = t / DP, c = t - j * DP;
      float v = 0.f;
      if (c < D) v = -2.f * cb[(int64_t)(base + j) * D + c];
      else if (c == D) v = norms[base + j];
      tile[t] = v;
    }
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < cnt; ++j) {
      const float* e = tile + j * DP;
      float s = e[D];
#pragma unroll
      for (int c = 0; c < D; ++c) s = __builtin_fmaf(zr[c], e[c], s);
      if (s < best) {
        best = s;
        bi = base + j;
      }
    }
  }
  if (!live) return;
  if (keys) {
    atomicMin(&keys[m], vq_key(best, bi));
    return;
  }
  idx[m] = bi;
#pragma unroll
  for (int c = 0; c < D; ++c) {
    const float ev = cb[(int64_t)bi * D + c];
    const float t = ev - zr[c];
    zq[off + (int64_t)c * HW] = zr[c] + t;
  }
}

// KS: k-steps (of 2) whose A fragments are held in registers, D <= 2 * KS
template <int KS>
__global__ void __launch_bounds__(256) vq_nearest_mfma_kernel(const float* __restrict__ z,
                                                              const float* __restrict__ cb,
                                                              const float* __restrict__ norms,
                                                              int64_t* __restrict__ idx, float* __restrict__ zq,
                                                              unsigned long long* __restrict__ keys, int64_t M, int N,
                                                              int D, int HW, int cps, int CT) {
  __shared__ float Bs[VQ_MFMA_LDS];
  __shared__ float Ns[VQ_MFMA_MAXCT];
  __shared__ int widx[4][32];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int nks = (D + 1) / 2, Dp = 2 * nks;
  const int64_t row0 = ((int64_t)blockIdx.x * (blockDim.x >> 6) + wave) * 32;
  float a[KS];
  {
    const int64_t m = row0 + r;
    const bool live = m < M;
    const int64_t mm = live ? m : 0;
    const int64_t b = mm / HW;
    const float* zp = z + b * D * HW + (mm - b * HW);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int k = 2 * ks + h;
      a[ks] = (live && k < D) ? zp[(int64_t)k * HW] : 0.f;
    }
  }
  const int c0 = blockIdx.y * cps, c1 = min(N, c0 + cps);
  float best[16];
  int bi[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    best[i] = INFINITY;
    bi[i] = c0;
  }
  for (int base = c0; base < c1; base += CT) {
    __syncthreads();
    // code tile in operand order: sub-tile s of 32 codes, k-step ks -> 64 floats [code & 31][k & 1]
    for (int t = threadIdx.x; t < CT * Dp; t += blockDim.x) {
      const int j = t / Dp, k = t - j * Dp;
      const int code = base + j;
      const float v = (code < c1 && k < D) ? cb[(int64_t)code * D + k] : 0.f;
      Bs[((j >> 5) * nks + (k >> 1)) * 64 + (j & 31) * 2 + (k & 1)] = v;
    }
    for (int t = threadIdx.x; t < CT; t += blockDim.x) Ns[t] = base + t < c1 ? norms[base + t] : INFINITY;
    __syncthreads();
    const int nsub = (min(CT, c1 - base) + 31) / 32;
    for (int s = 0; s < nsub; ++s) {
      f16v acc;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.f;
      const float* bp = Bs + s * nks * 64 + r * 2 + h;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        if (ks < nks) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ks], bp[ks * 64], acc, 0, 0, 0);
      const float nrm = Ns[s * 32 + r];
      const int code = base + s * 32 + r;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float sc = __builtin_fmaf(-2.f, acc[i], nrm);
        if (sc < best[i]) {
          best[i] = sc;
          bi[i] = code;
        }
      }
    }
  }
  // accumulator register i of lane (r, h) is row (i & 3) + 8 (i >> 2) + 4 h, column r: min over r
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    unsigned long long key = vq_key(best[i], bi[i]);
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) {
      const unsigned long long other = __shfl_xor(key, o);
      key = other < key ? other : key;
    }
    const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
    if (r == 0) {
      if (keys) {
        if (row0 + row < M) atomicMin(&keys[row0 + row], key);
      } else {
        widx[wave][row] = (int)(unsigned)key;
      }
    }
  }
  if (keys) return;
  __syncthreads();
  for (int t = lane; t < 32 * D; t += 64) {
    const int rr = t & 31, c = t >> 5;
    const int64_t m = row0 + rr;
    if (m >= M) continue;
    const int id = widx[wave][rr];
    const int64_t b = m / HW;
    const int64_t o = (b * D + c) * HW + (m - b * HW);
    const float zv = z[o];
    const float ev = cb[(int64_t)id * D + c];
    const float d = ev - zv;
    zq[o] = zv + d;
    if (c == 0) idx[m] = id;
  }
}

// split path, second pass: key -> index, z_q
__global__ void __launch_bounds__(256) vq_finalize_kernel(const float* __restrict__ z, const float* __restrict__ cb,
                                                          const unsigned long long* __restrict__ keys,
                                                          int64_t* __restrict__ idx, float* __restrict__ zq, int N,
                                                          int D, int HW, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += stride) {
    const int64_t p = e % HW;
    const int64_t bc = e / HW;
    const int c = (int)(bc % D);
    const int64_t m = (bc / D) * HW + p;
    const unsigned id = min((unsigned)keys[m], (unsigned)(N - 1));
    const float zv = z[e];
    const float ev = cb[(int64_t)id * D + c];
    const float d = ev - zv;
    zq[e] = zv + d;
    if (c == 0) idx[m] = id;
  }
}

// out[m][c] (nchw = 0) or out[b][c][p] (nchw = 1) = codebook[idx[m]][c]; the host range-checks idx,
// an index outside [0, N) reads nothing and yields 0
__global__ void __launch_bounds__(256) vq_lookup_kernel(const int64_t* __restrict__ idx, const float* __restrict__ cb,
                                                        float* __restrict__ out, int N, int D, int HW, int nchw,
                                                        int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += stride) {
    int64_t m;
    int c;
    if (nchw) {
      const int64_t p = e % HW, bc = e / HW;
      c = (int)(bc % D);
      m = (bc / D) * HW + p;
    } else {
      m = e / D;
      c = (int)(e - m * D);
    }
    const int64_t id = idx[m];
    out[e] = (id >= 0 && id < N) ? cb[id * D + c] : 0.f;
  }
}

// mode 0 (remap_to_used): position of the first entry of used[] equal to the index, else rnd[i] when
// rnd is given, else `unknown`.  mode 1 (unmap_to_all): used[index]; with `extra` an index >= U maps
// to used[0] first (the reference's "simply set to zero")
__global__ void __launch_bounds__(256) vq_remap_kernel(const int64_t* __restrict__ inds,
                                                       const int64_t* __restrict__ used,
                                                       const int64_t* __restrict__ rnd, int64_t* __restrict__ out,
                                                       int64_t n, int U, int mode, int64_t unknown, int extra) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) {
    int64_t v = inds[i];
    if (mode == 0) {
      int64_t pos = -1;
      for (int u = U - 1; u >= 0; --u)
        if (used[u] == v) pos = u;
      out[i] = pos >= 0 ? pos : (rnd ? rnd[i] : unknown);
    } else {
      if (extra && v >= U) v = 0;
      out[i] = (v >= 0 && v < U) ? used[v] : 0;
    }
  }
}

struct VqPlan {
  int mfma, block, rows_per_block, ct, splits, cps;
  int64_t row_blocks;
};

bool vq_plan(int64_t M, int N, int D, int force_splits, VqPlan& p) {
  if (M <= 0 || N <= 0 || D <= 0 || D > 256 || M > 0x7fffffffLL * 32) return false;
  p.mfma = D > 8;
  int unit;
  if (p.mfma) {
    const int Dp = (D + 1) / 2 * 2;
    p.ct = std::min(VQ_MFMA_MAXCT, VQ_MFMA_LDS / Dp / 32 * 32);
    const int waves = (int)std::min<int64_t>(4, (M + 31) / 32);
    p.block = 64 * waves;
    p.rows_per_block = 32 * waves;
    unit = p.ct;
  } else {
    p.ct = VQ_VALU_CH;
    p.block = (int)std::min<int64_t>(256, (M + 63) / 64 * 64);
    p.rows_per_block = p.block;
    unit = 256;
  }
  p.row_blocks = (M + p.rows_per_block - 1) / p.rows_per_block;
  const int max_splits = (N + unit - 1) / unit;
  int want = 1;
  if (force_splits > 0) want = force_splits;
  else if (p.row_blocks < 256) want = (int)((512 + p.row_blocks - 1) / p.row_blocks);
  want = std::max(1, std::min(want, max_splits));
  p.cps = ((N + want - 1) / want + unit - 1) / unit * unit;
  p.splits = (N + p.cps - 1) / p.cps;
  return p.row_blocks <= 0x7fffffffLL && p.splits <= 65535;
}

}  // namespace
}  // namespace sdk

using namespace sdk;

extern "C" int sdk_vq_code_norms(const float* codebook, float* norms, int32_t n, int32_t d, sdk_stream_t stream) {
  if (!codebook || !norms || n <= 0 || d <= 0) return fail(SDK_EINVAL, "vq_code_norms: bad args");
  hipLaunchKernelGGL(vq_code_norms_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, codebook, norms,
                     n, d);
  return check_launch("vq_code_norms");
}

extern "C" int32_t sdk_vq_nearest_splits(int64_t m, int32_t n, int32_t d) {
  VqPlan p;
  return vq_plan(m, n, d, 0, p) ? p.splits : 0;
}

extern "C" int sdk_vq_nearest(const float* z, const float* codebook, const float* norms, int64_t* idx, float* z_q,
                              int32_t batch, int32_t d, int32_t hw, int32_t n, void* keys, int64_t keys_bytes,
                              int32_t force_splits, sdk_stream_t stream) {
  if (!z || !codebook || !norms || !idx || !z_q || batch <= 0 || hw <= 0)
    return fail(SDK_EINVAL, "vq_nearest: bad args");
  const int64_t M = (int64_t)batch * hw;
  VqPlan p;
  if (!vq_plan(M, n, d, force_splits, p))
    return fail(SDK_EINVAL, "vq_nearest: unsupported shape (1 <= e_dim <= 256, n_e >= 1)");
  unsigned long long* k = nullptr;
  hipStream_t st = (hipStream_t)stream;
  if (p.splits > 1) {
    if (!keys || keys_bytes < M * 8) return fail(SDK_EWORKSPACE, "vq_nearest: split path needs 8 bytes per row of keys");
    k = (unsigned long long*)keys;
    if (hipMemsetAsync(k, 0xFF, (size_t)M * 8, st) != hipSuccess) return fail(SDK_EHIP, "vq_nearest: memset failed");
  }
  const dim3 grid((unsigned)p.row_blocks, (unsigned)p.splits), block(p.block);
#define VQ_VALU(DD)                                                                                               \
  case DD:                                                                                                        \
    hipLaunchKernelGGL(vq_nearest_valu_kernel<DD>, grid, block, 0, st, z, codebook, norms, idx, z_q, k, M, n, hw, \
                       p.cps);                                                                                    \
    break;
#define VQ_MFMA(KS)                                                                                                  \
  hipLaunchKernelGGL(vq_nearest_mfma_kernel<KS>, grid, block, 0, st, z, codebook, norms, idx, z_q, k, M, n, d, hw, \
                     p.cps, p.ct)
  if (!p.mfma) {
    switch (d) {
      VQ_VALU(1) VQ_VALU(2) VQ_VALU(3) VQ_VALU(4) VQ_VALU(5) VQ_VALU(6) VQ_VALU(7) VQ_VALU(8)
    }
  } else if (d <= 32) {
    VQ_MFMA(16);
  } else if (d <= 64) {
    VQ_MFMA(32);
  } else if (d <= 128) {
    VQ_MFMA(64);
  } else {
    VQ_MFMA(128);
  }
#undef VQ_VALU
#undef VQ_MFMA
  int rc = check_launch("vq_nearest");
  if (rc != SDK_OK || !k) return rc;
  const int64_t ne = M * d;
  const int blocks = (int)std::min<int64_t>((ne + 255) / 256, 4096);
  hipLaunchKernelGGL(vq_finalize_kernel, dim3(blocks), dim3(256), 0, st, z, codebook, k, idx, z_q, n, d, hw, ne);
  return check_launch("vq_nearest finalize");
}

extern "C" int sdk_vq_lookup(const int64_t* idx, const float* codebook, float* out, int64_t m, int32_t n, int32_t d,
                             int32_t hw, int32_t nchw, sdk_stream_t stream) {
  if (!idx || !codebook || !out || m <= 0 || n <= 0 || d <= 0 || (nchw && (hw <= 0 || m % hw)))
    return fail(SDK_EINVAL, "vq_lookup: bad args");
  const int64_t ne = m * d;
  const int blocks = (int)std::min<int64_t>((ne + 255) / 256, 4096);
  hipLaunchKernelGGL(vq_lookup_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, idx, codebook, out, n, d,
                     nchw ? hw : 1, nchw, ne);
  return check_launch("vq_lookup");
}

extern "C" int sdk_vq_remap(const int64_t* inds, const int64_t* used, const int64_t* rnd, int64_t* out, int64_t count,
                            int32_t n_used, int32_t mode, int64_t unknown, int32_t extra, sdk_stream_t stream) {
  if (!inds || !used || !out || count <= 0 || n_used <= 0 || (mode != 0 && mode != 1))
    return fail(SDK_EINVAL, "vq_remap: bad args");
  const int blocks = (int)std::min<int64_t>((count + 255) / 256, 4096);
  hipLaunchKernelGGL(vq_remap_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, inds, used, rnd, out, count,
                     n_used, mode, unknown, extra);
  return check_launch("vq_remap");
}
