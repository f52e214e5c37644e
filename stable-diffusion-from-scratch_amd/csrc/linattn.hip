// Linear attention for gfx950 (Unet/attention.py LinearAttention): per (batch, head)
//   ctx[d][e] = sum_n softmax_n(k)[n][d] v[n][e],   out[n][e] = sum_d q[n][d] ctx[d][e]
// fp16 I/O, fp32 accumulation, v_mfma_f32_32x32x16_f16.  Three launches, no floating-point atomics and a
// fixed summation order everywhere, so two evaluations agree bit for bit.
//
//  1. linattn_context_kernel: one workgroup (4 waves) per (token chunk, 32 columns d, batch*head).  A first
//     pass over the chunk's k finds the column maxima m_c[d] of k*log2(e).  The second pass walks the chunk in
//     tiles of 32 tokens: P = exp2(k*log2(e) - m_c) is rounded to fp16 and stored TRANSPOSED in LDS
//     ([d][token], the layout attention_wide.hip keeps its P in), V row-major; ctx_c^T (rows e, columns d) +=
//     V^T P is the PV product of the attention kernels with "query" = column d: V^T by ds_read_b64_tr_b16, P
//     by ds_read_b64, the waves split e.  The column sums den_c come from the fp32 P of the same pass.
//     (m_c, den_c, ctx_c^T) go to the workspace.
//  2. linattn_combine_kernel: elementwise over [e][d]: the chunks in ascending order, each weighted by
//     exp2(m_c - max_c m_c); ctx / den rounded to fp16, kept transposed ([e][d]) for the apply GEMM.
//  3. linattn_apply_kernel: out^T (rows e, columns n) = ctx^T q^T: both fragments are 16-B row reads (ctx^T
//     rows from L2, q rows from global), no LDS; 4 waves x 32 tokens, 128 columns e per workgroup.
// Memory- and launch-bound at the first stage's sizes (4 GF per 512^2 image at C = 512); not tuned further.
#include <algorithm>

#include "common.h"

namespace sdk {
namespace {

typedef __fp16 fp16x4_t __attribute__((ext_vector_type(4)));

constexpr float LOG2E = 1.4426950408889634f;
constexpr int LT = 32;             // tokens per tile of the context kernel
constexpr int LPLD = LT + 4;       // P^T row pitch (halfs): 72 B
constexpr int LVLD_MAX = 512 + 32;
constexpr int MAX_CHUNKS = 8;

struct LinParams {
  const half_t* q;
  const half_t* k;
  const half_t* v;
  half_t* o;
  int q_ld, k_ld, v_ld, o_ld;
  int batch, heads, n, d;
  int chunk, nchunks;   // tokens per chunk (a multiple of LT), chunks
  float* ws_m;          // [bh][chunk][d]
  float* ws_den;        // [bh][chunk][d]
  float* ws_ctx;        // [bh][chunk][e][d]
  half_t* ctx_t;        // [bh][e][d]
};

int chunk_tokens(int n) {
  const int want = std::min(MAX_CHUNKS, (n + 63) / 64);
  const int per = (n + want - 1) / want;
  return (per + LT - 1) / LT * LT;
}

__global__ void __launch_bounds__(256) linattn_context_kernel(LinParams p) {
  __shared__ __attribute__((aligned(16))) half_t Vs[LT * LVLD_MAX];
  __shared__ __attribute__((aligned(16))) half_t Pt[32 * LPLD];
  __shared__ float red[64 * 32];
  __shared__ float mcol[32];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = blockIdx.x, d0 = blockIdx.y * 32, bh = blockIdx.z;
  const int head = bh % p.heads, b = bh / p.heads;
  const int D = p.d;
  const int n0 = c * p.chunk, n1 = min(p.n, n0 + p.chunk);
  const int Dp = (D + 31) & ~31;
  const int VLD = ((Dp * 2 / 64) % 2 == 0) ? Dp + 32 : Dp;     // 64 or 192 B mod 256
  const int nchv = D >> 3;
  const size_t rowbase = (size_t)b * p.n;

  // V padding columns [D, VLD): zero once, the staged chunks never touch them
  {
    const int vpad = VLD / 8 - nchv;
    for (int e = tid; e < LT * vpad; e += 256) {
      const int row = e / vpad, cc = nchv + e - row * vpad;
      *reinterpret_cast<h8*>(Vs + row * VLD + cc * 8) = h8{};
    }
  }

  // ---- pass 1: column maxima of k*log2(e) over the chunk; thread = (token lane tl, 8 columns cc)
  const int tl = tid >> 2, cc = tid & 3;
  const bool colok = d0 + cc * 8 < D;           // D % 8 == 0: a chunk of 8 columns is whole or absent
  const half_t* kcol = p.k + head * D + d0 + cc * 8;
  float mx[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) mx[j] = -3.0e38f;
  if (colok)
    for (int n = n0 + tl; n < n1; n += 64) {
      const h8 kv = *reinterpret_cast<const h8*>(kcol + (rowbase + n) * p.k_ld);
#pragma unroll
      for (int j = 0; j < 8; ++j) mx[j] = fmaxf(mx[j], (float)kv[j] * LOG2E);
    }
#pragma unroll
  for (int j = 0; j < 8; ++j) red[tl * 32 + cc * 8 + j] = mx[j];
  __syncthreads();
  if (tid < 32) {
    float m = red[tid];
    for (int i = 1; i < 64; ++i) m = fmaxf(m, red[i * 32 + tid]);
    mcol[tid] = m;
  }
  __syncthreads();
  float mloc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) mloc[j] = mcol[cc * 8 + j];

  // ---- pass 2
  const int EB = Dp / 32;                        // 32-column blocks of e; wave w owns blocks w, w+4, ..
  f16v acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = f16v{};
  float dsum[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) dsum[j] = 0.f;
  const int fr = lane & 31, fh = lane >> 5, g = lane >> 4;
  const int q4 = (lane & 15) >> 2, pp = lane & 3;
  const int vrow_off = 4 * (g >> 1) + q4;
  const int vcol_off = 16 * (g & 1) + 4 * pp;

  for (int s0 = n0; s0 < n1; s0 += LT) {
    // P^T tile: threads 0..127 = (token tl < 32, 8 columns)
    if (tid < 128) {
      const int n = s0 + tl;
      h8 kv = {};
      const bool ok = colok && n < n1;
      if (ok) kv = *reinterpret_cast<const h8*>(kcol + (rowbase + n) * p.k_ld);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float e = ok ? __builtin_amdgcn_exp2f((float)kv[j] * LOG2E - mloc[j]) : 0.f;
        dsum[j] += e;
        Pt[(cc * 8 + j) * LPLD + tl] = (half_t)e;
      }
    }
    // V tile: 32 tokens x D columns, zero rows past the chunk
    for (int e = tid; e < LT * nchv; e += 256) {
      const int row = e / nchv, ch = e - row * nchv;
      h8 vv = {};
      if (s0 + row < n1) vv = *reinterpret_cast<const h8*>(p.v + (rowbase + s0 + row) * p.v_ld + head * D + ch * 8);
      *reinterpret_cast<h8*>(Vs + row * VLD + ch * 8) = vv;
    }
    __syncthreads();
    // element j of lane half fh in k-step ks is token 16ks + 8(j>>2) + 4fh + (j&3), on both operands
    h8 pf[LT / 16];
#pragma unroll
    for (int ks = 0; ks < LT / 16; ++ks) {
      const half_t* pr = Pt + fr * LPLD + 16 * ks + 4 * fh;
      const h4 lo = *reinterpret_cast<const h4*>(pr), hi = *reinterpret_cast<const h4*>(pr + 8);
      pf[ks] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int eb = wave + 4 * i;
      if (eb < EB) {
#pragma unroll
        for (int ks = 0; ks < LT / 16; ++ks) {
          const half_t* base = Vs + (16 * ks + vrow_off) * VLD + 32 * eb + vcol_off;
          const fp16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4_t*)(base));
          const fp16x4_t hi =
              __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4_t*)(base + 8 * VLD));
          const h4 lo4 = __builtin_bit_cast(h4, lo), hi4 = __builtin_bit_cast(h4, hi);
          const h8 a = __builtin_shufflevector(lo4, hi4, 0, 1, 2, 3, 4, 5, 6, 7);
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, pf[ks], acc[i], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

  // ---- partials: column sums (token lanes in ascending order), maxima, ctx_c^T
  if (tid < 128) {
#pragma unroll
    for (int j = 0; j < 8; ++j) red[tl * 32 + cc * 8 + j] = dsum[j];
  }
  __syncthreads();
  const size_t part = (size_t)bh * p.nchunks + c;
  if (tid < 32 && d0 + tid < D) {
    float s = red[tid];
    for (int i = 1; i < 32; ++i) s += red[i * 32 + tid];
    p.ws_den[part * D + d0 + tid] = s;
    p.ws_m[part * D + d0 + tid] = mcol[tid];
  }
  if (d0 + fr < D) {
    float* cw = p.ws_ctx + part * D * D + d0 + fr;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int eb = wave + 4 * i;
      if (eb < EB) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int e = eb * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
          if (e < D) cw[(size_t)e * D] = acc[i][r];
        }
      }
    }
  }
}

__global__ void __launch_bounds__(256) linattn_combine_kernel(LinParams p) {
  const int D = p.d, bh = blockIdx.y;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= D * D) return;
  const int d = idx % D;
  const size_t part0 = (size_t)bh * p.nchunks;
  float m = p.ws_m[part0 * D + d];
  for (int c = 1; c < p.nchunks; ++c) m = fmaxf(m, p.ws_m[(part0 + c) * D + d]);
  float den = 0.f, num = 0.f;
  for (int c = 0; c < p.nchunks; ++c) {
    const float w = __builtin_amdgcn_exp2f(p.ws_m[(part0 + c) * D + d] - m);
    den += w * p.ws_den[(part0 + c) * D + d];
    num += w * p.ws_ctx[(part0 + c) * D * D + idx];
  }
  p.ctx_t[(size_t)bh * D * D + idx] = (half_t)(num * (1.f / den));
}

__global__ void __launch_bounds__(256) linattn_apply_kernel(LinParams p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 31, fh = lane >> 5;
  const int D = p.d, bh = blockIdx.z;
  const int head = bh % p.heads, b = bh / p.heads;
  const int n = blockIdx.x * 128 + wave * 32 + fr;     // B operand: column = token
  const int e0 = blockIdx.y * 128;
  const bool nok = n < p.n;
  const half_t* qrow = p.q + ((size_t)b * p.n + (nok ? n : 0)) * p.q_ld + head * D;
  const half_t* ct = p.ctx_t + (size_t)bh * D * D;
  f16v acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = f16v{};
  for (int k0 = 0; k0 < D; k0 += 16) {
    const int kk = k0 + 8 * fh;
    h8 bq = {};
    if (nok && kk < D) bq = *reinterpret_cast<const h8*>(qrow + kk);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = e0 + 32 * i + fr;                  // A operand: row = e
      h8 a = {};
      if (e < D && kk < D) a = *reinterpret_cast<const h8*>(ct + (size_t)e * D + kk);
      acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bq, acc[i], 0, 0, 0);
    }
  }
  if (nok) {
    half_t* op = p.o + ((size_t)b * p.n + n) * p.o_ld + head * D;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int gg = 0; gg < 4; ++gg) {
        const int e = e0 + 32 * i + 8 * gg + 4 * fh;
        if (e < D) {
          h4 w;
#pragma unroll
          for (int j = 0; j < 4; ++j) w[j] = (half_t)acc[i][4 * gg + j];
          *reinterpret_cast<h4*>(op + e) = w;
        }
      }
  }
}

int validate(const sdk_linear_attention_args* a) {
  if (!a) return fail(SDK_EINVAL, "linear_attention: null arguments");
  if (a->dim_head <= 0 || a->dim_head % 8 || a->dim_head > 512)
    return fail(SDK_EINVAL, "linear_attention: dim_head must be a multiple of 8 in [8, 512]");
  if (a->n <= 0 || a->batch <= 0 || a->heads <= 0) return fail(SDK_EINVAL, "linear_attention: empty");
  if ((long long)a->batch * a->heads > 65535) return fail(SDK_EINVAL, "linear_attention: batch*heads exceeds 65535");
  return SDK_OK;
}

struct WsLayout {
  long long m, den, ctx, ctx_t, bytes;   // byte offsets
};
WsLayout ws_layout(const sdk_linear_attention_args* a) {
  const long long bh = (long long)a->batch * a->heads, D = a->dim_head;
  const long long nc = (a->n + chunk_tokens(a->n) - 1) / chunk_tokens(a->n);
  auto up = [](long long x) { return (x + 255) / 256 * 256; };
  WsLayout w;
  w.m = 0;
  w.den = up(bh * nc * D * 4);
  w.ctx = w.den + up(bh * nc * D * 4);
  w.ctx_t = w.ctx + up(bh * nc * D * D * 4);
  w.bytes = w.ctx_t + up(bh * D * D * 2);
  return w;
}

}  // namespace
}  // namespace sdk

using namespace sdk;

extern "C" int32_t sdk_linear_attention_chunks(int32_t n) {
  if (n <= 0) return 0;
  const int ch = chunk_tokens(n);
  return (n + ch - 1) / ch;
}

extern "C" int64_t sdk_linear_attention_workspace_bytes(const sdk_linear_attention_args* a) {
  if (validate(a) != SDK_OK) return -1;
  return ws_layout(a).bytes;
}

extern "C" int sdk_linear_attention(const sdk_linear_attention_args* a, sdk_stream_t stream) {
  const int rc = validate(a);
  if (rc != SDK_OK) return rc;
  if (!a->q || !a->k || !a->v || !a->o || !a->workspace) return fail(SDK_EINVAL, "linear_attention: null pointer");
  if (a->q_ld % 8 || a->k_ld % 8 || a->v_ld % 8 || a->o_ld % 4)
    return fail(SDK_EINVAL, "linear_attention: row strides must be multiples of 8 (o: 4)");
  const long long C = (long long)a->heads * a->dim_head;
  if (C > a->q_ld || C > a->k_ld || C > a->v_ld || C > a->o_ld)
    return fail(SDK_EINVAL, "linear_attention: row stride smaller than heads*dim_head");
  if ((uintptr_t)a->workspace % 16) return fail(SDK_EINVAL, "linear_attention: workspace must be 16-B aligned");
  const WsLayout w = ws_layout(a);
  if (a->workspace_bytes < w.bytes) return fail(SDK_EINVAL, "linear_attention: workspace too small");
  char* ws = (char*)a->workspace;
  const int D = a->dim_head, bh = a->batch * a->heads;
  const int ch = chunk_tokens(a->n), nc = (a->n + ch - 1) / ch;
  LinParams p{(const half_t*)a->q, (const half_t*)a->k, (const half_t*)a->v, (half_t*)a->o,
              a->q_ld, a->k_ld, a->v_ld, a->o_ld, a->batch, a->heads, a->n, D, ch, nc,
              (float*)(ws + w.m), (float*)(ws + w.den), (float*)(ws + w.ctx), (half_t*)(ws + w.ctx_t)};
  hipStream_t s = (hipStream_t)stream;
  const long long ntile = ((long long)a->n + 127) / 128;
  if (ntile > 0x7fffffffLL) return fail(SDK_EINVAL, "linear_attention: grid too large");
  hipLaunchKernelGGL(linattn_context_kernel, dim3(nc, (D + 31) / 32, bh), dim3(256), 0, s, p);
  int r = check_launch("linattn_context");
  if (r != SDK_OK) return r;
  hipLaunchKernelGGL(linattn_combine_kernel, dim3((D * D + 255) / 256, bh), dim3(256), 0, s, p);
  r = check_launch("linattn_combine");
  if (r != SDK_OK) return r;
  hipLaunchKernelGGL(linattn_apply_kernel, dim3((unsigned)ntile, (D + 127) / 128, bh), dim3(256), 0, s, p);
  return check_launch("linattn_apply");
}
