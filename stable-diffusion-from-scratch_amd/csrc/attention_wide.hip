// Wide-head flash attention forward for gfx950 (form SDK_ATTN_WIDE, 168 <= head_dim <= 512): the one-head
// attention of the CompVis first stage (AttnBlock, C = 512).  Same arithmetic as attn_fwd_kernel
// (attention.hip): fp16 I/O, fp32 scores, Q pre-scaled by scale*log2(e), exp2, online softmax with the
// deferred max, P rounded to fp16 before the PV MFMA, fp32 O and row sum, one multiply by the fp32
// reciprocal at the end, tile 0 rescales nothing.
//
// What changes is who owns what.  attn_fwd_kernel gives a wave 32 query rows with the whole O^T
// (DV x 32 fp32) and the whole Q^T fragment set in registers: 256 + 128 registers per lane at d = 512.
// Here the 8 waves of a workgroup SHARE one block of 64 query rows:
//  * Q (pre-scaled) is staged once in LDS, 64 rows x (D + 8) halfs (65 KiB at D = 512);
//  * the score tile S^T (32 keys x 64 queries) is computed ONCE per workgroup, one 16-key x 16-query block
//    per wave (v_mfma_f32_16x16x32_f16 over the whole d, K and Q fragments by ds_read_b128); the two key
//    halves of a query meet through LDS (row max after the first barrier, row sum after the second);
//  * P goes to LDS as fp16 [query][key]; every wave's PV MFMA reads it as the B operand;
//  * O^T += V^T P^T is split over d: wave w owns columns [w D/8, (w + 1) D/8) of O for all 64 rows
//    (64 fp32 registers at D = 512); V stays row-major in LDS, V^T is read with ds_read_b64_tr_b16.
// K and V stream through a two-slot LDS ring (one K slot, one V slot, 32 keys each): while the score phase
// reads K_t the registers hold V_t and K_t+1 (buffer loads, the range check supplies the rows past nk),
// which are written after the first barrier (K_t is read, V_t-1 was read before that barrier) and are
// visible after the second; V_t+1 and K_t+2 are issued right behind.  Two barriers per 32-key tile.
// LDS at D = 512: Q 66560 + K 33280 + V 34816 + P 4608 + 1536 = 140800 B, one workgroup per CU.
// Row pitches: Q/K D + 8 halfs (16 B past a multiple of 256 B: the 16 rows of a ds_read_b128 group land on
// 16 different 16-B slots); V D + 32 halfs (64 B mod 256, as in attention.hip); P 36 halfs (72 B: the 32
// rows of a ds_read_b64 half-wave cover the 64 banks once).
#include "common.h"

namespace sdk {
namespace {

struct WideParams {
  const half_t* q;
  const half_t* k;
  const half_t* v;
  half_t* o;
  int q_ld, k_ld, v_ld, o_ld;
  int batch, heads, nq, nk, d;
  float c;              // scale * log2(e)
};

typedef __fp16 fp16x4_t __attribute__((ext_vector_type(4)));
typedef unsigned int u4 __attribute__((ext_vector_type(4)));

constexpr int WKT = SDK_ATTN_WIDE_KT;        // keys per tile
constexpr int WROWS = SDK_ATTN_WIDE_ROWS;    // query rows per workgroup
constexpr int WNW = 8, WNT = WNW * 64;
constexpr int PLD = WKT + 4;
constexpr float DEFER = 8.0f;                // exp2-domain headroom before the running max is raised
static_assert(WKT == 32 && WROWS == 64, "the wave -> (16 queries, 16 keys) score block map assumes 64 x 32");

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void* base, long long bytes) {
  const uint64_t a = (uint64_t)base;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
  const int n = __builtin_amdgcn_readfirstlane((int)bytes);
  return __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)hi << 32) | lo), 0, n, 0x00020000);
}

template <int D>
struct WideLds {
  static constexpr int QLD = D + 8;
  static constexpr int VLD = ((D * 2 / 64) % 2 == 0) ? D + 32 : D;
  static constexpr int Q_OFF = 0, K_OFF = Q_OFF + WROWS * QLD, V_OFF = K_OFF + WKT * QLD,
                       P_OFF = V_OFF + WKT * VLD, HALFS = P_OFF + WROWS * PLD;
  static constexpr int FLOATS = 6 * WROWS;   // pmax[2][64] psum[2][64] alpha[64] lfin[64]
  static constexpr int BYTES = HALFS * 2 + FLOATS * 4;
  static_assert((HALFS * 2) % 16 == 0, "float arrays behind the fp16 images stay 16-B aligned");
};

template <int D>
__global__ void __launch_bounds__(WNT) attn_wide_kernel(WideParams p) {
  using L = WideLds<D>;
  constexpr int QLD = L::QLD, VLD = L::VLD;
  constexpr int DVS = D / WNW;                   // O columns per wave
  constexpr int NDB = DVS / 32;
  constexpr int SL = WKT * (D / 8) / WNT;        // staging slots per thread (K and V each)
  static_assert(DVS % 32 == 0 && (WKT * (D / 8)) % WNT == 0, "D: a multiple of 256");
  extern __shared__ __attribute__((aligned(16))) half_t smem[];
  half_t* Qs = smem + L::Q_OFF;
  half_t* Ks = smem + L::K_OFF;
  half_t* Vs = smem + L::V_OFF;
  half_t* Ps = smem + L::P_OFF;
  float* fl = reinterpret_cast<float*>(smem + L::HALFS);
  float* pmax = fl;                 // [2][64]
  float* psum = fl + 2 * WROWS;     // [2][64]
  float* alph = fl + 4 * WROWS;     // [64]
  float* lfin = fl + 5 * WROWS;     // [64]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nqb = (p.nq + WROWS - 1) / WROWS;
  const int lin = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int qblk = lin % nqb, bh = lin / nqb;
  const int head = bh % p.heads, b = bh / p.heads;
  const int q0 = qblk * WROWS;
  const int d = p.d, nch = d >> 3;               // real 16-B chunks per row (d % 8 == 0)

  // ---- once: Q (scaled, zero past nq and past d), and the zero padding of the K and V slots
  for (int e = tid; e < WROWS * (D / 8); e += WNT) {
    const int row = e / (D / 8), c = e - row * (D / 8);
    h8 v = {};
    if (q0 + row < p.nq && c < nch) {
      v = *reinterpret_cast<const h8*>(p.q + ((size_t)b * p.nq + q0 + row) * p.q_ld + head * d + c * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (half_t)((float)v[j] * p.c);   // scores land in the exp2 domain
    }
    *reinterpret_cast<h8*>(Qs + row * QLD + c * 8) = v;
  }
  {
    const int kpad = QLD / 8 - nch, vpad = VLD / 8 - nch;
    for (int e = tid; e < WKT * kpad; e += WNT) {
      const int row = e / kpad, c = nch + e - row * kpad;
      *reinterpret_cast<h8*>(Ks + row * QLD + c * 8) = h8{};
    }
    for (int e = tid; e < WKT * vpad; e += WNT) {
      const int row = e / vpad, c = nch + e - row * vpad;
      *reinterpret_cast<h8*>(Vs + row * VLD + c * 8) = h8{};
    }
  }

  // ---- K/V staging: chunk e = tid + WNT*i of a tile = (key e/nch, chunk e%nch)
  const __amdgpu_buffer_rsrc_t rk = rsrc(p.k + (size_t)b * p.nk * p.k_ld, (long long)p.nk * p.k_ld * 2);
  const __amdgpu_buffer_rsrc_t rv = rsrc(p.v + (size_t)b * p.nk * p.v_ld, (long long)p.nk * p.v_ld * 2);
  unsigned gk[SL], gv[SL];
  int lk[SL], lv[SL];
#pragma unroll
  for (int i = 0; i < SL; ++i) {
    const int e = tid + WNT * i;
    const int key = e / nch, c = e - key * nch;
    const bool ok = e < WKT * nch;
    gk[i] = (unsigned)((key * p.k_ld + head * d + c * 8) * 2);
    gv[i] = (unsigned)((key * p.v_ld + head * d + c * 8) * 2);
    lk[i] = ok ? key * QLD + c * 8 : -1;
    lv[i] = key * VLD + c * 8;
  }
  const unsigned kstep = (unsigned)(WKT * p.k_ld * 2), vstep = (unsigned)(WKT * p.v_ld * 2);
  u4 rk_[SL], rv_[SL];
  auto fetch_k = [&](int t) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < SL; ++i)
      if (lk[i] >= 0) rk_[i] = __builtin_amdgcn_raw_buffer_load_b128(rk, gk[i] + t * kstep, 0, 0);
  };
  auto fetch_v = [&](int t) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < SL; ++i)
      if (lk[i] >= 0) rv_[i] = __builtin_amdgcn_raw_buffer_load_b128(rv, gv[i] + t * vstep, 0, 0);
  };
  auto stage_k = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < SL; ++i)
      if (lk[i] >= 0) *reinterpret_cast<u4*>(Ks + lk[i]) = rk_[i];
  };
  auto stage_v = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < SL; ++i)
      if (lk[i] >= 0) *reinterpret_cast<u4*>(Vs + lv[i]) = rv_[i];
  };

  // ---- score block of this wave: queries 16*sq .. +15 (column = lane & 15), keys 16*kb + 4*g + r
  const int sq = wave >> 1, kb = wave & 1;
  const int fr16 = lane & 15, g = lane >> 4;
  const int qrow = sq * 16 + fr16;               // this lane's query row within the block
  const half_t* qfrag = Qs + qrow * QLD + 8 * g;
  const half_t* kfrag = Ks + (kb * 16 + fr16) * QLD + 8 * g;
  const int nks = (d + 31) >> 5;                 // 32-wide k-steps that hold a real column
  float m_run = 0.f, l_run = 0.f;

  // ---- PV block of this wave: O^T rows = columns wave*DVS .. +DVS-1 of O, 2 x 32 query columns
  const int fr = lane & 31, fh = lane >> 5;
  const int q4 = (lane & 15) >> 2, pp = lane & 3;
  const int vrow_off = 4 * (g >> 1) + q4;
  const int vcol_off = wave * DVS + 16 * (g & 1) + 4 * pp;
  const bool pv_active = wave * DVS < d;         // wave-uniform: a slice past d holds only padding
  f16v o[2][NDB];
#pragma unroll
  for (int qb = 0; qb < 2; ++qb)
#pragma unroll
    for (int i = 0; i < NDB; ++i) o[qb][i] = f16v{};

  const int ntiles = (p.nk + WKT - 1) / WKT;
  fetch_k(0);
  stage_k();
  fetch_v(0);
  if (ntiles > 1) fetch_k(1);
  __syncthreads();

  for (int t = 0; t < ntiles; ++t) {
    // ---- A: S'^T block = K (cQ)^T
    f4 s = {};
    for (int ks = 0; ks < nks; ++ks) {
      const h8 a = *reinterpret_cast<const h8*>(kfrag + ks * 32);
      const h8 bq = *reinterpret_cast<const h8*>(qfrag + ks * 32);
      s = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, bq, s, 0, 0, 0);
    }
    if (t * WKT + WKT > p.nk) {                  // ragged last tile only
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (t * WKT + kb * 16 + 4 * g + r >= p.nk) s[r] = -1e30f;
    }
    float mt = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
    mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
    if (g == 0) pmax[kb * WROWS + qrow] = mt;
    __syncthreads();   // (1) both key halves' maxima; K_t and V_t-1 are read by every wave

    // ---- B: the tile's row max, the (rare) raise of the running max, P
    mt = fmaxf(pmax[qrow], pmax[WROWS + qrow]);
    // raise the running max only on the first tile or past the headroom (P <= 2^DEFER); tile 0 has
    // nothing to rescale (o = l = 0), and exp2(m_old - m) overflows for a first-tile max below -128
    float alpha = 1.f;
    if (t == 0) {
      m_run = mt;
    } else if (mt > m_run + DEFER) {
      alpha = __builtin_amdgcn_exp2f(m_run - mt);
      m_run = mt;
    }
    float ls = 0.f;
    h4 pk;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float e = __builtin_amdgcn_exp2f(s[r] - m_run);
      ls += e;
      pk[r] = (half_t)e;
    }
    *reinterpret_cast<h4*>(Ps + qrow * PLD + kb * 16 + 4 * g) = pk;
    ls += __shfl_xor(ls, 16, 64);
    ls += __shfl_xor(ls, 32, 64);
    if (g == 0) {
      psum[kb * WROWS + qrow] = ls;
      if (kb == 0) alph[qrow] = alpha;
    }
    stage_v();                                   // V_t
    if (t + 1 < ntiles) {
      stage_k();                                 // K_t+1
      fetch_v(t + 1);
      if (t + 2 < ntiles) fetch_k(t + 2);
    }
    __syncthreads();   // (2) P, row sums, alpha, V_t and K_t+1 visible

    // ---- C: row sum, rescale, O^T += V^T P^T
    l_run = l_run * alpha + (psum[qrow] + psum[WROWS + qrow]);
    if (pv_active) {
      const float a0 = alph[fr], a1 = alph[32 + fr];
      if (__any(a0 != 1.f || a1 != 1.f)) {
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            o[0][db][r] *= a0;
            o[1][db][r] *= a1;
          }
      }
      // element j of lane half fh in k-step ks is key 16ks + 8(j>>2) + 4fh + (j&3), on both operands
      h8 pf[2][WKT / 16];
#pragma unroll
      for (int qb = 0; qb < 2; ++qb)
#pragma unroll
        for (int ks = 0; ks < WKT / 16; ++ks) {
          const half_t* pr = Ps + (qb * 32 + fr) * PLD + 16 * ks + 4 * fh;
          const h4 lo = *reinterpret_cast<const h4*>(pr), hi = *reinterpret_cast<const h4*>(pr + 8);
          pf[qb][ks] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        }
#pragma unroll
      for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int ks = 0; ks < WKT / 16; ++ks) {
          const half_t* base = Vs + (16 * ks + vrow_off) * VLD + 32 * db + vcol_off;
          const fp16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4_t*)(base));
          const fp16x4_t hi =
              __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4_t*)(base + 8 * VLD));
          const h4 lo4 = __builtin_bit_cast(h4, lo), hi4 = __builtin_bit_cast(h4, hi);
          const h8 a = __builtin_shufflevector(lo4, hi4, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
          for (int qb = 0; qb < 2; ++qb) o[qb][db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, pf[qb][ks], o[qb][db], 0, 0, 0);
        }
    }
  }

  if (kb == 0 && g == 0) lfin[qrow] = l_run;
  __syncthreads();
  if (pv_active) {
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      const int row = q0 + qb * 32 + fr;
      if (row < p.nq) {
        const float inv = 1.f / lfin[qb * 32 + fr];
        half_t* op = p.o + ((size_t)b * p.nq + row) * p.o_ld + head * d;
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
          for (int gg = 0; gg < 4; ++gg) {
            const int dd = wave * DVS + db * 32 + 8 * gg + 4 * fh;
            if (dd < d) {
              h4 w;
#pragma unroll
              for (int j = 0; j < 4; ++j) w[j] = (half_t)(o[qb][db][4 * gg + j] * inv);
              *reinterpret_cast<h4*>(op + dd) = w;
            }
          }
      }
    }
  }
}

template <int D>
int launch_wide(const WideParams& p, hipStream_t s, sdk_attention_form_info* ran) {
  static std::atomic<unsigned long long> done{0};
  const long long blocks = (long long)((p.nq + WROWS - 1) / WROWS) * p.heads * p.batch;
  if (blocks > 0x7fffffffLL) return fail(SDK_EINVAL, "attention: grid too large");
  const int rc = ensure_dyn_lds((const void*)attn_wide_kernel<D>, WideLds<D>::BYTES, done, "attention (wide)");
  if (rc != SDK_OK) return rc;
  if (ran) *ran = sdk_attention_form_info{SDK_ATTN_WIDE, D, D, WNW, WROWS / 32, 0, 0, 0, (int32_t)blocks};
  hipLaunchKernelGGL((attn_wide_kernel<D>), dim3((unsigned)blocks), dim3(WNT), WideLds<D>::BYTES, s, p);
  return check_launch("attn_wide");
}

}  // namespace

// called by sdk_attention_form (attention.hip) with validated arguments, 168 <= head_dim <= 512
int attention_wide(const sdk_attention_args* a, hipStream_t s, sdk_attention_form_info* ran) {
  if (a->causal) return fail(SDK_EINVAL, "attention: the wide form has no causal instantiation");
  WideParams p{(const half_t*)a->q, (const half_t*)a->k, (const half_t*)a->v, (half_t*)a->o,
               a->q_ld, a->k_ld, a->v_ld, a->o_ld, a->batch, a->heads, a->nq, a->nk, a->head_dim,
               a->scale * 1.4426950408889634f};
  return a->head_dim <= 256 ? launch_wide<256>(p, s, ran) : launch_wide<512>(p, s, ran);
}

}  // namespace sdk
