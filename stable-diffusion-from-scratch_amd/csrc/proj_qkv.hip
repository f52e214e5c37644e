// The entry of a 320-channel SpatialTransformer in one launch (sdk_proj_norm_qkv):
//   tok = proj_in(GroupNorm affine?(x)),  qkv = [to_q | to_k | to_v](norm1(tok))
// — the chained form of conv_rowpanel_kernel (conv_rowpanel.hip, which explains the scheme): the same 8-wave workgroup
// that keeps a 256-row x 320-channel panel in registers as the B operand fragments of v_mfma_f32_16x16x32_f16, the
// same 5-slot LDS-DMA ring that streams W past it in 160-column chunks under counted vmcnt waits, the same chunk
// epilogue — over ONE packed [1280][320] weight, proj_in's 320 rows first, then the 960 q|k|v rows, so the ring never
// drains between the two GEMMs.  The GroupNorm output and norm1(tok) exist only in registers: the launch reads x
// (42 MB at 65,536 rows) and writes tok and qkv (168 MB) where the three launches it replaces moved 420 MB.  A workgroup
//  a. loads its panel; GN: each element becomes (half)(x * scale + shift) with the fp32 per-(image, channel) scale /
//     shift of sdk_group_norm_affine / _finalize (gn_act, common.h: the bits of the materialised GroupNorm), the image
//     of a row being row / hw, the 8 + 8 floats of a K-step fetched as that K-step is converted;
//  b. runs proj_in as chunks 0 and 1.  The packed proj_in rows are permuted (ops.py proj_qkv_perm): accumulator
//     (chunk c, block nb, lane group cg, q) is output channel 32 (g / 2) + 8 cg + 4 (g % 2) + q with g = 10 c + nb,
//     so blocks 2 ks and 2 ks + 1 of a lane, rounded to fp16 (acc + bias, the token linear's rounding point), ARE that
//     lane's B fragment of K-step ks of the next GEMM: token r16, channels 32 ks + 8 kq + [0, 8).  No LDS trip, no
//     cross-lane move.  tok itself leaves through the chunk epilogue in natural channel order;
//  c. norm1 on those fragments: ln_quad_stats_on<10, LnFragLanes> (common.h — the row's four lanes are l, l ^ 16,
//     l ^ 32, l ^ 48; pivot, in-lane order and the order of the two cross-lane adds as in every other LayerNorm
//     route), ln_quad_apply with gamma | beta staged in LDS; the normalised fragments take the dead panel's registers;
//  d. runs q|k|v as chunks 2 .. 7.
// K-steps ascending on the 16x16x32 shape in both GEMMs: the sums of token_linear320_kernel and conv_rowpanel_kernel.
// Register peak in chunk 1: panel 80 + accumulator 80 + the first half of the tok fragments 40 + W queue 20; the
// build refuses scratch here (build.py NO_SCRATCH).
// The geometry constants and the two helpers below restate conv_rowpanel.hip's.  They are not shared through a
// header because the csrc/conv* files are the key of the committed conv tuning table (ops._conv_source_hash): this
// unit reads the conv headers but is not one of them.
#include "conv_cfg.h"
#include "conv_device.h"

namespace sdk {
namespace {

using RP = CfgRowPanel;
constexpr int RP_NW = 8, RP_NT = RP_NW * 64;
constexpr int RP_TG = RP::TBM / RP_NW / 16;           // 16-row blocks per wave (2)
constexpr int RP_NB = RP::TBN / 16;                   // 16-column blocks per chunk (10)
constexpr int RP_KS = RP::MAXK / 32;                  // K-steps held in registers (10)
constexpr int RP_KT = (RP::MAXK + BK - 1) / BK;       // 64-wide K tiles = ring slots per chunk (5)
constexpr int RP_SLOT_H = RP::TBN * BK;               // halfs per ring slot (20 KiB)
constexpr int RP_PIECES = RP::TBN / 8;                // 1-KiB pieces per slot (20)
constexpr int RP_PPW = (RP_PIECES + RP_NW - 1) / RP_NW;   // pieces per wave per slot (3: the same count in every wave
                                                          // keeps the vmcnt immediate exact; 4 of the 24 are padding)
constexpr int RP_NS = 5;                              // ring slots: 3 in flight behind the one being read
constexpr int RP_PFD = 4;                             // W fragment reads ahead of their MFMAs
constexpr int RP_RS = RP::TBN + 8;                    // epilogue scratch row stride (halfs) = 336 B
constexpr int RP_SCR = 16 * RP_RS * 2;                // per-wave epilogue scratch: 16 rows x 160 columns
constexpr int RP_CPR = RP::TBN / 8;                   // 16-B chunks per scratch row (20)
constexpr int RP_CPT = 16 * RP_CPR / 64;              // chunks per lane per 16-row block (5)
constexpr unsigned RP_OOB = 0x80000000u;              // an offset past every buffer: loads zeros, stores nothing
constexpr int RP_EST = RP_TG * RP_CPT;                // stores per wave per chunk epilogue (10)
// LDS: ring | 1-KiB dummy slot of the padding pieces | per-wave epilogue scratch | bias of every chunk | gamma | beta
constexpr int PQ_C = 320, PQ_NQKV = 960, PQ_N = PQ_C + PQ_NQKV;
constexpr int PQ_NCH = PQ_N / RP::TBN, PQ_NCH_IN = PQ_C / RP::TBN;      // 8 chunks, the first 2 are proj_in
constexpr int RP_OFF_DUMMY = RP_NS * RP_SLOT_H * 2;
constexpr int RP_OFF_SCR = RP_OFF_DUMMY + 1024;
constexpr int PQ_OFF_BIAS = RP_OFF_SCR + RP_NW * RP_SCR;
constexpr int PQ_OFF_GB = PQ_OFF_BIAS + PQ_N * 4;
constexpr int PQ_LDS = PQ_OFF_GB + 2 * PQ_C * 4;
static_assert(RP::TBM == RP_NW * 16 * RP_TG && RP::TBN % 16 == 0 && RP::MAXK % 32 == 0, "whole MFMA blocks");
static_assert(16 * RP_CPR % 64 == 0, "whole read-back instructions per 16-row block");
static_assert((RP_NS - 2) * RP_PPW + RP_EST <= 63, "vmcnt immediate");
static_assert(RP_NS - 1 <= RP_KT, "at most one epilogue between a slot's pieces and its wait");
static_assert(RP::MAXK == PQ_C && PQ_C % RP::TBN == 0 && PQ_NQKV % RP::TBN == 0 && PQ_C == RP_KT * BK, "whole chunks and slots");
static_assert(RP_NB % 2 == 0, "two accumulator blocks per operand fragment");
static_assert(PQ_LDS <= 160 * 1024, "LDS");

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rp_rsrc(const void* base, long long bytes) {
  const int n = (int)(bytes < 0x7fffffffLL ? bytes : 0x7fffffffLL);
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, n, 0x00020000);
}

// sched_group_barrier sequence of a slot's MFMA groups (conv_tile.h pin_fragment_groups): per group the W fragment
// read RP_PFD groups ahead (DS read), the group's RP_TG MFMAs, then its DMA piece (VMEM)
template <int G, int g = 0>
__device__ __forceinline__ void rp_pin_groups() {
  if constexpr (g < G) {
    if constexpr (g + RP_PFD < G) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, RP_TG, 0);
    if constexpr (g < RP_PPW) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
    rp_pin_groups<G, g + 1>();
  }
}

// The epilogue of one 16-row block of a chunk (conv_rowpanel.hip rp_rows16 without the residual): the wave rounds
// acc + bias to fp16 into its private scratch (16 rows x 160 columns), reads the rows back as 16-B chunks (chunk
// lane + 64 i of the block: whole 320-B rows) and stores them at voff.  acc[nb] lane l holds row l & 15 and columns
// 16 nb + 4 (l >> 4) + q of the chunk, or with PERM (the proj_in chunks, whose packed W rows are permuted) columns
// 32 (nb / 2) + 8 (l >> 4) + 4 (nb % 2) + q: the scratch write undoes the permutation, and the rounded values are
// also handed back (keep[nb]) as the halves of the next GEMM's operand fragments.
template <bool PERM>
__device__ __forceinline__ void pq_rows16(const f4* a, half_t* wbuf, const float* bias_c, __amdgpu_buffer_rsrc_t ro,
                                          const unsigned (&voff)[RP_CPT], h4* keep = nullptr) {
  const int lane = threadIdx.x & 63, px = lane & 15, cg = lane >> 4;
#pragma unroll
  for (int j = 0; j < RP_NB; ++j) {
    const f4 bb = *reinterpret_cast<const f4*>(bias_c + 16 * j + 4 * cg);
    h4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = (half_t)(a[j][q] + bb[q]);
    if constexpr (PERM) keep[j] = o;
    const int col = PERM ? 32 * (j / 2) + 8 * cg + 4 * (j % 2) : 16 * j + 4 * cg;
    *reinterpret_cast<h4*>(wbuf + px * RP_RS + col) = o;
  }
#pragma unroll
  for (int i = 0; i < RP_CPT; ++i) {
    const int idx = lane + 64 * i, row = idx / RP_CPR, ch = idx - row * RP_CPR;
    const h8 v = *reinterpret_cast<const h8*>(wbuf + row * RP_RS + ch * 8);
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, v), ro,
                                           voff[i], 0, 0);
  }
}

struct ChainParams {
  const half_t* x; const float* gn_scale; const float* gn_shift; const half_t* w; const float* bias;
  const float* gamma; const float* beta; half_t* tok; half_t* qkv;
  int x_ld, tok_ld, qkv_ld, M, hw, nimg;
  float eps;
};

template <bool GN>
__global__ void __launch_bounds__(RP_NT, 2) proj_norm_qkv_kernel(ChainParams p) {
  extern __shared__ __attribute__((aligned(16))) half_t lds[];   // the kernel's only LDS object
  char* const ldsb = reinterpret_cast<char*>(lds);
  half_t* const dummy = reinterpret_cast<half_t*>(ldsb + RP_OFF_DUMMY);
  float* const bias_s = reinterpret_cast<float*>(ldsb + PQ_OFF_BIAS);
  float* const gb = reinterpret_cast<float*>(ldsb + PQ_OFF_GB);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  __builtin_assume(wave >= 0 && wave < RP_NW);
  const int r16 = lane & 15, kq = lane >> 4;
  const int m0 = (int)blockIdx.x * RP::TBM;
  const int rows = min(RP::TBM, p.M - m0);
  constexpr int ldw = PQ_C;

  // bias of every chunk and gamma | beta; the first slot's barrier orders these writes
  for (int n = tid; n < PQ_N; n += RP_NT) bias_s[n] = p.bias[n];
  for (int n = tid; n < PQ_C; n += RP_NT) {
    gb[n] = p.gamma[n];
    gb[PQ_C + n] = p.beta[n];
  }

  // W pieces and the issue cursor: as in conv_rowpanel_kernel, over the 1280 packed rows
  const __amdgpu_buffer_rsrc_t rw = rp_rsrc(p.w, (long long)PQ_N * ldw * 2);
  // piece j of this wave is 64 rows below piece j - 1, and 64 rows keep the swizzle ((row >> 1) & 7): one per-lane
  // offset serves all; whether a piece exists (a padding piece, a slot past the last chunk) is wave-uniform here,
  // because the 1280 rows are whole chunks
  const int prow0 = wave * 8 + (lane >> 3);
  const unsigned vb0 = (unsigned)(prow0 * ldw) * 2u + (unsigned)((lane & 7) ^ ((prow0 >> 1) & 7)) * 16u;
  int ic = 0, ikt = 0, ipos = 0;
  auto issue_piece = [&](int j) __attribute__((always_inline)) {
    const unsigned off = (unsigned)((ic * RP::TBN + j * 8 * RP_NW) * ldw + ikt * BK) * 2u;
    const int piece = j * RP_NW + wave;
    half_t* dst = piece < RP_PIECES ? lds + ipos * RP_SLOT_H + piece * 8 * BK : dummy;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (__attribute__((address_space(3))) void*)dst, 16,
                                             piece < RP_PIECES && ic < PQ_NCH ? vb0 + off : RP_OOB, 0, 0, 0);
  };
  auto issue_next = [&]() __attribute__((always_inline)) {
    if (++ikt == RP_KT) {
      ikt = 0;
      ++ic;
    }
    ipos = ipos + 1 == RP_NS ? 0 : ipos + 1;
  };
#pragma unroll
  for (int s = 0; s < RP_NS - 1; ++s) {
#pragma unroll
    for (int j = 0; j < RP_PPW; ++j) issue_piece(j);
    issue_next();
  }

  // a. the panel: row 32 wave + 16 tg + r16, k = 32 ks + 8 kq + [0, 8); rows past M read zeros
  const __amdgpu_buffer_rsrc_t ra = rp_rsrc(p.x + (size_t)m0 * p.x_ld, ((long long)(rows - 1) * p.x_ld + PQ_C) * 2);
  h8 xf[RP_KS][RP_TG];
#pragma unroll
  for (int ks = 0; ks < RP_KS; ++ks)
#pragma unroll
    for (int tg = 0; tg < RP_TG; ++tg) {
      const unsigned row = (unsigned)(32 * wave + 16 * tg + r16);
      xf[ks][tg] = __builtin_bit_cast(
          h8, __builtin_amdgcn_raw_buffer_load_b128(ra, (row * (unsigned)p.x_ld + 8u * kq) * 2u + 64u * ks, 0, 0));
    }
  if constexpr (GN) {
    // scale / shift of this lane's two rows: image row / hw (the two 16-row blocks of a wave, and the rows of one
    // block, may lie in different images).  A row past M has an image past the last: its loads are out of range
    // and give 0 x 0 + 0
    const __amdgpu_buffer_rsrc_t rsc = rp_rsrc(p.gn_scale, (long long)p.nimg * PQ_C * 4);
    const __amdgpu_buffer_rsrc_t rsh = rp_rsrc(p.gn_shift, (long long)p.nimg * PQ_C * 4);
    unsigned goff[RP_TG];
#pragma unroll
    for (int tg = 0; tg < RP_TG; ++tg)
      goff[tg] = (unsigned)(((m0 + 32 * wave + 16 * tg + r16) / p.hw) * PQ_C + 8 * kq) * 4u;
#pragma unroll
    for (int ks = 0; ks < RP_KS; ++ks)
#pragma unroll
      for (int tg = 0; tg < RP_TG; ++tg) {
        const unsigned o = goff[tg] + 128u * ks;
        const f4 sc0 = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rsc, o, 0, 0));
        const f4 sc1 = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rsc, o + 16u, 0, 0));
        const f4 sh0 = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rsh, o, 0, 0));
        const f4 sh1 = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rsh, o + 16u, 0, 0));
        h8 v = xf[ks][tg];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[j] = (half_t)gn_act((float)v[j], sc0[j], sh0[j], 0);
          v[4 + j] = (half_t)gn_act((float)v[4 + j], sc1[j], sh1[j], 0);
        }
        xf[ks][tg] = v;
      }
  }
  // the panel is complete before the first slot (no wait on an ordinary load is left to drain the ring)
#pragma unroll
  for (int ks = 0; ks < RP_KS; ++ks)
#pragma unroll
    for (int tg = 0; tg < RP_TG; ++tg) asm volatile("" : "+v"(xf[ks][tg]));
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's bias / gamma / beta writes

  half_t* const wscr = reinterpret_cast<half_t*>(ldsb + RP_OFF_SCR + wave * RP_SCR);
  const __amdgpu_buffer_rsrc_t rt =
      rp_rsrc(p.tok + (size_t)m0 * p.tok_ld, ((long long)(rows - 1) * p.tok_ld + PQ_C) * 2);
  const __amdgpu_buffer_rsrc_t rq =
      rp_rsrc(p.qkv + (size_t)m0 * p.qkv_ld, ((long long)(rows - 1) * p.qkv_ld + PQ_NQKV) * 2);

  int rpos = 0;
  // one chunk's five slots: the body of conv_rowpanel_kernel's K loop.  `late`: a chunk epilogue lies between the
  // slot's pieces and its wait for every slot but the last, so its RP_EST stores may stay in flight
  auto chunk = [&](f4 (&acc)[RP_TG][RP_NB], const h8 (&b)[RP_KS][RP_TG], bool late) __attribute__((always_inline)) {
#pragma unroll
    for (int tg = 0; tg < RP_TG; ++tg)
#pragma unroll
      for (int nb = 0; nb < RP_NB; ++nb) acc[tg][nb] = f4{};
#pragma unroll
    for (int kt = 0; kt < RP_KT; ++kt) {
      __builtin_amdgcn_sched_barrier(0);   // the previous slot's last MFMAs stay above the wait
      if (late && kt < RP_KT - 1)
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((RP_NS - 2) * RP_PPW + RP_EST) : "memory");
      else
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((RP_NS - 2) * RP_PPW) : "memory");
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      const half_t* st = lds + rpos * RP_SLOT_H;
      constexpr int G = (BK / 32) * RP_NB;
      auto rd = [&](int gq) __attribute__((always_inline)) {
        return *reinterpret_cast<const h8*>(st + swz(16 * (gq % RP_NB) + r16, 4 * (gq / RP_NB) + kq));
      };
      h8 wq[RP_PFD + 1];
#pragma unroll
      for (int gq = 0; gq < RP_PFD; ++gq) wq[gq] = rd(gq);
#pragma unroll
      for (int gq = 0; gq < G; ++gq) {
        if (gq + RP_PFD < G) wq[(gq + RP_PFD) % (RP_PFD + 1)] = rd(gq + RP_PFD);
        const int nb = gq % RP_NB;
#pragma unroll
        for (int tg = 0; tg < RP_TG; ++tg)
          acc[tg][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wq[gq % (RP_PFD + 1)], b[2 * kt + gq / RP_NB][tg],
                                                               acc[tg][nb], 0, 0, 0);
        if (gq < RP_PPW) issue_piece(gq);
      }
      issue_next();
      __builtin_amdgcn_sched_group_barrier(0x100, RP_PFD, 0);
      rp_pin_groups<G>();
      rpos = rpos + 1 == RP_NS ? 0 : rpos + 1;
    }
  };
  // this lane's read-back chunks of a 16-row block (pq_rows16): row and 16-B chunk of chunk index lane + 64 i.
  // Worked out anew at every epilogue from a lane id the compiler cannot see through: hoisted out of the chunk
  // loop, the offsets of both outputs would hold some thirty registers across the MFMA loops, which have none to
  // spare in chunk 1
  auto offsets = [&](unsigned (&vo)[RP_CPT], int tg, int ld, int n0) __attribute__((always_inline)) {
    int l = lane;
    asm volatile("" : "+v"(l));
#pragma unroll
    for (int i = 0; i < RP_CPT; ++i) {
      const int idx = l + 64 * i, row = idx / RP_CPR;
      vo[i] = (unsigned)((32 * wave + 16 * tg + row) * ld + n0 + (idx - row * RP_CPR) * 8) * 2u;
    }
  };

  // b. proj_in: the rounded accumulators stay as the next GEMM's fragments tf[ks][tg]
  h8 tf[RP_KS][RP_TG];
#pragma unroll
  for (int c = 0; c < PQ_NCH_IN; ++c) {
    f4 acc[RP_TG][RP_NB];
    chunk(acc, xf, c > 0);
#pragma unroll
    for (int tg = 0; tg < RP_TG; ++tg) {
      unsigned vo[RP_CPT];
      offsets(vo, tg, p.tok_ld, c * RP::TBN);
      h4 keep[RP_NB];
      pq_rows16<true>(acc[tg], wscr, bias_s + c * RP::TBN, rt, vo, keep);
      // (the fragments stay packed fp16 until norm1: without the pin the compiler converts them back to fp32 for the
      // LayerNorm sums right here and carries 80 floats per 16-row block across chunk 1)
#pragma unroll
      for (int i = 0; i < RP_NB / 2; ++i) {
        h8& f = tf[c * (RP_NB / 2) + i][tg];
        f = __builtin_shufflevector(keep[2 * i], keep[2 * i + 1], 0, 1, 2, 3, 4, 5, 6, 7);
        asm volatile("" : "+v"(f));
      }
    }
  }

  // c. norm1 on the fragments; the normalised rows take the panel's place.  (The lane group is taken from a value
  // the compiler cannot see through, or the twenty gamma / beta addresses are worked out before chunk 0 and held)
  __builtin_amdgcn_sched_barrier(0);
  int kql = kq;
  asm volatile("" : "+v"(kql));
#pragma unroll
  for (int tg = 0; tg < RP_TG; ++tg) {
    h8 v[RP_KS];
#pragma unroll
    for (int ks = 0; ks < RP_KS; ++ks) v[ks] = tf[ks][tg];
    float mean, rstd;
    ln_quad_stats_on<RP_KS, LnFragLanes>(v, p.eps, mean, rstd);
#pragma unroll
    for (int ks = 0; ks < RP_KS; ++ks) xf[ks][tg] = ln_quad_apply(v[ks], mean, rstd, gb, PQ_C, kql + 4 * ks);
  }
  __builtin_amdgcn_sched_barrier(0);

  // d. q|k|v
#pragma unroll 1
  for (int c = PQ_NCH_IN; c < PQ_NCH; ++c) {
    f4 acc[RP_TG][RP_NB];
    chunk(acc, xf, true);
#pragma unroll
    for (int tg = 0; tg < RP_TG; ++tg) {
      unsigned vo[RP_CPT];
      offsets(vo, tg, p.qkv_ld, (c - PQ_NCH_IN) * RP::TBN);
      pq_rows16<false>(acc[tg], wscr, bias_s + c * RP::TBN, rq, vo);
    }
  }
  // the trailing pieces (zeros) must land before the workgroup's LDS is released
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

template <bool GN>
int proj_norm_qkv_launch(const ChainParams& p, hipStream_t s) {
  static std::atomic<unsigned long long> attr_set{0};
  if (int e = ensure_dyn_lds((const void*)proj_norm_qkv_kernel<GN>, PQ_LDS, attr_set, "proj_norm_qkv")) return e;
  hipLaunchKernelGGL((proj_norm_qkv_kernel<GN>), dim3((p.M + RP::TBM - 1) / RP::TBM), dim3(RP_NT), PQ_LDS, s, p);
  return check_launch("proj_norm_qkv");
}

bool pq_overlap(const void* a, long long ab, const void* b, long long bb) {
  const char *a0 = (const char*)a, *b0 = (const char*)b;
  return a0 < b0 + bb && b0 < a0 + ab;
}

}  // namespace
}  // namespace sdk

using namespace sdk;

extern "C" int sdk_proj_norm_qkv_supported(int32_t in_features, int32_t features, int32_t qkv_features) {
  return in_features == PQ_C && features == PQ_C && qkv_features == PQ_NQKV ? 1 : 0;
}

extern "C" int sdk_proj_norm_qkv(const sdk_proj_norm_qkv_args* a, sdk_stream_t stream) {
  if (!a || !a->x || !a->w || !a->bias || !a->gamma || !a->beta || !a->tok || !a->qkv)
    return fail(SDK_EINVAL, "proj_norm_qkv: null pointer");
  if (!sdk_proj_norm_qkv_supported(a->in_features, a->features, a->qkv_features))
    return fail(SDK_EINVAL, "proj_norm_qkv: in_features / features / qkv_features must be 320 / 320 / 960");
  if (a->rows <= 0) return fail(SDK_EINVAL, "proj_norm_qkv: empty");
  if (a->x_ld % 8 || a->tok_ld % 8 || a->qkv_ld % 8 || a->x_ld < PQ_C || a->tok_ld < PQ_C || a->qkv_ld < PQ_NQKV)
    return fail(SDK_EINVAL, "proj_norm_qkv: row strides must be multiples of 8 and at least the row widths");
  if (((uintptr_t)a->x | (uintptr_t)a->w | (uintptr_t)a->bias | (uintptr_t)a->gamma | (uintptr_t)a->beta |
       (uintptr_t)a->tok | (uintptr_t)a->qkv | (uintptr_t)a->gn_scale | (uintptr_t)a->gn_shift) & 15)
    return fail(SDK_EINVAL, "proj_norm_qkv: pointers must be 16-B aligned");
  const bool gn = a->gn_scale || a->gn_shift;
  if (gn && (!a->gn_scale || !a->gn_shift || a->hw <= 0 || a->rows % a->hw))
    return fail(SDK_EINVAL, "proj_norm_qkv: a GroupNorm affine needs scale, shift and hw (rows a multiple of hw)");
  // a panel's 256 rows are addressed by 32-bit byte offsets from its first row
  if (a->x_ld > (1 << 20) || a->tok_ld > (1 << 20) || a->qkv_ld > (1 << 20))
    return fail(SDK_EINVAL, "proj_norm_qkv: row stride too large");
  // a panel's x rows are read while other workgroups already store tok / qkv rows
  const long long xb = ((long long)(a->rows - 1) * a->x_ld + PQ_C) * 2;
  const long long tb = ((long long)(a->rows - 1) * a->tok_ld + PQ_C) * 2;
  const long long qb = ((long long)(a->rows - 1) * a->qkv_ld + PQ_NQKV) * 2;
  const long long gbytes = gn ? (long long)(a->rows / a->hw) * PQ_C * 4 : 0;
  const struct { const void* p; long long n; } in[] = {{a->x, xb}, {a->w, (long long)PQ_N * PQ_C * 2}, {a->bias, PQ_N * 4},
                                                        {a->gamma, PQ_C * 4}, {a->beta, PQ_C * 4},
                                                        {a->gn_scale, gbytes}, {a->gn_shift, gbytes}};
  for (const auto& i : in)
    if (i.p && (pq_overlap(i.p, i.n, a->tok, tb) || pq_overlap(i.p, i.n, a->qkv, qb)))
      return fail(SDK_EINVAL, "proj_norm_qkv: an output overlaps an input");
  if (pq_overlap(a->tok, tb, a->qkv, qb)) return fail(SDK_EINVAL, "proj_norm_qkv: tok and qkv overlap");
  ChainParams p;
  p.x = (const half_t*)a->x; p.gn_scale = a->gn_scale; p.gn_shift = a->gn_shift;
  p.w = (const half_t*)a->w; p.bias = a->bias; p.gamma = a->gamma; p.beta = a->beta;
  p.tok = (half_t*)a->tok; p.qkv = (half_t*)a->qkv;
  p.x_ld = a->x_ld; p.tok_ld = a->tok_ld; p.qkv_ld = a->qkv_ld; p.M = a->rows;
  p.hw = gn ? a->hw : 1; p.nimg = gn ? a->rows / a->hw : 0; p.eps = a->eps;
  return gn ? proj_norm_qkv_launch<true>(p, (hipStream_t)stream) : proj_norm_qkv_launch<false>(p, (hipStream_t)stream);
}
