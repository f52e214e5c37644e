// Row-panel-stationary GEMM for the short-K 1x1 problems (K = cin <= 320: the 64x64 level's q|k|v projection,
// (M, N, K) = (65536, 960, 320)):   out[m, n] = sum_k A[m, k] W[n, k] (+ bias) (+ residual),  fp16 NHWC rows.
//
// The tiled kernels (conv_tile.h) pay a prologue, a 5-step K loop and an epilogue per output tile and fetch the A rows
// once per N-tile; their stores come in one burst per round of tiles.  Here the operand that stays on chip is the other
// one — the mirror image of token_linear320_kernel (token.hip), which keeps W in registers and streams rows:
//  * one workgroup of 8 waves (two per SIMD, 256 registers) owns a 256-row panel of M; wave w holds rows 32 w .. 32 w + 31
//    as the B operand fragments of v_mfma_f32_16x16x32_f16 for its whole life (K / 4 registers: 80 at K = 320, what
//    ff_geglu_kernel spends on its token rows).  A is read from memory exactly once and never touches LDS;
//  * the workgroup walks N in chunks of 160 columns.  W streams through a ring of RP_NS slots shared by the eight
//    waves, one slot = the chunk's 160 rows x one 64-wide K tile (20 one-KiB buffer_load ... lds pieces, the 128-B rows
//    XOR-swizzled as in conv_device.h swz).  The ring runs on across chunk boundaries: a chunk has no prologue;
//  * one raw s_barrier per slot: wait for this wave's pieces of the slot (counted vmcnt), barrier (every wave's pieces
//    landed, every wave done with the previous slot), then the slot's two K-steps with the refill of the previous
//    slot's position issued between their first MFMA groups.  The wait counts the DMA pieces issued after the slot's
//    own ((RP_NS - 2) x RP_PPW): the epilogue's stores (and residual loads) share vmcnt but are issued after them, so
//    they can only make the wait retire more, never less; where the previous chunk's stores provably all lie behind
//    the slot's pieces they are counted too and stay in flight under the next chunk's MFMAs;
//  * per wave and chunk a 32 x 160 fp32 accumulator (80 registers), K-steps of 32 in ascending order on the 16x16x32
//    shape: the sums of variants 22 / 38, bit for bit.  The chunk epilogue has the rounding points of those variants
//    (conv_tile.h epi16_group: acc + bias rounded to fp16 through a private LDS scratch, 16-B row chunks stored, + the
//    residual chunk in fp32, rounded again), but one LDS round trip per 16 rows x 160 columns instead of one per 64
//    columns, whole 320-B row segments per store, and the bias of the whole launch staged in LDS once.  Stores and
//    residual loads go through buffer resources of the panel's rows: the range check drops the rows past M, a
//    per-lane offset select the columns past N — no branch, the same operations in every wave.
// Ragged M: rows past M load zeros (range check) and are not stored.  Ragged N: the last chunk's rows past the packed
// weight load zeros and columns past N are not stored.  K % 64 == 32: the panel's K-steps past cin are zeros, so the
// last slot's upper K-step adds 0 x the zero padding of the packed W.
// No GroupNorm statistics, no embedding row, no split of K (conv_plan.hip: rowpanel_ok).
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
constexpr int RP_NPAD = (RP::MAXN + RP::TBN - 1) / RP::TBN * RP::TBN;
constexpr int RP_RS = RP::TBN + 8;                    // epilogue scratch row stride (halfs) = 336 B
constexpr int RP_SCR = 16 * RP_RS * 2;                // per-wave epilogue scratch: 16 rows x 160 columns
constexpr int RP_CPR = RP::TBN / 8;                   // 16-B chunks per scratch row (20)
constexpr int RP_CPT = 16 * RP_CPR / 64;              // chunks per lane per 16-row block (5)
constexpr unsigned RP_OOB = 0x80000000u;              // an offset past every buffer: loads zeros, stores nothing
// LDS: ring | 1-KiB dummy slot of the padding pieces | per-wave epilogue scratch | bias of every chunk
constexpr int RP_OFF_DUMMY = RP_NS * RP_SLOT_H * 2;
constexpr int RP_OFF_SCR = RP_OFF_DUMMY + 1024;
constexpr int RP_OFF_BIAS = RP_OFF_SCR + RP_NW * RP_SCR;
constexpr int RP_LDS = RP_OFF_BIAS + RP_NPAD * 4;
static_assert(RP::TBM == RP_NW * 16 * RP_TG && RP::TBN % 16 == 0 && RP::MAXK % 32 == 0, "whole MFMA blocks");
static_assert(16 * RP_CPR % 64 == 0, "whole read-back instructions per 16-row block");
static_assert(RP_LDS <= 160 * 1024, "LDS");
#if defined(SDK_STORE_HINT) && SDK_STORE_HINT == 2
constexpr int RP_EST = 0;                             // A/B build without the stores: nothing to leave in flight
#else
constexpr int RP_EST = RP_TG * RP_CPT;                // stores per wave per chunk epilogue (10)
#endif
static_assert((RP_NS - 2) * RP_PPW + RP_EST <= 63, "vmcnt immediate");
static_assert(RP_NS - 1 <= RP_KT, "at most one epilogue between a slot's pieces and its wait");

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

// The epilogue of one 16-row block of a chunk: acc[nb] lane l holds row l & 15, columns 16 nb + 4 (l >> 4) + q.  The
// wave rounds acc + bias to fp16 into its private scratch (16 rows x 160 columns), reads the rows back as 16-B chunks
// (chunk lane + 64 i of the block: whole 320-B rows, 3.2 rows per instruction) and stores them (+ the residual chunk).
// voff / roff: this lane's byte offsets of its chunks in the panel's output / residual rows, RP_OOB for a chunk past N.
template <bool RES>
__device__ __forceinline__ void rp_rows16(const f4* a, half_t* wbuf, const float* bias_c, __amdgpu_buffer_rsrc_t ro,
                                          __amdgpu_buffer_rsrc_t rr, const unsigned (&voff)[RP_CPT],
                                          const unsigned (&roff)[RP_CPT]) {
  const int lane = threadIdx.x & 63, px = lane & 15, cg = lane >> 4;
  h8 res[RP_CPT];
  if constexpr (RES) {
#pragma unroll
    for (int i = 0; i < RP_CPT; ++i)
      res[i] = __builtin_bit_cast(h8, __builtin_amdgcn_raw_buffer_load_b128(rr, roff[i], 0, 0));
  }
#pragma unroll
  for (int j = 0; j < RP_NB; ++j) {
    const f4 bb = *reinterpret_cast<const f4*>(bias_c + 16 * j + 4 * cg);
    h4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = (half_t)(a[j][q] + bb[q]);
    *reinterpret_cast<h4*>(wbuf + px * RP_RS + 16 * j + 4 * cg) = o;
  }
#pragma unroll
  for (int i = 0; i < RP_CPT; ++i) {
    const int idx = lane + 64 * i, row = idx / RP_CPR, ch = idx - row * RP_CPR;
    h8 v = *reinterpret_cast<const h8*>(wbuf + row * RP_RS + ch * 8);
    if constexpr (RES) {
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = (half_t)((float)v[q] + (float)res[i][q]);
    }
#if defined(SDK_STORE_HINT) && SDK_STORE_HINT == 2
    asm volatile("" ::"v"(v), "v"(voff[i]));   // A/B build only (conv_device.h st_out16): the epilogue but its stores
#else
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, v), ro,
                                           voff[i], 0, 0);
#endif
  }
}

template <bool RES>
__global__ void __launch_bounds__(RP_NT, 2) conv_rowpanel_kernel(Params p) {
  extern __shared__ __attribute__((aligned(16))) half_t lds[];   // the kernel's only LDS object
  char* const ldsb = reinterpret_cast<char*>(lds);
  half_t* const dummy = reinterpret_cast<half_t*>(ldsb + RP_OFF_DUMMY);
  float* const bias_s = reinterpret_cast<float*>(ldsb + RP_OFF_BIAS);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  __builtin_assume(wave >= 0 && wave < RP_NW);
  const int r16 = lane & 15, kq = lane >> 4;
  const int m0 = (int)blockIdx.x * RP::TBM;
  const int rows = min(RP::TBM, p.M - m0);              // the panel's rows of the problem
  const int K = p.seg[0].cin, KT = (K + BK - 1) / BK;
  const int N = p.N, ldw = p.ldw, wrows = p.wrows;
  const int nch = (N + RP::TBN - 1) / RP::TBN;

  // the bias of every chunk (zeros where there is none or past N); the first slot's barrier orders these writes
  // (every wave waits for its own before it)
  for (int n = tid; n < nch * RP::TBN; n += RP_NT) bias_s[n] = (p.bias && n < N) ? p.bias[n] : 0.f;

  // W pieces of this wave: piece j * 8 + wave of a slot covers rows 8 piece .. 8 piece + 7 of the chunk, lane l its
  // row 8 piece + l / 8 and the 16-B chunk position l % 8, which holds K chunk (l % 8) ^ ((row >> 1) & 7) of that row
  const __amdgpu_buffer_rsrc_t rw = rp_rsrc(p.W, (long long)wrows * ldw * 2);
  unsigned vb[RP_PPW];
  int prow[RP_PPW];
#pragma unroll
  for (int j = 0; j < RP_PPW; ++j) {
    const int piece = j * RP_NW + wave, row = piece * 8 + (lane >> 3);
    const int rch = (lane & 7) ^ ((row >> 1) & 7);
    prow[j] = piece < RP_PIECES ? row : 0x40000000;   // a padding piece is past every chunk
    vb[j] = (unsigned)(row * ldw) * 2u + (unsigned)rch * 16u;
  }
  // the issue cursor: slot (chunk ic, K tile ikt) into ring position ipos.  Slots past the last chunk still issue
  // their pieces (zeros, range check) so that every iteration waits with the same immediate
  int ic = 0, ikt = 0, ipos = 0;
  auto issue_piece = [&](int j) __attribute__((always_inline)) {   // j: a compile-time index after unrolling
    const unsigned off = (unsigned)(ic * RP::TBN * ldw + ikt * BK) * 2u;
    const int rows_left = ic < nch ? wrows - ic * RP::TBN : 0;
    const int piece = j * RP_NW + wave;
    half_t* dst = piece < RP_PIECES ? lds + ipos * RP_SLOT_H + piece * 8 * BK : dummy;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (__attribute__((address_space(3))) void*)dst, 16,
                                             prow[j] < rows_left ? vb[j] + off : RP_OOB, 0, 0, 0);
  };
  auto issue_next = [&]() __attribute__((always_inline)) {
    if (++ikt == KT) {
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

  // the wave's rows as B operand fragments: panel row 32 wave + 16 tg + r16, k = 32 ks + 8 kq + [0, 8); rows past M
  // read zeros (range check: their offsets lie past the panel's last row), and so do the K-steps past cin (the upper
  // K-step of the last slot when K % 64 == 32 then adds 0 x the zero padding of the packed W): branch-free
  const Seg& g = p.seg[0];
  const __amdgpu_buffer_rsrc_t ra = rp_rsrc(g.src0 + (size_t)m0 * g.ld0, ((long long)(rows - 1) * g.ld0 + K) * 2);
  h8 xf[RP_KS][RP_TG];
#pragma unroll
  for (int ks = 0; ks < RP_KS; ++ks) {
    const unsigned kofs = 32 * ks < K ? 64u * ks : RP_OOB;
#pragma unroll
    for (int tg = 0; tg < RP_TG; ++tg) {
      const unsigned row = (unsigned)(32 * wave + 16 * tg + r16);
      xf[ks][tg] = __builtin_bit_cast(
          h8, __builtin_amdgcn_raw_buffer_load_b128(ra, (row * (unsigned)g.ld0 + 8u * kq) * 2u + kofs, 0, 0));
    }
  }
  // the panel is complete before the loop (with it the first ring slots): no wait on an ordinary load is left for
  // the compiler to place inside the loop, where it would drain the ring
#pragma unroll
  for (int ks = 0; ks < RP_KS; ++ks)
#pragma unroll
    for (int tg = 0; tg < RP_TG; ++tg) asm volatile("" : "+v"(xf[ks][tg]));
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's bias writes

  // epilogue addressing: buffer resources over the panel's rows of the output (and residual); this lane's read-back
  // chunks of a 16-row block (rp_rows16): row and 16-B chunk of chunk index lane + 64 i
  half_t* const wscr = reinterpret_cast<half_t*>(ldsb + RP_OFF_SCR + wave * RP_SCR);
  const int out_ld = p.out_ld, res_ld = p.res_ld;
  const __amdgpu_buffer_rsrc_t ro =
      rp_rsrc(reinterpret_cast<half_t*>(p.out) + (size_t)m0 * out_ld, ((long long)(rows - 1) * out_ld + N) * 2);
  const __amdgpu_buffer_rsrc_t rr =
      RES ? rp_rsrc(p.res + (size_t)m0 * res_ld, ((long long)(rows - 1) * res_ld + N) * 2) : ro;
  int erow[RP_CPT], ecol[RP_CPT];
#pragma unroll
  for (int i = 0; i < RP_CPT; ++i) {
    const int idx = lane + 64 * i;
    erow[i] = 32 * wave + idx / RP_CPR;
    ecol[i] = (idx % RP_CPR) * 8;
  }

  // (no static wave priority here: raising the younger wave of each SIMD, as conv_glds_kernel does, measured
  // 56-58 us against 54-56 us without on the flagship launch)
  int rpos = 0;
  for (int c = 0; c < nch; ++c) {
    f4 acc[RP_TG][RP_NB];
#pragma unroll
    for (int tg = 0; tg < RP_TG; ++tg)
#pragma unroll
      for (int nb = 0; nb < RP_NB; ++nb) acc[tg][nb] = f4{};
#pragma unroll
    for (int kt = 0; kt < RP_KT; ++kt) {
      if (kt < KT) {
        // this wave's pieces of the slot have landed (the RP_NS - 2 younger slots may stay in flight), then all waves'
        // With the full five slots per chunk, the previous chunk's epilogue lies between this slot's pieces and this
        // wait for every slot but the chunk's last: its RP_EST stores (exactly that many in every wave: rp_rows16 is
        // branch-free) were all issued after the pieces, so they may stay in flight as well.  Shorter chunks keep the
        // plain count, which only waits for more
        if (KT == RP_KT && c > 0 && kt < RP_KT - 1)
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"((RP_NS - 2) * RP_PPW + RP_EST) : "memory");
        else
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"((RP_NS - 2) * RP_PPW) : "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        const half_t* st = lds + rpos * RP_SLOT_H;
        // the slot's two K-steps as 2 x RP_NB groups (group gq: W column block gq % RP_NB of K-step gq / RP_NB against
        // the wave's RP_TG row fragments); W fragments run RP_PFD groups ahead of their MFMAs in a small queue (the
        // panel and the accumulator leave no room for a K-step's ten at once).  Every wave is past the previous
        // slot, so its ring position takes the slot RP_NS - 1 ahead: one piece after each of the first RP_PPW groups,
        // issued under the MFMAs instead of ahead of them
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
            acc[tg][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wq[gq % (RP_PFD + 1)], xf[2 * kt + gq / RP_NB][tg],
                                                                 acc[tg][nb], 0, 0, 0);
          if (gq < RP_PPW) issue_piece(gq);
        }
        issue_next();
        // pin that order (the scheduler otherwise sinks each W read to just before its MFMAs, which then wait out
        // the LDS latency every two groups): the reads up front, then per group the read RP_PFD groups ahead, the
        // group's MFMAs and its DMA piece
        __builtin_amdgcn_sched_group_barrier(0x100, RP_PFD, 0);
        rp_pin_groups<G>();
        rpos = rpos + 1 == RP_NS ? 0 : rpos + 1;
      }
    }
    // acc[tg][nb] lane l: panel row 32 wave + 16 tg + (l & 15), columns 160 c + 16 nb + 4 (l >> 4) + q.  A block's
    // offsets carry the row guard (range check of the panel's resource) and the column guard
    const int n0 = c * RP::TBN;
#pragma unroll
    for (int tg = 0; tg < RP_TG; ++tg) {
      unsigned vo[RP_CPT], rf[RP_CPT];
#pragma unroll
      for (int i = 0; i < RP_CPT; ++i) {
        const int row = erow[i] + 16 * tg, n = n0 + ecol[i];
        vo[i] = n < N ? (unsigned)(row * out_ld + n) * 2u : RP_OOB;
        rf[i] = RES && n < N ? (unsigned)(row * res_ld + n) * 2u : RP_OOB;
      }
      rp_rows16<RES>(acc[tg], wscr, bias_s + n0, ro, rr, vo, rf);
    }
  }
  // the trailing pieces (zeros) must land before the workgroup's LDS is released
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

template <bool RES>
int rowpanel_launch(const Params& p, hipStream_t s) {
  static std::atomic<unsigned long long> attr_set{0};   // per device: the dynamic-LDS cap, once
  if (int e = ensure_dyn_lds((const void*)conv_rowpanel_kernel<RES>, RP_LDS, attr_set, "conv2d")) return e;
  hipLaunchKernelGGL((conv_rowpanel_kernel<RES>), dim3(p.tiles_m), dim3(RP_NT), RP_LDS, s, p);
  return check_launch("conv_rowpanel");
}

}  // namespace

namespace conv {

int launch_rowpanel(const Params& p, hipStream_t s) {
  return p.res ? rowpanel_launch<true>(p, s) : rowpanel_launch<false>(p, s);
}

}  // namespace conv
}  // namespace sdk
