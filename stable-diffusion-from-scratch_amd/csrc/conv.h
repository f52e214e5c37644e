// Implicit-GEMM convolution / GEMM for gfx950 (MI355X), fp16 in, fp32 accumulate on MFMA.
//
// One kernel covers every conv and Linear of the UNet and the VAE decoder:
//   out[m, n] = sum_k A[m, k] * W[n, k] + epilogue
// m = output pixel (b, oy, ox) of an NHWC tensor, k = (segment, tap, channel).
//
// Tile: 128(M) x 128(N) x 64(K), 256 threads = 4 waves in 2x2, each wave a
// 64x64 sub-tile = 2x2 v_mfma_f32_32x32x16_f16.  A and W tiles are staged
// global -> registers -> LDS (double buffer, one barrier per K step); the
// register stage is where the A prologue runs: channel-concat source select,
// nearest-x2 upsample indexing, GroupNorm affine + SiLU and zero padding.  The
// next tile's global loads are issued before the current tile's MFMAs and
// written to LDS after them (issue-early / write-late).  LDS rows are 128 B,
// XOR-swizzled on the 16-B chunk index with (row>>1)&7 so the MFMA fragment
// reads (ds_read_b128, 16 distinct rows per lane group) are conflict-free.
// The epilogue adds bias and the per-(batch, channel) timestep-embedding
// broadcast in registers, optionally pairs (x, gate) columns for GEGLU,
// stages the fp16 tile through LDS and writes it with 16-B coalesced stores
// fused with the residual add.  Low-parallelism shapes (the 16x16 / 8x8 UNet
// levels) split K across workgroups into fp32 slabs reduced by a second kernel.
//
// Shared declarations of the conv units: the launch parameters, the tile constants, the variant table's rows and
// the typed launchers through which the planner (conv_plan.hip) reaches the kernels of conv_small.hip and of the
// tile-kernel parts (conv_tile.hip, conv_tile.h).  Seg and Params live in a named namespace: one type in every unit.
#pragma once
#include <algorithm>
#include <string>
#include <type_traits>
#include <cstdio>
#include <cstdlib>

#include "common.h"

namespace sdk {
namespace conv {

constexpr int BM = 128, BN = 128, BK = 64, NT = 256;
constexpr int TILE_H = BM * BK;          // halfs per A (or B) tile
constexpr int CT_LD = BN + 8;            // epilogue LDS row stride (halfs)

struct Seg {
  const half_t* src0;
  const half_t* src1;
  const float* gscale;
  const float* gshift;
  int c_split, cin, cin_pad, ld0, ld1;
  int h, w, ksize, stride, pad, upsample, silu;
  int k_off;            // first packed-K column of this segment
  int tiles_per_tap;    // cin_pad / BK
  int kt_begin;         // first global K tile of this segment
};

struct Params {
  Seg seg[2];
  int nseg, kt_total;
  int M, N, Npad, batch, ho, wo, hw_out;
  const half_t* W;
  int ldw, wrows;       // packed weight rows (>= N); reads beyond are clamped
  long long wbs;        // per-image weights: W of image b at W + b * wbs (0: one W); LDS-DMA kernels only
  const float* bias;
  const float* row_bias;
  int rb_ld;
  const half_t* res;
  int res_ld;
  void* out;
  int out_ld, out_mode;
  float* partial;       // split-K slabs [split][M][Npad]
  int split, kt_per_split;
  int tiles_m, tiles_n;
  int variant;          // 0: register-staged 128x128 (A transforms); 2/3/4: LDS-DMA 256x256 / 256x128 / 128x128
  int act;              // epilogue activation after bias / embedding, before the residual (sdk_conv_act);
                        // only the register-staged kernel and the split-K reduce apply it (act forces
                        // variant 0), so the LDS-DMA kernels' epilogues carry no activation code
  int nomask;           // segment 0 has every tap in range (pad 0, no pad_end / upsample, cin % 64 == 0):
                        // the LDS-DMA A gather is a lane base + a scalar tap offset, no masks
  float2* gnp;          // GroupNorm statistics of the fp16 output: [batch][gn_nch][N] (mean, M2) over
  int gn_nch;           // hw_out / gn_nch rows each (one chunk = one M-tile, or 64 rows of the split-K reduce)
  // in-launch split-K (LDS-DMA tile kernels, split == 2): the K halves of a tile combine inside the launch;
  // partial = one fp32 accumulator blob per (tile, half), tcnt = per-tile arrival counters (left zero)
  int inl;
  unsigned* tcnt;
  int gm;               // unsplit plans: tiles visited in groups of gm M-panels, N-tile major inside a group
  unsigned long long* stamps;   // diagnostics build only: 8 shader-clock stamps per workgroup, or null
  int stamps_rt;                // diagnostics: slots 6 / 7 = s_memrealtime at entry / end (SDK_CONV_STAMPS=2)
  int simple;           // token GEMM (one segment, 1x1 stride 1, no masks, one source): linear A / W K offsets
  // phase form of nearest-x2 + 3x3 (sdk_conv_args.upsample_phase): four 2x2 convs over the zero-bordered low-res
  // image, one per output parity (a, b).  GEMM rows are phase major, each phase's ph_rows = batch * hw_out rows
  // padded to ph_rows_pad (a multiple of the M-tile, so no tile straddles two phases' weights): row
  // m = phase * ph_rows_pad + (img * ho + i) * wo + j gathers the 2x2 window at (i + a, j + b) and stores to
  // output pixel (img, 2i + a, 2j + b); ho / wo / hw_out are the LOW-RES extents, M = 4 * ph_rows_pad
  int phase, ph_rows, ph_rows_pad;
};

// direct (<= DC_MAXN output channels) and skinny (<= SK_MAXM rows) kernels of conv_small.hip
constexpr int DC_TX = 32, DC_LD = BK + 8;
constexpr int DC_MAXN = 8;
constexpr int SK_MAXM = 64, SK_PF = 8;

// ---------------------------------------------------------------------- the variant table
// One row per variant id; the planner, the part launchers, the dispatch of sdk_conv2d and sdk_kernel_name
// all read it, and nothing else says what an id means.  A row's columns:
//   id | kernel family | config type (its TBM x TBN is the tile) | DBG mask (DIAG only) |
//   workgroups per CU for the planner's fill estimate (not Cfg::OCC: 4 shares a CU at OCC 1) |
//   whether the epilogue pairs the (x, gate) halves of a GEGLU projection | sdk_kernel_name
// The sublist a row sits in is the conv_tile.hip part that instantiates its kernel (P0: none).  Families: NONE no such id;
// IGEMM register-staged conv_igemm_kernel; GLDS the LDS-DMA tile conv_glds_kernel; PH32 / PH16 the phased 256x256
// conv_ph_kernel on 32x32x16 / 16x16x32; DIRECT (<= 8 output channels); SKINNY (<= 64 rows); DIAG a phased
// ablation (wrong outputs by design, launched by the diagnostics build only); RETIRED named, never planned;
// ROWPANEL the row-panel-stationary conv_rowpanel_kernel (conv_rowpanel.hip: 1x1, cin <= 320; TBM x TBN is the
// 256-row panel and the 160-column W chunk of its N loop), reached only when forced or tuned, never scored.
enum class Fam { NONE, IGEMM, GLDS, PH32, PH16, DIRECT, SKINNY, DIAG, RETIRED, ROWPANEL };

// variant 5 (256x320 on 32x32x16, 16 waves) spilled at the 128-VGPR cap of 4 waves per SIMD; its row keeps the
// name and carries the config of 22, the same tile on 16x16x32 (8 to 16 B/lane of scratch: not spill-free either), which
// a forced 5 runs as after a one-time warning.  36 / 37 (halo tiles) and 39 (the 8-wave 256x320 on 32x32x16, spilled,
// never built) have no row: unknown.  41 .. 48 have none either: tests/golden/conv_plans.npz records them as unknown
// (names up to 48, forced ids up to 43), so the first id a new kernel can take is 49.
#define SDK_CONV_VARIANTS_P0(X, P)                                                                      \
  X(P, 0, IGEMM, CfgIgemm, 0, 2, true, "conv_igemm_kernel")                                             \
  X(P, 5, RETIRED, Cfg256x320m, 0, 1, false, "conv_glds_kernel<Cfg<256,320,8,2>>")                      \
  X(P, 34, DIRECT, CfgUntiled, 0, 1, false, "conv_direct_kernel")                                       \
  X(P, 35, SKINNY, CfgUntiled, 0, 1, false, "conv_skinny_kernel")                                       \
  X(P, 49, ROWPANEL, CfgRowPanel, 0, 1, false, "conv_rowpanel_kernel")
#define SDK_CONV_VARIANTS_P1(X, P)                                                                      \
  X(P, 2, GLDS, Cfg256x256, 0, 1, true, "conv_glds_kernel<Cfg<256,256,2,4>>")                           \
  X(P, 3, GLDS, Cfg256x128, 0, 1, true, "conv_glds_kernel<Cfg<256,128,4,2>>")                           \
  X(P, 4, GLDS, Cfg128x128, 0, 2, true, "conv_glds_kernel<Cfg<128,128,2,2>>")                           \
  X(P, 6, GLDS, Cfg256x160, 0, 1, false, "conv_glds_kernel<Cfg<256,160,8,1>>")                          \
  X(P, 7, GLDS, Cfg128x320, 0, 1, false, "conv_glds_kernel<Cfg<128,320,4,2>>")
#define SDK_CONV_VARIANTS_P2(X, P)                                                                      \
  X(P, 16, GLDS, Cfg128x128r4, 0, 1, true, "conv_glds_kernel<Cfg<128,128,2,2,4>>")                      \
  X(P, 17, GLDS, Cfg256x128r3, 0, 1, true, "conv_glds_kernel<Cfg<256,128,4,2,3>>")                      \
  X(P, 18, GLDS, Cfg128x128r3, 0, 1, true, "conv_glds_kernel<Cfg<128,128,2,2,3>>")                      \
  X(P, 19, GLDS, Cfg128x256r3, 0, 1, true, "conv_glds_kernel<Cfg<128,256,2,4,3>>")                      \
  X(P, 22, GLDS, Cfg256x320m, 0, 1, false, "conv_glds_kernel<Cfg<256,320,8,2,2,m16>>")                  \
  X(P, 23, GLDS, Cfg128x320m, 0, 1, false, "conv_glds_kernel<Cfg<128,320,4,2,2,m16>>")
#define SDK_CONV_VARIANTS_P3(X, P)                                                                      \
  X(P, 24, GLDS, Cfg256x160m, 0, 1, false, "conv_glds_kernel<Cfg<256,160,8,1,2,m16>>")                  \
  X(P, 25, GLDS, Cfg128x256r3m, 0, 1, true, "conv_glds_kernel<Cfg<128,256,2,4,3,m16>>")                 \
  X(P, 26, GLDS, Cfg128x128r3m, 0, 1, true, "conv_glds_kernel<Cfg<128,128,2,2,3,m16>>")                 \
  X(P, 31, GLDS, Cfg128x160o2m, 0, 2, false, "conv_glds_kernel<Cfg<128,160,4,1,2,m16,occ2>>")           \
  X(P, 32, GLDS, Cfg128x128o2m, 0, 2, true, "conv_glds_kernel<Cfg<128,128,2,2,2,m16,occ2>>")            \
  X(P, 33, GLDS, Cfg128x160r4m, 0, 1, false, "conv_glds_kernel<Cfg<128,160,4,1,4,m16>>")
// the ablations are not named (sdk_kernel_name: "unknown"): no DMA, no MFMA, DMA from the zero page, no epilogue
// stores, W / A from the zero page, no W / A DMA issued, A DMAs read W rows (cheap addressing, L2), A DMAs read
// the centre tap (no masks / halo)
#define SDK_CONV_VARIANTS_P4(X, P)                                                                      \
  X(P, 8, PH32, PhCfg8, 0, 1, true, "conv_ph_kernel<256x256,ring8>")                                    \
  X(P, 9, PH32, PhCfg10, 0, 1, true, "conv_ph_kernel<256x256,ring10>")                                  \
  X(P, 20, PH16, PhCfg8, 0, 1, true, "conv_ph_kernel<256x256,ring8,m16>")                               \
  X(P, 21, PH16, PhCfg10, 0, 1, true, "conv_ph_kernel<256x256,ring10,m16>")                             \
  X(P, 10, DIAG, PhCfg8, 1, 1, true, "unknown")                                                         \
  X(P, 11, DIAG, PhCfg8, 2, 1, true, "unknown")                                                         \
  X(P, 12, DIAG, PhCfg8, 4, 1, true, "unknown")                                                         \
  X(P, 13, DIAG, PhCfg8, 64, 1, true, "unknown")                                                        \
  X(P, 14, DIAG, PhCfg8, 16, 1, true, "unknown")                                                        \
  X(P, 15, DIAG, PhCfg8, 32, 1, true, "unknown")                                                        \
  X(P, 27, DIAG, PhCfg8, 128, 1, true, "unknown")                                                       \
  X(P, 28, DIAG, PhCfg8, 256, 1, true, "unknown")                                                       \
  X(P, 29, DIAG, PhCfg8, 512, 1, true, "unknown")                                                       \
  X(P, 30, DIAG, PhCfg8, 1024, 1, true, "unknown")
// 8-wave 256-row tiles on 16x16x32 (64 / 128-row wave tiles)
#define SDK_CONV_VARIANTS_P5(X, P)                                                                      \
  X(P, 38, GLDS, Cfg256x320w8m, 0, 1, false, "conv_glds_kernel<Cfg<256,320,4,2,2,m16>>")                \
  X(P, 40, GLDS, Cfg256x256w8m, 0, 1, true, "conv_glds_kernel<Cfg<256,256,2,4,2,m16>>")
#define SDK_CONV_VARIANTS(X)                                                                            \
  SDK_CONV_VARIANTS_P0(X, 0) SDK_CONV_VARIANTS_P1(X, 1) SDK_CONV_VARIANTS_P2(X, 2) SDK_CONV_VARIANTS_P3(X, 3) \
  SDK_CONV_VARIANTS_P4(X, 4) SDK_CONV_VARIANTS_P5(X, 5)
constexpr int kVariantIds = 50;      // ids are 0 .. 49 (a row past the end does not compile)
constexpr int kRetiredRunsAs = 22;

#ifdef SDK_CONV_DIAGNOSTICS
constexpr bool kDiagnostics = true;
#else
constexpr bool kDiagnostics = false;
#endif

#define SDK_HIDDEN __attribute__((visibility("hidden")))
// conv_small.hip: the register-staged kernel, the two split-K reduces, the direct and the skinny kernel
SDK_HIDDEN int launch_igemm(const Params& p, hipStream_t s);
SDK_HIDDEN int launch_splitk_reduce(const Params& p, hipStream_t s);
SDK_HIDDEN int launch_splitk_reduce_gn(const Params& p, hipStream_t s);
SDK_HIDDEN int launch_direct(const Params& p, hipStream_t s);
SDK_HIDDEN int launch_skinny(const Params& p, hipStream_t s);
// conv_rowpanel.hip: the row-panel-stationary kernel
SDK_HIDDEN int launch_rowpanel(const Params& p, hipStream_t s);
// conv_tile.hip, one object per part k (-DSDK_CONV_PART=k): the tile kernels of the rows of SDK_CONV_VARIANTS_Pk
#define SDK_PART_DECL(k) SDK_HIDDEN int launch_part##k(int v, const Params& p, hipStream_t s)
SDK_PART_DECL(1); SDK_PART_DECL(2); SDK_PART_DECL(3); SDK_PART_DECL(4); SDK_PART_DECL(5);

}  // namespace conv
using namespace conv;
}  // namespace sdk
