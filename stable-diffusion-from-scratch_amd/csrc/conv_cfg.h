// The constexpr tile configurations of the conv tile kernels (conv_tile.h).  No device code: the planner
// (conv_plan.hip) reads TBM / TBN of the variant table's config types from here.
#pragma once
#include "conv.h"

namespace sdk {
namespace {

// per-wave LDS scratch of the LDS-transposed epilogue (conv_tile.h: epilogue_lds)
constexpr int EPI_RS = 72;                 // scratch row stride (halfs) = 144 B
constexpr int EPI_BYTES = 32 * EPI_RS * 2;  // per-wave scratch

template <int BM_, int BN_, int WM_, int WN_, int NS_ = 2, bool M16_ = false, int OCC_ = 1>
struct Cfg {
  static constexpr int TBM = BM_, TBN = BN_, WM = WM_, WN = WN_;
  static constexpr int NS = NS_;                         // LDS ring stages (NS - 1 K-steps of DMA in flight)
  static constexpr bool M16 = M16_;                      // v_mfma_f32_16x16x32_f16 instead of 32x32x16
  static constexpr int OCC = OCC_;                       // workgroups meant to share a CU (LDS and VGPR budget)
  static constexpr int NW = WM * WN, NT = NW * 64;
  static constexpr int TM = TBM / WM, TN = TBN / WN;
  static constexpr int FM = TM / 32, FN = TN / 32;
  static constexpr int FM16 = TM / 16, FN16 = TN / 16;
  static constexpr int ROWS = TBM + TBN;                 // LDS rows (128 B) per stage
  static constexpr int STAGE_H = ROWS * BK;              // halfs per stage
  static constexpr int NINSTR = ROWS / 8;                // 1-KiB DMA pieces per stage
  static constexpr int GPW = (NINSTR + NW - 1) / NW;     // pieces per wave (padded: the same count in
                                                         // every wave keeps the vmcnt immediate exact)
  static_assert(TBM % 8 == 0 && TBN % 8 == 0, "A/B boundary must align to an 8-row piece");
  static constexpr int RING_BYTES = NS * STAGE_H * 2 + (GPW * NW > NINSTR ? 1024 : 0);  // + dummy slot
  static constexpr int LDS_BYTES = RING_BYTES + 2 * TBN * 4;   // + staged bias / embedding row
  static_assert(LDS_BYTES * OCC <= 160 * 1024, "OCC rings must fit the 160 KiB LDS");
  static_assert(RING_BYTES / NW >= EPI_BYTES + TM / 16 * TN * 8, "per-wave epilogue scratch + parked GN statistics");
  static_assert(TBN <= NT, "one staged bias element per thread");
};

using Cfg256x256 = Cfg<256, 256, 2, 4>;
using Cfg256x128 = Cfg<256, 128, 4, 2>;
using Cfg128x128 = Cfg<128, 128, 2, 2>;
// N = 320 / 640 / 960 levels of SD: 32x160 wave tiles (5 MFMA tiles per wave)
using Cfg256x160 = Cfg<256, 160, 8, 1>;
using Cfg128x320 = Cfg<128, 320, 4, 2>;
// deeper rings for tiles whose K-step is shorter than the DMA latency (~1 us issue -> landed):
// 128x128 (512 MFMA cycles per K-step per CU) and 256x128 / 128x256 (1024)
using Cfg128x128r4 = Cfg<128, 128, 2, 2, 4>;   // 128 KiB
using Cfg128x128r3 = Cfg<128, 128, 2, 2, 3>;   // 96 KiB
using Cfg256x128r3 = Cfg<256, 128, 4, 2, 3>;   // 144 KiB
using Cfg128x256r3 = Cfg<128, 256, 2, 4, 3>;   // 144 KiB
// the same tiles on v_mfma_f32_16x16x32_f16 (on random data the 16x16 shape holds a higher clock
// under load than 32x32 at equal cycles per FLOP: MI355X_MICROARCH.md 'DVFS give-back' (7))
using Cfg256x320m = Cfg<256, 320, 8, 2, 2, true>;
using Cfg128x320m = Cfg<128, 320, 4, 2, 2, true>;
using Cfg256x160m = Cfg<256, 160, 8, 1, 2, true>;
using Cfg128x256r3m = Cfg<128, 256, 2, 4, 3, true>;
using Cfg128x128r3m = Cfg<128, 128, 2, 2, 3, true>;
// short-K token GEMMs (K = 320-1280): two workgroups per CU, so one's epilogue (store drain) runs
// under the other's K loop — a 2-stage 128x160 / 128x128 ring is 74 / 65 KiB
using Cfg128x160o2m = Cfg<128, 160, 4, 1, 2, true, 2>;
using Cfg128x128o2m = Cfg<128, 128, 2, 2, 2, true, 2>;
using Cfg128x160r4m = Cfg<128, 160, 4, 1, 4, true>;      // one workgroup, 3 K-steps of DMA in flight
// 8-wave 256-row tiles with 64-row (256x320) / 128-row (256x256) wave tiles at two waves per SIMD (256 VGPRs): half
// the LDS fragment reads per MFMA of the 16-wave 256x320 (each B fragment feeds 4 or 8 MFMAs instead of 2) and room
// for the fragment reads of the next group to be in flight under the current one's MFMAs (round-6 ablation, profiles/
// r6_conv_ablation.txt: the 16-wave 256x320 runs at 1.16 PF/s with no DMA at all — its LDS-read -> MFMA chain, not
// the fill, bounds it)
using Cfg256x320w8m = Cfg<256, 320, 4, 2, 2, true>;
using Cfg256x256w8m = Cfg<256, 256, 2, 4, 2, true>;

// ring of S half-tile slots, DMA issued D phases ahead (conv_tile.h: conv_ph_kernel)
template <int S_, int D_>
struct PhCfg {
  static constexpr int S = S_, D = D_;
  static constexpr int RING_BYTES = S * 128 * BK * 2;
  static constexpr bool VEC = RING_BYTES + 2 * 256 * 4 <= 160 * 1024;   // room for the staged bias / embedding
  static constexpr int LDS_BYTES = RING_BYTES + (VEC ? 2 * 256 * 4 : 0);
  static_assert(S >= D + 2 && D >= 2 && RING_BYTES <= 160 * 1024, "ring too small / too large");
};
using PhCfg8 = PhCfg<8, 6>;
using PhCfg10 = PhCfg<10, 8>;

// the row-panel-stationary kernel (conv_rowpanel.hip): a workgroup keeps a TBM-row panel of A in registers and walks
// N in TBN-column chunks of W; MAXK bounds the panel's register cost (MAXK / 4 VGPRs per lane), MAXN the bias
// vector staged in LDS for the whole launch
struct CfgRowPanel { static constexpr int TBM = 256, TBN = 160, MAXK = 320, MAXN = 2560; };

// the tile of a variant-table row's config type
struct CfgIgemm { static constexpr int TBM = BM, TBN = BN; };
struct CfgUntiled { static constexpr int TBM = 0, TBN = 0; };   // direct / skinny: no BM x BN tiling
template <class CF> struct TileOf { static constexpr int TBM = CF::TBM, TBN = CF::TBN; };
template <int S, int D> struct TileOf<PhCfg<S, D>> { static constexpr int TBM = 256, TBN = 256; };

}  // namespace
}  // namespace sdk
