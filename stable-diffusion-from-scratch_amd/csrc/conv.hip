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
#include <algorithm>
#include <string>
#include <type_traits>
#include <cstdio>
#include <cstdlib>

#include "common.h"

#ifndef SDK_CONV_PART
#define SDK_CONV_PART -1
#endif
#define SDK_PART(k) (SDK_CONV_PART < 0 || SDK_CONV_PART == (k))

namespace sdk {
namespace {

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

// epilogue activation (CLIP's quick_gelu x*sigmoid(1.702x), transformers activations.py QuickGELUActivation)
__device__ __forceinline__ float act_fn(int act, float x) {
  if (act == SDK_ACT_QUICK_GELU) return x * __builtin_amdgcn_rcpf(1.0f + __expf(-1.702f * x));
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

// A-row context: per thread 4 rows (r = (tid>>3) + 32*i), fixed over the K loop.
struct RowCtx {
  int b[4], oy[4], ox[4];
  bool valid[4];
};

__device__ __forceinline__ void load_a(const Params& p, const RowCtx& rc, int kt, int chunk, h8 (&va)[4],
                                       bool (&ok)[4], int& cglob, int& segi) {
  segi = (p.nseg > 1 && kt >= p.seg[1].kt_begin) ? 1 : 0;
  const Seg& s = p.seg[segi];
  const int local = kt - s.kt_begin, taps = s.ksize * s.ksize;
  const int cblk = local / taps, tap = local - cblk * taps;   // K order: channel block, then tap
  const int c = cblk * BK + chunk * 8;
  const int ky = tap / s.ksize, kx = tap - ky * s.ksize;
  cglob = c;
  const bool cok = c < s.cin;
  const half_t* base;
  int ld, cc;
  if (c < s.c_split) { base = s.src0; ld = s.ld0; cc = c; }
  else { base = s.src1; ld = s.ld1; cc = c - s.c_split; }
  const int lh = s.upsample ? 2 * s.h : s.h, lw = s.upsample ? 2 * s.w : s.w;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int iy = rc.oy[i] * s.stride - s.pad + ky;
    int ix = rc.ox[i] * s.stride - s.pad + kx;
    bool in = rc.valid[i] && cok && iy >= 0 && iy < lh && ix >= 0 && ix < lw;
    ok[i] = in;
    if (s.upsample) { iy >>= 1; ix >>= 1; }
    h8 v = {};
    if (in) v = ldg16(base + ((size_t)((size_t)rc.b[i] * s.h + iy) * s.w + ix) * ld + cc);
    va[i] = v;
  }
}

// GroupNorm affine + SiLU on the staged registers; zero after the transform
// (the conv pads the *normalised* activation).
__device__ __forceinline__ void transform_a(const Params& p, const RowCtx& rc, int segi, int c, h8 (&va)[4],
                                            const bool (&ok)[4]) {
  const Seg& s = p.seg[segi];
  if (s.gscale == nullptr && !s.silu) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (!ok[i]) va[i] = h8{};
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    h8 v = va[i];
    if (ok[i]) {
      float sc[8], sh[8];
      if (s.gscale) {
        const f4* ps = reinterpret_cast<const f4*>(s.gscale + (size_t)rc.b[i] * s.cin + c);
        const f4* pt = reinterpret_cast<const f4*>(s.gshift + (size_t)rc.b[i] * s.cin + c);
        f4 s0 = ps[0], s1 = ps[1], t0 = pt[0], t1 = pt[1];
        sc[0] = s0[0]; sc[1] = s0[1]; sc[2] = s0[2]; sc[3] = s0[3];
        sc[4] = s1[0]; sc[5] = s1[1]; sc[6] = s1[2]; sc[7] = s1[3];
        sh[0] = t0[0]; sh[1] = t0[1]; sh[2] = t0[2]; sh[3] = t0[3];
        sh[4] = t1[0]; sh[5] = t1[1]; sh[6] = t1[2]; sh[7] = t1[3];
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) { sc[j] = 1.f; sh[j] = 0.f; }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float x = (float)v[j] * sc[j] + sh[j];
        if (s.silu) x = x * __builtin_amdgcn_rcpf(1.0f + __expf(-x));
        v[j] = (half_t)x;
      }
    } else {
      v = h8{};
    }
    va[i] = v;
  }
}


// ---------------------------------------------------------------------- shared epilogue
// acc[i][j] (32x32 MFMA tile) element r of lane (fr = lane&31, fh = lane>>5):
//   row = m_w + i*32 + (r&3) + 8*(r>>2) + 4*fh, col = n_w + j*32 + fr   (block-local)
// LDS `smem` must be free (all waves past their last LDS read) on entry.
template <int FM, int FN, int TBM, int TBN, int TNT>
__device__ __forceinline__ void epilogue(const Params& p, f16v (&acc)[FM][FN], half_t* smem, int m0, int n0, int m_w,
                                         int n_w, int split_idx) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int fr = lane & 31, fh = lane >> 5;
  constexpr int CLD = TBN + 8;
  if (p.split > 1) {
    float* slab = p.partial + (size_t)split_idx * p.M * p.Npad;
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + m_w + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
          const int n = n0 + n_w + j * 32 + fr;
          if (m < p.M) slab[(size_t)m * p.Npad + n] = acc[i][j][r];
        }
    return;
  }
  const int mode = p.out_mode;
  if (mode == SDK_OUT_GEGLU_F16) {
    // weight rows of each 64-wide column pair: [x (32) | gate (32)] -> output col = (n_w + j*32)/2 + fr
    static_assert(FN % 2 == 0, "GEGLU needs an even number of 32-col tiles per wave");
#pragma unroll
    for (int jp = 0; jp < FN / 2; ++jp) {
      const int nx = n0 + n_w + jp * 64 + fr, ng = nx + 32;
      const float bx = (p.bias && nx < p.N) ? p.bias[nx] : 0.f, bg = (p.bias && ng < p.N) ? p.bias[ng] : 0.f;
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rl = m_w + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
          const float x = acc[i][2 * jp][r] + bx, g = acc[i][2 * jp + 1][r] + bg;
          smem[rl * CLD + n_w / 2 + jp * 32 + fr] = (half_t)(x * gelu_erf(g));
        }
    }
    __syncthreads();
    constexpr int OW = TBN / 2;
    const int ncol0 = n0 / 2;
    half_t* out = reinterpret_cast<half_t*>(p.out);
    for (int e = tid; e < TBM * (OW / 8); e += TNT) {
      const int rl = e / (OW / 8), c8 = (e - rl * (OW / 8)) * 8;
      const int m = m0 + rl, n = ncol0 + c8;
      if (m >= p.M || n >= p.N / 2) continue;
      h8 v = *reinterpret_cast<const h8*>(smem + rl * CLD + c8);
      if (p.res) {
        h8 rr = ldg16(p.res + (size_t)m * p.res_ld + n);
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = (half_t)((float)v[q] + (float)rr[q]);
      }
      st_out16(out + (size_t)m * p.out_ld + n, v);
    }
    return;
  }
  float bn[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const int n = n0 + n_w + j * 32 + fr;
    bn[j] = (p.bias && n < p.N) ? p.bias[n] : 0.f;
  }
  if (mode == SDK_OUT_NHWC_F16) {
    const bool uniform_b = (p.hw_out % 32) == 0;
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const int mblk = m0 + m_w + i * 32;
      const int bidx = min(mblk, p.M - 1) / p.hw_out;
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const int n = n0 + n_w + j * 32 + fr;
        float add = bn[j];
        if (p.row_bias && n < p.N && uniform_b) add += p.row_bias[(size_t)bidx * p.rb_ld + n];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rl = m_w + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
          float v = acc[i][j][r] + add;
          if (p.row_bias && n < p.N && !uniform_b) {
            const int m = min(m0 + rl, p.M - 1);
            v += p.row_bias[(size_t)(m / p.hw_out) * p.rb_ld + n];
          }
          smem[rl * CLD + n_w + j * 32 + fr] = (half_t)act_fn(p.act, v);
        }
      }
    }
    __syncthreads();
    half_t* out = reinterpret_cast<half_t*>(p.out);
    for (int e = tid; e < TBM * (TBN / 8); e += TNT) {
      const int rl = e / (TBN / 8), c8 = (e - rl * (TBN / 8)) * 8;
      const int m = m0 + rl, n = n0 + c8;
      if (m >= p.M || n >= p.N) continue;
      h8 v = *reinterpret_cast<const h8*>(smem + rl * CLD + c8);
      if (p.res) {
        h8 rr = ldg16(p.res + (size_t)m * p.res_ld + n);
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = (half_t)((float)v[q] + (float)rr[q]);
      }
      st_out16(out + (size_t)m * p.out_ld + n, v);
    }
    return;
  }
  // fp32 outputs (small: time-embedding projections, final 4/3-channel convs)
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int n = n0 + n_w + j * 32 + fr;
      if (n >= p.N) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + m_w + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
        if (m >= p.M) continue;
        const int b = m / p.hw_out;
        float v = acc[i][j][r] + bn[j];
        if (p.row_bias) v += p.row_bias[(size_t)b * p.rb_ld + n];
        v = act_fn(p.act, v);
        if (p.res) v += (float)p.res[(size_t)m * p.res_ld + n];
        float* out = reinterpret_cast<float*>(p.out);
        if (mode == SDK_OUT_NCHW_F32)
          out[((size_t)b * p.N + n) * p.hw_out + (m - b * p.hw_out)] = v;
        else
          out[(size_t)m * p.out_ld + n] = v;
      }
    }
}

#if SDK_PART(0)   // the register-staged kernel: host planner part only
__global__ void __launch_bounds__(NT, 2) conv_igemm_kernel(Params p) {
  __shared__ __attribute__((aligned(16))) half_t smem[4 * TILE_H];   // A0 A1 B0 B1 = 64 KiB
  half_t* As = smem;
  half_t* Bs = smem + 2 * TILE_H;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int ntiles = p.tiles_m * p.tiles_n;
  const int tile = xcd_remap(blockIdx.x, ntiles);
  const int tm = tile / p.tiles_n, tn = tile - tm * p.tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;
  const int kt0 = blockIdx.y * p.kt_per_split;
  const int kt1 = min(p.kt_total, kt0 + p.kt_per_split);

  const int lrow = tid >> 3, chunk = tid & 7;
  RowCtx rc;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int m = m0 + lrow + 32 * i;
    rc.valid[i] = m < p.M;
    int mm = rc.valid[i] ? m : 0;
    int b = mm / p.hw_out, rem = mm - b * p.hw_out;
    int oy = rem / p.wo;
    rc.b[i] = b; rc.oy[i] = oy; rc.ox[i] = rem - oy * p.wo;
  }
  const half_t* wrow[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) wrow[i] = p.W + (size_t)min(n0 + lrow + 32 * i, p.wrows - 1) * p.ldw + chunk * 8;

  f16v acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = f16v{};

  h8 va[4], vb[4];
  bool ok[4];
  int cglob = 0, segi = 0;

  auto load_b = [&](int kt) {
    const int si = (p.nseg > 1 && kt >= p.seg[1].kt_begin) ? 1 : 0;
    const int kcol = p.seg[si].k_off + (kt - p.seg[si].kt_begin) * BK;
#pragma unroll
    for (int i = 0; i < 4; ++i) vb[i] = ldg16(wrow[i] + kcol);
  };
  auto store_tiles = [&](int buf) {
    half_t* a = As + buf * TILE_H;
    half_t* bsh = Bs + buf * TILE_H;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = lrow + 32 * i;
      *reinterpret_cast<h8*>(a + swz(r, chunk)) = va[i];
      *reinterpret_cast<h8*>(bsh + swz(r, chunk)) = vb[i];
    }
  };

  if (kt0 < kt1) {
    load_a(p, rc, kt0, chunk, va, ok, cglob, segi);
    load_b(kt0);
    transform_a(p, rc, segi, cglob, va, ok);
    store_tiles(0);
  }
  __syncthreads();

  const int fr = lane & 31, fh = lane >> 5;
  for (int kt = kt0; kt < kt1; ++kt) {
    const int cur = (kt - kt0) & 1;
    const bool more = kt + 1 < kt1;
    if (more) {
      load_a(p, rc, kt + 1, chunk, va, ok, cglob, segi);
      load_b(kt + 1);
    }
    const half_t* a = As + cur * TILE_H;
    const half_t* bsh = Bs + cur * TILE_H;
#pragma unroll
    for (int kk = 0; kk < BK / 16; ++kk) {
      h8 fa[2], fb[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        fa[t] = *reinterpret_cast<const h8*>(a + swz(wm * 64 + t * 32 + fr, kk * 2 + fh));
        fb[t] = *reinterpret_cast<const h8*>(bsh + swz(wn * 64 + t * 32 + fr, kk * 2 + fh));
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
    if (more) {
      transform_a(p, rc, segi, cglob, va, ok);
      store_tiles(cur ^ 1);
    }
    __syncthreads();
  }

  const int m_w = wm * 64, n_w = wn * 64;
  epilogue<2, 2, BM, BN, NT>(p, acc, smem, m0, n0, m_w, n_w, blockIdx.y);
}
#endif  // SDK_PART(0)



// ---------------------------------------------------------------------- direct epilogue
// Transposed accumulator (D^T = W A^T): lane (fr = lane&31, fh = lane>>5) owns output
// pixel m = m0 + m_w + i*32 + fr; register group g (r = 4g..4g+3) of tile j holds the 4
// consecutive channels n = n0 + n_w + j*32 + 8g + 4fh + (0..3) -> one 8-byte store per
// group straight from registers (no LDS round trip, so the tile width is not bounded
// by LDS), channel-contiguous in NHWC and pixel-contiguous for the NCHW fp32 output.
template <int FM, int FN>
__device__ __forceinline__ void epilogue_direct(const Params& p, f16v (&acc)[FM][FN], int m0, int n0, int m_w,
                                                int n_w, int split_idx) {
  const int lane = threadIdx.x & 63;
  const int fr = lane & 31, fh = lane >> 5;
  const int mode = p.out_mode;
  // 16-B vector loads of the bias / embedding rows when aligned (channels come in 4s)
  const bool rb_vec = p.row_bias && !((uintptr_t)p.row_bias & 15) && !(p.rb_ld & 3);
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int m = m0 + m_w + i * 32 + fr;
    if (m >= p.M) continue;
    const int b = m / p.hw_out;
    if (p.split > 1 && !p.inl) {
      float* slab = p.partial + ((size_t)split_idx * p.M + m) * p.Npad;
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int n = n0 + n_w + j * 32 + 8 * g + 4 * fh;
          f4 v = {acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
          *reinterpret_cast<f4*>(slab + n) = v;
        }
      continue;
    }
    if (mode == SDK_OUT_GEGLU_F16) {
      half_t* out = reinterpret_cast<half_t*>(p.out) + (size_t)m * p.out_ld;
#pragma unroll
      for (int jp = 0; jp < FN / 2; ++jp)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int nx = n0 + n_w + jp * 64 + 8 * g + 4 * fh;      // x rows; gate rows = nx + 32
          const int no = (n0 + n_w) / 2 + jp * 32 + 8 * g + 4 * fh; // output channel
          if (no >= p.N / 2) continue;
          f4 bx = {0.f, 0.f, 0.f, 0.f}, bg = {0.f, 0.f, 0.f, 0.f};
          if (p.bias) {
            bx = *reinterpret_cast<const f4*>(p.bias + nx);
            bg = *reinterpret_cast<const f4*>(p.bias + nx + 32);
          }
          h4 o;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float x = acc[i][2 * jp][4 * g + q] + bx[q], gt = acc[i][2 * jp + 1][4 * g + q] + bg[q];
            o[q] = (half_t)(x * gelu_erf(gt));
          }
          if (p.res) {
            const h4 rr = *reinterpret_cast<const h4*>(p.res + (size_t)m * p.res_ld + no);
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = (half_t)((float)o[q] + (float)rr[q]);
          }
          *reinterpret_cast<h4*>(out + no) = o;
        }
      continue;
    }
    if (mode == SDK_OUT_NHWC_F16) {
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int n = n0 + n_w + j * 32 + 8 * g + 4 * fh;
          if (n >= p.N) continue;                       // N % 8 == 0 in this mode
          float v[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] = acc[i][j][4 * g + q];
          if (p.bias) {
            const f4 bb = *reinterpret_cast<const f4*>(p.bias + n);
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] += bb[q];
          }
          if (p.row_bias) {
            const float* rb = p.row_bias + (size_t)b * p.rb_ld + n;
            if (rb_vec) {
              const f4 r4 = *reinterpret_cast<const f4*>(rb);
#pragma unroll
              for (int q = 0; q < 4; ++q) v[q] += r4[q];
            } else {
#pragma unroll
              for (int q = 0; q < 4; ++q) v[q] += rb[q];
            }
          }
          h4 o;
#pragma unroll
          for (int q = 0; q < 4; ++q) o[q] = (half_t)v[q];
          if (p.res) {
            const h4 rr = *reinterpret_cast<const h4*>(p.res + (size_t)m * p.res_ld + n);
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = (half_t)((float)o[q] + (float)rr[q]);
          }
          *reinterpret_cast<h4*>(reinterpret_cast<half_t*>(p.out) + (size_t)m * p.out_ld + n) = o;
        }
      continue;
    }
    // fp32 outputs (NCHW image, token rows): any N
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = n0 + n_w + j * 32 + 8 * g + 4 * fh;
        if (n >= p.N) continue;
        float* out = reinterpret_cast<float*>(p.out);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (n + q >= p.N) continue;
          float x = acc[i][j][4 * g + q];
          if (p.bias) x += p.bias[n + q];
          if (p.row_bias) x += p.row_bias[(size_t)b * p.rb_ld + n + q];
          if (p.res) x += (float)p.res[(size_t)m * p.res_ld + n + q];
          if (mode == SDK_OUT_NCHW_F32)
            out[((size_t)b * p.N + n + q) * p.hw_out + (m - b * p.hw_out)] = x;
          else
            out[(size_t)m * p.out_ld + n + q] = x;
        }
      }
  }
}

// ---------------------------------------------------------------------- LDS-transposed epilogue
// The transposed accumulator gives each lane one pixel and 4 consecutive channels per
// register group, so direct stores are 8 B per lane into 32 different rows: store-issue
// bound (a 256x256 fp16 tile ~9 us).  For the fp16 NHWC / GEGLU outputs each wave instead
// writes a 32-pixel x (32|64)-channel block (bias / embedding / GEGLU applied in fp32) to
// its own LDS scratch (144-B rows: conflict-free 8-B writes), reads it back as 16-B row
// chunks and issues coalesced 16-B stores (+ 16-B residual loads): 64-128 contiguous
// bytes per pixel row per instruction.  Wave-private scratch: no barrier, LDS ops of one
// wave complete in order.
constexpr int EPI_RS = 72;                 // scratch row stride (halfs) = 144 B
constexpr int EPI_BYTES = 32 * EPI_RS * 2;  // per-wave scratch

// ---------------------------------------------------------------------- GroupNorm statistics in the epilogue
// The convs that produce a GroupNorm input (ResBlock conv1 / conv2, Down/Upsample, proj_out, conv_in)
// emit per-channel statistics of the fp16 values they store (after bias / embedding / residual),
// so GroupNorm needs no statistics pass over the tensor: per (image, M-tile, channel) the tile's
// (mean, M2) — Chan's parallel form; sdk_group_norm merges the tiles and the group's channels in
// double.  Register-free design (the 16-wave tiles run at a 128-VGPR cap): the epilogue's read-back
// writes the final values back into the wave's LDS scratch block, then a column pass reads the
// block per channel pair (exact two-pass mean / M2 over a few rows in registers), merges the lane
// row slices with xor shuffles (equal counts) and parks one pair per (row block, channel) in the
// wave's scratch; after the epilogue one thread per tile channel merges its column's blocks.
//
// Column pass over a block of ROWS x CH fp16 values at `blk` (row stride RS halfs); writes
// dst[c] = (mean, M2) for c < CH.
template <int ROWS, int CH, int RS>
__device__ __forceinline__ void gn_block_stats(const half_t* blk, float2* dst) {
  constexpr int CP = CH / 2, SL = 64 / CP, RPL = ROWS / SL;   // channel pairs, row slices, rows per lane
  static_assert(CP * SL == 64 && RPL * SL == ROWS, "block shape");
  const int lane = threadIdx.x & 63, cp = lane % CP, sl = lane / CP;
  const half_t* col = blk + sl * RPL * RS + 2 * cp;
  // two passes over the lane's rows (the second re-reads LDS instead of holding 2*RPL floats)
  float a0 = 0.f, a1 = 0.f;
#pragma unroll
  for (int k = 0; k < RPL; ++k) {
    const h2 v = *reinterpret_cast<const h2*>(col + k * RS);
    a0 += (float)v[0];
    a1 += (float)v[1];
  }
  float m0 = a0 * (1.f / RPL), m1 = a1 * (1.f / RPL), q0 = 0.f, q1 = 0.f;
#pragma unroll
  for (int k = 0; k < RPL; ++k) {
    const h2 v = *reinterpret_cast<const h2*>(col + k * RS);
    const float d0 = (float)v[0] - m0, d1 = (float)v[1] - m1;
    q0 = fmaf(d0, d0, q0);
    q1 = fmaf(d1, d1, q1);
  }
  float n = (float)RPL;
#pragma unroll
  for (int off = CP; off < 64; off <<= 1) {          // equal counts: mean = average, M2 += d^2 n/2
    const float mb0 = __shfl_xor(m0, off, 64), qb0 = __shfl_xor(q0, off, 64);
    const float mb1 = __shfl_xor(m1, off, 64), qb1 = __shfl_xor(q1, off, 64);
    const float d0 = mb0 - m0, d1 = mb1 - m1;
    m0 = 0.5f * (m0 + mb0);
    m1 = 0.5f * (m1 + mb1);
    q0 += qb0 + d0 * d0 * (0.5f * n);
    q1 += qb1 + d1 * d1 * (0.5f * n);
    n *= 2.f;
  }
  if (lane < CP) {
    dst[2 * cp] = make_float2(m0, q0);
    dst[2 * cp + 1] = make_float2(m1, q1);
  }
}

// after every wave parked its blocks: one thread per tile channel merges the WM waves x NBLK row
// blocks (BR rows each) of its column and stores the tile's pair; `wave_stats(w)` = wave w's
// parked array [NBLK][TN]
template <int WM, int WN, int TN, int NBLK, int BR, int TBM, int TBN, bool PH = false, class F>
__device__ __forceinline__ void gn_tile_store(const Params& p, int m0, int n0, F wave_stats) {
  const int t = threadIdx.x;
  if (t >= TBN || n0 + t >= p.N) return;
  const int wn = t / TN, c = t - wn * TN;
  float2 r = make_float2(0.f, 0.f);
  float n = 0.f;
#pragma unroll
  for (int wm = 0; wm < WM; ++wm)
#pragma unroll
    for (int k = 0; k < NBLK; ++k) {
      const float2 b = wave_stats(wm * WN + wn)[k * TN + c];
      const float dl = b.x - r.x, f = (float)BR / (n + (float)BR);
      r.x += dl * f;
      r.y += b.y + dl * dl * n * f;
      n += (float)BR;
    }
  int b0 = m0 / p.hw_out, chunk = (m0 - b0 * p.hw_out) / TBM;
  if (PH && p.phase) {   // an image's chunks: phase major, then the phase's M-tiles inside the image (equal counts)
    const int ph = m0 / p.ph_rows_pad, rp = m0 - ph * p.ph_rows_pad;
    b0 = rp / p.hw_out;
    chunk = ph * (p.hw_out / TBM) + (rp - b0 * p.hw_out) / TBM;
  }
  p.gnp[((size_t)b0 * p.gn_nch + chunk) * p.N + n0 + t] = r;
}

// split-K reduce: a lane's pivot-shifted sums over its rows (registers are plentiful there)
struct GnAcc {
  float piv[8], s1[8], s2[8];
};

__device__ __forceinline__ void gn_acc_add(GnAcc& a, const h8& v, bool first) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float x = (float)v[j];
    if (first) {
      a.piv[j] = x;
      a.s1[j] = 0.f;
      a.s2[j] = 0.f;
    }
    const float d = x - a.piv[j];
    a.s1[j] += d;
    a.s2[j] = fmaf(d, d, a.s2[j]);
  }
}

// Bias and the timestep-embedding row (row_bias of the tile's image) are staged in LDS once per
// workgroup (stage_epi_vectors, before the K loop): the epilogue reads them with ds_read instead of
// waiting on a global load per 32-row block.  ``bias_s`` / ``rb_s`` = nullptr fall back to global.
// Residual rows are loaded one block ahead (issued before the current block's LDS round trip).
template <int FM, int FN, bool GN = false, bool PH = false>
__device__ __forceinline__ void epilogue_lds(const Params& p, f16v (&acc)[FM][FN], int m0, int n0, int m_w, int n_w,
                                             half_t* wbuf, const float* bias_s = nullptr,
                                             const float* rb_s = nullptr) {
  const int lane = threadIdx.x & 63;
  const int fr = lane & 31, fh = lane >> 5;
  const bool rb_vec = p.row_bias && !((uintptr_t)p.row_bias & 15) && !(p.rb_ld & 3);
  half_t* out = reinterpret_cast<half_t*>(p.out);
  auto bias4 = [&](int n) __attribute__((always_inline)) {
    return bias_s ? *reinterpret_cast<const f4*>(bias_s + (n - n0)) : *reinterpret_cast<const f4*>(p.bias + n);
  };
  if (p.out_mode == SDK_OUT_GEGLU_F16) {
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const int mt = m0 + m_w + i * 32;
      if (mt >= p.M) continue;
#pragma unroll
      for (int jp = 0; jp < FN / 2; ++jp) {
        const int nob = (n0 + n_w) / 2 + jp * 32;   // first output channel of the block
        if (nob >= p.N / 2) continue;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int nx = n0 + n_w + jp * 64 + 8 * g + 4 * fh;
          f4 bx = {0.f, 0.f, 0.f, 0.f}, bg = {0.f, 0.f, 0.f, 0.f};
          if (bias_s || p.bias) {
            bx = bias4(nx);
            bg = bias4(nx + 32);
          }
          h4 o;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float x = acc[i][2 * jp][4 * g + q] + bx[q], gt = acc[i][2 * jp + 1][4 * g + q] + bg[q];
            o[q] = (half_t)(x * gelu_erf(gt));
          }
          *reinterpret_cast<h4*>(wbuf + fr * EPI_RS + 8 * g + 4 * fh) = o;
        }
        // read back: 4 lanes x 16 B per pixel row, 16 rows per instruction
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const int row = r * 16 + (lane >> 2), c8 = lane & 3;
          h8 v = *reinterpret_cast<const h8*>(wbuf + row * EPI_RS + c8 * 8);
          const int m = mt + row, no = nob + c8 * 8;
          if (m < p.M && no < p.N / 2) {
            if (p.res) {
              const h8 rr = *reinterpret_cast<const h8*>(p.res + (size_t)m * p.res_ld + no);
#pragma unroll
              for (int q = 0; q < 8; ++q) v[q] = (half_t)((float)v[q] + (float)rr[q]);
            }
            st_out16(out + (size_t)m * p.out_ld + no, v);
          }
        }
      }
    }
    return;
  }
  // fp16 NHWC: blocks (i, jp) of 32 pixels x (32|64) channels, flattened so the residual rows of
  // block q+1 are in flight while block q makes its LDS round trip
  // channel-block major (jp outer, 32-pixel block i inner): one block's GN statistics live at a time
  constexpr int NJP = (FN + 1) / 2, NBLK = FM * NJP;
  h8 rcur[4], rnext[4];
  constexpr int TN = FN * 32;
  float2* gst = reinterpret_cast<float2*>(wbuf + EPI_BYTES / 2);   // GN: parked [FM][TN] (mean, M2)
  auto block_geom = [&](int q, int& mt, int& nb, int& nt) __attribute__((always_inline)) {
    const int jp = (q / FM) * 2, i = q % FM;
    mt = m0 + m_w + i * 32;
    nb = n0 + n_w + jp * 32;
    nt = (FN - jp >= 2) ? 2 : 1;
  };
  auto load_res = [&](int q, h8 (&rr)[4]) __attribute__((always_inline)) {
    int mt, nb, nt;
    block_geom(q, mt, nb, nt);
    const int lpr = nt * 4, rpi = 64 / lpr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      rr[r] = h8{};
      if (r >= 2 * nt) continue;
      const int m = mt + r * rpi + lane / lpr, n = nb + (lane % lpr) * 8;
      if (m < p.M && n < p.N) rr[r] = *reinterpret_cast<const h8*>(p.res + (size_t)m * p.res_ld + n);
    }
  };
  // one block ahead when the accumulators leave room (<= 96 VGPRs with the prefetch), else the
  // block's own residual rows are issued before its LDS round trip
  constexpr bool AHEAD = FM * FN * 16 + 32 <= 96;
  if (p.res && AHEAD) load_res(0, rcur);
#pragma unroll
  for (int q = 0; q < NBLK; ++q) {
    int mt, nb, nt;
    block_geom(q, mt, nb, nt);
    const int jp = (q / FM) * 2, i = q % FM;
    if (p.res && AHEAD && q + 1 < NBLK) load_res(q + 1, rnext);
    if (p.res && !AHEAD) load_res(q, rcur);
    if (mt < p.M && nb < p.N) {
      const int mw = min(mt + fr, p.M - 1);   // the writer lane's pixel (clamped: its row is never stored)
      const int bw = mw / p.hw_out;
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        if (jj >= nt) continue;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int n = nb + jj * 32 + 8 * g + 4 * fh;
          float v[4];
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) v[qq] = acc[i][jp + jj][4 * g + qq];
          if (rb_s) {                             // staged vectors (zeros where absent): branch-free
            const f4 bb = *reinterpret_cast<const f4*>(bias_s + (n - n0));
            const f4 r4 = *reinterpret_cast<const f4*>(rb_s + (n - n0));
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) v[qq] = (v[qq] + bb[qq]) + r4[qq];
          } else if (n < p.N) {                   // N % 8 == 0 in this mode
            if (p.bias) {
              const f4 bb = bias4(n);
#pragma unroll
              for (int qq = 0; qq < 4; ++qq) v[qq] += bb[qq];
            }
            if (p.row_bias) {
              if (rb_s) {
                const f4 r4 = *reinterpret_cast<const f4*>(rb_s + (n - n0));
#pragma unroll
                for (int qq = 0; qq < 4; ++qq) v[qq] += r4[qq];
              } else {
                const float* rb = p.row_bias + (size_t)bw * p.rb_ld + n;
                if (rb_vec) {
                  const f4 r4 = *reinterpret_cast<const f4*>(rb);
#pragma unroll
                  for (int qq = 0; qq < 4; ++qq) v[qq] += r4[qq];
                } else {
#pragma unroll
                  for (int qq = 0; qq < 4; ++qq) v[qq] += rb[qq];
                }
              }
            }
          }
          h4 o;
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) o[qq] = (half_t)v[qq];
          *reinterpret_cast<h4*>(wbuf + fr * EPI_RS + jj * 32 + 8 * g + 4 * fh) = o;
        }
      }
      // read back: nt*4 lanes x 16 B per pixel row
      const int lpr = nt * 4, rpi = 64 / lpr;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (r >= 2 * nt) continue;
        const int row = r * rpi + lane / lpr, c8 = lane % lpr;
        h8 v = *reinterpret_cast<const h8*>(wbuf + row * EPI_RS + c8 * 8);
        const int m = mt + row, n = nb + c8 * 8;
        if (p.res) {
#pragma unroll
          for (int qq = 0; qq < 8; ++qq) v[qq] = (half_t)((float)v[qq] + (float)rcur[r][qq]);
        }
        if constexpr (GN) *reinterpret_cast<h8*>(wbuf + row * EPI_RS + c8 * 8) = v;   // final values for the stats
        const int mo = out_row<PH>(p, m);
        if (mo >= 0 && n < p.N) st_out16(out + (size_t)mo * p.out_ld + n, v);
      }
      if constexpr (GN) {   // full tiles only: every row stored
        if (nt == 2) gn_block_stats<32, 64, EPI_RS>(wbuf, gst + i * TN + jp * 32);
        else gn_block_stats<32, 32, EPI_RS>(wbuf, gst + i * TN + jp * 32);
      }
    }
    if (p.res && AHEAD && q + 1 < NBLK) {
#pragma unroll
      for (int r = 0; r < 4; ++r) rcur[r] = rnext[r];
    }
  }
}

// ---------------------------------------------------------------------- 16x16x32 wave-tile epilogues
// Transposed 16x16 accumulator of a TM x TN wave tile (D^T = W A^T, v_mfma_f32_16x16x32_f16):
// acc[i][j] lane l holds pixel m_w + 16*i + (l & 15) and channels n_w + 16*j + 4*(l >> 4) + q.
// fp16 NHWC / GEGLU: per 16-pixel block and 64-channel group (NB = 4 blocks of 16; a trailing
// 32-channel group has NB = 2) the wave writes its fp32->fp16 values (bias, embedding, GEGLU
// applied) to a private 16 x 72-half LDS scratch and stores 16-B row chunks (+ residual).
constexpr int EPG_RS = 72;                          // scratch row stride (halfs) = 144 B
constexpr int EPG_BYTES = 16 * EPG_RS * 2;          // per-wave scratch

// residual rows of one group (16 pixels x 16*NB channels) in read-back order
template <int NB>
__device__ __forceinline__ void epi16_load_res(const Params& p, int mt, int nb, h8 (&rr)[2]) {
  const int lane = threadIdx.x & 63;
  constexpr int LPR = NB * 2, RPI = 64 / LPR;
  const bool geglu = p.out_mode == SDK_OUT_GEGLU_F16;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    rr[r] = h8{};
    if (geglu ? r > 0 : r >= 16 / RPI) continue;
    const int row = geglu ? (lane >> 2) : r * RPI + lane / LPR;
    const int n = geglu ? nb / 2 + (lane & 3) * 8 : nb + (lane % LPR) * 8;
    const int m = mt + row;
    if (m < p.M && n < (geglu ? p.N / 2 : p.N)) rr[r] = *reinterpret_cast<const h8*>(p.res + (size_t)m * p.res_ld + n);
  }
}

template <int NB, bool GN = false, bool PH = false>
__device__ __forceinline__ void epi16_group(const Params& p, const f4* a, int mt, int nb, int n0, int bw, bool rb_vec,
                                            half_t* wbuf, const float* bias_s, const float* rb_s, const h8 (&rr)[2],
                                            float2* gdst = nullptr) {
  const int lane = threadIdx.x & 63, px = lane & 15, cg = lane >> 4;
  half_t* out = reinterpret_cast<half_t*>(p.out);
  auto bias4 = [&](int n) __attribute__((always_inline)) {
    return bias_s ? *reinterpret_cast<const f4*>(bias_s + (n - n0)) : *reinterpret_cast<const f4*>(p.bias + n);
  };
  if (p.out_mode == SDK_OUT_GEGLU_F16) {            // NB == 4: blocks 0,1 = x rows, 2,3 = gate rows
    const int nob = nb / 2;
    if (nob >= p.N / 2) return;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int nx = nb + 16 * j + 4 * cg;
      f4 bx = {0.f, 0.f, 0.f, 0.f}, bg = {0.f, 0.f, 0.f, 0.f};
      if (bias_s || p.bias) {
        bx = bias4(nx);
        bg = bias4(nx + 32);
      }
      h4 o;
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q] = (half_t)((a[j][q] + bx[q]) * gelu_erf(a[2 + j][q] + bg[q]));
      *reinterpret_cast<h4*>(wbuf + px * EPG_RS + 16 * j + 4 * cg) = o;
    }
    const int row = lane >> 2, c8 = lane & 3;       // 16 rows x 32 channels
    h8 v = *reinterpret_cast<const h8*>(wbuf + row * EPG_RS + c8 * 8);
    const int m = mt + row, no = nob + c8 * 8;
    if (m < p.M && no < p.N / 2) {
      if (p.res) {
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = (half_t)((float)v[q] + (float)rr[0][q]);
      }
      st_out16(out + (size_t)m * p.out_ld + no, v);
    }
    return;
  }
  if (nb >= p.N) return;
  if (rb_s) {
    // staged bias and embedding row (zeros where absent or past N; the read-back masks columns >= N):
    // the same two adds in the same order as below, no per-chunk branches
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int off = nb - n0 + 16 * j + 4 * cg;
      const f4 bb = *reinterpret_cast<const f4*>(bias_s + off);
      const f4 r4 = *reinterpret_cast<const f4*>(rb_s + off);
      h4 o;
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q] = (half_t)((a[j][q] + bb[q]) + r4[q]);
      *reinterpret_cast<h4*>(wbuf + px * EPG_RS + 16 * j + 4 * cg) = o;
    }
  } else
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int n = nb + 16 * j + 4 * cg;
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = a[j][q];
    if (n < p.N) {                                  // N % 8 == 0 in this mode
      if (p.bias) {
        const f4 bb = bias4(n);
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] += bb[q];
      }
      if (p.row_bias) {
        if (rb_s) {
          const f4 r4 = *reinterpret_cast<const f4*>(rb_s + (n - n0));
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] += r4[q];
        } else {
          const float* rb = p.row_bias + (size_t)bw * p.rb_ld + n;
          if (rb_vec) {
            const f4 r4 = *reinterpret_cast<const f4*>(rb);
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] += r4[q];
          } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] += rb[q];
          }
        }
      }
    }
    h4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = (half_t)v[q];
    *reinterpret_cast<h4*>(wbuf + px * EPG_RS + 16 * j + 4 * cg) = o;
  }
  constexpr int LPR = NB * 2, RPI = 64 / LPR;       // lanes per row, rows per instruction
#pragma unroll
  for (int r = 0; r < 16 / RPI; ++r) {
    const int row = r * RPI + lane / LPR, c8 = lane % LPR;
    h8 v = *reinterpret_cast<const h8*>(wbuf + row * EPG_RS + c8 * 8);
    const int m = mt + row, n = nb + c8 * 8;
    if (p.res) {
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = (half_t)((float)v[q] + (float)rr[r][q]);
    }
    if constexpr (GN) *reinterpret_cast<h8*>(wbuf + row * EPG_RS + c8 * 8) = v;   // final values for the stats
    const int mo = out_row<PH>(p, m);
    if (mo >= 0 && n < p.N) st_out16(out + (size_t)mo * p.out_ld + n, v);
  }
  if constexpr (GN) gn_block_stats<16, 16 * NB, EPG_RS>(wbuf, gdst);   // full tiles only: every row stored
}

// groups (i, g) flattened; the residual rows of group q+1 are loaded while group q is written
// (GN: per-channel statistics of the stored values, parked at wbuf + EPG_BYTES — gn_tile_store)
template <int FM, int FN, bool GN = false, bool PH = false>
__device__ __forceinline__ void epilogue16_tile(const Params& p, f4 (&acc)[FM][FN], int m0, int n0, int m_w, int n_w,
                                                half_t* wbuf, const float* bias_s = nullptr,
                                                const float* rb_s = nullptr) {
  const int lane = threadIdx.x & 63, px = lane & 15;
  const bool rb_vec = p.row_bias && !((uintptr_t)p.row_bias & 15) && !(p.rb_ld & 3);
  constexpr int NG = FN / 4 + (FN % 4 == 2 ? 1 : 0), NQ = FM * NG;
  constexpr bool AHEAD = FM * FN * 4 + 16 <= 96;
  h8 rcur[2], rnext[2];
  constexpr int TN = FN * 16;
  float2* gst = reinterpret_cast<float2*>(wbuf + EPG_BYTES / 2);   // GN: parked [FM][TN] (mean, M2)
  auto load = [&](int q, h8 (&rr)[2]) __attribute__((always_inline)) {
    const int g = q / FM, i = q - g * FM;
    const int mt = m0 + m_w + 16 * i;
    if (g < FN / 4) epi16_load_res<4>(p, mt, n0 + n_w + 64 * g, rr);
    else epi16_load_res<2>(p, mt, n0 + n_w + 16 * (FN - 2), rr);
  };
  if (p.res && AHEAD) load(0, rcur);
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int g = q / FM, i = q - g * FM;
    if (p.res && AHEAD && q + 1 < NQ) load(q + 1, rnext);
    if (p.res && !AHEAD) load(q, rcur);
    const int mt = m0 + m_w + 16 * i;
    if (mt < p.M) {
      const int bw = min(mt + px, p.M - 1) / p.hw_out;
      if (g < FN / 4)
        epi16_group<4, GN, PH>(p, &acc[i][4 * g], mt, n0 + n_w + 64 * g, n0, bw, rb_vec, wbuf, bias_s, rb_s, rcur,
                           gst + i * TN + 64 * g);
      else
        epi16_group<2, GN, PH>(p, &acc[i][FN - 2], mt, n0 + n_w + 16 * (FN - 2), n0, bw, rb_vec, wbuf, bias_s, rb_s,
                           rcur, gst + i * TN + 64 * g);
    }
    if (q < 4) ph_stamp(p, 4 + q);
    if (p.res && AHEAD && q + 1 < NQ) {
      rcur[0] = rnext[0];
      rcur[1] = rnext[1];
    }
  }
}

// split-K fp32 slabs and the fp32 output modes (NCHW image, token rows)
template <int FM, int FN>
__device__ __forceinline__ void epilogue16_tile_direct(const Params& p, f4 (&acc)[FM][FN], int m0, int n0, int m_w,
                                                       int n_w, int split_idx) {
  const int lane = threadIdx.x & 63, px = lane & 15, cg = lane >> 4;
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int m = m0 + m_w + 16 * i + px;
    if (m >= p.M) continue;
    const int b = m / p.hw_out;
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int n = n0 + n_w + 16 * j + 4 * cg;
      if (p.split > 1 && !p.inl) {
        *reinterpret_cast<f4*>(p.partial + ((size_t)split_idx * p.M + m) * p.Npad + n) = acc[i][j];
        continue;
      }
      float* out = reinterpret_cast<float*>(p.out);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (n + q >= p.N) continue;
        float x = acc[i][j][q];
        if (p.bias) x += p.bias[n + q];
        if (p.row_bias) x += p.row_bias[(size_t)b * p.rb_ld + n + q];
        if (p.res) x += (float)p.res[(size_t)m * p.res_ld + n + q];
        if (p.out_mode == SDK_OUT_NCHW_F32)
          out[((size_t)b * p.N + n + q) * p.hw_out + (m - b * p.hw_out)] = x;
        else
          out[(size_t)m * p.out_ld + n + q] = x;
      }
    }
  }
}

// ---------------------------------------------------------------------- LDS-DMA kernel
// A and W tiles are loaded straight into LDS with global_load_lds_dwordx4 (one
// 1-KiB wave instruction = 8 rows x 128 B); the per-lane SOURCE address carries
// the implicit-GEMM gather (pixel + tap + channel), the XOR swizzle of the LDS
// image (rule: linear LDS destination, permuted source, same permutation on the
// read) and zero padding (out-of-image taps read a 16-B zero page).  Two LDS
// stages; the next tile's DMA is in flight across the barrier of the current
// one (counted s_waitcnt vmcnt, raw s_barrier — never __syncthreads(), which
// would drain it).  No VGPR staging, no A-side transform (GroupNorm+SiLU is
// applied by gn_apply before 3x3 convs); every segment must be transform-free.
__device__ __attribute__((aligned(16))) half_t g_zero_page[8];

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

#define SDK_SEGF(f) (s1 ? p.seg[1].f : p.seg[0].f)

// The DMA goes through buffer resources: 32-bit byte offsets and the hardware range
// check — an offset past num_records loads zeros, which is the conv's zero padding and
// the ragged tile edge, with no per-lane pointer select.
constexpr unsigned PH_OOB = 0x80000000u;

__device__ __forceinline__ __amdgpu_buffer_rsrc_t ph_rsrc(const void* base, long long bytes) {
  const int n = (int)(bytes < 0x7fffffffLL ? bytes : 0x7fffffffLL);
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, n, 0x00020000);
}

__device__ __forceinline__ void ph_dma(__amdgpu_buffer_rsrc_t r, half_t* dst, unsigned voff, int soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)dst, 16, voff, soff, 0, 0);
}

// K-step -> (segment, tap row, tap column, channel base); scalar.  K order inside a
// segment: 64-channel block major, tap minor — the nine taps of one channel block read
// overlapping pixel windows back to back, so a 3x3 conv re-reads its A tile from L2
// (a workgroup's window over one block is ~48 KiB) instead of after a sweep over all
// channels (which overflows the 4 MiB L2 of an XCD at the 64x64 level).
__device__ __forceinline__ void ph_kstate(const Params& p, int kt, int& seg, int& ky, int& kx, int& cb) {
  const bool s1 = p.nseg > 1 && kt >= p.seg[1].kt_begin;
  seg = s1 ? 1 : 0;
  const int local = kt - SDK_SEGF(kt_begin), ks = SDK_SEGF(ksize), taps = ks * ks;
  const int cblk = local / taps, tap = local - cblk * taps;
  cb = cblk * BK;
  ky = tap / ks;
  kx = tap - ky * ks;
}

__device__ __forceinline__ void ph_kadv(const Params& p, int& seg, int& ky, int& kx, int& cb) {
  const bool s1 = seg != 0;
  const int ks = SDK_SEGF(ksize);
  if (++kx == ks) {
    kx = 0;
    if (++ky == ks) {
      ky = 0;
      cb += BK;
      if (cb >= SDK_SEGF(cin_pad)) { cb = 0; ++seg; }
    }
  }
}

struct DmaSrc {
  __amdgpu_buffer_rsrc_t a0, a1, s0, s1, w;
};

template <bool PH = false>
__device__ __forceinline__ DmaSrc make_dma_src(const Params& p, int m0) {
  const Seg& g0 = p.seg[0];
  const Seg& g1 = p.seg[1];
  const long long npix0 = (long long)p.batch * g0.h * g0.w;
  const bool two = p.nseg > 1;
  DmaSrc d;
  d.a0 = ph_rsrc(g0.src0, npix0 * g0.ld0 * 2);
  d.a1 = ph_rsrc(g0.src1 ? g0.src1 : g0.src0, npix0 * (g0.src1 ? g0.ld1 : g0.ld0) * 2);
  d.s0 = ph_rsrc(two ? g1.src0 : g0.src0, two ? (long long)p.M * g1.ld0 * 2 : 0);
  d.s1 = ph_rsrc(two && g1.src1 ? g1.src1 : g0.src0, two && g1.src1 ? (long long)p.M * g1.ld1 * 2 : 0);
  // per-image weights: an M-tile lies inside one image (planner), so one base per workgroup
  // (phase form: one base per phase — the planner pads every phase to whole M-tiles)
  const int wi = (PH && p.phase) ? m0 / p.ph_rows_pad : m0 / p.hw_out;
  d.w = ph_rsrc(p.wbs ? p.W + (size_t)wi * p.wbs : p.W, (long long)p.wrows * p.ldw * 2);
  return d;
}

// Per-lane context of A row m (output pixel) for segment 0: pixb = source pixel index of
// the tap window origin, msk = bit per in-image tap; upsample: pixb = b*h, msk = oy<<16|ox.
// Phase form: pixb = the 2x2 window origin (i + a, j + b) of the row's phase in the zero-bordered low-res image
// (every tap in range).  Returns whether m is a row of the problem (not past M, not a phase's padding row).
template <bool PH = false>
__device__ __forceinline__ bool a_row_ctx(const Params& p, int m, unsigned& pixb, unsigned& msk) {
  const Seg& g0 = p.seg[0];
  if (PH && p.phase) {
    const int ph = m / p.ph_rows_pad, rp = m - ph * p.ph_rows_pad;
    const bool valid = m < p.M && rp < p.ph_rows;
    const int rr = valid ? rp : 0;
    const int b = rr / p.hw_out, rem = rr - b * p.hw_out;
    const int oy = rem / p.wo, ox = rem - oy * p.wo;
    pixb = (unsigned)((b * g0.h + oy + (ph >> 1)) * g0.w + ox + (ph & 1));
    msk = valid ? 0xfu : 0u;
    return valid;
  }
  const bool valid = m < p.M;
  const int mm = valid ? m : 0;
  const int b = mm / p.hw_out, rem = mm - b * p.hw_out;
  const int oy = rem / p.wo, ox = rem - oy * p.wo;
  unsigned pb, mk = 0;
  if (!g0.upsample) {
    const int oys = oy * g0.stride, oxs = ox * g0.stride;
    pb = (unsigned)((b * g0.h + oys) * g0.w + oxs);
    for (int ky = 0; ky < g0.ksize; ++ky)
      for (int kx = 0; kx < g0.ksize; ++kx) {
        const int iy = oys + ky - g0.pad, ix = oxs + kx - g0.pad;
        const bool in = valid & ((unsigned)iy < (unsigned)g0.h) & ((unsigned)ix < (unsigned)g0.w);
        mk |= (in ? 1u : 0u) << (ky * g0.ksize + kx);
      }
  } else {
    pb = (unsigned)(b * g0.h);
    mk = valid ? ((unsigned)oy << 16 | (unsigned)ox) : 0x7fff7fffu;
  }
  pixb = pb;
  msk = mk;
  return valid;
}

__device__ __forceinline__ unsigned w_row_ctx(const Params& p, int n, int rch) {
  return n < p.wrows ? (unsigned)(n * p.ldw) * 2u + (unsigned)rch * 16u : PH_OOB;
}

// One 1-KiB A piece (8 rows x 64 channels) of K-step (seg, ky, kx, cb) into dst.
__device__ __forceinline__ void dma_a_piece(const Params& p, const DmaSrc& d, half_t* dst, unsigned pixb,
                                            unsigned msk, int m, int rch, int seg, int ky, int kx, int cb) {
  const Seg& g0 = p.seg[0];
  const Seg& g1 = p.seg[1];
  const unsigned rch16 = (unsigned)rch * 16u;
  if (seg == 0 && p.nomask) {
    const bool second = cb >= g0.c_split;
    const unsigned ld2 = (unsigned)(second ? g0.ld1 : g0.ld0) * 2u;
    const unsigned toff = (unsigned)((ky * g0.w + kx) * (int)ld2 + (cb - (second ? g0.c_split : 0)) * 2);
    ph_dma(second ? d.a1 : d.a0, dst, __umul24(pixb, ld2) + rch16 + toff, 0);
    return;
  }
  if (seg == 0) {
    const bool second = cb >= g0.c_split;
    const __amdgpu_buffer_rsrc_t r = second ? d.a1 : d.a0;
    const unsigned ld2 = (unsigned)(second ? g0.ld1 : g0.ld0) * 2u;
    const int coff2 = (cb - (second ? g0.c_split : 0)) * 2;
    const bool cok = (cb + BK <= g0.cin) || (cb + rch * 8 < g0.cin);
    const int dy = ky - g0.pad, dx = kx - g0.pad;
    unsigned off;
    bool ok;
    if (!g0.upsample) {
      const int tapb = ky * g0.ksize + kx;
      off = __umul24(pixb, ld2) + rch16 + (unsigned)((dy * g0.w + dx) * (int)ld2 + coff2);
      ok = ((msk >> tapb) & 1u) && cok;
    } else {
      const int iy = (int)(msk >> 16) + dy, ix = (int)(msk & 0xffffu) + dx;
      ok = ((unsigned)iy < 2u * g0.h) && ((unsigned)ix < 2u * g0.w) && cok;
      const unsigned pix = (pixb + (unsigned)(iy >> 1)) * (unsigned)g0.w + (unsigned)(ix >> 1);
      off = __umul24(pix, ld2) + rch16 + (unsigned)coff2;
    }
    ph_dma(r, dst, ok ? off : PH_OOB, 0);
  } else {
    const bool second = cb >= g1.c_split;
    const __amdgpu_buffer_rsrc_t r = second ? d.s1 : d.s0;
    const unsigned ld2 = (unsigned)(second ? g1.ld1 : g1.ld0) * 2u;
    const unsigned coff2 = (unsigned)(cb - (second ? g1.c_split : 0)) * 2u;
    const bool cok = (cb + BK <= g1.cin) || (cb + rch * 8 < g1.cin);
    const bool ok = (m < p.M) && cok;
    ph_dma(r, dst, ok ? __umul24((unsigned)m, ld2) + rch16 + coff2 : PH_OOB, 0);
  }
}

// Epilogue vectors of a tile, loaded into registers before the K loop (one element per thread,
// tid < tbn) and written to LDS after it: bias[n0 + tid] and, when the tile's rows lie in one
// image, that image's embedding row row_bias[b][n0 + tid].
struct EpiVec {
  float bias, rb;
  bool one_img;
};

__device__ __forceinline__ EpiVec epi_vec_load(const Params& p, int m0, int n0, int tbm, int tbn) {
  const int tid = threadIdx.x;
  EpiVec e{0.f, 0.f, false};
  const int b0 = m0 / p.hw_out;
  e.one_img = p.row_bias && (p.split == 1 || p.inl) && b0 == (min(m0 + tbm, p.M) - 1) / p.hw_out;
  if (tid < tbn && n0 + tid < p.N) {
    if (p.bias) e.bias = p.bias[n0 + tid];
    if (e.one_img) e.rb = p.row_bias[(size_t)b0 * p.rb_ld + n0 + tid];
  }
  return e;
}

__device__ __forceinline__ void epi_vec_store(const EpiVec& e, float* vec_s, int tbn) {
  const int tid = threadIdx.x;
  if (tid < tbn) {
    vec_s[tid] = e.bias;
    vec_s[tbn + tid] = e.rb;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// Work-item order (xcd_remap then puts consecutive items on one XCD, sharing its L2).  Without
// split-K: M-tile major — the N-tiles of one pixel panel share its A rows.  With split-K (the
// 16x16 / 8x8 UNet levels: M = 1024-4096 rows against a 15-60 MB weight matrix) the weight slice
// is the large operand: (N-tile, K-slice) major, M-tile minor, so the M-tiles that read one weight
// slice are co-resident on an XCD and the slice comes from L2 instead of once per M-tile.
__device__ __forceinline__ void item_coords(const Params& p, int it, int& tm, int& tn, int& sidx) {
  if (p.inl) {   // the two halves of a tile are neighbouring items (one XCD under xcd_remap)
    const int t = it >> 1;
    sidx = it & 1;
    tm = t / p.tiles_n;
    tn = t - tm * p.tiles_n;
    return;
  }
  if (p.split == 1) {
    sidx = 0;
    if (p.gm > 1) {   // groups of gm M-panels (the last one shorter), N-tile major inside a group
      const int gsz = p.gm * p.tiles_n, g = it / gsz, l = it - g * gsz;
      const int rows = min(p.gm, p.tiles_m - g * p.gm);
      tn = l / rows;
      tm = g * p.gm + (l - tn * rows);
      return;
    }
    tm = it / p.tiles_n;
    tn = it - tm * p.tiles_n;
    return;
  }
  const int slab = it / p.tiles_m;
  tm = it - slab * p.tiles_m;
  tn = slab / p.split;
  sidx = slab - tn * p.split;
}

// sched_group_barrier sequence of the pipelined 16x16x32 K-step (conv_glds_kernel, PFD > 0): per MFMA group g the
// W fragment read PFD groups ahead (DS read), the group's FM MFMAs, then its np DMA pieces (VMEM)
template <int G, int PFD, int FM, int PPG, int GPW, int g = 0>
__device__ __forceinline__ void pin_fragment_groups() {
  if constexpr (g < G) {
    if constexpr (g + PFD < G) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, FM, 0);
    constexpr int np = GPW - g * PPG < 0 ? 0 : (GPW - g * PPG < PPG ? GPW - g * PPG : PPG);
    if constexpr (np > 0) __builtin_amdgcn_sched_group_barrier(0x020, np, 0);
    pin_fragment_groups<G, PFD, FM, PPG, GPW, g + 1>();
  }
}

// One (tile, K-split) work item per workgroup, two LDS stages.
// SIMPLE: the instantiation for one-segment, one-source convs without masks (build_params sets p.simple:
// token GEMMs and the 3x3 convs over zero-bordered inputs): a lane's A row offset is fixed (the tap window's
// origin pixel) and a K step adds one wave-uniform offset (tap + channel block), so an A piece is one DMA
// with that offset in the scalar soffset like a W piece — no per-piece segment / tap / mask branch chains in
// the K loop (their scalar work bounded the loop: +19-28 % on the UNet token GEMMs).
// SIMPLE = 2: the same with a second, 1x1 segment over the output grid (a ResBlock's fused shortcut, one or two
// concat sources): the K step's segment / source picks one of three per-lane row offsets.
template <class CF, int SIMPLE = 0>
__global__ void __launch_bounds__(CF::NT, CF::OCC * CF::NW / 4) conv_glds_kernel(Params p) {
  extern __shared__ __attribute__((aligned(16))) half_t lds[];
  constexpr int GPW = CF::GPW;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  __builtin_assume(wave >= 0 && wave < CF::NW);   // lets the piece loops resolve real / A / W pieces at compile time
  const int wm = wave / CF::WN, wn = wave % CF::WN;
  const int nitems = p.tiles_m * p.tiles_n * p.split;
  // XCD-aware item order: neighbouring tiles (shared A rows / W rows) share an L2
  const int it = xcd_remap((int)blockIdx.x + (int)blockIdx.y * (int)gridDim.x, nitems);
  int tm, tn, sidx;
  item_coords(p, it, tm, tn, sidx);
  ph_stamp(p, 0);
  const int m0 = tm * CF::TBM, n0 = tn * CF::TBN;
  const int kt0 = sidx * p.kt_per_split, kt1 = min(p.kt_total, kt0 + p.kt_per_split);
  const int lrow = lane >> 3;
  constexpr bool PH = SIMPLE == 1;   // the phase form runs on this instantiation only (build_params)
  const DmaSrc d = make_dma_src<PH>(p, m0);
  // per piece j (rows (j*NW + wave)*8 + lrow of the stage): A -> (pixb, msk), W -> byte offset
  unsigned cx[GPW], cy[GPW], cz[SIMPLE == 2 ? GPW : 1];
#pragma unroll
  for (int j = 0; j < GPW; ++j) {
    const int piece = j * CF::NW + wave;
    const int rch = (lane & 7) ^ ((4 * piece + (lrow >> 1)) & 7);
    unsigned x = PH_OOB, y = 0;
    if (piece < CF::NINSTR) {
      if (piece * 8 < CF::TBM) {
        if constexpr (SIMPLE != 0) {   // the tap window origin's row, 16-B chunk rch of the K step
          const int m = m0 + piece * 8 + lrow;
          const bool live = a_row_ctx<PH>(p, m, x, y);
          x = live ? __umul24(x, (unsigned)p.seg[0].ld0 * 2u) + (unsigned)rch * 16u : PH_OOB;
          if constexpr (SIMPLE == 2) {   // the shortcut segment: output pixel m of each concat source
            y = m < p.M ? __umul24((unsigned)m, (unsigned)p.seg[1].ld0 * 2u) + (unsigned)rch * 16u : PH_OOB;
            cz[j] = m < p.M ? __umul24((unsigned)m, (unsigned)p.seg[1].ld1 * 2u) + (unsigned)rch * 16u : PH_OOB;
          }
        } else {
          a_row_ctx(p, m0 + piece * 8 + lrow, x, y);
        }
      } else {
        x = w_row_ctx(p, n0 + piece * 8 + lrow - CF::TBM, rch);
      }
    }
    cx[j] = x;
    cy[j] = y;
  }
  const EpiVec ev = epi_vec_load(p, m0, n0, CF::TBM, CF::TBN);
  int sg, ky, kx, cb;
  ph_kstate(p, kt0, sg, ky, kx, cb);
  // K-steps past kt1 still issue their pieces (zero-page DMAs into the idle stage) so every
  // iteration waits with the same vmcnt immediate
#define SDK_STAGE(KT_, BUF_)                                                                 \
  do {                                                                                       \
    const bool live_ = (KT_) < kt1;                                                          \
    if constexpr (SIMPLE != 0) {                                                             \
      int toff_ = (ky * p.seg[0].w + kx) * p.seg[0].ld0 * 2 + cb * 2;                        \
      __amdgpu_buffer_rsrc_t ra_ = d.a0;                                                     \
      bool s1_ = false, sec_ = false;                                                        \
      if constexpr (SIMPLE == 2) {                                                           \
        s1_ = sg != 0;                                                                       \
        sec_ = s1_ && cb >= p.seg[1].c_split;                                                \
        if (s1_) {                                                                           \
          toff_ = (cb - (sec_ ? p.seg[1].c_split : 0)) * 2;                                  \
          ra_ = sec_ ? d.s1 : d.s0;                                                          \
        }                                                                                    \
      }                                                                                      \
      _Pragma("unroll") for (int j = 0; j < GPW; ++j) {                                      \
        const int piece = j * CF::NW + wave;                                                 \
        if (piece >= CF::NINSTR) {                                                           \
          ph_dma(d.w, lds + CF::NS * CF::STAGE_H, PH_OOB, 0);                                \
        } else {                                                                             \
          const bool a_ = piece * 8 < CF::TBM;                                               \
          unsigned base_ = cx[j];                                                            \
          if constexpr (SIMPLE == 2) base_ = (a_ && s1_) ? (sec_ ? cz[j] : cy[j]) : cx[j];   \
          ph_dma(a_ ? ra_ : d.w, lds + (BUF_) * CF::STAGE_H + piece * 8 * BK,                \
                 live_ ? base_ : PH_OOB, a_ ? toff_ : (KT_) * BK * 2);                       \
        }                                                                                    \
      }                                                                                      \
      if (live_) ph_kadv(p, sg, ky, kx, cb);                                                 \
      break;                                                                                 \
    }                                                                                        \
    _Pragma("unroll") for (int j = 0; j < GPW; ++j) {                                        \
      const int piece = j * CF::NW + wave;                                                   \
      const int rch = (lane & 7) ^ ((4 * piece + (lrow >> 1)) & 7);                          \
      if (piece >= CF::NINSTR) {                                                             \
        ph_dma(d.w, lds + CF::NS * CF::STAGE_H, PH_OOB, 0);                                  \
      } else if (!live_) {                                                                   \
        ph_dma(d.w, lds + (BUF_) * CF::STAGE_H + piece * 8 * BK, PH_OOB, 0);                 \
      } else if (piece * 8 < CF::TBM) {                                                      \
        dma_a_piece(p, d, lds + (BUF_) * CF::STAGE_H + piece * 8 * BK, cx[j], cy[j],         \
                    m0 + piece * 8 + lrow, rch, sg, ky, kx, cb);                             \
      } else {                                                                               \
        ph_dma(d.w, lds + (BUF_) * CF::STAGE_H + piece * 8 * BK, cx[j], (KT_) * BK * 2);     \
      }                                                                                      \
    }                                                                                        \
    if (live_) ph_kadv(p, sg, ky, kx, cb);                                                   \
  } while (0)

  f16v acc[CF::FM][CF::FN];
  f4 acc16[CF::FM16][CF::FN16];
  if constexpr (CF::M16) {
#pragma unroll
    for (int i = 0; i < CF::FM16; ++i)
#pragma unroll
      for (int j = 0; j < CF::FN16; ++j) acc16[i][j] = f4{};
  } else {
#pragma unroll
    for (int i = 0; i < CF::FM; ++i)
#pragma unroll
      for (int j = 0; j < CF::FN; ++j) acc[i][j] = f16v{};
  }

  const int fr = lane & 31, fh = lane >> 5;
  const int arow0 = wm * CF::TM + fr;
  const int brow0 = CF::TBM + wn * CF::TN + fr;
  const int r16 = lane & 15, c16 = lane >> 4;   // 16x16x32 operand: row in block, 8-half K chunk
  const int arow16 = wm * CF::TM + r16;
  const int brow16 = CF::TBM + wn * CF::TN + r16;

  // ring of NS stages: K-step kt lives in stage (kt - kt0) % NS; iteration kt refills the stage
  // iteration kt - 1 read (its closing barrier makes that safe) with K-step kt + NS - 1
#pragma unroll
  for (int s = 0; s < CF::NS - 1; ++s) SDK_STAGE(kt0 + s, s);
  int buf = 0, wbuf = CF::NS - 1;
#if !defined(SDK_NO_PRIO)
  // static priority for the younger half of the workgroup's waves (the arbitration loser on every
  // K-step otherwise; UNet step -0.4 %, profiles/r2_static_priority_ab.txt — priority flips around
  // each K-step's MFMA cluster measured +0.2 %)
  if (__builtin_amdgcn_readfirstlane(threadIdx.x) >= CF::NT / 2) __builtin_amdgcn_s_setprio(1);
#endif
  ph_stamp(p, 1);
  // K loop form: the one-barrier loop with the DMA issue interleaved into the MFMAs where a SIMD holds at
  // least two of the kernel's waves (one stalls on a DMA issue while another computes); configs with one
  // wave per SIMD keep the two-barrier loop whose issue overlaps the other waves' finishing MFMAs (the
  // interleaved form measured 18-23 % slower on the 4-wave 128x128 ring, +4-20 % on the 8- and 16-wave
  // tiles: profiles/r5_glds_loop_ab.txt).  SDK_GLDS_LOOP_OLD: the two-barrier loop everywhere (A/B builds).
#if defined(SDK_GLDS_LOOP_OLD)
  constexpr bool ILV = false;
#else
  constexpr bool ILV = CF::NW * CF::OCC >= 8;
#endif
  if constexpr (ILV) {
  // One barrier per K-step.  Iteration kt: wait for this wave's pieces of K-step kt (the newer NS - 2
  // stages stay in flight), barrier (every wave's pieces of kt landed, every wave done reading the slot of
  // kt - 1), then the MFMAs on kt with the DMA of K-step kt + NS - 1 — into the slot kt - 1 used — issued
  // between the first MFMA groups, so the DMA issue runs under the MFMAs instead of ahead of them
  // (round 4: ~6k cycles per 256x320 K-step for ~2.6k of MFMA, the pieces issued behind a barrier and
  // landed before the next one).  SIMPLE plans only; the generic gather issues its stage after the barrier.
  struct Iss {
    __amdgpu_buffer_rsrc_t ra;
    int toff, woff;
    bool live, s1, sec;
  };
  // A/B builds only (-DSDK_ABL_DMA=1 / 2 / 3, wrong outputs by design): the K loop issues no A / W / A and W
  // pieces after the prologue — the ablations that say which operand's fill bounds the loop
#if defined(SDK_ABL_DMA)
#define SDK_ABL_DMA_SKIP(IS_A) (((SDK_ABL_DMA) & 1) && (IS_A)) || (((SDK_ABL_DMA) & 2) && !(IS_A))
#else
#define SDK_ABL_DMA_SKIP(IS_A) false
#endif
  auto stage_prep = [&](int KT) __attribute__((always_inline)) {
    Iss q;
    q.live = KT < kt1;
    q.ra = d.a0;
    q.s1 = q.sec = false;
    q.toff = (ky * p.seg[0].w + kx) * p.seg[0].ld0 * 2 + cb * 2;
    if constexpr (SIMPLE == 2) {
      q.s1 = sg != 0;
      q.sec = q.s1 && cb >= p.seg[1].c_split;
      if (q.s1) {
        q.toff = (cb - (q.sec ? p.seg[1].c_split : 0)) * 2;
        q.ra = q.sec ? d.s1 : d.s0;
      }
    }
    q.woff = KT * BK * 2;
    if (q.live) ph_kadv(p, sg, ky, kx, cb);
    return q;
  };
  // piece J (a compile-time index after unrolling: the per-lane offset arrays stay in registers) of the
  // stage described by Q into ring slot BUF
// Branch-free: a padding piece (piece >= NINSTR, every wave issues GPW so the vmcnt immediates are exact) differs
// from a real one only in its operands — its per-lane offset is PH_OOB (cx set up so) and it lands in the dummy slot
// past the ring — so the K-step stays one basic block and the scheduler can hoist the fragment reads across the
// DMA issue (a uniform branch per piece split the unrolled K-step into ~12 blocks, each B fragment read right before
// its MFMAs)
#define SDK_PIECE(Q, J, BUF)                                                                             \
  do {                                                                                                   \
    const int piece_ = (J) * CF::NW + wave;                                                              \
    const bool real_ = piece_ < CF::NINSTR;                                                              \
    const bool a_ = piece_ * 8 < CF::TBM;                                                                \
    if (real_ && SDK_ABL_DMA_SKIP(a_)) break;                                                            \
    unsigned base_ = cx[J];                                                                              \
    if constexpr (SIMPLE == 2) base_ = (a_ && (Q).s1) ? ((Q).sec ? cz[J] : cy[J]) : cx[J];               \
    ph_dma(a_ ? (Q).ra : d.w, real_ ? lds + (BUF) * CF::STAGE_H + piece_ * 8 * BK : lds + CF::NS * CF::STAGE_H, \
           (Q).live ? base_ : PH_OOB, a_ ? (Q).toff : (Q).woff);                                         \
  } while (0)
  for (int kt = kt0; kt < kt1; ++kt) {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((CF::NS - 2) * GPW) : "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    Iss q{};
    if constexpr (SIMPLE != 0) {
      q = stage_prep(kt + CF::NS - 1);
    } else {
      SDK_STAGE(kt + CF::NS - 1, wbuf);
    }
    const half_t* st = lds + buf * CF::STAGE_H;
    if constexpr (CF::M16) {
      // the K-step as G = (BK / 32) x FN16 MFMA groups (group g: W fragment j = g % FN16 of K half kk = g / FN16
      // against the wave's FM16 A fragments).  PFD > 0 (the 8-wave configs, 256 VGPRs): every A fragment of the
      // K-step is read up front and W fragments run PFD groups ahead of their MFMAs, so an LDS read's latency
      // hides under the MFMAs of the groups before it; PFD = 0 (16 waves at 128 VGPRs): one W fragment at a time
      // (the 32x160 wave tiles keep 80 accumulator VGPRs), A fragments per K half
      constexpr int G = (BK / 32) * CF::FN16;
      constexpr int PFD = CF::NW * CF::OCC <= 8 ? 2 : 0;
      constexpr int NKA = PFD ? BK / 32 : 1;
      auto rd_b = [&](int g) __attribute__((always_inline)) {
        return *reinterpret_cast<const h8*>(st + swz(brow16 + (g % CF::FN16) * 16, (g / CF::FN16) * 4 + c16));
      };
      h8 fa[NKA][CF::FM16];
      h8 fbq[PFD + 1];
      if constexpr (PFD > 0) {
#pragma unroll
        for (int kk = 0; kk < BK / 32; ++kk)
#pragma unroll
          for (int i = 0; i < CF::FM16; ++i)
            fa[kk][i] = *reinterpret_cast<const h8*>(st + swz(arow16 + i * 16, kk * 4 + c16));
#pragma unroll
        for (int g = 0; g < PFD; ++g) fbq[g] = rd_b(g);
      }
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const int kk = g / CF::FN16, j = g % CF::FN16;
        if constexpr (PFD == 0) {
          if (j == 0) {
#pragma unroll
            for (int i = 0; i < CF::FM16; ++i)
              fa[0][i] = *reinterpret_cast<const h8*>(st + swz(arow16 + i * 16, kk * 4 + c16));
          }
        }
        const h8 fb = PFD ? fbq[g % (PFD + 1)] : rd_b(g);
        if constexpr (PFD > 0) {
          if (g + PFD < G) fbq[(g + PFD) % (PFD + 1)] = rd_b(g + PFD);
        }
#pragma unroll
        for (int i = 0; i < CF::FM16; ++i) {
          const h8 fai = fa[PFD ? kk : 0][i];
#if defined(SDK_ABL_MFMA)   // A/B builds only: the fragments are consumed by one VALU add instead of the MFMA
          acc16[i][j][0] += (float)fb[0] + (float)fai[0];
#else
          acc16[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb, fai, acc16[i][j], 0, 0, 0);
#endif
        }
        // pieces [g * PPG, (g + 1) * PPG) after MFMA group g: all issued within the first half of the
        // K-step's groups, so they land while the rest of it computes
        if constexpr (SIMPLE != 0) {
          constexpr int PPG = (2 * GPW + G - 1) / G;
#pragma unroll
          for (int r = 0; r < PPG; ++r)
            if (g * PPG + r < GPW) SDK_PIECE(q, g * PPG + r < GPW ? g * PPG + r : 0, wbuf);
        }
      }
      if constexpr (PFD > 0 && SIMPLE != 0) {
        // pin the order the fragment pipeline needs (the scheduler otherwise sinks each W read to just before its
        // MFMAs next to a DMA issue, and the MFMAs wait lgkmcnt(0) on it): the up-front reads, then per group the
        // read PFD groups ahead, the group's MFMAs and its DMA pieces
        __builtin_amdgcn_sched_group_barrier(0x100, NKA * CF::FM16 + PFD, 0);
        pin_fragment_groups<G, PFD, CF::FM16, (2 * GPW + G - 1) / G, GPW>();
      }
    } else {
#pragma unroll
      for (int kk = 0; kk < BK / 16; ++kk) {
        h8 fa[CF::FM], fb[CF::FN];
#pragma unroll
        for (int i = 0; i < CF::FM; ++i)
          fa[i] = *reinterpret_cast<const h8*>(st + swz(arow0 + i * 32, kk * 2 + fh));
#pragma unroll
        for (int j = 0; j < CF::FN; ++j)
          fb[j] = *reinterpret_cast<const h8*>(st + swz(brow0 + j * 32, kk * 2 + fh));
#pragma unroll
        for (int i = 0; i < CF::FM; ++i) {
#pragma unroll
          for (int j = 0; j < CF::FN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fb[j], fa[i], acc[i][j], 0, 0, 0);
          const int g = kk * CF::FM + i;
          if constexpr (SIMPLE != 0) {
            constexpr int PPG = (2 * GPW + CF::FM * (BK / 16) - 1) / (CF::FM * (BK / 16));
#pragma unroll
            for (int r = 0; r < PPG; ++r)
              if (g * PPG + r < GPW) SDK_PIECE(q, g * PPG + r < GPW ? g * PPG + r : 0, wbuf);
          }
        }
      }
    }
    buf = buf + 1 == CF::NS ? 0 : buf + 1;
    wbuf = wbuf + 1 == CF::NS ? 0 : wbuf + 1;
  }
#undef SDK_PIECE
  // (the ring becomes epilogue scratch after the post-loop barrier below: every wave's last ring read
  // precedes its last MFMA, which precedes that barrier)
  } else {
  for (int kt = kt0; kt < kt1; ++kt) {
    SDK_STAGE(kt + CF::NS - 1, wbuf);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((CF::NS - 1) * GPW) : "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    const half_t* st = lds + buf * CF::STAGE_H;
    if constexpr (CF::M16) {
#pragma unroll
      for (int kk = 0; kk < BK / 32; ++kk) {
        h8 fa[CF::FM16];
#pragma unroll
        for (int i = 0; i < CF::FM16; ++i)
          fa[i] = *reinterpret_cast<const h8*>(st + swz(arow16 + i * 16, kk * 4 + c16));
        // one W fragment at a time: the 32x160 wave tiles of the 16-wave configs keep
        // 80 accumulator VGPRs and must stay within 128
#pragma unroll
        for (int j = 0; j < CF::FN16; ++j) {
          const h8 fb = *reinterpret_cast<const h8*>(st + swz(brow16 + j * 16, kk * 4 + c16));
#pragma unroll
          for (int i = 0; i < CF::FM16; ++i)
            acc16[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb, fa[i], acc16[i][j], 0, 0, 0);
        }
      }
    } else
#pragma unroll
    for (int kk = 0; kk < BK / 16; ++kk) {
      h8 fa[CF::FM], fb[CF::FN];
#pragma unroll
      for (int i = 0; i < CF::FM; ++i)
        fa[i] = *reinterpret_cast<const h8*>(st + swz(arow0 + i * 32, kk * 2 + fh));
#pragma unroll
      for (int j = 0; j < CF::FN; ++j)
        fb[j] = *reinterpret_cast<const h8*>(st + swz(brow0 + j * 32, kk * 2 + fh));
#pragma unroll
      for (int i = 0; i < CF::FM; ++i)
#pragma unroll
        for (int j = 0; j < CF::FN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fb[j], fa[i], acc[i][j], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();      // everyone done reading `buf` before it is restaged
    __builtin_amdgcn_sched_barrier(0);
    buf = buf + 1 == CF::NS ? 0 : buf + 1;
    wbuf = wbuf + 1 == CF::NS ? 0 : wbuf + 1;
  }
  }
#undef SDK_STAGE
  // the trailing zero-page DMAs land before the ring is reused as epilogue scratch
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  ph_stamp(p, 2);
  if (p.inl) {
    // in-launch split-K: both halves dump their accumulators as a lane-major blob (16-B stores, every wave
    // instruction a contiguous KiB), publish with an agent-scope release and take a ticket; the second
    // arrival acquires, adds the other half's blob and runs the epilogue as an unsplit tile
    // (cdna_hip_programming.md §5 'In-launch split-K reduction').  fp32 a + b == b + a: the sum is the
    // same whichever half arrives last.
    constexpr int NQ = CF::M16 ? CF::FM16 * CF::FN16 : CF::FM * CF::FN * 4;   // f4 groups per thread
    const int tile = tm * p.tiles_n + tn;
    f4* mine = reinterpret_cast<f4*>(p.partial) + ((size_t)tile * 2 + sidx) * NQ * CF::NT + tid;
    const f4* other = reinterpret_cast<const f4*>(p.partial) + ((size_t)tile * 2 + (sidx ^ 1)) * NQ * CF::NT + tid;
    if constexpr (CF::M16) {
#pragma unroll
      for (int i = 0; i < CF::FM16; ++i)
#pragma unroll
        for (int j = 0; j < CF::FN16; ++j) mine[(i * CF::FN16 + j) * CF::NT] = acc16[i][j];
    } else {
#pragma unroll
      for (int i = 0; i < CF::FM; ++i)
#pragma unroll
        for (int j = 0; j < CF::FN; ++j)
#pragma unroll
          for (int g = 0; g < 4; ++g)
            mine[((i * CF::FN + j) * 4 + g) * CF::NT] =
                f4{acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    unsigned* flag = reinterpret_cast<unsigned*>(lds);   // the ring is idle: every wave is past its last read
    if (tid == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const unsigned ticket = __hip_atomic_fetch_add(p.tcnt + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (ticket == 1) {
        __hip_atomic_store(p.tcnt + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // left zero
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      *flag = ticket;
    }
    __syncthreads();
    if (*flag != 1) return;
    __syncthreads();   // every wave read the flag before the ring becomes epilogue scratch
    if constexpr (CF::M16) {
#pragma unroll
      for (int i = 0; i < CF::FM16; ++i)
#pragma unroll
        for (int j = 0; j < CF::FN16; ++j) {
          const f4 o = other[(i * CF::FN16 + j) * CF::NT];
#pragma unroll
          for (int r = 0; r < 4; ++r) acc16[i][j][r] += o[r];
        }
    } else {
#pragma unroll
      for (int i = 0; i < CF::FM; ++i)
#pragma unroll
        for (int j = 0; j < CF::FN; ++j)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const f4 o = other[((i * CF::FN + j) * 4 + g) * CF::NT];
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][j][4 * g + r] += o[r];
          }
    }
  }
  float* vec_s = reinterpret_cast<float*>(reinterpret_cast<char*>(lds) + CF::RING_BYTES);
  epi_vec_store(ev, vec_s, CF::TBN);
  __builtin_amdgcn_s_barrier();
  // the staged vectors hold zeros where there is no bias / embedding row; rb_s = nullptr only where the
  // tile's rows span two images' embedding rows (the epilogue then reads them per row from global)
  const float* bias_s = vec_s;
  const float* rb_s = (ev.one_img || !p.row_bias) ? vec_s + CF::TBN : nullptr;
  constexpr int WSCR = CF::RING_BYTES / CF::NW / 16 * 8;   // per-wave epilogue scratch (halfs)
  half_t* wscr = lds + wave * WSCR;
  const bool lds_epi = (p.split == 1 || p.inl) && (p.out_mode == SDK_OUT_NHWC_F16 || p.out_mode == SDK_OUT_GEGLU_F16);
  // the tile's GroupNorm statistics (build_params enables p.gnp for full fp16 NHWC tiles only)
  auto gn_store = [&](int scratch_halfs, auto blk_rows) __attribute__((always_inline)) {
    constexpr int BR = decltype(blk_rows)::value;
    __syncthreads();
    gn_tile_store<CF::WM, CF::WN, CF::TN, CF::TM / BR, BR, CF::TBM, CF::TBN, PH>(
        p, m0, n0, [&](int w) { return reinterpret_cast<const float2*>(lds + w * WSCR + scratch_halfs); });
  };
  if constexpr (CF::M16) {
    static_assert(CF::FN16 % 4 == 0 || CF::FN16 % 4 == 2, "epilogue16_tile groups: 64- and 32-channel groups");
    if (lds_epi && p.gnp) {
      epilogue16_tile<CF::FM16, CF::FN16, true, PH>(p, acc16, m0, n0, wm * CF::TM, wn * CF::TN, wscr, bias_s, rb_s);
      gn_store(EPG_BYTES / 2, std::integral_constant<int, 16>{});
    } else if (lds_epi) {
      epilogue16_tile<CF::FM16, CF::FN16, false, PH>(p, acc16, m0, n0, wm * CF::TM, wn * CF::TN, wscr, bias_s, rb_s);
    } else {
      epilogue16_tile_direct<CF::FM16, CF::FN16>(p, acc16, m0, n0, wm * CF::TM, wn * CF::TN, sidx);
    }
    ph_stamp(p, 3);
    return;
  }
  if (lds_epi && p.gnp) {
    epilogue_lds<CF::FM, CF::FN, true, PH>(p, acc, m0, n0, wm * CF::TM, wn * CF::TN, wscr, bias_s, rb_s);
    gn_store(EPI_BYTES / 2, std::integral_constant<int, 32>{});
  } else if (lds_epi) {
    epilogue_lds<CF::FM, CF::FN, false, PH>(p, acc, m0, n0, wm * CF::TM, wn * CF::TN, wscr, bias_s, rb_s);
  } else {
    epilogue_direct<CF::FM, CF::FN>(p, acc, m0, n0, wm * CF::TM, wn * CF::TN, sidx);
  }
  ph_stamp(p, 3);
}

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

// ---------------------------------------------------------------------- 16x16x32 epilogues
// Transposed 16x16 accumulator (D^T = W A^T, v_mfma_f32_16x16x32_f16): lane l holds pixel
// m = m_w + 16*i + (l & 15) and the 4 consecutive channels n = n_w + 32*b + 16*j + 4*(l >> 4) + q.
// acc[i][b][j]: i = 16-pixel block (4 per 64-pixel wave half), b = 32-channel half of the wave's
// 64 channels (GEGLU: b = 0 x, b = 1 gate), j = 16-channel block.
constexpr int EPI16_RS = 72;                          // scratch row stride (halfs) = 144 B
constexpr int EPI16_BYTES = 16 * EPI16_RS * 2;        // per-wave scratch: 16 pixels x 64 channels

__device__ __forceinline__ void epilogue16_lds(const Params& p, f4 (&acc)[4][2][2], int m0, int n0, int m_w, int n_w,
                                               half_t* wbuf, const float* bias_s = nullptr,
                                               const float* rb_s = nullptr) {
  const int lane = threadIdx.x & 63, px = lane & 15, cg = lane >> 4;
  const bool rb_vec = p.row_bias && !((uintptr_t)p.row_bias & 15) && !(p.rb_ld & 3);
  half_t* out = reinterpret_cast<half_t*>(p.out);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int mt = m0 + m_w + 16 * i;                 // first pixel of the block (wave-uniform)
    if (mt >= p.M) continue;
    const int bw = min(mt + px, p.M - 1) / p.hw_out;  // the writer lane's image
    if (p.out_mode == SDK_OUT_GEGLU_F16) {
      const int nob = (n0 + n_w) / 2;                 // first output channel of the wave
      if (nob >= p.N / 2) continue;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int nx = n0 + n_w + 16 * j + 4 * cg;    // x rows; gate rows = nx + 32
        f4 bx = {0.f, 0.f, 0.f, 0.f}, bg = {0.f, 0.f, 0.f, 0.f};
        if (bias_s) {                                 // staged (zeros where there is no bias)
          bx = *reinterpret_cast<const f4*>(bias_s + (nx - n0));
          bg = *reinterpret_cast<const f4*>(bias_s + (nx + 32 - n0));
        } else if (p.bias) {
          bx = *reinterpret_cast<const f4*>(p.bias + nx);
          bg = *reinterpret_cast<const f4*>(p.bias + nx + 32);
        }
        h4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = (half_t)((acc[i][0][j][q] + bx[q]) * gelu_erf(acc[i][1][j][q] + bg[q]));
        *reinterpret_cast<h4*>(wbuf + px * EPI16_RS + 16 * j + 4 * cg) = o;
      }
      // read back: 16 pixel rows x 32 channels = 4 lanes x 16 B per row
      const int row = lane >> 2, c8 = lane & 3;
      h8 v = *reinterpret_cast<const h8*>(wbuf + row * EPI16_RS + c8 * 8);
      const int m = mt + row, no = nob + c8 * 8;
      if (m < p.M && no < p.N / 2) {
        if (p.res) {
          const h8 rr = *reinterpret_cast<const h8*>(p.res + (size_t)m * p.res_ld + no);
#pragma unroll
          for (int q = 0; q < 8; ++q) v[q] = (half_t)((float)v[q] + (float)rr[q]);
        }
        st_out16(out + (size_t)m * p.out_ld + no, v);
      }
      continue;
    }
    if (n0 + n_w >= p.N) continue;
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int n = n0 + n_w + 32 * b + 16 * j + 4 * cg;
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = acc[i][b][j][q];
        if (rb_s) {                                   // staged vectors (zeros where absent): branch-free
          const f4 bb = *reinterpret_cast<const f4*>(bias_s + (n - n0));
          const f4 r4 = *reinterpret_cast<const f4*>(rb_s + (n - n0));
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] = (v[q] + bb[q]) + r4[q];
        } else if (n < p.N) {                         // N % 8 == 0 in this mode
          if (p.bias) {
            const f4 bb = *reinterpret_cast<const f4*>(p.bias + n);
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] += bb[q];
          }
          if (p.row_bias) {
            const float* rb = p.row_bias + (size_t)bw * p.rb_ld + n;
            if (rb_vec) {
              const f4 r4 = *reinterpret_cast<const f4*>(rb);
#pragma unroll
              for (int q = 0; q < 4; ++q) v[q] += r4[q];
            } else {
#pragma unroll
              for (int q = 0; q < 4; ++q) v[q] += rb[q];
            }
          }
        }
        h4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = (half_t)v[q];
        *reinterpret_cast<h4*>(wbuf + px * EPI16_RS + 32 * b + 16 * j + 4 * cg) = o;
      }
    // read back: 16 pixel rows x 64 channels = 8 lanes x 16 B per row, 8 rows per instruction
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int row = 8 * r + (lane >> 3), c8 = lane & 7;
      h8 v = *reinterpret_cast<const h8*>(wbuf + row * EPI16_RS + c8 * 8);
      const int m = mt + row, n = n0 + n_w + c8 * 8;
      if (m < p.M && n < p.N) {
        if (p.res) {
          const h8 rr = *reinterpret_cast<const h8*>(p.res + (size_t)m * p.res_ld + n);
#pragma unroll
          for (int q = 0; q < 8; ++q) v[q] = (half_t)((float)v[q] + (float)rr[q]);
        }
        st_out16(out + (size_t)m * p.out_ld + n, v);
      }
    }
  }
}

// split-K fp32 slabs and the fp32 output modes (NCHW image, token rows)
__device__ __forceinline__ void epilogue16_direct(const Params& p, f4 (&acc)[4][2][2], int m0, int n0, int m_w,
                                                  int n_w, int split_idx) {
  const int lane = threadIdx.x & 63, px = lane & 15, cg = lane >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + m_w + 16 * i + px;
    if (m >= p.M) continue;
    const int b = m / p.hw_out;
#pragma unroll
    for (int b2 = 0; b2 < 2; ++b2)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int n = n0 + n_w + 32 * b2 + 16 * j + 4 * cg;
        if (p.split > 1) {
          *reinterpret_cast<f4*>(p.partial + ((size_t)split_idx * p.M + m) * p.Npad + n) = acc[i][b2][j];
          continue;
        }
        float* out = reinterpret_cast<float*>(p.out);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (n + q >= p.N) continue;
          float x = acc[i][b2][j][q];
          if (p.bias) x += p.bias[n + q];
          if (p.row_bias) x += p.row_bias[(size_t)b * p.rb_ld + n + q];
          if (p.res) x += (float)p.res[(size_t)m * p.res_ld + n + q];
          if (p.out_mode == SDK_OUT_NCHW_F32)
            out[((size_t)b * p.N + n + q) * p.hw_out + (m - b * p.hw_out)] = x;
          else
            out[(size_t)m * p.out_ld + n + q] = x;
        }
      }
  }
}

// ---------------------------------------------------------------------- phased LDS-DMA kernel
// 256x256 tile, 8 waves (2 x 4), K-step 64 cut into four 16-KiB half-tiles streamed in
// the order A0 (pixels 0-127), W0 (even 32-channel groups), W1 (odd groups), A1
// (pixels 128-255).  One phase multiplies one (A half, W half) quadrant: 8 MFMAs per
// wave, fragments for the phase read from LDS at its start; a phase is two sections
// (reads + DMA issue + address math | MFMAs) separated by barriers, and the two wave
// rows run one barrier apart (ping-pong) so each SIMD overlaps one wave's MFMAs with
// the other wave's loads.
// Each phase issues the DMA of the half-tile D phases ahead into a ring of S slots
// (S >= D + 2: a slot is refilled >= 2 phases after its last read, which covers the
// one-barrier skew of the wave rows), and waits with a
// counted vmcnt that leaves D-2 (or D-1) half-tiles in flight — the loads of the next
// K-steps stream under the MFMAs instead of once per K-step behind a full barrier.
// Past the last K-step the same slots receive zero-page DMAs so every phase keeps
// the same vmcnt immediates.  A wave owns pixels {a*128 + wr*64 + (0..63)} and
// channels {64*wc + 32*b + (0..31)}, so a GEGLU (x, gate) 32-channel pair sits in one
// wave (W0 / W1 halves) and the direct epilogue applies unchanged.
template <int S_, int D_>
struct PhCfg {
  static constexpr int S = S_, D = D_;
  static constexpr int RING_BYTES = S * 128 * BK * 2;
  static constexpr bool VEC = RING_BYTES + 2 * 256 * 4 <= 160 * 1024;   // room for the staged bias / embedding
  static constexpr int LDS_BYTES = RING_BYTES + (VEC ? 2 * 256 * 4 : 0);
  static_assert(S >= D + 2 && D >= 2 && RING_BYTES <= 160 * 1024, "ring too small / too large");
};
constexpr int PH_HALF = 128 * BK;   // halfs per half-tile slot

// SIMPLE (p.simple, DBG == 0): the linear A issue of conv_glds_kernel — per-lane row offsets fixed, the K step's
// tap / channel offset in the scalar soffset
template <class PC, int DBG = 0, bool M16 = false, bool SIMPLE = false>
__global__ void __launch_bounds__(512) conv_ph_kernel(Params p) {
  extern __shared__ __attribute__((aligned(16))) half_t lds[];
  constexpr int S = PC::S, D = PC::D;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  const int nitems = p.tiles_m * p.tiles_n * p.split;
  const int it = xcd_remap((int)blockIdx.x + (int)blockIdx.y * (int)gridDim.x, nitems);
  int tm, tn, sidx;
  ph_stamp(p, 0);
  item_coords(p, it, tm, tn, sidx);
  const int m0 = tm * 256, n0 = tn * 256;
  const int kt0 = sidx * p.kt_per_split, kt1 = min(p.kt_total, kt0 + p.kt_per_split);
  const int nk = kt1 - kt0;
  const int lrow = lane >> 3;
  const int rch = (lane & 7) ^ ((wave * 4 + (lrow >> 1)) & 7);

  const DmaSrc d = make_dma_src(p, m0);
  const EpiVec ev = epi_vec_load(p, m0, n0, 256, 256);
  // this lane's DMA rows: slot row j*64 + wave*8 + lrow of every half (q = half*2 + j)
  unsigned pixb[4], msk[4], wv[4];
  const int mrow = m0 + wave * 8 + lrow;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int a = q >> 1, j = q & 1;
    a_row_ctx(p, mrow + a * 128 + j * 64, pixb[q], msk[q]);
    if constexpr (SIMPLE)   // pixb -> the lane's byte offset (tap window origin, chunk rch), or out of range
      pixb[q] = mrow + a * 128 + j * 64 < p.M ? __umul24(pixb[q], (unsigned)p.seg[0].ld0 * 2u) + (unsigned)rch * 16u
                                              : PH_OOB;
    const int pc = j * 8 + wave;
    wv[q] = w_row_ctx(p, n0 + 64 * (pc >> 2) + 32 * a + 8 * (pc & 3) + lrow, rch);
  }

#define SDK_PH_ISSUE_A(A_, SEG, KY, KX, CB, T, SLOT)                                       \
  do {                                                                                     \
    half_t* sl_ = lds + (SLOT) * PH_HALF + wave * 8 * BK;                                  \
    const int kt_ = kt0 + (T);                                                             \
    if constexpr (SIMPLE && DBG == 0) {                                                    \
      const int toff_ = ((KY) * p.seg[0].w + (KX)) * p.seg[0].ld0 * 2 + (CB) * 2;          \
      _Pragma("unroll") for (int j = 0; j < 2; ++j)                                        \
        ph_dma(d.a0, sl_ + j * 64 * BK, kt_ < kt1 ? pixb[(A_) * 2 + j] : PH_OOB, toff_);    \
    } else if (DBG & (1 | 256)) {                                                          \
    } else if (kt_ >= kt1) {                                                               \
      _Pragma("unroll") for (int j = 0; j < 2; ++j) ph_dma(d.w, sl_ + j * 64 * BK, PH_OOB, 0); \
    } else if (DBG & 512) {                                                                \
      _Pragma("unroll") for (int j = 0; j < 2; ++j)                                        \
        ph_dma(d.w, sl_ + j * 64 * BK, wv[(A_) * 2 + j], kt_ * BK * 2);                    \
    } else if (DBG & 1024) {                                                               \
      _Pragma("unroll") for (int j = 0; j < 2; ++j)                                        \
        ph_dma(SEG == 0 ? d.a0 : d.s0, sl_ + j * 64 * BK,                                  \
               __umul24(pixb[(A_) * 2 + j], (unsigned)p.seg[0].ld0 * 2u) + rch * 16u + (unsigned)(CB) * 2u, 0); \
    } else {                                                                               \
      _Pragma("unroll") for (int j = 0; j < 2; ++j)                                        \
        dma_a_piece(p, d, sl_ + j * 64 * BK, pixb[(A_) * 2 + j], msk[(A_) * 2 + j],         \
                    mrow + (A_) * 128 + j * 64, rch, SEG, KY, KX, CB);                     \
    }                                                                                      \
  } while (0)
#define SDK_PH_ISSUE_W(B_, T, SLOT)                                                        \
  do {                                                                                     \
    half_t* sl_ = lds + (SLOT) * PH_HALF + wave * 8 * BK;                                  \
    const int kt_ = kt0 + (T);                                                             \
    if (DBG & (1 | 128)) {                                                                 \
    } else if (kt_ >= kt1) {                                                               \
      _Pragma("unroll") for (int j = 0; j < 2; ++j) ph_dma(d.w, sl_ + j * 64 * BK, PH_OOB, 0); \
    } else {                                                                               \
      _Pragma("unroll") for (int j = 0; j < 2; ++j)                                        \
        ph_dma(d.w, sl_ + j * 64 * BK, wv[(B_) * 2 + j], kt_ * BK * 2);                    \
    }                                                                                      \
  } while (0)

  // prologue: half-tiles 0 .. D-1 (K-state decoded directly)
#pragma unroll
  for (int h = 0; h < D; ++h) {
    const int idx = h & 3;
    if (idx == 1 || idx == 2) {
      SDK_PH_ISSUE_W(idx - 1, h >> 2, h % S);
    } else {
      int sg, ky, kx, cb;
      ph_kstate(p, kt0 + (h >> 2), sg, ky, kx, cb);
      SDK_PH_ISSUE_A(idx == 3 ? 1 : 0, sg, ky, kx, cb, h >> 2, h % S);
    }
  }
  // in-loop A K-states: A0 / A1 half-tiles are issued for K-step t + TO0 / t + TO1
  constexpr int Q0 = ((0 - D) % 4 + 4) % 4, TO0 = (Q0 + D) >> 2;
  constexpr int Q3 = ((3 - D) % 4 + 4) % 4, TO3 = (Q3 + D) >> 2;
  int a0g, a0y, a0x, a0c, a1g, a1y, a1x, a1c;
  ph_kstate(p, kt0 + TO0, a0g, a0y, a0x, a0c);
  ph_kstate(p, kt0 + TO3, a1g, a1y, a1x, a1c);
#define SDK_PH_ISSUE(IDX, T, SLOT)                                                         \
  do {                                                                                     \
    if ((IDX) == 0) {                                                                      \
      SDK_PH_ISSUE_A(0, a0g, a0y, a0x, a0c, T, SLOT);                                      \
      ph_kadv(p, a0g, a0y, a0x, a0c);                                                      \
    } else if ((IDX) == 3) {                                                               \
      SDK_PH_ISSUE_A(1, a1g, a1y, a1x, a1c, T, SLOT);                                      \
      ph_kadv(p, a1g, a1y, a1x, a1c);                                                      \
    } else {                                                                               \
      SDK_PH_ISSUE_W((IDX) - 1, T, SLOT);                                                  \
    }                                                                                      \
  } while (0)
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (D - 2)) : "memory");
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  ph_stamp(p, 1);

  f16v acc[2][2][2];   // [A half][pixel tile][W half]                      (32x32x16 path)
  f4 acc16[2][4][2][2];   // [A half][16-pixel block][W half][16-channel block] (16x16x32 path)
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int b = 0; b < 2; ++b) acc[a][i][b] = f16v{};
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc16[a][i][b][j] = f4{};
  const int fr = lane & 31, fh = lane >> 5;
  const int r16 = lane & 15, c16 = lane >> 4;   // 16x16x32 operand: row in block, 8-half k chunk
  h8 fa[2][4], fb0[4], fb1[4];           // 32x32x16: [pixel tile][k16] / [k16]
  h8 ga[4][2], gb0[2][2], gb1[2][2];     // 16x16x32: [16-pixel block][k32] / [16-channel block][k32]
#define SDK_PH_READ_A(SLOT)                                                                \
  do {                                                                                     \
    const half_t* s_ = lds + (SLOT) * PH_HALF;                                             \
    if constexpr (M16) {                                                                   \
      _Pragma("unroll") for (int i = 0; i < 4; ++i)                                        \
        _Pragma("unroll") for (int k = 0; k < 2; ++k)                                      \
          ga[i][k] = *reinterpret_cast<const h8*>(s_ + swz(wr * 64 + i * 16 + r16, 4 * k + c16)); \
    } else {                                                                               \
      _Pragma("unroll") for (int i = 0; i < 2; ++i)                                        \
        _Pragma("unroll") for (int kk = 0; kk < 4; ++kk)                                   \
          fa[i][kk] = *reinterpret_cast<const h8*>(s_ + swz(wr * 64 + i * 32 + fr, kk * 2 + fh)); \
    }                                                                                      \
  } while (0)
#define SDK_PH_READ_B(FB, SLOT)                                                            \
  do {                                                                                     \
    const half_t* s_ = lds + (SLOT) * PH_HALF;                                             \
    if constexpr (M16) {                                                                   \
      _Pragma("unroll") for (int j = 0; j < 2; ++j)                                        \
        _Pragma("unroll") for (int k = 0; k < 2; ++k)                                      \
          g##FB[j][k] = *reinterpret_cast<const h8*>(s_ + swz(wc * 32 + j * 16 + r16, 4 * k + c16)); \
    } else {                                                                               \
      _Pragma("unroll") for (int kk = 0; kk < 4; ++kk)                                     \
        f##FB[kk] = *reinterpret_cast<const h8*>(s_ + swz(wc * 32 + fr, kk * 2 + fh));     \
    }                                                                                      \
  } while (0)
#define SDK_PH_SYNC(NOUT)                                                                  \
  do {                                                                                     \
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (NOUT)) : "memory");                      \
    __builtin_amdgcn_sched_barrier(0);                                                     \
    __builtin_amdgcn_s_barrier();                                                          \
    __builtin_amdgcn_sched_barrier(0);                                                     \
  } while (0)
#define SDK_PH_MMA(A, FB)                                                                  \
  do {                                                                                     \
    __builtin_amdgcn_s_setprio(1);                                                         \
    if constexpr (M16) {                                                                   \
      if (!(DBG & 2)) _Pragma("unroll") for (int k = 0; k < 2; ++k)                        \
        _Pragma("unroll") for (int i = 0; i < 4; ++i)                                      \
          _Pragma("unroll") for (int j = 0; j < 2; ++j)                                    \
            acc16[A][i][(FB) == 1][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(            \
                (FB) ? gb1[j][k] : gb0[j][k], ga[i][k], acc16[A][i][(FB) == 1][j], 0, 0, 0); \
    } else {                                                                               \
      if (!(DBG & 2)) _Pragma("unroll") for (int kk = 0; kk < 4; ++kk)                     \
        _Pragma("unroll") for (int i = 0; i < 2; ++i)                                      \
          acc[A][i][(FB) == 1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(                   \
              (FB) ? fb1[kk] : fb0[kk], fa[i][kk], acc[A][i][(FB) == 1], 0, 0, 0);         \
    }                                                                                      \
    __builtin_amdgcn_s_setprio(0);                                                         \
  } while (0)

#define SDK_PH_BAR()                                                                       \
  do {                                                                                     \
    __builtin_amdgcn_sched_barrier(0);                                                     \
    __builtin_amdgcn_s_barrier();                                                          \
    __builtin_amdgcn_sched_barrier(0);                                                     \
  } while (0)
  // ping-pong: the wr = 1 waves run one barrier behind, so on every SIMD one wave's
  // MFMA section overlaps the other wave's fragment reads / DMA issue / address math
  if (wr == 1) SDK_PH_BAR();
  for (int t = 0; t < nk; ++t) {
    const int g = 4 * t;
    // phase 0: (A0, W0)
    SDK_PH_READ_A(g % S);
    SDK_PH_READ_B(b0, (g + 1) % S);
    SDK_PH_ISSUE((0 + D) & 3, (g + 0 + D) >> 2, (g + 0 + D) % S);
    SDK_PH_SYNC(D - 2);
    SDK_PH_MMA(0, 0);
    SDK_PH_BAR();
    // phase 1: (A0, W1)
    SDK_PH_READ_B(b1, (g + 2) % S);
    SDK_PH_ISSUE((1 + D) & 3, (g + 1 + D) >> 2, (g + 1 + D) % S);
    SDK_PH_SYNC(D - 2);
    SDK_PH_MMA(0, 1);
    SDK_PH_BAR();
    // phase 2: (A1, W1)
    SDK_PH_READ_A((g + 3) % S);
    SDK_PH_ISSUE((2 + D) & 3, (g + 2 + D) >> 2, (g + 2 + D) % S);
    SDK_PH_SYNC(D - 1);
    SDK_PH_MMA(1, 1);
    SDK_PH_BAR();
    // phase 3: (A1, W0) — fragments already in registers
    SDK_PH_ISSUE((3 + D) & 3, (g + 3 + D) >> 2, (g + 3 + D) % S);
    SDK_PH_SYNC(D - 2);
    SDK_PH_MMA(1, 0);
    SDK_PH_BAR();
  }
  if (wr == 0) SDK_PH_BAR();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  ph_stamp(p, 2);
#undef SDK_PH_BAR
#undef SDK_PH_ISSUE
#undef SDK_PH_ISSUE_A
#undef SDK_PH_ISSUE_W
#undef SDK_PH_READ_A
#undef SDK_PH_READ_B
#undef SDK_PH_SYNC
#undef SDK_PH_MMA
  if (DBG & 64) {      // diagnostics: keep the accumulators alive, store nothing
    float sink = 0.f;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int b = 0; b < 2; ++b) sink += acc[a][i][b][0];
    if (sink == 12345.678f) reinterpret_cast<float*>(p.out)[0] = sink;
    return;
  }
  // every wave past its last ring read before the ring is reused as epilogue scratch
  float* vec_s = reinterpret_cast<float*>(reinterpret_cast<char*>(lds) + PC::RING_BYTES);
  if constexpr (PC::VEC) epi_vec_store(ev, vec_s, 256);
  __builtin_amdgcn_s_barrier();
  const float* bias_s = PC::VEC ? vec_s : nullptr;   // zeros where absent (as in conv_glds_kernel)
  const float* rb_s = (PC::VEC && (ev.one_img || !p.row_bias)) ? vec_s + 256 : nullptr;
  if constexpr (M16) {
    if (p.split == 1 && (p.out_mode == SDK_OUT_NHWC_F16 || p.out_mode == SDK_OUT_GEGLU_F16)) {
      epilogue16_lds(p, acc16[0], m0, n0, wr * 64, wc * 64, lds + wave * (EPI16_BYTES / 2), bias_s, rb_s);
      epilogue16_lds(p, acc16[1], m0, n0, 128 + wr * 64, wc * 64, lds + wave * (EPI16_BYTES / 2), bias_s, rb_s);
      ph_stamp(p, 3);
    } else {
      epilogue16_direct(p, acc16[0], m0, n0, wr * 64, wc * 64, sidx);
      epilogue16_direct(p, acc16[1], m0, n0, 128 + wr * 64, wc * 64, sidx);
    }
    return;
  }
  if (p.split == 1 && (p.out_mode == SDK_OUT_NHWC_F16 || p.out_mode == SDK_OUT_GEGLU_F16)) {
    if (p.gnp) {
      // GroupNorm statistics of the stored tile (build_params: full fp16 NHWC tiles only): each of the
      // two 128-row halves gets its own per-wave scratch + parked (mean, M2) [2][64] (5.5 KiB per wave,
      // 16 areas in the idle ring), then one thread per tile channel merges the 8 row blocks of 32 —
      // "virtual" wave rows 2 * half + wr in row order
      constexpr int PWS = (EPI_BYTES + 2 * 64 * 8) / 2;   // halfs per scratch area
      static_assert(16 * PWS * 2 <= PC::RING_BYTES, "GN scratch fits the ring");
      epilogue_lds<2, 2, true>(p, acc[0], m0, n0, wr * 64, wc * 64, lds + wave * PWS, bias_s, rb_s);
      epilogue_lds<2, 2, true>(p, acc[1], m0, n0, 128 + wr * 64, wc * 64, lds + (8 + wave) * PWS, bias_s, rb_s);
      __syncthreads();
      gn_tile_store<4, 4, 64, 2, 32, 256, 256>(p, m0, n0, [&](int w) {
        const int vm = w >> 2, wn = w & 3;   // virtual wave row = 2 * half + wr
        return reinterpret_cast<const float2*>(lds + ((vm >> 1) * 8 + (vm & 1) * 4 + wn) * PWS + EPI_BYTES / 2);
      });
      return;
    }
    epilogue_lds<2, 2>(p, acc[0], m0, n0, wr * 64, wc * 64, lds + wave * (EPI_BYTES / 2), bias_s, rb_s);
    epilogue_lds<2, 2>(p, acc[1], m0, n0, 128 + wr * 64, wc * 64, lds + wave * (EPI_BYTES / 2), bias_s, rb_s);
    ph_stamp(p, 3);
  } else {
    epilogue_direct<2, 2>(p, acc[0], m0, n0, wr * 64, wc * 64, sidx);
    epilogue_direct<2, 2>(p, acc[1], m0, n0, 128 + wr * 64, wc * 64, sidx);
  }
}

using PhCfg8 = PhCfg<8, 6>;
using PhCfg10 = PhCfg<10, 8>;

template <class PC, int DBG = 0, bool M16 = false>
int launch_ph(const Params& p, hipStream_t s) {
  static std::atomic<unsigned long long> attr_set{0}, attr_simple{0};
  if constexpr (DBG == 0) {
    if (p.simple == 1) {
      if (int e = ensure_dyn_lds((const void*)conv_ph_kernel<PC, 0, M16, true>, PC::LDS_BYTES, attr_simple, "conv2d"))
        return e;
      hipLaunchKernelGGL((conv_ph_kernel<PC, 0, M16, true>), dim3(p.tiles_m * p.tiles_n, p.split), dim3(512),
                         PC::LDS_BYTES, s, p);
      return check_launch("conv_ph");
    }
  }
  if (int e = ensure_dyn_lds((const void*)conv_ph_kernel<PC, DBG, M16>, PC::LDS_BYTES, attr_set, "conv2d")) return e;
  hipLaunchKernelGGL((conv_ph_kernel<PC, DBG, M16>), dim3(p.tiles_m * p.tiles_n, p.split), dim3(512),
                     PC::LDS_BYTES, s, p);
  return check_launch("conv_ph");
}

#if SDK_PART(0)   // split-K reduces, direct and skinny kernels: host planner part only
// Split-K reduction + epilogue: 8 columns per thread.
// Slab sum of one (row, 8-column) octet: the slabs' 32-B pieces are loaded SK_U splits at a time
// (independent loads in flight, instead of one dependent round trip per split) and added in split
// order — a clamped slab past the end is loaded and selected away, never branched around (hipcc
// would sink a conditional load under its branch and wait for each) — so the sum equals a plain loop's.
constexpr int SK_U = 4;
template <int NR>   // NR rows at once: their loads are in flight together
__device__ __forceinline__ void slab_sum8(const Params& p, const int (&m)[NR], int n, float (&v)[NR][8]) {
#pragma unroll
  for (int q = 0; q < NR; ++q)
#pragma unroll
    for (int j = 0; j < 8; ++j) v[q][j] = 0.f;
  for (int s0 = 0; s0 < p.split; s0 += SK_U) {
    f4 a[NR][SK_U], b[NR][SK_U];
#pragma unroll
    for (int u = 0; u < SK_U; ++u) {
      const int su = min(s0 + u, p.split - 1);
#pragma unroll
      for (int q = 0; q < NR; ++q) {
        const f4* src = reinterpret_cast<const f4*>(p.partial + ((size_t)su * p.M + m[q]) * p.Npad + n);
        a[q][u] = src[0];
        b[q][u] = src[1];
      }
    }
#pragma unroll
    for (int u = 0; u < SK_U; ++u) {
      const bool in = s0 + u < p.split;
#pragma unroll
      for (int q = 0; q < NR; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[q][j] += in ? a[q][u][j] : 0.f;
          v[q][4 + j] += in ? b[q][u][j] : 0.f;
        }
    }
  }
}

// bias[n..n+7] + row_bias[b][n..n+7] as two vector loads each (scalar loads only for an unaligned
// row_bias view), issued together instead of one dependent load per element
__device__ __forceinline__ void epi_add8(const Params& p, int b, int n, float (&bi)[8], float (&rbv)[8]) {
  f4 b0 = f4{}, b1 = f4{}, r0 = f4{}, r1 = f4{};
  if (p.bias) {
    const f4* q = reinterpret_cast<const f4*>(p.bias + n);
    b0 = q[0];
    b1 = q[1];
  }
  if (p.row_bias) {
    const float* rb = p.row_bias + (size_t)b * p.rb_ld + n;
    if (!((uintptr_t)rb & 15)) {
      const f4* q = reinterpret_cast<const f4*>(rb);
      r0 = q[0];
      r1 = q[1];
    } else {
      r0 = f4{rb[0], rb[1], rb[2], rb[3]};
      r1 = f4{rb[4], rb[5], rb[6], rb[7]};
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    bi[j] = b0[j];
    bi[4 + j] = b1[j];
    rbv[j] = r0[j];
    rbv[4 + j] = r1[j];
  }
}

__global__ void __launch_bounds__(256) splitk_reduce_kernel(Params p) {
  const int groups = p.N / 8;
  const size_t total = (size_t)p.M * groups;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int m = (int)(e / groups), n = (int)(e - (size_t)m * groups) * 8;
    const int mo = out_row<true>(p, m);   // phase form (fp16 NHWC only): the slab row's output pixel; padding rows skipped
    if (mo < 0) continue;
    float vv[1][8];
    slab_sum8<1>(p, {m}, n, vv);
    float (&v)[8] = vv[0];
    const int b = m / p.hw_out;
    float bi[8], rbv[8];
    epi_add8(p, b, n, bi, rbv);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = act_fn(p.act, (v[j] + bi[j]) + rbv[j]);
    if (p.out_mode == SDK_OUT_NHWC_F16) {
      h8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (half_t)v[j];
      if (p.res) {
        h8 rr = ldg16(p.res + (size_t)m * p.res_ld + n);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (half_t)((float)o[j] + (float)rr[j]);
      }
      *reinterpret_cast<h8*>(reinterpret_cast<half_t*>(p.out) + (size_t)mo * p.out_ld + n) = o;
    } else {
      float* out = reinterpret_cast<float*>(p.out);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float x = v[j];
        if (p.res) x += (float)p.res[(size_t)m * p.res_ld + n + j];
        if (p.out_mode == SDK_OUT_NCHW_F32)
          out[((size_t)b * p.N + n + j) * p.hw_out + (m - b * p.hw_out)] = x;
        else
          out[(size_t)m * p.out_ld + n + j] = x;
      }
    }
  }
}

// Split-K reduction + epilogue that also emits the GroupNorm statistics of its rows (p.gnp):
// grid (batch * gn_nch, ceil(N / 64)); 256 threads = 32 row lanes x 8 column octets over one chunk
// (hw_out / gn_nch rows of one image); per-lane pivot-shifted sums, Chan merge of the 32 row lanes
// through LDS, one (mean, M2) per chunk and channel.
__global__ void __launch_bounds__(256) splitk_reduce_gn_kernel(Params p) {
  __shared__ float2 red[32][64];
  const int tc = threadIdx.x & 7, tr = threadIdx.x >> 3;
  const int b = blockIdx.x / p.gn_nch, chunk = blockIdx.x - b * p.gn_nch;
  // phase form: an image's rows in chunk order are phase major (4 * hw_out of them); row ri of the image is
  // slab row ph * ph_rows_pad + b * hw_out + rem and output pixel (b, 2i + a, 2j + b)
  const int R = (p.phase ? 4 : 1) * p.hw_out / p.gn_nch;
  auto row_of = [&](int ri, int& mv, int& mo) __attribute__((always_inline)) {
    if (!p.phase) {
      mv = mo = b * p.hw_out + ri;
      return;
    }
    const int ph = ri / p.hw_out, rem = ri - ph * p.hw_out;
    const int i = rem / p.wo, j = rem - i * p.wo;
    mv = ph * p.ph_rows_pad + b * p.hw_out + rem;
    mo = (b * 2 * p.ho + 2 * i + (ph >> 1)) * (2 * p.wo) + 2 * j + (ph & 1);
  };
  const int n = blockIdx.y * 64 + tc * 8;
  const bool colok = n < p.N;
  GnAcc ga;
  float bi[8], rbv[8];
  if (colok) epi_add8(p, b, n, bi, rbv);   // the thread's columns and image are fixed
  for (int r = tr; r < R && colok; r += 64) {   // rows r and r + 32 together
    const bool two = r + 32 < R;
    int mm[2], mo[2];
    row_of(chunk * R + r, mm[0], mo[0]);
    row_of(chunk * R + (two ? r + 32 : r), mm[1], mo[1]);
    h8 rr[2] = {h8{}, h8{}};
    if (p.res) {
#pragma unroll
      for (int q = 0; q < 2; ++q) rr[q] = ldg16(p.res + (size_t)mm[q] * p.res_ld + n);
    }
    float v[2][8];
    slab_sum8<2>(p, mm, n, v);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      if (q == 1 && !two) break;
      h8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (half_t)act_fn(p.act, (v[q][j] + bi[j]) + rbv[j]);
      if (p.res) {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (half_t)((float)o[j] + (float)rr[q][j]);
      }
      *reinterpret_cast<h8*>(reinterpret_cast<half_t*>(p.out) + (size_t)mo[q] * p.out_ld + n) = o;
      gn_acc_add(ga, o, r == tr && q == 0);
    }
  }
  const int cnt = R > tr ? (R - tr + 31) / 32 : 0;
  if (cnt > 0 && colok) {
    const float inv = 1.f / (float)cnt;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      red[tr][tc * 8 + j] = make_float2(ga.piv[j] + ga.s1[j] * inv, fmaxf(ga.s2[j] - ga.s1[j] * ga.s1[j] * inv, 0.f));
  }
  __syncthreads();
  const int c = threadIdx.x, nn = blockIdx.y * 64 + c;
  if (c >= 64 || nn >= p.N) return;
  float2 acc = red[0][c];
  float na = (float)((R + 31) / 32);
  for (int t = 1; t < 32 && t < R; ++t) {
    const float nb = (float)((R - t + 31) / 32);
    const float2 q = red[t][c];
    const float dl = q.x - acc.x, f = nb / (na + nb);
    acc.x += dl * f;
    acc.y += q.y + dl * dl * na * f;
    na += nb;
  }
  p.gnp[((size_t)b * p.gn_nch + chunk) * p.N + nn] = acc;
}

// Direct convolution for a handful of output channels (variant 34): the UNet's conv_out (320 -> 4)
// and the VAE decoder's conv_out (128 -> 3).  The implicit GEMM pads N to a 128-wide tile (32-43x
// wasted MFMA work) and re-reads every input pixel per tap through LDS-DMA; here a workgroup owns an
// 8 x 32 output patch, stages its (8+2) x (32+2) input halo of one 64-channel block in LDS once, and
// each thread accumulates its pixel's <= 8 outputs with v_dot2_f32_f16 from the halo and the
// block's weights (LDS broadcast reads).  Input read ~1.3x once; the FMAs run on the vector ALUs.
constexpr int DC_TX = 32, DC_LD = BK + 8;
constexpr int DC_MAXN = 8;

// TY output rows x 32 columns per workgroup; QS threads per pixel split the 64-channel block
// (QS = 4: 2 x 32 pixels, each thread 16 channels — 4x the threads for the small UNet maps, partial
// sums reduced through LDS; QS = 1: 8 x 32 pixels, one thread per pixel — the 512x512 VAE map)
template <int NO, int TY, int QS>
__global__ void __launch_bounds__(256) conv_direct_kernel(Params p) {
  constexpr int HY = TY + 2, HX = DC_TX + 2, CPQ = BK / QS;   // halo rows / cols, channels per thread
  static_assert(TY * DC_TX * QS == 256, "one thread per (pixel, channel split)");
  __shared__ __attribute__((aligned(16))) half_t xs[HY * HX * DC_LD];
  __shared__ __attribute__((aligned(16))) half_t ws[NO * 9 * BK];
  __shared__ float red[QS > 1 ? QS * TY * DC_TX * NO : 1];
  const Seg& g = p.seg[0];
  const int tid = threadIdx.x;
  const int tiles_x = (p.wo + DC_TX - 1) / DC_TX, tiles_y = (p.ho + TY - 1) / TY;
  const int b = blockIdx.x / (tiles_x * tiles_y), t = blockIdx.x - b * tiles_x * tiles_y;
  const int oy0 = (t / tiles_x) * TY, ox0 = (t % tiles_x) * DC_TX;
  const int pix = tid % (TY * DC_TX), q = tid / (TY * DC_TX);
  const int ty = pix / DC_TX, tx = pix % DC_TX;
  // halo origin: input (oy0 - org, ox0 - org); 3x3 taps read halo (ty + ky, tx + kx), a 1x1 reads its centre
  const int ks = g.ksize, org = ks == 3 ? g.pad : 1, off = ks == 3 ? 0 : 1;
  float acc[NO];
#pragma unroll
  for (int o = 0; o < NO; ++o) acc[o] = 0.f;
  const int nblk = g.cin_pad / BK;
  for (int cb = 0; cb < nblk; ++cb) {
    // halo: HY x HX pixels x 64 channels, 16-B vectors; zeros outside the image (pad) and past cin
    for (int e = tid; e < HY * HX * (BK / 8); e += 256) {
      const int px = e / (BK / 8), v = e - px * (BK / 8);
      const int hy = px / HX, hx = px - hy * HX;
      const int iy = oy0 - org + hy, ix = ox0 - org + hx;
      const int c = cb * BK + v * 8;
      h8 val = {};
      if ((unsigned)iy < (unsigned)g.h && (unsigned)ix < (unsigned)g.w && c < g.cin)
        val = *reinterpret_cast<const h8*>(g.src0 + ((size_t)(b * g.h + iy) * g.w + ix) * g.ld0 + c);
      *reinterpret_cast<h8*>(xs + px * DC_LD + v * 8) = val;
    }
    // weights of the block: packed row n, columns (cb * taps + tap) * 64 + j
    for (int e = tid; e < NO * ks * ks * (BK / 8); e += 256) {
      const int n = e / (ks * ks * (BK / 8)), r = e - n * (ks * ks * (BK / 8));
      const int tap = r / (BK / 8), v = r - tap * (BK / 8);
      h8 wv = {};
      if (n < p.N) wv = *reinterpret_cast<const h8*>(p.W + (size_t)n * p.ldw + (size_t)(cb * ks * ks + tap) * BK + v * 8);
      *reinterpret_cast<h8*>(ws + (n * 9 + tap) * BK + v * 8) = wv;
    }
    __syncthreads();
    for (int tap = 0; tap < ks * ks; ++tap) {
      const int dy = tap / ks + off, dx = tap % ks + off;
      const half_t* xr = xs + ((ty + dy) * HX + tx + dx) * DC_LD + q * CPQ;
#pragma unroll
      for (int v = 0; v < CPQ / 8; ++v) {
        const h8 xv = *reinterpret_cast<const h8*>(xr + v * 8);
#pragma unroll
        for (int o = 0; o < NO; ++o) {
          const h8 wv = *reinterpret_cast<const h8*>(ws + (o * 9 + tap) * BK + q * CPQ + v * 8);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const h2 xa = {xv[2 * j], xv[2 * j + 1]}, wa = {wv[2 * j], wv[2 * j + 1]};
            acc[o] = __builtin_amdgcn_fdot2(xa, wa, acc[o], false);
          }
        }
      }
    }
    __syncthreads();
  }
  if constexpr (QS > 1) {
#pragma unroll
    for (int o = 0; o < NO; ++o) red[(q * TY * DC_TX + pix) * NO + o] = acc[o];
    __syncthreads();
    if (q != 0) return;
#pragma unroll
    for (int o = 0; o < NO; ++o) {
      float a = acc[o];
#pragma unroll
      for (int k = 1; k < QS; ++k) a += red[(k * TY * DC_TX + pix) * NO + o];
      acc[o] = a;
    }
  }
  const int oy = oy0 + ty, ox = ox0 + tx;
  if (oy >= p.ho || ox >= p.wo) return;
  const int m = (b * p.ho + oy) * p.wo + ox;
#pragma unroll
  for (int o = 0; o < NO; ++o) {
    if (o >= p.N) break;
    const float val = acc[o] + (p.bias ? p.bias[o] : 0.f);
    if (p.out_mode == SDK_OUT_NCHW_F32)
      reinterpret_cast<float*>(p.out)[((size_t)b * p.N + o) * p.hw_out + oy * p.wo + ox] = val;
    else if (p.out_mode == SDK_OUT_ROWS_F32)
      reinterpret_cast<float*>(p.out)[(size_t)m * p.out_ld + o] = val;
    else
      reinterpret_cast<half_t*>(p.out)[(size_t)m * p.out_ld + o] = (half_t)val;
  }
}

// pixel tiles: 8 x 32 with one thread per pixel when that already fills the chip (>= 4 workgroups
// per CU), else 2 x 32 with four channel splits per pixel
template <int NO>
int launch_direct_n(const Params& p, hipStream_t s) {
  const int big = ((p.wo + DC_TX - 1) / DC_TX) * ((p.ho + 7) / 8) * p.batch;
  if (big >= 1024) {
    hipLaunchKernelGGL((conv_direct_kernel<NO, 8, 1>), dim3(big), dim3(256), 0, s, p);
  } else {
    const int small = ((p.wo + DC_TX - 1) / DC_TX) * ((p.ho + 1) / 2) * p.batch;
    hipLaunchKernelGGL((conv_direct_kernel<NO, 2, 4>), dim3(small), dim3(256), 0, s, p);
  }
  return check_launch("conv_direct");
}

int launch_direct(const Params& p, hipStream_t s) {
  return p.N <= 4 ? launch_direct_n<4>(p, s) : launch_direct_n<8>(p, s);
}

// Skinny GEMM for M <= 64 rows (variant 35): the time-embedding MLP and the ResBlock embedding
// projections run at M = batch (16 at the bench), where a 128-row tile wastes 7/8 of its MFMA work
// and the 1280 x 20160 weight is streamed by a few dozen workgroups (~30 us per launch).  Here a
// workgroup owns 16 output columns and its 4 waves split K; each lane streams 16-B pieces of its
// column's packed weight row straight from HBM (every weight byte is read once, SK_PF K-steps in
// flight), the A fragments (x rows, SiLU applied on load) come from L2, v_mfma_f32_16x16x32_f16
// accumulates M/16 row blocks per weight fragment, and the 4 wave partials are summed through LDS.
// 16x16x32 operand layout: lane l supplies A[row l%16][k 8(l/16)..+8] and B[k 8(l/16)..+8][col l%16];
// D element i of lane l is D[4(l/16) + i][l%16].
constexpr int SK_MAXM = 64, SK_PF = 8;

template <int MB>   // 16-row blocks
__global__ void __launch_bounds__(256) conv_skinny_kernel(Params p) {
  __shared__ float red[4][MB][4][64];
  const Seg& g = p.seg[0];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * 16, K = g.cin;
  const int ksteps = (K + 31) / 32, per = (ksteps + 3) / 4;
  const int kb = min(ksteps, wave * per), ke = min(ksteps, kb + per);
  const int kl = (lane >> 4) * 8;
  const half_t* wrow = p.W + (size_t)(n0 + (lane & 15)) * p.ldw;   // rows < wrows (N padded to 128)
  f4 acc[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) acc[mb] = f4{};
  for (int k0 = kb; k0 < ke; k0 += SK_PF) {
    h8 w[SK_PF];
#pragma unroll
    for (int u = 0; u < SK_PF; ++u) {
      const int k = (k0 + u) * 32 + kl;
      w[u] = (k0 + u < ke && k < K) ? ldg16(wrow + k) : h8{};
    }
#pragma unroll
    for (int u = 0; u < SK_PF; ++u) {
      if (k0 + u >= ke) break;
      const int k = (k0 + u) * 32 + kl;
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) {
        const int row = mb * 16 + (lane & 15);
        h8 a = {};
        if (row < p.M && k < K) {
          a = ldg16(g.src0 + (size_t)row * g.ld0 + k);
          if (g.silu) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const float x = (float)a[j];
              a[j] = (half_t)(x * __builtin_amdgcn_rcpf(1.0f + __expf(-x)));
            }
          }
        }
        acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, w[u], acc[mb], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int i = 0; i < 4; ++i) red[wave][mb][i][lane] = acc[mb][i];
  __syncthreads();
  for (int e = tid; e < MB * 4 * 64; e += 256) {
    const int mb = e / 256, i = (e >> 6) & 3, l = e & 63;
    const int row = mb * 16 + 4 * (l >> 4) + i, n = n0 + (l & 15);
    if (row >= p.M || n >= p.N) continue;
    float v = red[0][mb][i][l] + red[1][mb][i][l] + red[2][mb][i][l] + red[3][mb][i][l];
    if (p.bias) v += p.bias[n];
    if (p.row_bias) v += p.row_bias[(size_t)(row / p.hw_out) * p.rb_ld + n];
    v = act_fn(p.act, v);
    if (p.res) v += (float)p.res[(size_t)row * p.res_ld + n];
    if (p.out_mode == SDK_OUT_ROWS_F32)
      reinterpret_cast<float*>(p.out)[(size_t)row * p.out_ld + n] = v;
    else
      reinterpret_cast<half_t*>(p.out)[(size_t)row * p.out_ld + n] = (half_t)v;
  }
}

int launch_skinny(const Params& p, hipStream_t s) {
  const dim3 grid((p.N + 15) / 16);
  if (p.M <= 16) hipLaunchKernelGGL(conv_skinny_kernel<1>, grid, dim3(256), 0, s, p);
  else if (p.M <= 32) hipLaunchKernelGGL(conv_skinny_kernel<2>, grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL(conv_skinny_kernel<4>, grid, dim3(256), 0, s, p);
  return check_launch("conv_skinny");
}

#endif  // SDK_PART(0)

template <class CF, int SIMPLE>
int launch_glds_as(const Params& p, hipStream_t s) {
  static std::atomic<unsigned long long> attr_set{0};   // per device: the dynamic-LDS cap, once
  if (int e = ensure_dyn_lds((const void*)conv_glds_kernel<CF, SIMPLE>, CF::LDS_BYTES, attr_set, "conv2d")) return e;
  hipLaunchKernelGGL((conv_glds_kernel<CF, SIMPLE>), dim3(p.tiles_m * p.tiles_n, p.split), dim3(CF::NT),
                     CF::LDS_BYTES, s, p);
  return check_launch("conv_glds");
}

template <class CF>
int launch_glds(const Params& p, hipStream_t s) {
  switch (p.simple) {
    case 1: return launch_glds_as<CF, 1>(p, s);
    case 2: return launch_glds_as<CF, 2>(p, s);
    default: return launch_glds_as<CF, 0>(p, s);
  }
}

// ---------------------------------------------------------------------- the variant table
// One row per variant id; the planner, the part launchers, the dispatch of sdk_conv2d and sdk_kernel_name
// all read it, and nothing else says what an id means.  A row's columns:
//   id | kernel family | config type (its TBM x TBN is the tile) | DBG mask (DIAG only) |
//   workgroups per CU for the planner's fill estimate (not Cfg::OCC: 4 shares a CU at OCC 1) |
//   whether the epilogue pairs the (x, gate) halves of a GEGLU projection | sdk_kernel_name
// The sublist a row sits in is the compile part that instantiates its kernel (below).  Families: NONE no such id;
// IGEMM register-staged conv_igemm_kernel; GLDS the LDS-DMA tile conv_glds_kernel; PH32 / PH16 the phased 256x256
// conv_ph_kernel on 32x32x16 / 16x16x32; DIRECT (<= 8 output channels); SKINNY (<= 64 rows); DIAG a phased
// ablation (wrong outputs by design, launched by the diagnostics build only); RETIRED named, never planned.
enum class Fam { NONE, IGEMM, GLDS, PH32, PH16, DIRECT, SKINNY, DIAG, RETIRED };
struct CfgIgemm { static constexpr int TBM = BM, TBN = BN; };
struct CfgUntiled { static constexpr int TBM = 0, TBN = 0; };   // direct / skinny: no BM x BN tiling
template <class CF> struct TileOf { static constexpr int TBM = CF::TBM, TBN = CF::TBN; };
template <int S, int D> struct TileOf<PhCfg<S, D>> { static constexpr int TBM = 256, TBN = 256; };

// variant 5 (256x320 on 32x32x16, 16 waves) spilled at the 128-VGPR cap of 4 waves per SIMD; its row keeps the
// name and carries the config of 22, the same tile on 16x16x32, which a forced 5 runs as.  36 / 37 (halo tiles)
// and 39 (the 8-wave 256x320 on 32x32x16, spilled, never built) have no row: unknown.
#define SDK_CONV_VARIANTS_P0(X, P)                                                                      \
  X(P, 0, IGEMM, CfgIgemm, 0, 2, true, "conv_igemm_kernel")                                             \
  X(P, 5, RETIRED, Cfg256x320m, 0, 1, false, "conv_glds_kernel<Cfg<256,320,8,2>>")                      \
  X(P, 34, DIRECT, CfgUntiled, 0, 1, false, "conv_direct_kernel")                                       \
  X(P, 35, SKINNY, CfgUntiled, 0, 1, false, "conv_skinny_kernel")
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
constexpr int kVariantIds = 41;      // ids are 0 .. 40 (a row past the end does not compile)
constexpr int kRetiredRunsAs = 22;

#ifdef SDK_CONV_DIAGNOSTICS
constexpr bool kDiagnostics = true;
#else
constexpr bool kDiagnostics = false;
#endif

// A tile-kernel row's launch.  A template, so `if constexpr` keeps each row to its own family's kernel: a
// kernel template is instantiated only in the part whose sublist names it.
template <Fam F, class CF, int DBG>
int launch_variant(const Params& p, hipStream_t s) {
  if constexpr (F == Fam::GLDS) return launch_glds<CF>(p, s);
  else if constexpr (F == Fam::PH32) return launch_ph<CF>(p, s);
  else if constexpr (F == Fam::PH16) return launch_ph<CF, 0, true>(p, s);
  else if constexpr (F == Fam::DIAG && kDiagnostics) return launch_ph<CF, DBG>(p, s);
  else return fail(SDK_EINVAL, "conv2d: this build has no kernel for the planned variant");
}

// ---------------------------------------------------------------------- compile partition
// build.py compiles this file once per part (-DSDK_CONV_PART=k, in parallel; one monolithic object took
// ~10 minutes): part 0 holds the host planner, the ABI entry points and the small kernels, parts 1-5 the
// tile-kernel instantiations, reached through these hidden C-linkage launchers (the kernel templates are
// visible everywhere, each is instantiated only in the part whose launcher expands its row).  Without
// SDK_CONV_PART every part is in one object.
#define SDK_HIDDEN __attribute__((visibility("hidden")))
}  // namespace
}  // namespace sdk
// Params lives in an anonymous namespace, so each part compiles its own copy of the type: the caller passes
// its sizeof(Params) and a part whose layout differs (a part-only preprocessor state) refuses the launch
#define SDK_PART_DECL(k) extern "C" SDK_HIDDEN int sdk_conv_launch_part##k(int v, const void* pp, int psize, void* st)
#define SDK_LAUNCH_CASE(P, ID, FAM, CF, DBG, PER_CU, GEGLU, NAME) \
    case ID: return launch_variant<Fam::FAM, CF, DBG>(p, s);
#define SDK_PART_FN(k) SDK_PART_FN_(k)   /* k may itself be a macro (SDK_CONV_PART) */
#define SDK_PART_FN_(k) SDK_PART_DECL(k) {                                                              \
    using namespace sdk;                                                                               \
    if (psize != (int)sizeof(Params))                                                                   \
      return fail(SDK_EINVAL, "conv2d: Params layout differs between compile parts (" +                 \
                                  std::to_string(psize) + " vs " + std::to_string(sizeof(Params)) + ")"); \
    const Params& p = *static_cast<const Params*>(pp);                                                 \
    const hipStream_t s = (hipStream_t)st;                                                              \
    switch (v) { SDK_CONV_VARIANTS_P##k(SDK_LAUNCH_CASE, k) }                                           \
    return fail(SDK_EINVAL, "conv2d: variant " + std::to_string(v) + " is not in this launcher part");  \
  }
SDK_PART_DECL(1); SDK_PART_DECL(2); SDK_PART_DECL(3); SDK_PART_DECL(4); SDK_PART_DECL(5);
#if SDK_CONV_PART > 0   // this object's own part
SDK_PART_FN(SDK_CONV_PART)
#elif SDK_CONV_PART < 0
SDK_PART_FN(1) SDK_PART_FN(2) SDK_PART_FN(3) SDK_PART_FN(4) SDK_PART_FN(5)
#endif
#if SDK_PART(0)
namespace sdk {
namespace {

struct Variant { Fam fam; int part, bm, bn, per_cu; bool geglu; const char* name; };
struct VariantTable { Variant row[kVariantIds]; };
constexpr VariantTable make_variant_table() {
  VariantTable t{};
#define SDK_ROW(P, ID, FAM, CF, DBG, PER_CU, GEGLU, NAME) \
  t.row[ID] = Variant{Fam::FAM, P, TileOf<CF>::TBM, TileOf<CF>::TBN, PER_CU, GEGLU, NAME};
  SDK_CONV_VARIANTS(SDK_ROW)
#undef SDK_ROW
  return t;
}
constexpr VariantTable kVariants = make_variant_table();
// the row of an id, nullptr when there is none
inline const Variant* variant_row(int v) {
  return v >= 0 && v < kVariantIds && kVariants.row[v].fam != Fam::NONE ? &kVariants.row[v] : nullptr;
}
constexpr int variant_of(Fam f) {   // the id of a one-kernel family
  for (int v = 0; v < kVariantIds; ++v)
    if (kVariants.row[v].fam == f) return v;
  return -1;
}
constexpr int kIgemm = variant_of(Fam::IGEMM), kDirect = variant_of(Fam::DIRECT), kSkinny = variant_of(Fam::SKINNY);
// the phase form's row map and the in-launch split live in conv_glds_kernel (and the split-K reduces)
inline bool lds_dma_tile(const Variant& r) { return r.fam == Fam::GLDS; }
// the fp16 epilogues that emit GroupNorm statistics without a split: conv_glds_kernel's and the phased 32x32x16 one
inline bool emits_gn_stats(const Variant& r) { return r.fam == Fam::GLDS || r.fam == Fam::PH32; }
using PartLaunch = int (*)(int, const void*, int, void*);
constexpr PartLaunch kPartLaunch[] = {nullptr, sdk_conv_launch_part1, sdk_conv_launch_part2, sdk_conv_launch_part3,
                                      sdk_conv_launch_part4, sdk_conv_launch_part5};

#ifdef SDK_CONV_DIAGNOSTICS
unsigned long long* g_conv_stamps = nullptr;   // 8 stamps x 65536 workgroups (SDK_CONV_STAMPS=1)
constexpr int kStampWgs = 65536;
#endif
// benchmark override of the tile configuration, read once when the library loads
const int g_env_variant = [] {
  const char* fe = getenv("SDK_CONV_VARIANT");
  return fe ? atoi(fe) : -1;
}();

// M-panels per tile group of an unsplit plan (item_coords): the caller's value, else M-panel major
// (SDK_CONV_GM overrides the default, for measurements)
int tile_group_m(const sdk_conv_args* a, const Params& p) {
  static const int env_gm = getenv("SDK_CONV_GM") ? atoi(getenv("SDK_CONV_GM")) : 0;
  const int g = a->tile_group_m > 0 ? a->tile_group_m : env_gm > 0 ? env_gm : 1;
  return std::max(1, std::min(g, p.tiles_m));
}

// the plan of the direct and skinny kernels: one launch of `grid` workgroups, no split, no workspace, no
// GroupNorm statistics
void plan_untiled(Params& p, sdk_conv_plan_info* info, int variant, int tiles_n, int grid, int kt, double kreal) {
  p.variant = variant; p.split = 1; p.tiles_m = 1; p.tiles_n = tiles_n; p.Npad = p.N; p.kt_per_split = kt;
  if (info) {
    info->split_k = 1; info->grid_tiles = grid; info->workspace_bytes = 0; info->variant = variant;
    info->flops = 2.0 * p.M * (double)p.N * kreal; info->gn_chunks = 0;
  }
}

int build_params(const sdk_conv_args* a, Params& p, sdk_conv_plan_info* info) {
  if (!a) return fail(SDK_EINVAL, "conv2d: null args");
  if (a->nseg < 1 || a->nseg > 2) return fail(SDK_EINVAL, "conv2d: nseg must be 1 or 2");
  if (a->batch <= 0 || a->ho <= 0 || a->wo <= 0 || a->cout <= 0)
    return fail(SDK_EINVAL, "conv2d: empty output shape");
  if (!a->weight || !a->out) return fail(SDK_EINVAL, "conv2d: null weight/out");
  p = Params{};
  if (a->act != SDK_ACT_NONE && a->act != SDK_ACT_QUICK_GELU) return fail(SDK_EINVAL, "conv2d: unknown act");
  if (a->act != SDK_ACT_NONE && a->out_mode == SDK_OUT_GEGLU_F16)
    return fail(SDK_EINVAL, "conv2d: act does not combine with the GEGLU epilogue");
  p.act = a->act;
  p.batch = a->batch; p.ho = a->ho; p.wo = a->wo; p.hw_out = a->ho * a->wo;
  p.M = a->batch * p.hw_out;
  p.N = a->cout;
  p.nseg = a->nseg;
  // phase form of nearest-x2 + 3x3 (Params::phase): the kernels see the low-res grid, four times
  const bool phase = a->upsample_phase != 0;
  if (phase) {
    if (a->nseg != 1 || a->out_mode != SDK_OUT_NHWC_F16 || a->residual || a->row_bias || a->act != SDK_ACT_NONE ||
        a->split_inlaunch || (a->ho & 1) || (a->wo & 1))
      return fail(SDK_EINVAL, "conv2d: the phase form is one segment, fp16 NHWC, even output extents, no residual / "
                              "row_bias / act / in-launch split");
    if (a->weight_batch_stride <= 0)
      return fail(SDK_EINVAL, "conv2d: the phase form needs the four phase matrices (weight_batch_stride)");
    if ((double)a->batch * p.hw_out >= 2147483647.0 / 8) return fail(SDK_EINVAL, "conv2d: phase form: too many rows");
    p.phase = 1;
    p.ho = a->ho / 2; p.wo = a->wo / 2; p.hw_out = p.ho * p.wo;
    p.ph_rows = p.ph_rows_pad = a->batch * p.hw_out;
    p.M = 4 * p.ph_rows;   // the planner pads it per phase once the M-tile is known
  }
  double kreal = 0;
  int kt = 0, koff = 0;
  for (int s = 0; s < a->nseg; ++s) {
    const sdk_conv_src& g = a->seg[s];
    Seg& d = p.seg[s];
    if (!g.src0) return fail(SDK_EINVAL, "conv2d: null src0");
    if (g.cin <= 0 || g.cin % 8 || g.c_split % 8 || g.c_split <= 0 || g.c_split > g.cin)
      return fail(SDK_EINVAL, "conv2d: cin/c_split must be positive multiples of 8 (c_split <= cin)");
    if (g.c_split < g.cin && !g.src1) return fail(SDK_EINVAL, "conv2d: concat without src1");
    if (g.ld0 % 8 || (g.c_split < g.cin && g.ld1 % 8)) return fail(SDK_EINVAL, "conv2d: ld must be a multiple of 8");
    if (g.ksize != 1 && g.ksize != 3 && !(phase && g.ksize == 2))
      return fail(SDK_EINVAL, "conv2d: ksize must be 1 or 3 (2: the phase form)");
    if ((g.gn_scale == nullptr) != (g.gn_shift == nullptr)) return fail(SDK_EINVAL, "conv2d: gn scale/shift pair");
    const int lh = g.upsample ? 2 * g.h : g.h, lw = g.upsample ? 2 * g.w : g.w;
    if (g.pad_end < 0 || g.pad_end > 2 || (g.pad_end && g.upsample))
      return fail(SDK_EINVAL, "conv2d: pad_end must be 0..2 (no upsample)");
    // zero padding is implicit (taps outside the source read zeros), so pad_end only widens the grid
    int eh = (lh + 2 * g.pad + g.pad_end - g.ksize) / g.stride + 1;
    int ew = (lw + 2 * g.pad + g.pad_end - g.ksize) / g.stride + 1;
    if (phase) {   // the source is the low-res image with its 1-pixel zero border; the output is the x2 image
      if (g.ksize != 2 || g.stride != 1 || g.pad || g.pad_end || g.upsample || g.h < 3 || g.w < 3 || g.cin % BK ||
          g.c_split != g.cin || g.gn_scale || g.silu)
        return fail(SDK_EINVAL, "conv2d: the phase form reads one zero-bordered source with 2x2 taps, stride 1, "
                                "pad 0, cin % 64 == 0, no transform");
      eh = 2 * (g.h - 2);
      ew = 2 * (g.w - 2);
    }
    if (eh != a->ho || ew != a->wo) return fail(SDK_EINVAL, "conv2d: output size does not match source geometry");
    d.src0 = (const half_t*)g.src0; d.src1 = (const half_t*)g.src1;
    d.gscale = g.gn_scale; d.gshift = g.gn_shift;
    d.c_split = g.c_split; d.cin = g.cin; d.cin_pad = (g.cin + BK - 1) / BK * BK;
    d.ld0 = g.ld0; d.ld1 = g.ld1; d.h = g.h; d.w = g.w; d.ksize = g.ksize; d.stride = g.stride; d.pad = g.pad;
    d.upsample = g.upsample; d.silu = g.silu;
    d.k_off = koff; d.tiles_per_tap = d.cin_pad / BK; d.kt_begin = kt;
    const int taps = g.ksize * g.ksize;
    kt += taps * d.tiles_per_tap;
    koff += taps * d.cin_pad;
    kreal += (double)taps * g.cin;
  }
  if (koff != a->k_total) return fail(SDK_EINVAL, "conv2d: k_total does not match the packed segment layout");
  {
    const sdk_conv_src& g = a->seg[0];
    p.nomask = g.pad == 0 && g.pad_end == 0 && !g.upsample && g.cin % BK == 0 &&
               (g.c_split == g.cin || g.c_split % BK == 0) && g.gn_scale == nullptr && !g.silu;
    // the linear K loop of the LDS-DMA kernels (conv_glds_kernel SIMPLE): one segment, one source, no masks
    const sdk_conv_src& g1 = a->seg[1];
    const bool one_src = !g.src1 || g.c_split >= g.cin;
    // a second segment qualifies when it is a plain 1x1 over the output grid (the fused ResBlock shortcut)
    const bool lin1 = a->nseg == 2 && g1.ksize == 1 && g1.stride == 1 && g1.pad == 0 && g1.pad_end == 0 &&
                      !g1.upsample && g1.cin % BK == 0 && (!g1.src1 || g1.c_split >= g1.cin || g1.c_split % BK == 0) &&
                      g1.gn_scale == nullptr && !g1.silu && g1.h == a->ho && g1.w == a->wo;
    p.simple = !(p.nomask && one_src) ? 0 : a->nseg == 1 ? 1 : lin1 ? 2 : 0;
  }
  if (a->out_mode == SDK_OUT_NHWC_F16 || a->out_mode == SDK_OUT_GEGLU_F16) {
    if (a->cout % 8 || a->out_ld % 8 || (a->residual && a->res_ld % 8))
      return fail(SDK_EINVAL, "conv2d: fp16 NHWC output needs cout/out_ld/res_ld multiples of 8");
  }
  if (a->out_mode == SDK_OUT_GEGLU_F16 && (a->cout % 64)) return fail(SDK_EINVAL, "conv2d: GEGLU cout % 64");
  p.kt_total = kt;
  p.W = (const half_t*)a->weight; p.ldw = a->k_total; p.wrows = (a->cout + 127) / 128 * 128;
  p.wbs = a->weight_batch_stride;
  if (p.wbs < 0 || (p.wbs && p.wbs < (long long)p.wrows * p.ldw))
    return fail(SDK_EINVAL, "conv2d: weight_batch_stride smaller than one packed weight matrix");
  p.bias = a->bias; p.row_bias = a->row_bias; p.rb_ld = a->row_bias_ld;
  p.res = (const half_t*)a->residual; p.res_ld = a->res_ld;
  p.out = a->out; p.out_ld = a->out_ld; p.out_mode = a->out_mode;
  bool transform = false;
  for (int s = 0; s < a->nseg; ++s) {
    const sdk_conv_src& g = a->seg[s];
    transform |= (g.gn_scale != nullptr) || g.silu;
    // the LDS-DMA kernels: buffer resources (31-bit byte offsets), a K-step's 64 channels
    // from one concat source, and a second segment that is a plain 1x1 over the output grid
    if ((double)a->batch * g.h * g.w * std::max(g.ld0, g.ld1) * 2 >= 2147483647.0) transform = true;
    if (g.c_split < g.cin && g.c_split % BK) transform = true;
    if (s == 1 && (g.ksize != 1 || g.stride != 1 || g.pad != 0 || g.pad_end || g.upsample || g.h != a->ho || g.w != a->wo))
      transform = true;
  }
  if ((double)((a->cout + 127) / 128 * 128) * a->k_total * 2 >= 2147483647.0) transform = true;
  if (a->act != SDK_ACT_NONE) transform = true;   // the CLIP fc1 (once per prompt, not per step)
  // tile configuration: LDS-DMA kernels for transform-free operands, scored by
  // padded-work efficiency x whole-chip wave quantisation x measured per-config
  // throughput
  struct Opt { int variant; double pref; };
  // relative throughput of each config on shapes it tiles exactly (tools/bench_conv.py, MI355X)
  const Opt opts[] = {{8, 1.05}, {2, 1.00}, {22, 0.92}, {7, 0.88}, {6, 0.72}, {4, 0.72}, {3, 0.65}};
  int var = kIgemm, best_split = 0;
  auto pick_split = [&](int tiles, int slots, double& fill) {
    int best = 1;
    double bf = -1;
    for (int sp = 1; sp <= 16; sp *= 2) {
      if (sp > 1 && kt / sp < 8) break;
      const int blocks = tiles * sp;
      const double waves = (double)((blocks + slots - 1) / slots);
      double f = (double)blocks / (waves * slots);
      for (int q = 1; q < sp; q *= 2) f *= 0.95;      // slab write + reduce traffic
      if (f > bf + 1e-9) { bf = f; best = sp; }
    }
    fill = bf;
    return best;
  };
  if (p.wbs && transform) return fail(SDK_EINVAL, "conv2d: per-image weights need a transform-free operand");
  if (phase && p.simple != 1) return fail(SDK_EINVAL, "conv2d: the phase form runs on the linear A issue only");
  if (!transform) {
    double best = -1;
    for (const Opt& o : opts) {
      const Variant& r = kVariants.row[o.variant];
      if (a->out_mode == SDK_OUT_GEGLU_F16 && !r.geglu) continue;
      if (phase ? !lds_dma_tile(r) : (p.wbs && p.hw_out % r.bm)) continue;   // per-image weights: M-tiles inside one image
      const int tmm = phase ? 4 * ((p.ph_rows + r.bm - 1) / r.bm) : (p.M + r.bm - 1) / r.bm;
      const int tnn = (p.N + r.bn - 1) / r.bn;
      const double eff = (double)p.M * p.N / ((double)tmm * r.bm * tnn * r.bn);
      double fill;
      const bool can_split = a->out_mode != SDK_OUT_GEGLU_F16 && a->cout % 8 == 0;
      const int slots = 256 * r.per_cu;
      const int sp = can_split ? pick_split(tmm * tnn, slots, fill) : 1;
      if (!can_split) {
        const int blocks = tmm * tnn;
        fill = (double)blocks / ((double)((blocks + slots - 1) / slots) * slots);
      }
      const double score = eff * fill * o.pref;
      if (score > best) { best = score; var = o.variant; best_split = sp; }
    }
  }
  // forced configuration: the caller's autotuner (variant_hint = 1 + id) or, for
  // benchmarks, SDK_CONV_VARIANT=id (read once, at library load)
  int forced = a->variant_hint > 0 ? a->variant_hint - 1 : g_env_variant;
  // variant 34: direct convolution for <= 8 output channels (conv_out of the UNet / VAE decoder)
  {
    const sdk_conv_src& g = a->seg[0];
    const bool direct_ok = a->nseg == 1 && a->cout <= DC_MAXN && (g.ksize == 3 || (g.ksize == 1 && g.pad == 0)) &&
                           g.stride == 1 && !g.upsample && g.pad_end == 0 && g.pad <= 1 && g.c_split == g.cin &&
                           g.gn_scale == nullptr && !g.silu && !a->residual && !a->row_bias &&
                           a->act == SDK_ACT_NONE && a->out_mode != SDK_OUT_GEGLU_F16 && !p.wbs;
    if (forced == kDirect && !direct_ok) return fail(SDK_EINVAL, "conv2d: variant 34 (direct) does not fit this conv");
    if (direct_ok && (forced < 0 || forced == kDirect)) {
      plan_untiled(p, info, kDirect, 1, ((a->wo + DC_TX - 1) / DC_TX) * ((a->ho + 7) / 8) * a->batch, kt, kreal);
      if (a->gn_partial) return fail(SDK_EINVAL, "conv2d: the direct variant emits no GroupNorm statistics");
      return SDK_OK;
    }
  }
  // variant 35: skinny GEMM for <= 64 rows (token GEMMs at M = batch: the time-embedding MLP)
  {
    const sdk_conv_src& g = a->seg[0];
    const bool skinny_ok = a->nseg == 1 && p.M <= SK_MAXM && g.ksize == 1 && g.stride == 1 && g.pad == 0 &&
                           g.pad_end == 0 && !g.upsample && g.c_split == g.cin && g.gn_scale == nullptr &&
                           (a->out_mode == SDK_OUT_NHWC_F16 || a->out_mode == SDK_OUT_ROWS_F32) && !a->gn_partial &&
                           !p.wbs;
    if (forced == kSkinny && !skinny_ok) return fail(SDK_EINVAL, "conv2d: variant 35 (skinny) does not fit this GEMM");
    if (skinny_ok && (forced < 0 || forced == kSkinny)) {
      plan_untiled(p, info, kSkinny, (p.N + 15) / 16, (p.N + 15) / 16, kt, kreal);
      return SDK_OK;
    }
  }
  // What a forced id means is its row of the variant table.  The diagnostic ablations compute wrong outputs by
  // design: the product library rejects them, only the separate diagnostics build (-DSDK_CONV_DIAGNOSTICS,
  // libsdk_amd_diag.so) runs them.
  const Variant* fr = variant_row(forced);
  if (fr && fr->fam == Fam::DIAG && !kDiagnostics)
    return fail(SDK_EINVAL, "conv2d: variant " + std::to_string(forced) +
                                " is a diagnostic ablation (only in libsdk_amd_diag.so)");
  if (forced >= 0 && !fr) return fail(SDK_EINVAL, "conv2d: unknown variant " + std::to_string(forced));
  // a forced 5 (a leftover SDK_CONV_VARIANT=5 or an old tuning entry) runs as 22, the same 256x320 tile on 16x16x32
  // (which is not spill-free either: 8 to 16 B/lane of scratch in build*/resource_usage.txt), with a one-time warning
  if (fr && fr->fam == Fam::RETIRED) {
    static std::atomic<bool> warned{false};
    if (!warned.exchange(true))
      fprintf(stderr, "sd_amd conv2d: variant 5 is retired; running the same 256x320 tile as variant 22\n");
    forced = kRetiredRunsAs;
    fr = &kVariants.row[forced];
  }
  // honoured when the kernel can run this conv: the register-staged kernel takes every operand but per-image
  // weights, the others need a transform-free one, a GEGLU-pairing epilogue for the GEGLU output, the LDS-DMA
  // tile family for the phase form, and per-image weights need M-tiles inside one image
  if (fr && (fr->fam == Fam::IGEMM || !transform) && (fr->geglu || a->out_mode != SDK_OUT_GEGLU_F16) &&
      (phase ? lds_dma_tile(*fr) : (!p.wbs || (fr->fam != Fam::IGEMM && p.hw_out % fr->bm == 0)))) {
    var = forced;
    best_split = 0;
  }
  const Variant& row = kVariants.row[var];
  const int tbm = row.bm, tbn = row.bn;
  if (phase) {
    if (!lds_dma_tile(row)) return fail(SDK_EINVAL, "conv2d: the phase form found no LDS-DMA tile plan");
    p.ph_rows_pad = (p.ph_rows + tbm - 1) / tbm * tbm;   // no M-tile straddles two phases
    p.M = 4 * p.ph_rows_pad;
  } else if (p.wbs && (row.fam == Fam::IGEMM || p.hw_out % tbm)) {
    return fail(SDK_EINVAL, "conv2d: per-image weights: no LDS-DMA tile fits inside one image");
  }
  p.variant = var;
  p.tiles_m = (p.M + tbm - 1) / tbm;
  p.tiles_n = (p.N + tbn - 1) / tbn;
  p.Npad = p.tiles_n * tbn;                       // split-K slab row stride
  const int tiles = p.tiles_m * p.tiles_n;
  int split = a->split_k;
  if (split <= 0) {
    if (best_split > 0) {
      split = best_split;
    } else {
      split = 1;
      while (tiles * split < 256 * row.per_cu && kt / (split * 2) >= 8 && split < 16) split *= 2;
    }
  }
  if (a->out_mode == SDK_OUT_GEGLU_F16 || a->cout % 8) split = 1;
  if (split > kt) split = kt;
  p.kt_per_split = (kt + split - 1) / split;
  split = (kt + p.kt_per_split - 1) / p.kt_per_split;
  p.split = split;
  p.gm = split == 1 ? tile_group_m(a, p) : 1;
#ifdef SDK_CONV_DIAGNOSTICS
  if (getenv("SDK_CONV_STAMPS")) {
    if (!g_conv_stamps && (hipMalloc((void**)&g_conv_stamps, (size_t)kStampWgs * 8 * 8) != hipSuccess ||
                           hipMemset(g_conv_stamps, 0, (size_t)kStampWgs * 8 * 8) != hipSuccess)) g_conv_stamps = nullptr;
    if ((long long)p.tiles_m * p.tiles_n * p.split <= kStampWgs) p.stamps = g_conv_stamps;
    p.stamps_rt = atoi(getenv("SDK_CONV_STAMPS")) == 2;
  }
#endif
  int64_t ws = split > 1 ? (int64_t)split * p.M * p.Npad * 4 : 0;
  if (a->split_inlaunch) {
    if (!lds_dma_tile(row))
      return fail(SDK_EINVAL, "conv2d: in-launch split-K needs an LDS-DMA tile plan (a conv_glds_kernel variant)");
    if (split != 2) return fail(SDK_EINVAL, "conv2d: in-launch split-K combines exactly two K halves (split_k = 2)");
    if (!a->tile_counters) return fail(SDK_EINVAL, "conv2d: in-launch split-K needs tile_counters");
    if (tiles > SDK_TILE_COUNTERS) return fail(SDK_EINVAL, "conv2d: in-launch split-K: more tiles than counters");
    p.inl = 1;
    p.tcnt = a->tile_counters;
    ws = (int64_t)2 * tiles * tbm * tbn * 4;   // one fp32 accumulator blob per (tile, half)
  }
  if (info) {
    info->split_k = split;
    info->grid_tiles = tiles;
    info->workspace_bytes = ws;
    info->variant = var;
    // the executed FLOPs: the phase form's K is 4 * cin over the same output pixels (padding rows not counted)
    info->flops = 2.0 * (phase ? 4.0 * p.ph_rows : (double)p.M) * (double)p.N * kreal;
  }
  if (split > 1) {
    if (a->cout % 8) return fail(SDK_EINVAL, "conv2d: split-K needs cout % 8 == 0 (pass split_k = 1)");
    p.partial = a->workspace;
  }
  // GroupNorm statistics of the output: chunks per image the plan can emit (0 = none).  Split-K: the
  // reduce kernel, 64-row chunks (one chunk when hw_out is not a multiple of 64); otherwise the
  // LDS-DMA kernels' fp16 epilogue, one chunk per M-tile when tiles do not straddle images.
  int gn_nch = 0;
  if (a->out_mode == SDK_OUT_NHWC_F16) {
    const int hw_img = (phase ? 4 : 1) * p.hw_out;   // output pixels of one image
    if (split > 1 && !p.inl) gn_nch = hw_img % 64 == 0 ? hw_img / 64 : 1;
    else if (emits_gn_stats(row) && p.hw_out % tbm == 0) gn_nch = hw_img / tbm;   // in-launch: the combining tile emits
  }
  if (info) info->gn_chunks = gn_nch;
  if (a->gn_partial) {
    if (gn_nch == 0)
      return fail(SDK_EINVAL, "conv2d: this plan emits no GroupNorm statistics (sdk_conv_plan_info.gn_chunks == 0)");
    p.gnp = reinterpret_cast<float2*>(a->gn_partial);
    p.gn_nch = gn_nch;
  }
  return SDK_OK;
}

}  // namespace
}  // namespace sdk

using namespace sdk;

extern "C" const char* sdk_kernel_name(int32_t variant) {
  const Variant* r = variant_row(variant);
  return r ? r->name : "unknown";
}

extern "C" int sdk_conv2d_plan(const sdk_conv_args* a, sdk_conv_plan_info* info) {
  Params p;
  return build_params(a, p, info);
}

extern "C" int sdk_conv2d(const sdk_conv_args* a, sdk_stream_t stream) {
  Params p;
  sdk_conv_plan_info info;
  int rc = build_params(a, p, &info);
  if (rc) return rc;
  if (p.split > 1 && (!a->workspace || a->workspace_bytes < info.workspace_bytes))
    return fail(SDK_EWORKSPACE, "conv2d: split-K workspace too small");
  hipStream_t s = (hipStream_t)stream;
  dim3 grid(p.tiles_m * p.tiles_n, p.split);
  const Variant& row = kVariants.row[p.variant];   // build_params plans ids of the table only
  switch (row.fam) {
    case Fam::IGEMM:
      hipLaunchKernelGGL(conv_igemm_kernel, grid, dim3(NT), 0, s, p);
      rc = check_launch("conv_igemm");
      break;
    case Fam::DIRECT: rc = launch_direct(p, s); break;
    case Fam::SKINNY: rc = launch_skinny(p, s); break;
    default:   // the tile kernels, each in its compile part (part 0 rows have no launcher: never planned)
      rc = row.part ? kPartLaunch[row.part](p.variant, &p, (int)sizeof(Params), s)
                    : fail(SDK_EINVAL, "conv2d: planned variant " + std::to_string(p.variant) + " has no kernel");
  }
  if (rc) return rc;
  if (p.inl) return SDK_OK;   // combined inside the launch
  if (p.split > 1 && p.gnp) {
    hipLaunchKernelGGL(splitk_reduce_gn_kernel, dim3(p.batch * p.gn_nch, (p.N + 63) / 64), dim3(256), 0, s, p);
    if (int e = check_launch("splitk_reduce_gn")) return e;
  } else if (p.split > 1) {
    const size_t total = (size_t)p.M * (p.N / 8);
    int blocks = (int)std::min<size_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3(blocks), dim3(256), 0, s, p);
    if (int e = check_launch("splitk_reduce")) return e;
  }
  return SDK_OK;
}

#ifdef SDK_CONV_DIAGNOSTICS
// diagnostics build only (not in include/sdk_amd.h): copy the phase stamps of the last stamped launches
extern "C" int sdk_diag_conv_stamps(unsigned long long* host, long long n) {
  if (!g_conv_stamps || n <= 0 || n > (long long)kStampWgs * 8) return SDK_EINVAL;
  return hipMemcpy(host, g_conv_stamps, (size_t)n * 8, hipMemcpyDeviceToHost) == hipSuccess ? SDK_OK : SDK_EINVAL;
}
#endif
#endif  // SDK_PART(0)
