// The conv tile kernels: the LDS-DMA conv_glds_kernel and the phased conv_ph_kernel, their epilogues and their
// launchers.  conv_tile.hip includes this once per compile part and instantiates that part's kernels only.
#pragma once
#include "conv_cfg.h"
#include "conv_device.h"

namespace sdk {
namespace {

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
#define SDK_ABL_DMA_SKIP(IS_A) ((((SDK_ABL_DMA) & 1) && (IS_A)) || (((SDK_ABL_DMA) & 2) && !(IS_A)))
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

}  // namespace
}  // namespace sdk
