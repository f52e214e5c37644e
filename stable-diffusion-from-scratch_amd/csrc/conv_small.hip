// The small conv kernels: the register-staged conv_igemm_kernel (every A transform), the two split-K reduces,
// the direct kernel (<= 8 output channels) and the skinny GEMM (<= 64 rows), behind the typed launchers of conv.h.
#include "conv_device.h"

namespace sdk {
namespace {

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

// ---------------------------------------------------------------------- epilogue of conv_igemm_kernel
// acc[i][j] (32x32 MFMA tile) element r of lane (fr = lane&31, fh = lane>>5):
//   row = m_w + i*32 + (r&3) + 8*(r>>2) + 4*fh, col = n_w + j*32 + fr   (block-local)
// LDS `smem` must be free (all waves past their last LDS read) on entry.
template <int FM, int FN, int TBM, int TBN, int TNT, bool ERF>
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
          smem[rl * CLD + n_w + j * 32 + fr] = (half_t)act_fn<ERF>(p.act, v);
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
        v = act_fn<ERF>(p.act, v);
        if (p.res) v += (float)p.res[(size_t)m * p.res_ld + n];
        float* out = reinterpret_cast<float*>(p.out);
        if (mode == SDK_OUT_NCHW_F32)
          out[((size_t)b * p.N + n) * p.hw_out + (m - b * p.hw_out)] = v;
        else
          out[(size_t)m * p.out_ld + n] = v;
      }
    }
}

// ERF (here and on the split-K reduces and the skinny kernel): the instantiation that runs SDK_ACT_GELU.  The
// launchers send every other act to the ERF = false one, whose code is what it was before the erf branch existed:
// the diffusion step runs these kernels with act none (profiles/act_gelu_resources.txt)
template <bool ERF>
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
  epilogue<2, 2, BM, BN, NT, ERF>(p, acc, smem, m0, n0, m_w, n_w, blockIdx.y);
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

template <bool ERF>
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
    for (int j = 0; j < 8; ++j) v[j] = act_fn<ERF>(p.act, (v[j] + bi[j]) + rbv[j]);
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
template <bool ERF>
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
      for (int j = 0; j < 8; ++j) o[j] = (half_t)act_fn<ERF>(p.act, (v[q][j] + bi[j]) + rbv[j]);
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

// Skinny GEMM for M <= 64 rows (variant 35): the time-embedding MLP and the ResBlock embedding
// projections run at M = batch (16 at the bench), where a 128-row tile wastes 7/8 of its MFMA work
// and the 1280 x 20160 weight is streamed by a few dozen workgroups (~30 us per launch).  Here a
// workgroup owns 16 output columns and its 4 waves split K; each lane streams 16-B pieces of its
// column's packed weight row straight from HBM (every weight byte is read once, SK_PF K-steps in
// flight), the A fragments (x rows, SiLU applied on load) come from L2, v_mfma_f32_16x16x32_f16
// accumulates M/16 row blocks per weight fragment, and the 4 wave partials are summed through LDS.
// 16x16x32 operand layout: lane l supplies A[row l%16][k 8(l/16)..+8] and B[k 8(l/16)..+8][col l%16];
// D element i of lane l is D[4(l/16) + i][l%16].

template <int MB, bool ERF>   // 16-row blocks
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
    v = act_fn<ERF>(p.act, v);
    if (p.res) v += (float)p.res[(size_t)row * p.res_ld + n];
    if (p.out_mode == SDK_OUT_ROWS_F32)
      reinterpret_cast<float*>(p.out)[(size_t)row * p.out_ld + n] = v;
    else
      reinterpret_cast<half_t*>(p.out)[(size_t)row * p.out_ld + n] = (half_t)v;
  }
}

}  // namespace

namespace conv {

int launch_igemm(const Params& p, hipStream_t s) {
  const dim3 grid(p.tiles_m * p.tiles_n, p.split);
  if (p.act == SDK_ACT_GELU) hipLaunchKernelGGL(conv_igemm_kernel<true>, grid, dim3(NT), 0, s, p);
  else hipLaunchKernelGGL(conv_igemm_kernel<false>, grid, dim3(NT), 0, s, p);
  return check_launch("conv_igemm");
}

int launch_splitk_reduce(const Params& p, hipStream_t s) {
  const size_t total = (size_t)p.M * (p.N / 8);
  int blocks = (int)std::min<size_t>((total + 255) / 256, 4096);
  if (p.act == SDK_ACT_GELU)
    hipLaunchKernelGGL(splitk_reduce_kernel<true>, dim3(blocks), dim3(256), 0, s, p);
  else
    hipLaunchKernelGGL(splitk_reduce_kernel<false>, dim3(blocks), dim3(256), 0, s, p);
  return check_launch("splitk_reduce");
}

int launch_splitk_reduce_gn(const Params& p, hipStream_t s) {
  const dim3 grid(p.batch * p.gn_nch, (p.N + 63) / 64);
  if (p.act == SDK_ACT_GELU) hipLaunchKernelGGL(splitk_reduce_gn_kernel<true>, grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL(splitk_reduce_gn_kernel<false>, grid, dim3(256), 0, s, p);
  return check_launch("splitk_reduce_gn");
}

int launch_direct(const Params& p, hipStream_t s) {
  return p.N <= 4 ? launch_direct_n<4>(p, s) : launch_direct_n<8>(p, s);
}

template <bool ERF>
static void launch_skinny_rows(const Params& p, hipStream_t s) {
  const dim3 grid((p.N + 15) / 16);
  if (p.M <= 16) hipLaunchKernelGGL((conv_skinny_kernel<1, ERF>), grid, dim3(256), 0, s, p);
  else if (p.M <= 32) hipLaunchKernelGGL((conv_skinny_kernel<2, ERF>), grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL((conv_skinny_kernel<4, ERF>), grid, dim3(256), 0, s, p);
}

int launch_skinny(const Params& p, hipStream_t s) {
  if (p.act == SDK_ACT_GELU) launch_skinny_rows<true>(p, s);
  else launch_skinny_rows<false>(p, s);
  return check_launch("conv_skinny");
}

}  // namespace conv
}  // namespace sdk
