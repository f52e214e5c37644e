// The conv host planner and the ABI entry points: the variant table, build_params (sdk_conv_args -> Params: the
// kernel variant, tiling and split of a conv), sdk_conv2d_plan, sdk_conv2d and sdk_kernel_name.  Host code only:
// no kernel is defined or instantiated here, every launch goes through the typed launchers of conv.h.
#include "conv_cfg.h"

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
using PartLaunch = int (*)(int, const Params&, hipStream_t);
constexpr PartLaunch kPartLaunch[] = {nullptr, launch_part1, launch_part2, launch_part3, launch_part4, launch_part5};

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
  if (a->act != SDK_ACT_NONE && a->act != SDK_ACT_QUICK_GELU && a->act != SDK_ACT_GELU)
    return fail(SDK_EINVAL, "conv2d: unknown act");
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
  // the row-panel kernel (conv_rowpanel.hip): a 1x1 over one source with K = cin <= 320 in whole 32-wide K-steps,
  // fp16 NHWC rows, bias and residual only (no embedding row), one W for every image, no split of K
  bool rowpanel_ok = false;
  {
    const sdk_conv_src& g = a->seg[0];
    rowpanel_ok = !transform && !phase && a->nseg == 1 && g.ksize == 1 && g.stride == 1 && g.pad == 0 &&
                  g.pad_end == 0 && !g.upsample && (!g.src1 || g.c_split >= g.cin) && g.cin % 32 == 0 &&
                  g.cin <= CfgRowPanel::MAXK && a->cout <= CfgRowPanel::MAXN && a->out_mode == SDK_OUT_NHWC_F16 &&
                  !a->row_bias && !p.wbs && a->split_k <= 1 && !a->split_inlaunch;
  }
  // honoured when the kernel can run this conv: the register-staged kernel takes every operand but per-image
  // weights, the others need a transform-free one, a GEGLU-pairing epilogue for the GEGLU output, the LDS-DMA
  // tile family for the phase form, and per-image weights need M-tiles inside one image
  if (fr && (fr->fam != Fam::ROWPANEL || rowpanel_ok) &&
      (fr->fam == Fam::IGEMM || !transform) && (fr->geglu || a->out_mode != SDK_OUT_GEGLU_F16) &&
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
  if (a->out_mode == SDK_OUT_GEGLU_F16 || a->cout % 8 || row.fam == Fam::ROWPANEL) split = 1;
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
  const Variant& row = kVariants.row[p.variant];   // build_params plans ids of the table only
  switch (row.fam) {
    case Fam::IGEMM: rc = launch_igemm(p, s); break;
    case Fam::DIRECT: rc = launch_direct(p, s); break;
    case Fam::SKINNY: rc = launch_skinny(p, s); break;
    case Fam::ROWPANEL: rc = launch_rowpanel(p, s); break;
    default:   // the tile kernels, each in its compile part (part 0 rows have no launcher: never planned)
      rc = row.part ? kPartLaunch[row.part](p.variant, p, s)
                    : fail(SDK_EINVAL, "conv2d: planned variant " + std::to_string(p.variant) + " has no kernel");
  }
  if (rc) return rc;
  if (p.inl) return SDK_OK;   // combined inside the launch
  if (p.split > 1) return p.gnp ? launch_splitk_reduce_gn(p, s) : launch_splitk_reduce(p, s);
  return SDK_OK;
}

#ifdef SDK_CONV_DIAGNOSTICS
// diagnostics build only (not in include/sdk_amd.h): copy the phase stamps of the last stamped launches
extern "C" int sdk_diag_conv_stamps(unsigned long long* host, long long n) {
  if (!g_conv_stamps || n <= 0 || n > (long long)kStampWgs * 8) return SDK_EINVAL;
  return hipMemcpy(host, g_conv_stamps, (size_t)n * 8, hipMemcpyDeviceToHost) == hipSuccess ? SDK_OK : SDK_EINVAL;
}
#endif
