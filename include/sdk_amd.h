/*
 * sdk_amd.h — C ABI of the MI355X (gfx950) latent-diffusion hot path.
 *
 * The reference (ProgramerSalar/stable-diffusion-from-scratch) has no FFI: its
 * hot path is a chain of stock torch.nn ops plus two un-vendored flash_attn
 * entry points.  Each entry point below replaces a family of those call sites
 * (cited per function, file:line into the reference).  The library is driven
 * by the Python mirror of the reference's modules (UNetModel, AutoEncoderKL,
 * DDIMSampler) in stable-diffusion-from-scratch_amd/ through ctypes.
 *
 * Conventions (all entry points):
 *   - activations are NHWC (token-major) IEEE fp16; statistics and the sampler
 *     state are fp32; every pointer is device memory owned by the caller;
 *   - the library allocates nothing per call; work launches on `stream`
 *     (a hipStream_t, NULL = legacy default) and never synchronises, so a
 *     caller may capture the calls into a hipGraph;
 *   - return 0 on success or a negative sdk_status; sdk_last_error() returns a
 *     thread-local message for the last failure.
 */
#ifndef SDK_AMD_H
#define SDK_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* sdk_stream_t;

enum sdk_status {
  SDK_OK = 0,
  SDK_EINVAL = -1,      /* bad shape / pointer / alignment */
  SDK_EHIP = -2,        /* HIP launch error */
  SDK_EWORKSPACE = -3   /* workspace too small */
};

/* ---------------------------------------------------------------- convolution / GEMM
 * Implicit-GEMM convolution on MFMA (v_mfma_f32_32x32x16_f16, fp32 accumulate).
 * out[m, n] = sum_k A[m, k] * W[n, k]  (+ bias[n] + row_bias[b(m), n]) (+ residual[m, n])
 * where A is the im2col view of up to two K segments.  Each segment reads one
 * or two NHWC sources (a channel concat, zero-copy), optionally through a
 * GroupNorm affine (per (batch, channel) scale/shift) and SiLU, optionally
 * nearest-x2 upsampled, with zero padding applied AFTER the transform.
 * A plain Linear on tokens is the 1x1 case with h = tokens, w = 1.
 *
 * Replaces: nn.Conv2d 3x3/1x1/s2 (openai_model/utils.py:26-39 via model.py:117,181,207,218,365,531,88-90;
 *   Unet/unet.py:84-112; Encoder_Decoder/encoder.py:133,171), nn.Linear
 *   (openai_model/attention.py:40-47,133,164-168; model.py:197-200,352-357), the
 *   GroupNorm32/Normalize + SiLU in front of them (openai_model/utils.py:15-22,
 *   attention.py:10-11, Unet/unet.py:9-28), F.interpolate nearest x2 (model.py:127,
 *   Unet/unet.py:46), torch.cat skip concat (model.py:586), the emb broadcast add
 *   (model.py:241-250), the residual adds (model.py:252, attention.py:251-253,363,
 *   Unet/unet.py:135, Unet/attention.py:264) and GEGLU x*gelu(gate) (attention.py:140-141).
 */
typedef struct {
  const void* src0;        /* NHWC fp16, channels [0, c_split) */
  const void* src1;        /* NHWC fp16, channels [c_split, cin) (NULL if c_split == cin) */
  int32_t c_split;         /* multiple of 8 */
  int32_t cin;             /* multiple of 8 */
  int32_t ld0, ld1;        /* elements between consecutive pixels of src0 / src1 */
  int32_t h, w;            /* source spatial size (before upsampling) */
  int32_t ksize;           /* 1 or 3 (2: sdk_conv_args.upsample_phase only) */
  int32_t stride, pad;
  int32_t upsample;        /* 1: source is read nearest-x2 upsampled (logical 2h x 2w) */
  const float* gn_scale;   /* [batch][cin] or NULL */
  const float* gn_shift;   /* [batch][cin] or NULL */
  int32_t silu;            /* apply x*sigmoid(x) after the affine */
  int32_t pad_end;         /* extra zero rows/cols after the source (bottom/right) on top of pad:
                              the KL-VAE Downsample's F.pad(x, (0,1,0,1)) + conv s2 p0 (Unet/unet.py:64-68) */
} sdk_conv_src;

enum sdk_out_mode {
  SDK_OUT_NHWC_F16 = 0,    /* out[m*out_ld + n] fp16 */
  SDK_OUT_NCHW_F32 = 1,    /* out[(b*cout + n)*ho*wo + pix] fp32 */
  SDK_OUT_GEGLU_F16 = 2,   /* weight rows packed in 32-row (x, gate) pairs; out width cout/2 */
  SDK_OUT_ROWS_F32 = 3     /* out[m*out_ld + n] fp32 */
};

typedef struct {
  int32_t batch, ho, wo, cout;
  int32_t nseg;            /* 1 or 2 (segment 1 = fused 1x1 shortcut) */
  sdk_conv_src seg[2];
  const void* weight;      /* fp16 [cout_pad][k_total]; cout_pad = roundup(cout, 128);
                              per segment: roundup(cin, 64) / 64 channel blocks x taps x 64
                              columns (channel-block major, tap minor) */
  int32_t k_total;
  const float* bias;       /* [cout] or NULL */
  const float* row_bias;   /* [batch][row_bias_ld] or NULL (timestep-embedding broadcast) */
  int32_t row_bias_ld;
  const void* residual;    /* fp16 [M][res_ld] or NULL */
  int32_t res_ld;
  void* out;
  int32_t out_ld;
  int32_t out_mode;        /* enum sdk_out_mode */
  int32_t split_k;         /* 0 = choose; 1 = off */
  float* workspace;        /* split-K fp32 partials */
  int64_t workspace_bytes;
  int32_t variant_hint;    /* 0 = choose; 1 + variant id forces a tile configuration (autotuning) */
  int32_t act;             /* enum sdk_conv_act: applied after bias / row_bias, before the residual */
  float* gn_partial;       /* NULL, or GroupNorm statistics of the fp16 NHWC output (only when the plan's
                              gn_chunks > 0): [batch][gn_chunks][cout] float pairs (mean, M2) over
                              ho*wo/gn_chunks output pixels each — sdk_group_norm merges them instead of
                              a statistics pass over the tensor */
  int64_t weight_batch_stride;  /* 0, or per-image weights: output rows of image b (b = m / (ho*wo)) use
                                   weight + b * weight_batch_stride (elements); only the LDS-DMA tile
                                   kernels, with M-tiles inside one image (the reassociated
                                   cross-attention's per-prompt matrices) */
  int32_t split_inlaunch;  /* 1: split_k must be 2 and the plan an LDS-DMA tile kernel; the two K halves of a
                              tile are combined INSIDE the launch (each writes its fp32 accumulator blob to the
                              workspace; the second to arrive adds the first's and runs the full epilogue,
                              GroupNorm statistics included): no reduce kernel, no slab round trip through it */
  uint32_t* tile_counters; /* with split_inlaunch: >= SDK_TILE_COUNTERS zero-initialised words, one arrival
                              counter per output tile (device memory); every launch leaves them zero */
  int32_t tile_group_m;    /* unsplit LDS-DMA / phased plans: output tiles are visited in groups of this
                              many M-panels, N-tile major inside a group, so the tiles co-resident on one XCD
                              share both their A panels and their W tiles in its L2; 0: the library's choice,
                              1: M-panel major (every N-tile of a panel, then the next panel) */
  int32_t upsample_phase;  /* 1: the phase form of nearest-x2 + conv3x3 pad 1 (F.interpolate + nn.Conv2d of the
                              Upsample modules).  Output pixel (2i+a, 2j+b) sees only a 2x2 window of the low-res
                              image, so the layer is four 2x2 convs, one per parity (a, b), each with K = 4 * cin:
                              seg[0] = the low-res image with a 1-pixel zero border ([batch][h][w], h = ho/2 + 2,
                              w = wo/2 + 2), ksize 2, stride 1, pad 0, cin % 64 == 0; weight = the four phase
                              matrices (phase = 2a + b, weight_batch_stride apart; taps (dy, dx) hold the 3x3
                              weights that land on window pixel (i+a+dy, j+b+dx)); ho / wo / out = the ordinary x2
                              NHWC fp16 output.  One segment, no residual / row_bias / act / in-launch split; only
                              the LDS-DMA tile kernels (a forced variant without the form is not honoured).
                              gn_partial chunks are phase major inside an image */
} sdk_conv_args;

#define SDK_TILE_COUNTERS 16384

enum sdk_conv_act {
  SDK_ACT_NONE = 0,
  SDK_ACT_QUICK_GELU = 1,  /* x * sigmoid(1.702 x): CLIP MLP fc1 (transformers QuickGELUActivation) */
  SDK_ACT_GELU = 2         /* 0.5 x (1 + erf(x / sqrt 2)): nn.GELU(), the OpenCLIP MLP c_fc; applied at the same
                              place: after bias / row_bias, before the residual */
};

typedef struct {
  int32_t split_k;
  int32_t grid_tiles;
  int64_t workspace_bytes;
  int32_t variant;         /* kernel variant id (sdk_kernel_name); split_k > 1 adds splitk_reduce_kernel */
  double flops;            /* algorithmic 2*M*N*K over the unpadded K */
  int32_t gn_chunks;       /* > 0: the plan can emit GroupNorm statistics (sdk_conv_args.gn_partial) */
} sdk_conv_plan_info;

int sdk_conv2d_plan(const sdk_conv_args* a, sdk_conv_plan_info* info);
int sdk_conv2d(const sdk_conv_args* a, sdk_stream_t stream);

/* ---------------------------------------------------------------- GroupNorm statistics
 * Per (batch, group) mean / variance over an NHWC tensor (optionally a 2-source
 * channel concat), folded with gamma/beta into per (batch, channel)
 * scale = gamma*rstd, shift = beta - mean*gamma*rstd consumed by sdk_conv2d.
 * Replaces the statistics half of GroupNorm32 (openai_model/utils.py:15-22, eps 1e-5),
 * Normalize (openai_model/attention.py:10-11; Unet/unet.py:9-19, eps 1e-6) and
 * FlashAttentionBlock.norm (Unet/attention.py:231, eps 1e-5).
 */
typedef struct {
  const void* src0; const void* src1;
  int32_t c_split, ld0, ld1;
  int32_t batch, hw, channels, groups;
  float eps;
  const float* gamma; const float* beta;   /* [channels] */
  float* scale; float* shift;              /* [batch][channels] */
  float* workspace; int64_t workspace_bytes;
} sdk_group_norm_args;

int64_t sdk_group_norm_workspace(int32_t batch, int32_t hw, int32_t channels);
int sdk_group_norm_affine(const sdk_group_norm_args* a, sdk_stream_t stream);

/* y = silu?(x*scale + shift) with the scale/shift of sdk_group_norm_affine; writes the
 * (possibly 2-source) input contiguous [batch*hw][ld_y].  Used in front of 3x3 convs,
 * where a per-tap prologue would repeat the transform 9x (GroupNorm32 + nn.SiLU,
 * openai_model/model.py:178-181,202-205,528-530; Unet/unet.py:116-125; encoder.py:205-206). */
int sdk_group_norm_apply(const sdk_group_norm_args* a, int32_t silu, void* y, int32_t ld_y, sdk_stream_t stream);

/* The same, written into a zero-bordered image y [batch][h+2*pad][w+2*pad][ld_y] (h*w == hw): the
 * 3x3 conv that consumes it runs with pad 0, so its implicit-GEMM gather has every tap in range
 * (no per-tap masks — the zero padding of nn.Conv2d(padding=1) is stored, not computed). */
int sdk_group_norm_apply_padded(const sdk_group_norm_args* a, int32_t silu, void* y, int32_t ld_y, int32_t h,
                                int32_t w, int32_t pad, sdk_stream_t stream);

/* GroupNorm (+ SiLU) end to end — the whole GroupNorm32 / Normalize module + nn.SiLU of the call
 * sites above: y = silu?(x*scale + shift) into y [batch][h+2*pad][w+2*pad][ld_y] (pad 0: contiguous).
 * Statistics: merged from the per-chunk channel statistics the producing sdk_conv2d emitted
 * (sdk_conv_args.gn_partial; part0 = source 0's [batch][nch0][c_split], part1 = source 1's
 * [batch][nch1][channels - c_split] for a concat; NULL = none), else computed from x (one fused
 * statistics + apply launch at hw <= 64).  a->scale / a->shift / a->workspace as for
 * sdk_group_norm_affine (the fused launch does not touch them). */
int sdk_group_norm(const sdk_group_norm_args* a, int32_t silu, void* y, int32_t ld_y, int32_t h, int32_t w,
                   int32_t pad, const float* part0, int32_t nch0, const float* part1, int32_t nch1,
                   sdk_stream_t stream);

/* The statistics half of sdk_group_norm alone: a->scale / a->shift [batch][channels] of the
 * GroupNorm affine, merged from the producers' per-chunk statistics (part0 / part1 as above) or, with
 * none, computed from x (sdk_group_norm_affine).  For a conv that applies GroupNorm + SiLU to its own
 * A operand (sdk_conv_src.gn_scale / gn_shift / silu), so the normalised tensor is never written: only
 * variant 0, the register-staged kernel, takes the GroupNorm scale / shift prologue; variant 35 (skinny)
 * is planned only without gn_scale and applies SiLU alone. */
int sdk_group_norm_finalize(const sdk_group_norm_args* a, const float* part0, int32_t nch0, const float* part1,
                            int32_t nch1, sdk_stream_t stream);

/* The post-activation GroupNorm of the DDPM (config C1) UNet (DDPM/models/layers.py:23-38 ConvBlock,
 * :311-338 ResNetBlock, :154 attention post-norm): y = [silu](x*scale + shift) + post_bias[b][c]
 * (the time embedding added after block1) + residual[pix][c] (the ResNet skip); both optional. */
int sdk_group_norm_apply_ex(const sdk_group_norm_args* a, int32_t silu, const float* post_bias, int32_t pb_ld,
                            const void* residual, int32_t res_ld, void* y, int32_t ld_y, sdk_stream_t stream);

/* The launches a GroupNorm call takes, decided on the host exactly as the entry points above decide them
 * (they route through the same planner): no device is touched and no pointer is followed beyond `a`, so
 * tests and tools can ask which form runs.  want_stats / want_apply: the affine is computed / the transform
 * is written (sdk_group_norm: both; sdk_group_norm_affine / _finalize: statistics only; sdk_group_norm_apply /
 * _apply_padded: apply only, a->scale / a->shift given).  h * w == a->hw, pad in [0, 4] (pad 0 is applied as the
 * image 1 x hw).  nch0 / nch1 != 0: the producers' partials are given with that many chunks.
 * allow_single_launch = 0 is sdk_group_norm_film, which folds FiLM into the affine between the two passes.
 * Validates as those entry points do (non-zero = they reject the call). */
enum { SDK_GN_STATS_GIVEN = 0,   /* a->scale / a->shift already hold the affine */
       SDK_GN_STATS_SLICE,       /* gn_stats_fused_kernel: one launch, no workspace */
       SDK_GN_STATS_CHUNKED,     /* gn_partial + gn_finalize: two launches, workspace */
       SDK_GN_STATS_PARTS };     /* merged from the producing convs' partials */
enum { SDK_GN_APPLY_NONE = 0,    /* statistics only */
       SDK_GN_APPLY_IN_STATS,    /* same launch as the statistics (fused / from-partials single launch) */
       SDK_GN_APPLY_FLAT, SDK_GN_APPLY_ROW, SDK_GN_APPLY_STRIDE };
typedef struct { int32_t stats, apply, launches; int64_t workspace_bytes; } sdk_group_norm_plan_info;
int sdk_group_norm_plan(const sdk_group_norm_args* a, int32_t want_stats, int32_t want_apply, int32_t h, int32_t w,
                        int32_t pad, int32_t nch0, int32_t nch1, int32_t allow_single_launch,
                        sdk_group_norm_plan_info* info);

/* ---------------------------------------------------------------- device calibration probes
 * Not on the sampling path: measure, on the box the bench runs on, the dense fp16 MFMA rate held
 * under load (back-to-back v_mfma_f32_16x16x32_f16 (m16 = 1) or 32x32x16 on random register
 * operands, `blocks` workgroups of 4 waves, `iters` iterations; seed = 32768 random fp16, sink =
 * blocks*4 floats) and the HBM copy rate, next to the spec peaks the roofline is quoted against.
 */
double sdk_probe_mfma_flops(int32_t m16, int32_t blocks, int32_t iters);
int sdk_probe_mfma(int32_t m16, int32_t blocks, int32_t iters, const void* seed, float* sink, sdk_stream_t stream);
int sdk_probe_copy(const void* src, void* dst, int64_t bytes, sdk_stream_t stream);
/* the copy with its shape chosen: mode bit 0 = 8 loads in flight per thread (else 4), bit 1 = non-temporal
   loads / stores, bits 2-7 = workgroups per CU (0: 16), bit 8 = one pass with a grid covering the buffer
   (each workgroup one contiguous chunk; bits 2-7 ignored); sdk_probe_copy is mode 0 */
int sdk_probe_copy_ex(const void* src, void* dst, int64_t bytes, int32_t mode, sdk_stream_t stream);

/* ---------------------------------------------------------------- LayerNorm
 * y = (x - mean) * rstd * gamma + beta over the last dim, fp16 in/out, fp32 math; gamma / beta fp32,
 * 16-byte aligned; cols a multiple of 8, <= 2048.
 * Replaces nn.LayerNorm norm1/2/3 (openai_model/attention.py:216-218,251-253).
 */
int sdk_layer_norm(const void* x, void* y, int32_t rows, int32_t cols, int32_t ld_x, int32_t ld_y,
                   const float* gamma, const float* beta, float eps, sdk_stream_t stream);

/* ---------------------------------------------------------------- attention
 * O = softmax(scale * Q K^T) V per (batch, head), non-causal, fp16 in/out, fp32
 * softmax; flash-style (online softmax, scores never leave the CU).
 * q/k/v/o are token-major: element (b, token, head, d) at ptr[(b*n + token)*ld + head*head_dim + d].
 * Replaces flash_attn_func (openai_model/attention.py:106-112; Unet/attention.py:257)
 * and flash_attn_qkvpacked_func (openai_model/attention.py:389-394,516-521).
 */
typedef struct {
  const void* q; const void* k; const void* v; void* o;
  int32_t q_ld, k_ld, v_ld, o_ld;
  int32_t batch, heads, nq, nk, head_dim;
  float scale;
  int32_t causal;          /* 1: key j is masked for query i when j > i (CLIP text encoder) */
} sdk_attention_args;

int sdk_attention(const sdk_attention_args* a, sdk_stream_t stream);

/* The same launch with the kernel form chosen by the caller and read back (tests and tools;
 * sdk_attention(a, s) is sdk_attention_form(a, SDK_ATTN_AUTO, NULL, s)).
 *   SDK_ATTN_AUTO      the default of the head dim: 4 waves for head_dim <= 32 and > 80, 8 waves for
 *                      40..48, 8 waves staggered for 56..80; the environment's tuning knobs apply
 *                      (SDK_ATTN_NW=4, SDK_ATTN_STAG=0/1, SDK_ATTN_QB=2, read once per process)
 *   SDK_ATTN_NW4       4 waves = 128 query rows per workgroup; every head_dim
 *   SDK_ATTN_NW8       8 waves = 256 query rows; head_dim 40..80
 *   SDK_ATTN_NW8_STAG  8 waves, waves 4..7 run half a key tile behind waves 0..3 (three LDS stages);
 *                      head_dim 40..80
 *   SDK_ATTN_QB2       4 waves with two 32-row query blocks each; head_dim 40..48, non-causal
 *   SDK_ATTN_WIDE      head_dim 168..512 (AUTO's choice above 160), non-causal: the 8 waves of a workgroup
 *                      share SDK_ATTN_WIDE_ROWS = 64 query rows, staged once in LDS, compute each
 *                      SDK_ATTN_WIDE_KT = 32-key score tile once and split head_dim between them for
 *                      O += P V (the first stage's one-head AttnBlock, C = 512).  Instantiated for padded
 *                      head dims 256 (head_dim <= 256) and 512.  At head_dim <= 160, or with causal,
 *                      SDK_EINVAL
 * A form other than AUTO that has no instantiation at a->head_dim (or QB2 with a->causal) returns
 * SDK_EINVAL; it never falls back to another form.
 * ran (may be NULL) receives what was launched, from the launched kernel's template arguments: form (the
 * form after AUTO is resolved), dqk / dv (the padded head dim of the QK^T and the PV products), waves per
 * workgroup, qblocks (32-row query blocks per wave; under SDK_ATTN_WIDE the 32-row query blocks per
 * WORKGROUP, SDK_ATTN_WIDE_ROWS / 32 = 2, which all its waves share: grid = ceil(nq / 64) * heads * batch), stagger, seed_col (head_dim 40 with 8 waves: the
 * padding column of Q that carries the running max; else 0), causal and grid (workgroups).  The causal
 * kernels are neither staggered nor seeded through a column, so a causal launch reports stagger = 0 and
 * seed_col = 0 under every form.  ran is written on the host before the launch: it costs nothing and is
 * the same under stream capture. */
enum { SDK_ATTN_AUTO = 0, SDK_ATTN_NW4, SDK_ATTN_NW8, SDK_ATTN_NW8_STAG, SDK_ATTN_QB2, SDK_ATTN_WIDE };
#define SDK_ATTN_WIDE_ROWS 64   /* query rows per workgroup of SDK_ATTN_WIDE */
#define SDK_ATTN_WIDE_KT 32     /* keys per tile of SDK_ATTN_WIDE (two-slot K / V ring) */
typedef struct { int32_t form, dqk, dv, waves, qblocks, stagger, seed_col, causal, grid; } sdk_attention_form_info;
int sdk_attention_form(const sdk_attention_args* a, int32_t form, sdk_attention_form_info* ran /* may be NULL */,
                       sdk_stream_t stream);

/* Linear attention (Unet/attention.py:131-181, LinearAttention.forward after to_qkv), per (batch, head):
 *   ctx[d][e] = sum_n softmax_n(k)[n][d] * v[n][e],   out[n][e] = sum_d q[n][d] * ctx[d][e]
 * q / k / v / o: 2-D fp16 views [batch*n, ld], head h at columns h*dim_head.. (as sdk_attention).
 * dim_head: a multiple of 8 in [8, 512]; any heads.  No scale and no softmax over q (the reference has neither).
 * Three launches, no floating-point atomics, a fixed summation order (bitwise reproducible):
 *  1. context: the tokens are cut into sdk_linear_attention_chunks(n) chunks; per chunk and column d the
 *     maximum m_c[d] of k*log2(e), P = exp2(k*log2(e) - m_c) rounded to fp16, ctx_c = P^T V by MFMA into fp32,
 *     den_c = the column sums of P (fp32, before rounding); (m_c, den_c, ctx_c) go to the workspace;
 *  2. combine: the chunks in ascending order, each weighted by exp2(m_c - max_c m_c); ctx / den, rounded to
 *     fp16, stored transposed ([e][d]) in the workspace;
 *  3. apply: out = q ctx, an MFMA GEMM whose B operand is per (batch, head).
 * workspace: sdk_linear_attention_workspace_bytes(a) bytes, 16-B aligned. */
typedef struct {
  const void* q; const void* k; const void* v; void* o;
  int32_t q_ld, k_ld, v_ld, o_ld;
  int32_t batch, heads, n, dim_head;
  void* workspace; int64_t workspace_bytes;
} sdk_linear_attention_args;
int32_t sdk_linear_attention_chunks(int32_t n);
int64_t sdk_linear_attention_workspace_bytes(const sdk_linear_attention_args* a);
int sdk_linear_attention(const sdk_linear_attention_args* a, sdk_stream_t stream);

/* Fused cross-attention block on a cached context K|V: out = (softmax(scale * (t Wq^T)_h K_h^T) V_h)_h
 * Wo^T + bias + res, one kernel, q and o kept in LDS.  Replaces, per denoising step, the
 * to_q Linear + flash_attn_func + to_out Linear of CrossAttention.forward with a context
 * (openai_model/attention.py:63-117) and the residual add of BasicTransformerBlock
 * (attention.py:249).  t / res / out: [batch*n_img, ld] fp16; kv: [batch*nk, kv_ld] fp16
 * with K at columns [0, channels) and V at [channels, 2*channels); wq / wo: fp16 [>= channels
 * rows][w_ld = channels] (row n = output channel), or w_ld = 0: both in the fragment-packed layout of
 * sdk_xattn_pack_weight (channels * channels fp16, one contiguous KiB per MFMA fragment: whole-line weight
 * fetches); bias fp32 [channels] or NULL.
 * Shapes: sdk_cross_attention_block_supported() (channels 320 / 640, head_dim 40 / 64 / 80,
 * nk <= 80, n_img % 64 == 0); others return SDK_EINVAL (callers use the three-launch path).
 */
typedef struct {
  const void* t; const void* kv; const void* wq; const void* wo; const float* bias; const void* res;
  void* out;
  int32_t t_ld, kv_ld, w_ld, res_ld, out_ld;
  int32_t batch, n_img, nk, channels, head_dim;
  float scale;
} sdk_xattn_args;

int sdk_cross_attention_block_supported(int32_t channels, int32_t head_dim, int32_t nk, int32_t n_img);
/* One-time pack of a projection weight (fp16 [channels rows][w_ld], nn.Linear layout) into packed
 * (channels * channels fp16, 16-B aligned, device) for sdk_xattn_args.w_ld = 0; channels 320 / 640. */
int sdk_xattn_pack_weight(const void* w, int32_t w_ld, void* packed, int32_t channels, sdk_stream_t stream);
int sdk_cross_attention_block(const sdk_xattn_args* a, sdk_stream_t stream);

/* The same block with BasicTransformerBlock's two LayerNorms around it fused in
 * (openai_model/attention.py:249-250: x = attn2(norm2(x), context) + x; ... ff(norm3(x))):
 *  - in_gamma != NULL: a->t holds norm2's INPUT (the token rows, normally a->res as well) and is
 *    normalised inside the kernel (eps in_eps, fp32 gamma / beta, 16-B aligned);
 *  - out_gamma != NULL: out_ln[M, out_ln_ld] = norm3(out) is written as well.
 * Both norms produce the same bits as sdk_layer_norm on the same rows.  Either may be NULL.
 */
typedef struct {
  const float* in_gamma; const float* in_beta; float in_eps;
  const float* out_gamma; const float* out_beta; float out_eps;
  void* out_ln; int32_t out_ln_ld;
} sdk_xattn_ln_args;

int sdk_cross_attention_block_ln(const sdk_xattn_args* a, const sdk_xattn_ln_args* ln, sdk_stream_t stream);

/* ---------------------------------------------------------------- segment softmax
 * p[m, h*seglen + j] = softmax_j(scale * s[m, h*seglen + j]) for each of nseg segments of a row (fp32 in,
 * fp16 out), columns [nseg*seglen, ld_p) of p written as zeros (the K padding of the GEMM that consumes
 * p).  The middle step of the reassociated cross-attention at the 1280-channel levels, where the
 * scores of all heads against the cached context come out of ONE GEMM with per-prompt weights
 * (K_h Wq_h per head, sdk_conv_args.weight_batch_stride) and the output of another (Wo_h V_h^T).
 * Replaces: the sim.softmax(dim=-1) of CrossAttention.forward (openai_model/attention.py:106-112, in
 * flash_attn_func at the call sites :216-257).  seglen <= 128. */
int sdk_segment_softmax(const float* s, int32_t ld_s, void* p, int32_t ld_p, int32_t rows, int32_t nseg,
                        int32_t seglen, float scale, sdk_stream_t stream);

/* ---------------------------------------------------------------- fused feed-forward
 * out[m] = res[m] + W2 (a * gelu(g)) + b2,  [a | g] = t[m] W1^T + b1  — the GEGLU FeedForward of
 * BasicTransformerBlock in ONE kernel (GEGLU -> Dropout(0) -> Linear, openai_model/attention.py:129-172,
 * called as x = self.ff(self.norm3(x)) + x at :253); the 4*channels-wide intermediate stays in registers.
 * Shapes: channels == 320 (SD's 64x64-level blocks), features (the GEGLU width, 4*channels in SD) a
 * multiple of 32 (sdk_ff_supported).  t / res / out: [rows, ld] fp16, 16-B aligned, ld % 8 == 0 and
 * ld >= channels (t_ld, out_ld, and res_ld when res is given; anything else is SDK_EINVAL); res may
 * be NULL or alias out.  Weights go through a one-time pack: w1 fp16 [2*features][channels] (rows
 * [0, features) = a, [features, 2*features) = gate, as nn.Linear(channels, 2*features).weight), b1 fp32
 * [2*features] or NULL, w2 fp16 [channels][features] (nn.Linear(features, channels).weight) ->
 * `packed` (sdk_ff_packed_bytes bytes, 16-B aligned, device); b2 fp32 [channels] (16-B aligned) or NULL.
 */
typedef struct {
  const void* t; const void* res; void* out; const void* packed; const float* b2;
  int32_t t_ld, res_ld, out_ld;
  int32_t rows, channels, features;
} sdk_ff_args;

int sdk_ff_supported(int32_t channels, int32_t features);
int64_t sdk_ff_packed_bytes(int32_t channels, int32_t features);
int sdk_ff_pack(const void* w1, const float* b1, const void* w2, void* packed, int32_t channels, int32_t features,
                sdk_stream_t stream);
int sdk_feed_forward(const sdk_ff_args* a, sdk_stream_t stream);

/* ---------------------------------------------------------------- 320-channel token linear
 * out[m] = [res[m] +] x[m] W^T + b for the 64x64-level transformer blocks' 320 -> 320 projections:
 * SpatialTransformer.proj_in (openai_model/attention.py:293-300, a 1x1 conv = per-token linear) and the
 * self-attention's to_out with its residual (:203-206, x = attn1(norm1(x)) + x at :251).  W stays in
 * registers, the grid walks 32-token blocks (csrc/token.hip).  x / res / out: [rows, ld] fp16, 16-B
 * aligned, ld % 8 == 0; res may be NULL or alias out; x must not overlap out.  w fp16 [320][320]
 * (nn.Linear.weight: [out][in]), 16-B aligned; bias fp32 [320] (16-B aligned) or NULL.
 */
typedef struct {
  const void* x; const void* w; const float* bias; const void* res; void* out;
  int32_t x_ld, res_ld, out_ld;
  int32_t rows, in_features, out_features;
} sdk_token_linear_args;

int sdk_token_linear_supported(int32_t in_features, int32_t out_features);
int sdk_token_linear(const sdk_token_linear_args* a, sdk_stream_t stream);

/* The same projection, also writing out_ln[m] = LayerNorm(out[m]) (fp32 gamma / beta [320], 16-B aligned;
 * the same bits as sdk_layer_norm on out): SpatialTransformer.proj_in followed by the first
 * BasicTransformerBlock's norm1 (openai_model/attention.py:330 then :251, x = attn1(norm1(x)) + x), one
 * launch instead of two.  out_ln [rows, out_ln_ld] must not overlap x, res or out. */
int sdk_token_linear_ln(const sdk_token_linear_args* a, const float* gamma, const float* beta, float eps,
                        void* out_ln, int32_t out_ln_ld, sdk_stream_t stream);

/* ---------------------------------------------------------------- SpatialTransformer entry, chained
 * The entry of a 320-channel SpatialTransformer in one launch (csrc/conv_rowpanel.hip, proj_norm_qkv_kernel):
 *   tok = proj_in(xn),  qkv = [to_q | to_k | to_v](LayerNorm(tok)),   xn = x, or (half)(x * scale + shift)
 * (openai_model/attention.py:328-330 then :251 and :96-99).  tok and qkv carry the bits of sdk_group_norm (no SiLU)
 * -> sdk_token_linear_ln -> sdk_conv2d on the q|k|v weight; the GroupNorm output and LayerNorm(tok) are never
 * written.  x [rows, x_ld], tok [rows, tok_ld], qkv [rows, qkv_ld]: fp16, 16-B aligned, strides multiples of 8;
 * neither output may overlap an input or the other output.
 * w: fp16 [1280][320], bias: fp32 [1280] — proj_in's rows first, PERMUTED: packed row 160 c + 16 nb + 4 cg + q
 * (c < 2, nb < 10, cg < 4, q < 4) holds output channel 32 (g / 2) + 8 cg + 4 (g % 2) + q with g = 10 c + nb; then
 * the 960 q|k|v rows in order (their bias entries zero where the projections have none).
 * gamma / beta: fp32 [320] of the LayerNorm.  gn_scale / gn_shift: NULL, or the fp32 [rows / hw][320] affine of
 * sdk_group_norm_affine with hw = rows per image (rows % hw == 0).  in_features / features / qkv_features must be
 * 320 / 320 / 960 (sdk_proj_norm_qkv_supported).
 */
typedef struct {
  const void* x; const float* gn_scale; const float* gn_shift; const void* w; const float* bias;
  const float* gamma; const float* beta; void* tok; void* qkv;
  int32_t x_ld, tok_ld, qkv_ld, rows, hw;
  int32_t in_features, features, qkv_features;
  float eps;
} sdk_proj_norm_qkv_args;

int sdk_proj_norm_qkv_supported(int32_t in_features, int32_t features, int32_t qkv_features);
int sdk_proj_norm_qkv(const sdk_proj_norm_qkv_args* a, sdk_stream_t stream);

/* ---------------------------------------------------------------- sampler / glue
 * DDIM update (DDIM/ddim.py:194-204 == ldm/diffusion/ddim.py:197-205), fp32,
 * evaluated op by op without contraction so it is bit-identical to torch's CPU
 * kernels on the same inputs.  Optional fused classifier-free guidance
 * (ddim.py:171-178: e = e_u + g*(e_c - e_u)) and v-prediction (extension: e =
 * sqrt(a)*v + sqrt(1-a)*x).
 */
typedef struct {
  const float* x; const float* e; const float* e_uncond; const float* noise;
  float* x_prev; float* pred_x0;
  int64_t n;
  float sqrt_one_minus_at, sqrt_at, dir_coef, sqrt_a_prev, sigma, temperature;
  float guidance;          /* used when e_uncond != NULL */
  int32_t v_param;         /* 1: e holds v; convert with v_sqrt_a / v_sqrt_1ma */
  float v_sqrt_a, v_sqrt_1ma;
} sdk_ddim_args;

int sdk_ddim_step(const sdk_ddim_args* a, sdk_stream_t stream);

/* Second half of the DDIM update for quantize_denoised (DDIM/ddim.py:196-203): the reference
 * quantises pred_x0 between the two halves, so here a->pred_x0 is an INPUT and only
 * x_prev = sqrt_a_prev*pred_x0 + dir_coef*e + sigma*noise*temperature is written (e after the same
 * guidance combine / v conversion as sdk_ddim_step; x is read only when v_param).  Same operations in
 * the same order as sdk_ddim_step: fed that call's pred_x0 it reproduces its x_prev bit for bit. */
int sdk_ddim_xprev(const sdk_ddim_args* a, sdk_stream_t stream);

/* ---------------------------------------------------------------- ancestral sampler (LatentDiffusion.p_sample)
 * Fused posterior step (ldm/diffusion/ddpm.py:1528-1636), fp32, every product and sum rounded on its own:
 *   1. x_recon = c_recip*x - c_recipm1*model_out   (eps)   |   x_recon = model_out   (x0_param)
 *   2. clip: x_recon = clamp(x_recon, -1, 1)
 *   3. mean = coef1*x_recon + coef2*x
 *   4. x_prev = mean + ((nonzero*sigma) * (noise*temperature))
 * The scalars are the fp32 schedule entries at one timestep t (sqrt_recip_alphas_cumprod,
 * sqrt_recipm1_alphas_cumprod, posterior_mean_coef1 / 2, sigma = exp(0.5*posterior_log_variance_clipped)
 * evaluated by the caller on the host and correctly rounded to fp32, nonzero = t != 0); a batch with
 * several t is one call per run of equal t.  stage 0: steps 1-4 (x_recon written when non-NULL).  stage 1: steps 1-2 only, x_recon is
 * the output.  stage 2: steps 3-4 with x_recon_in as INPUT (quantize_denoised quantises it in between;
 * no clamp is applied again) -- fed stage 1's x_recon it reproduces stage 0's x_prev bit for bit.
 * noise may be NULL where nonzero == 0.  Any n >= 1; 16-byte accesses when every pointer is 16-byte
 * aligned, scalar otherwise and for the tail.  x_prev may alias x; x_recon may alias model_out. */
typedef struct {
  const float* x; const float* model_out; const float* noise; const float* x_recon_in;
  float* x_prev; float* x_recon;
  int64_t n;
  int32_t stage, x0_param, clip;
  float c_recip, c_recipm1, coef1, coef2, sigma, nonzero, temperature;
} sdk_posterior_args;

int sdk_posterior_step(const sdk_posterior_args* a, sdk_stream_t stream);

/* Known-region blend of p_sample_loop (ldm/diffusion/ddpm.py:1783-1784) at one timestep:
 * out = (sqrt_acp*x0 + sqrt_1m_acp*noise)*mask + (1 - mask)*img, op by op in that order.  x0, noise, img,
 * out: n = batch*per_sample fp32, per_sample = channels*hw.  The mask is read by index, never expanded:
 * mask_mode 0 [batch][1][hw], 1 [1][1][hw], 2 [batch][channels][hw].  out may alias img. */
typedef struct {
  const float* x0; const float* noise; const float* mask; const float* img;
  float* out;
  int64_t n, per_sample;
  int32_t hw, mask_mode;
  float sqrt_acp, sqrt_1m_acp;
} sdk_masked_q_args;

int sdk_masked_q_sample(const sdk_masked_q_args* a, sdk_stream_t stream);

/* Classifier-free-guidance combine on its own (ddim.py:178): out = e_uncond + guidance*(e_cond - e_uncond),
 * the same two fp32 operations as the combine fused into sdk_ddim_step, so sdk_cfg_combine followed by an
 * unguided step gives the guided step's bits (a score corrector needs the combined e as a tensor).  Any
 * n >= 1; 16-byte accesses when every pointer is 16-byte aligned, scalar otherwise and for the tail.
 * out may alias either input. */
int sdk_cfg_combine(const float* e_uncond, const float* e_cond, float* out, int64_t n, float guidance,
                    sdk_stream_t stream);

/* DDIM update with the sampler options (ddim.py:144-204); sdk_ddim_step and sdk_ddim_xprev launch the same
 * kernel with everything after `step` zero.
 *   step        the fields of sdk_ddim_step.
 *   pred_x0_in  1: step.pred_x0 is an INPUT (sdk_ddim_xprev); step.x is then read only with v_param.
 *   keep        noise dropout (ddim.py:201-202), one byte (0 / 1) per element, or NULL; needs step.noise.  The
 *               noise term becomes ((sigma*noise)*temperature) * (keep*drop_scale), drop_scale = fp32(1/(1-p)):
 *               a multiply as in F.dropout, never a select, so the signed zeros match.
 *   blend       with blend.mask != NULL the known-region blend that opens the NEXT loop iteration
 *               (ddim.py:146-147) is applied to x_prev: blend.out = (sqrt_acp*x0 + sqrt_1m_acp*noise)*mask +
 *               (1 - mask)*x_prev, sqrt_acp / sqrt_1m_acp the model's schedule entries at the next timestep;
 *               blend.img and blend.n are ignored, the mask is read as by sdk_masked_q_sample.  step.x_prev
 *               and pred_x0 hold the unblended values.  blend.out may alias step.x.
 * Any n >= 1; 16-byte accesses when every pointer is 16-byte aligned (keep: 4-byte), scalar otherwise and
 * for the tail. */
typedef struct {
  sdk_ddim_args step;
  int32_t pred_x0_in;
  float drop_scale;
  const uint8_t* keep;
  sdk_masked_q_args blend;
} sdk_ddim_ex_args;

int sdk_ddim_step_ex(const sdk_ddim_ex_args* a, sdk_stream_t stream);

/* sdk_posterior_step with noise dropout (ldm/diffusion/ddpm.py:1621-1636): step 4 becomes
 * x_prev = mean + ((nonzero*sigma) * ((noise*temperature) * (keep*drop_scale))); keep / drop_scale as in
 * sdk_ddim_ex_args, keep NULL: sdk_posterior_step (which launches the same kernel). */
typedef struct {
  sdk_posterior_args step;
  const uint8_t* keep;
  float drop_scale;
} sdk_posterior_ex_args;

int sdk_posterior_step_ex(const sdk_posterior_ex_args* a, sdk_stream_t stream);

/* Multistep sampler update (extension: PLMS as CompVis' ldm/models/diffusion/plms.py, DPM-Solver++(2M)
 * on the DDIM timestep grid), one launch, fp32, every product, sum and quotient rounded on its own.  e below is
 * the model output after the guidance combine and v conversion of sdk_ddim_step (step.e, e_uncond, guidance,
 * v_param, v_sqrt_a, v_sqrt_1ma); step.noise must be NULL and step.sigma 0, temperature is ignored.
 *   SDK_MULTISTEP_PLMS         hist[0..nhist-1] hold the guided e of the previous 1-3 steps, most recent first:
 *                                nhist 0  e' = e                          1  e' = (3 e - h1) / 2
 *                                      2  e' = ((23 e - 16 h1) + 5 h2) / 12
 *                                      3  e' = (((55 e - 59 h1) + 37 h2) - 9 h3) / 24        (true divisions)
 *                              then pred_x0 and x_prev are what sdk_ddim_step computes at sigma 0 with e' for e
 *                              (v conversion, if any, happens before: e' is never converted); hist_out = e.
 *   SDK_MULTISTEP_PLMS_WARMUP  the first step's second half: e' = (e + e_next) / 2, e_next the (guided, eps)
 *                              output of the model at the tentative x_prev; the rest as above.
 *   SDK_MULTISTEP_DPM          D = (x - sqrt_one_minus_at e) / sqrt_at (the bits of sdk_ddim_step's pred_x0);
 *                              nhist 0: x_prev = c_x x + c_0 D;  nhist 1: x_prev = (c_x x + c_0 D) + c_1 hist[0],
 *                              hist[0] the previous step's D; pred_x0 = D, hist_out = D.  c_x, c_0, c_1 are the
 *                              caller's fp32 coefficients; dir_coef and sqrt_a_prev are ignored.
 * pred_x0 and hist_out are written when non-NULL.  hist_out may alias any history pointer (the ring's oldest
 * entry) and blend.out may alias step.x: each element is read before the same thread writes it.  blend as in
 * sdk_ddim_ex_args.  Any n >= 1; 16-byte accesses when every pointer is 16-byte aligned, scalar otherwise and for
 * the tail. */
enum { SDK_MULTISTEP_PLMS = 0, SDK_MULTISTEP_PLMS_WARMUP = 1, SDK_MULTISTEP_DPM = 2 };

typedef struct {
  sdk_ddim_args step;
  const float* hist[3];
  const float* e_next;
  float* hist_out;
  int32_t form, nhist;
  float c_x, c_0, c_1;
  int32_t reserved;        /* 0 */
  sdk_masked_q_args blend;
} sdk_multistep_args;

int sdk_multistep_step(const sdk_multistep_args* a, sdk_stream_t stream);

/* sdk_nchw_to_nhwc (scale 1) of torch.cat(src, 1) without the concatenated fp32 tensor
 * (DiffusionWrapper.forward 'concat' / 'hybrid', Diffusion/ddpm.py:51-63): nsrc (1..4) NCHW fp32 sources
 * [batch][channels[i]][hw] -> y NHWC fp16 [batch][hw][c_pad]; source i lands at channel offset
 * sum(channels[<i]), channels from the sum up to c_pad are zero. */
typedef struct {
  const float* src[4];
  int32_t channels[4];
  int32_t nsrc;
  void* y;
  int32_t batch, hw, c_pad;
} sdk_concat_args;

int sdk_concat_nchw_to_nhwc(const sdk_concat_args* a, sdk_stream_t stream);

/* The UNet input of np patches of a large latent, gathered from the full-size tensors (LatentDiffusion.apply_model
 * with split_input_params, Diffusion/ddpm.py:1151-1266: Unfold of z and of every c_concat entry, then the channel
 * concat and the input cast): sdk_concat_nchw_to_nhwc applied to the sdk_extract_patches output of every source,
 * restricted to patches [p0, p0 + np), without any fp32 patch tensor.  nsrc (1..4) NCHW fp32 sources
 * [batch][channels[i]][h][w] -> y NHWC fp16 [np][kh*kw][c_pad]; patches of kh x kw every (sy, sx), Ly = (h-kh)/sy+1,
 * Lx = (w-kw)/sx+1, patch index p = l*batch + b with l = ly*Lx + lx (torch.nn.Unfold order); source i lands at
 * channel offset sum(channels[<i]), channels from the sum up to c_pad are zero.  No scratch.  SDK_EINVAL for a null
 * pointer, nsrc outside 1..4, kh > h, kw > w, a stride <= 0, c_pad below the channel sum, or a window with p0 < 0,
 * np < 1 or p0 + np > Ly*Lx*batch. */
typedef struct {
  const float* src[4];
  int32_t channels[4];
  int32_t nsrc;
  void* y;
  int32_t batch, h, w, c_pad;
  int32_t kh, kw, sy, sx;
  int32_t p0, np;
} sdk_patch_pack_args;

int sdk_patch_pack(const sdk_patch_pack_args* a, sdk_stream_t stream);

/* ---------------------------------------------------------------- vector quantiser (vqvae/quantize.py)
 * norms[j] = |codebook[j]|^2 (fp32 fma chain), computed once per codebook [n][d]. */
int sdk_vq_code_norms(const float* codebook, float* norms, int32_t n, int32_t d, sdk_stream_t stream);

/* Number of codebook splits sdk_vq_nearest uses for m rows (0: unsupported shape).  With more than
 * one split the call needs `keys`: 8 bytes per row. */
int32_t sdk_vq_nearest_splits(int64_t m, int32_t n, int32_t d);

/* Nearest code per row of z (VectorQuantize2.forward, vqvae/quantize.py:131-163) without the [M, n]
 * distance matrix.  z, z_q: NCHW fp32 [batch][d][hw], read / written in place (row m = (b, pixel));
 * codebook [n][d] fp32; norms from sdk_vq_code_norms.  idx[m] = argmin_j |e_j|^2 - 2 z_m.e_j in fp32,
 * the lowest index among equal scores; z_q = z + (e[idx] - z), two roundings.  1 <= d <= 256.
 * force_splits > 0 overrides the split count (tests); keys may be NULL when one split is used. */
int sdk_vq_nearest(const float* z, const float* codebook, const float* norms, int64_t* idx, float* z_q,
                   int32_t batch, int32_t d, int32_t hw, int32_t n, void* keys, int64_t keys_bytes,
                   int32_t force_splits, sdk_stream_t stream);

/* out = codebook[idx] for m indices: [m][d] (nchw = 0) or [m / hw][d][hw] (nchw = 1)
 * (get_codebook_entry, ldm/tamming/quantize.py:314-329).  The caller range-checks idx on the host. */
int sdk_vq_lookup(const int64_t* idx, const float* codebook, float* out, int64_t m, int32_t n, int32_t d,
                  int32_t hw, int32_t nchw, sdk_stream_t stream);

/* Index remap (vqvae/quantize.py:67-101, ldm/tamming/quantize.py:261-269).  mode 0, remap_to_used:
 * first position in used[n_used] equal to the index, else rnd[i] (when rnd != NULL) or `unknown`.
 * mode 1, unmap_to_all: used[index]; with `extra` an index >= n_used is first set to 0. */
int sdk_vq_remap(const int64_t* inds, const int64_t* used, const int64_t* rnd, int64_t* out, int64_t count,
                 int32_t n_used, int32_t mode, int64_t unknown, int32_t extra, sdk_stream_t stream);

/* DDPM ancestral update (DDPM/ddpm.py:84-86):
 * x = inv_sqrt_alpha*(x - coef*eps) + sigma*noise. */
int sdk_ddpm_step(const float* x, const float* eps, const float* noise, float* out, int64_t n,
                  float inv_sqrt_alpha, float coef, float sigma, sdk_stream_t stream);

/* Sinusoidal timestep embedding cat[cos(t*f), sin(t*f)] -> fp16 (openai_model/utils.py:225-245;
 * the reference feeds time_embed with t_emb.half(), model.py:566). */
int sdk_timestep_embedding(const int64_t* t, const float* freqs, void* out, int32_t batch, int32_t dim,
                           sdk_stream_t stream);

/* NCHW fp32 -> NHWC fp16 with channel zero-padding to c_pad and a scalar pre-scale
 * (x.type(dtype), model.py:572; 1/scale_factor*z, ldm/diffusion/ddpm.py:1095). */
int sdk_nchw_to_nhwc(const float* x, void* y, int32_t batch, int32_t channels, int32_t hw, int32_t c_pad,
                     float scale, sdk_stream_t stream);

/* KL posterior sample scaled into the diffusion latent space:
 * z = scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * noise), or scale * mean when noise is NULL
 * (the posterior mode).  moments: NCHW fp32 [batch][2*channels][hw] (mean | logvar, the quant_conv
 * output), z: [batch][channels][hw].  Replaces DiagonalGaussianDistribution.sample/mode
 * (Distribution/distribution.py:31-50) + get_first_stage_encoding's scale (ldm/diffusion/ddpm.py:795-806). */
int sdk_diag_gaussian_sample(const float* moments, const float* noise, float* z, int32_t batch, int32_t channels,
                             int32_t hw, float scale, sdk_stream_t stream);

/* DDIM stochastic encode (ldm/diffusion/ddim.py:209-222 == DDIM/ddim.py:207-220) for one timestep:
 * out = sqrt_a * x0 + sqrt_1ma * noise, two correctly-rounded products and a sum (no contraction),
 * bit-identical to torch's CPU evaluation of the reference expression. */
int sdk_stochastic_encode(const float* x0, const float* noise, float* out, int64_t n, float sqrt_a,
                          float sqrt_1ma, sdk_stream_t stream);

/* Token + position embedding of the CLIP text transformer (transformers CLIPTextEmbeddings,
 * called by FrozenCLIPEmbedder.forward, clip_encoder/modules.py:241-256):
 * out[b][t][:] = fp16(tok[ids[b][t]][:] + pos[t][:]), fp32 tables [vocab][dim] / [>= seq][dim].
 * Ids outside [0, vocab) are an error (reported through sdk_last_error after the launch
 * is skipped: the ids are checked on the host by the caller). */
int sdk_token_embedding(const int64_t* ids, const float* tok, const float* pos, void* out, int32_t batch,
                        int32_t seq, int32_t dim, sdk_stream_t stream);

/* Tiled first-stage decode (ldm/diffusion/ddpm.py:1097-1139 with
 * get_fold_unfold / get_weighting / delta_border :829-997, CompVis semantics — see DESIGN.md Q14):
 * extract: latent NCHW fp32 [batch][channels][h][w] -> patches [L][batch][channels][kh][kw],
 *   L = Ly*Lx, Ly = (h-kh)/sy + 1, patch l = ly*Lx + lx (torch.nn.Unfold order);
 * fold: decoded patches [L][batch][channels][ph][pw] -> out [batch][channels][h][w] =
 *   sum_l w*patch / sum_l w with w = pix_w[i][j] * l_w[l] (l_w may be NULL), the per-pixel
 *   normalised overlap-add that Fold(o*weighting) / Fold(weighting) computes. */
int sdk_extract_patches(const float* z, float* out, int32_t batch, int32_t channels, int32_t h, int32_t w,
                        int32_t kh, int32_t kw, int32_t sy, int32_t sx, sdk_stream_t stream);
int sdk_fold_patches(const float* patches, const float* pix_w, const float* l_w, float* out, int32_t batch,
                     int32_t channels, int32_t h, int32_t w, int32_t ph, int32_t pw, int32_t sy, int32_t sx,
                     int32_t ly, int32_t lx, sdk_stream_t stream);

/* DDPM (C1) UNet glue: F.interpolate(x2, bilinear, align_corners=True) on NHWC fp16
 * (DDPM/models/layers.py:55-66 UpsampleBlock) and the exact GELU of its time MLP (unet.py:27-32). */
int sdk_upsample_bilinear2x(const void* x, void* y, int32_t batch, int32_t h, int32_t w, int32_t channels,
                            sdk_stream_t stream);
int sdk_gelu(const void* x, void* y, int64_t n, sdk_stream_t stream);

/* UNet Upsample (openai_model/model.py:120-131: F.interpolate(x, scale_factor=2, mode="nearest") then
 * conv3x3 with padding `pad`): y = [batch][2h + 2pad][2w + 2pad][channels] fp16, the nearest-x2 image with a
 * zero border of `pad`, for an unmasked (pad 0) sdk_conv2d.  x rows have stride ld_x (halfs). */
int sdk_upsample_nearest2x_padded(const void* x, int32_t ld_x, void* y, int32_t batch, int32_t h, int32_t w,
                                  int32_t channels, int32_t pad, sdk_stream_t stream);

/* The image itself with a zero border of `pad`: y = [batch][h + 2pad][w + 2pad][channels] fp16 — the source of
 * the phase-form Upsample conv (sdk_conv_args.upsample_phase, pad 1): a quarter of the x2 image's bytes. */
int sdk_zero_border(const void* x, int32_t ld_x, void* y, int32_t batch, int32_t h, int32_t w, int32_t channels,
                    int32_t pad, sdk_stream_t stream);

/* ---------------------------------------------------------------- ADM("guided diffusion") UNet options
 * GroupNorm with FiLM conditioning (+ SiLU), the `use_scale_shift_norm` ResBlock (openai_model/model.py:244-248:
 * out_norm(h) * (1 + scale) + shift, then SiLU): as sdk_group_norm, with film = fp32 [batch][film_ld], the
 * scale at film[b*film_ld + film_off + c] and the shift at film[b*film_ld + film_off + channels + c] (this
 * block's columns of the batched emb_layers GEMM).  The FiLM terms are folded into the per-(batch, channel)
 * affine in fp32 (s' = s*(1+f), t' = t*(1+f) + g) before the apply pass, so x is still read once and y written
 * once.  Statistics from part0 / part1 or a statistics pass, then the fold, then the apply pass at every level;
 * a->scale / a->shift are required and hold the folded affine afterwards. */
int sdk_group_norm_film(const sdk_group_norm_args* a, const float* film, int32_t film_ld, int32_t film_off,
                        int32_t silu, void* y, int32_t ld_y, int32_t h, int32_t w, int32_t pad, const float* part0,
                        int32_t nch0, const float* part1, int32_t nch1, sdk_stream_t stream);

/* GroupNorm apply (+ SiLU) + 2x resample with two outputs from one read of x — the resampling ResBlock
 * (`resblock_updown`, openai_model/model.py:233-238: h = h_upd(SiLU(GN(x))), x = x_upd(x)) and, with
 * a->scale == NULL, the stand-alone Downsample / Upsample of `conv_resample=False` (:91-97, :119-131).
 * mode: SDK_RESAMPLE_AVGPOOL2 = F.avg_pool2d(., 2) (odd h / w floor), SDK_RESAMPLE_NEAREST2 = nearest x2.
 * x = a->src0 (| a->src1 as a 2-source concat) [batch][h][w], a->scale / a->shift the per-(batch, channel)
 * affine (sdk_group_norm_finalize).  y_act = resample(silu?(x*scale + shift)) in a zero-bordered
 * [batch][ho+2pad][wo+2pad][channels] image (pooling averages the four activated values in fp32, rounded to
 * fp16 once); y_raw = resample(x), contiguous [batch][ho][wo][channels].  Either output may be NULL; y_act
 * needs the affine.  channels % 8 == 0 (else SDK_EINVAL), channels <= 4096. */
enum { SDK_RESAMPLE_AVGPOOL2 = 0, SDK_RESAMPLE_NEAREST2 = 1 };
int sdk_group_norm_resample(const sdk_group_norm_args* a, int32_t mode, int32_t silu, int32_t h, int32_t w,
                            int32_t pad, void* y_act, void* y_raw, sdk_stream_t stream);

/* Class-label embedding add (openai_model/model.py:568-570: emb = emb + label_emb(y)):
 * out[b][:] = fp16(float(emb[b][:]) + table[ids[b]][:]); emb / out fp16 [batch][dim], table fp32 [n][dim],
 * ids int64 [batch], dim % 8 == 0.  The table is never read outside [0, n): an id out of range writes NaN
 * into that whole row of out. */
int sdk_embedding_add(const void* emb, const float* table, const int64_t* ids, void* out, int32_t batch, int32_t dim,
                      int32_t n, sdk_stream_t stream);

/* ---------------------------------------------------------------- condition encoders (clip_encoder/modules.py)
 * Row gather of ClassEmbedder (clip_encoder/modules.py:37-45: embedding(batch[key][:, None])):
 * out[i][:] = fp16(table[ids[i]][:]); ids int64 [n], table fp32 [rows][dim], out fp16 [n][dim], any dim >= 1.
 * 16-byte accesses when dim % 8 == 0 and table / out are 16-byte aligned, scalar otherwise.  The caller
 * range-checks ids on the host (as for sdk_vq_lookup). */
int sdk_embedding_rows(const int64_t* ids, const float* table, void* out, int32_t n, int32_t dim,
                       sdk_stream_t stream);

/* SpatialRescaler's F.interpolate(x, scale_factor=s, mode=...) (clip_encoder/modules.py:197-205) on NCHW fp32
 * with torch's defaults: align_corners=False, no antialias, the given scale factor used for the coordinates
 * (source step (float)(1 / s)), out = floor(in * s) per axis (checked: any other out_h / out_w is
 * SDK_EINVAL).  x [planes][h][w] -> y [planes][out_h][out_w], planes = batch * channels.
 *   SDK_RESIZE_NEAREST   src = min(floor(dst * step), in - 1)                      (torch's legacy "nearest")
 *   SDK_RESIZE_BILINEAR  src = max(step * (dst + 0.5) - 0.5, 0); wy0*(wx0*p00 + wx1*p01) + wy1*(wx0*p10 + wx1*p11)
 *   SDK_RESIZE_BICUBIC   src = step * (dst + 0.5) - 0.5, A = -0.75, border taps clamped; rows combined as above
 *   SDK_RESIZE_AREA      adaptive average: rows [floor(o*in/out), ceil((o+1)*in/out)), sum / kh / kw
 * Weights, coordinates and sums in fp32 in the order torch's CPU kernels evaluate them, no contraction.
 * One thread per output element, consecutive lanes on consecutive output columns. */
enum { SDK_RESIZE_NEAREST = 0, SDK_RESIZE_BILINEAR = 1, SDK_RESIZE_BICUBIC = 2, SDK_RESIZE_AREA = 3 };
typedef struct {
  const float* x;
  float* y;
  int32_t planes, h, w, out_h, out_w, mode;
  double scale_h, scale_w;
} sdk_resize2d_args;

int sdk_resize2d(const sdk_resize2d_args* a, sdk_stream_t stream);

/* ---------------------------------------------------------------- introspection */
const char* sdk_last_error(void);
int sdk_version(void);
const char* sdk_kernel_name(int32_t variant);

#ifdef __cplusplus
}
#endif
#endif /* SDK_AMD_H */
