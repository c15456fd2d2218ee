/*
 * ldm_hip.h -- C ABI of libldm_hip.so: hand-written HIP kernels (gfx950 / MI355X)
 * for the latent-diffusion SAMPLING path of chao-ji/ldm_tf2.
 *
 * The reference has no FFI/plugin interface (it is pure Python on TensorFlow;
 * SURVEY.md section 8b), so this ABI is build-defined.  Each entry point names the
 * reference call site(s) whose arithmetic it replaces.  Conventions:
 *   - extern "C", plain pointers and sizes, no torch / C++ types;
 *   - every pointer is a DEVICE pointer unless it says "host";
 *   - the library never allocates, frees or synchronises; every kernel is
 *     enqueued on the caller's `stream` (a hipStream_t passed as void*), so the
 *     caller may capture any sequence of calls into a HIP graph;
 *   - return value: 0 = ok, negative = error (ldm_last_error() has the text);
 *   - activations are NHWC ("pixel rows" of C channels, explicit pixel stride
 *     `ld*` in ELEMENTS so a tensor may be a channel slice of a wider buffer:
 *     that is how the U-Net skip concatenation (unet.py:135) costs nothing);
 *   - dtype: 0 = float32, 1 = bfloat16 (storage; accumulation, statistics,
 *     softmax and the DDIM scheduler are always float32);
 *   - biases / gammas / betas / per-row addends are always float32.
 *
 * Why there is no opaque context (no ldm_create / ldm_destroy / *_sync): every entry point is
 * a pure function of its arguments that only ENQUEUES work on the caller's stream.  The library
 * owns no device memory (scratch such as the split-K workspace is passed in by the caller, who
 * therefore decides which stream / model it belongs to), keeps no per-call state (the only
 * mutable datum is the thread-local last-error string) and never synchronises, so there is
 * nothing for a handle to hold and nothing for a *_sync to wait on: the caller synchronises its
 * own stream.  Re-entrancy follows from that: concurrent calls on different streams are safe as
 * long as they do not share caller-owned scratch.  The library reads NO environment variable (the
 * timing ablations and A/B switches of the tools exist only in the separate tools build,
 * -DLDM_TOOLS_BUILD, which the product never loads).
 */
#ifndef LDM_HIP_H
#define LDM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LDM_F32 0
#define LDM_BF16 1

#define LDM_OK 0
#define LDM_ERR_ARG (-1)
#define LDM_ERR_LAUNCH (-2)
#define LDM_ERR_WORKSPACE (-3)

/* epilogue activations of ldm_gemm */
#define LDM_ACT_NONE 0
#define LDM_ACT_GELU 1  /* exact erf gelu: transformer.py:169 (tf.nn.gelu)        */
#define LDM_ACT_GEGLU 2 /* value*gelu(gate): unet.py:323-325; weight rows interleaved
                           in blocks of 64 = 32 value rows then their 32 gate rows.
                           Tile 0 (auto) and the LDM_TILE_GEGLU ones.  Takes no addend
                           (LDM_ERR_ARG).  On LDM_TILE_GEGLU_VEC tiles without split-K the output
                           must qualify for the 16-byte vector epilogue (out, bias and
                           residual 16-byte aligned, row pitches multiples of 8
                           elements), else LDM_ERR_ARG; the automatic plan (tile 0)
                           does not pick them for such a call                      */
#define LDM_ACT_SILU 3  /* unet.py:72 Dense(activation="silu")                     */

int ldm_version(void);
/* copies the calling thread's last error text into buf (host), returns its length */
int ldm_last_error(char* buf, int n);

/*
 * Dense / 1x1-conv / attention-projection GEMM and implicit-GEMM 3x3 convolution.
 *
 *   out[b][m][n] = act( alpha * sum_k A[b][m][k] * Wt[b][n][k] + bias[n]
 *                       + addend[(m / add_rows) * add_ld + n] ) + residual[b][m][n]
 *
 * A rows are K-contiguous; Wt is the weight matrix stored [N][K] (K contiguous),
 * i.e. the TRANSPOSE of the reference's Dense kernel [in,out] / the OHWI form of
 * its HWIO conv kernel -- the host re-lays weights out once at load time.
 *
 * conv = 1: A is gathered on the fly from an NHWC image [B][H][W][Cin] (pixel
 *   stride lda): m = (b, oy, ox) over [B][OH][OW], k = (kh, kw, ci) over 3x3xCin,
 *   source pixel (oy*stride + kh - 1, ox*stride + kw - 1), zero outside; with
 *   upsample = 1 the source image is first nearest-2x upsampled
 *   (src[i][j] = img[i/2][j/2]; 2H and 2W must then stay below 32768, H and W otherwise).
 *   upsample = 2 computes the same convolution over the upsampled image as four 2x2 "phase"
 *   convolutions over the image itself: output pixel (2i + a, 2j + b) is
 *     sum over dy, dx in {0,1}, ci of img[i - 1 + a + dy][j - 1 + b + dx][ci] * w[2a + b][n][(dy, dx, ci)],
 *   w being [4][N][K = 4*Cin] with the 3x3 taps that fall on one image pixel summed beforehand
 *   (layout.upsample_phase_kernel): 4/9 of the multiply-adds.  Stride 1; M = B*2H*2W as with
 *   upsample = 1; bias / addend / residual and split-K as ever; no a2, out2, ln_out, GEGLU;
 *   tiles with LDM_TILE_PHASE_BF16 / LDM_TILE_PHASE_F32 (ldm_gemm_tile_info).
 *   Cin must be a multiple of 128/sizeof(elem).
 *   Replaces: Conv2D 3x3 SAME (unet.py:22,40,71,375,378; autoencoder.py:32,35,
 *   148,275), pad(1,1)+stride-2 VALID (unet.py:26-27), ResizeNearestNeighbor+conv
 *   (unet.py:44-47, autoencoder.py:152-155).
 * conv = 0: plain rows.  Replaces Dense (unet.py:72-73,320,332,350,353,376,379;
 *   autoencoder.py:36,69-72; transformer.py:137-138), Projection einsums
 *   (transformer.py:68,70) and, batched, the materialised attention einsums of
 *   autoencoder.py:86,93.
 *
 * Output element (m, n) of batch b is stored at out + b*stride_c + m*ldc_m + n*ldc_n
 * (ldc_n = 1 for row-major; ldc_m = 1 gives the transposed store used for V^T).
 * With LDM_ACT_GEGLU the stored width is N/2.
 * split_k > 1 needs `workspace` >= split_k*M*N*4 bytes (batch must be 1); the f32 partial
 * slabs are reduced (+ epilogue) by a second small launch.  (An in-kernel "last block
 * reduces" fix-up was measured and rejected: on this multi-XCD part the agent-scope fence /
 * device-coherent accesses it needs cost far more than the launch it saves; DESIGN.md.)
 * One workspace serves one stream at a time.
 */
typedef struct {
  const void* a;
  const void* w;
  const float* bias;     /* [N] or NULL */
  const float* addend;   /* per-row-group addend or NULL (ResBlock temb: unet.py:386-388) */
  const void* residual;  /* same dtype as out, or NULL */
  void* out;
  void* workspace;
  size_t workspace_bytes;
  int64_t lda, ldr, ldc_m, ldc_n;
  int64_t stride_a, stride_w, stride_c, stride_r; /* per batch, elements */
  int64_t add_ld;        /* row stride of addend (0 = one row for all groups) */
  int32_t M, N, K, batch;
  int32_t add_rows;      /* rows of out per addend row (OH*OW) */
  int32_t conv, B, H, W, Cin, OH, OW, stride, upsample;
  int32_t act;
  int32_t dtype;         /* of a, w */
  int32_t out_dtype;     /* of out, residual */
  int32_t split_k;       /* 0 = let the library choose */
  int32_t tile;          /* 0 = auto; 1 .. ldm_gemm_tile_count() - 1 force a tile: ldm_gemm_tile_info tells its shape, family and what it accepts (on a persistent tile split_k < 0 sets the workgroups per row panel) */
  float alpha;
  /* conv: 0 = one zero row/column before the image (Keras SAME at stride 1; pad (1,1)+VALID at
   * stride 2, unet.py:26-27); 1 = none before, one after -- the autoencoder's
   * pad [[0,1],[0,1]] + stride-2 VALID downsample (autoencoder.py:133-136); stride 2 only. */
  int32_t no_lead_pad;
  /* Second output: LayerNormalization of the row just written (unet.py:309-313: every
   * residual-stream update of the BasicTransformerBlock is followed by a LayerNorm whose output
   * feeds the next projection).  ln_out[m][:] = LN(out[m][:]) * ln_gamma + ln_beta over all N
   * columns, computed from the values as stored (i.e. after rounding to out_dtype), same dtype
   * as out, row stride ld_ln.  Needs a tile that holds whole rows: plain rows, batch 1,
   * N == 320, row-major 16-byte-aligned output, no GEGLU (ldm_gemm_ln_supported).  NULL = off. */
  void* ln_out;
  const float* ln_gamma;
  const float* ln_beta;
  int64_t ld_ln;
  float ln_eps;
  /* Second, TRANSPOSED output for the columns n >= n_split (the self-attention q|k|v projection
   * in one launch: q|k row-major into `out`, v straight into the V^T layout the attention kernel
   * reads, unet.py:270-276): element (m, n) goes to
   *   out2 + (m / rows2) * stride2 + (n - n_split) * ld2 + (m % rows2)      (dtype of out).
   * n_split must be a multiple of 160 and 128 or the forced tile's width (every tile then lies on
   * one side), rows2 a multiple of 4; plain rows, batch 1, no split-K, no residual on that part.
   * NULL = off. */
  void* out2;
  int64_t ld2, stride2;
  int32_t n_split, rows2;
  /* LayerNormalization of the A ROWS folded into the product (unet.py:309-313: LN -> q|k / v / q /
   * GEGLU projections).  With w = bf16(gamma (.) W), bias = b + W beta and ln_cs[n] = sum_k w[n][k]
   * (all prepared by the host, float32 [N], 16-byte aligned),
   *     LN(a) W^T + b  =  rstd_m * (sum_k a[m][k] w[n][k]  -  mean_m * ln_cs[n]) + bias[n],
   * and the kernel derives mean_m / rstd_m (eps = ln_eps, biased variance over the K columns) from
   * the A tiles it stages anyway: no LayerNorm launch, no normalised copy of the rows.  bf16 plain
   * rows (conv = 0), batch 1, persistent tiles (chosen automatically), epilogues: bias,
   * bias + GEGLU, or the transposed store (out2 with n_split = 0).  NULL = off. */
  const float* ln_cs;
  /* Split-K only: 1 = leave the float32 partial slabs in `workspace` and do NOT launch the reduce.  The
   * caller completes the product later, on the same stream and with the SAME parameters, either with
   * ldm_gemm_reduce (the plain reduce + epilogue) or with ldm_groupnorm_splitk (reduce + epilogue +
   * the GroupNormalization that follows, one launch).  Ignored when the plan does not split K
   * (ldm_gemm_splits tells: the product is then complete when ldm_gemm returns). */
  int32_t defer_reduce;
  /* conv = 1, stride 1, no upsample: a SECOND A operand for the K columns beyond 9*Cin.  K = 9*Cin + Cin2 and
   *     out = conv3x3(a) . W[:, :9*Cin]^T  +  a2 . W[:, 9*Cin:]^T  (+ bias ...),
   * the extra columns being a 1x1 convolution over the NHWC image a2 [B][H][W][Cin2] (pixel stride lda2, dtype of
   * a) read at the output pixel.  The ResidualBlock's shortcut (unet.py:379-380, :393-397: a Dense over the block
   * input where the channel count changes, added to the second convolution's output) then accumulates inside that
   * convolution's K loop: no launch and no [M][Cout] tensor of its own; pass bias = conv bias + shortcut bias.
   * Cin2 a multiple of the K-tile (64 bf16 / 32 f32 elements); LDM_TILE_A2 tiles (not the
   * persistent or halo-staged ones); split-K, deferred reduce and every epilogue as without it.  NULL = off. */
  const void* a2;
  int64_t lda2;
  int32_t Cin2;
} ldm_gemm_params;

int ldm_gemm(const ldm_gemm_params* p, void* stream);
/* number of K slabs ldm_gemm writes for these parameters (1 = no split-K; host only) */
int ldm_gemm_splits(const ldm_gemm_params* p);
/* completes a product whose reduce was deferred (defer_reduce = 1): slabs -> bias / addend /
 * activation / residual -> out.  Same parameters as the ldm_gemm call. */
int ldm_gemm_reduce(const ldm_gemm_params* p, void* stream);
/*
 * Completes a deferred split-K product AND applies the GroupNormalization (+SiLU) that consumes it
 * (unet.py:383-392: conv -> GroupNorm -> SiLU -> conv), in ONE launch: a workgroup owns whole
 * groups of one sample, sums the slabs of its [HW][channels] slab (+ bias / per-sample addend /
 * residual, in the order of the plain reduce: the stored value is bit-identical), keeps the values
 * ROUNDED to the output dtype in registers, writes them to p->out when `store_out` (skip it when
 * nothing else reads the product: conv1 of a ResBlock) and writes GroupNorm(+SiLU) of them to
 * gn_out (pixel stride ld_gn, dtype of p->out).  p: the parameters of the deferred ldm_gemm call
 * (M = B*HW rows, N = C channels, row-major output, no activation, batch 1).  Shapes:
 * ldm_groupnorm_splitk_supported(B, HW, C, groups, out dtype).
 */
/* 1 if ldm_groupnorm_splitk supports this shape (host query; a subset of ldm_groupnorm_fused's) */
int ldm_groupnorm_splitk_supported(int B, int HW, int C, int groups, int dtype);
/* the launch form ldm_groupnorm_splitk runs for this shape (host query, the plan of the launch itself):
 * form[4] = {GB groups per workgroup, S 16-byte chunks per pixel, NT threads, MAXCH chunks per thread};
 * LDM_OK, or LDM_ERR_ARG when the shape is not supported (form untouched) */
int ldm_groupnorm_splitk_form(int B, int HW, int C, int groups, int dtype, int* form);
int ldm_groupnorm_splitk(const ldm_gemm_params* p, const float* gamma, const float* beta, void* gn_out,
                         int64_t ld_gn, int B, int HW, int groups, float eps, int silu, int store_out,
                         void* stream);
/* 1 if ldm_gemm accepts ln_out for a [M][N] output of this dtype (host query) */
int ldm_gemm_ln_supported(int N, int dtype);
/* the tile configuration and split-K factor ldm_gemm would pick for these params (host only;
 * nothing is launched) -- for tools and tests of the cost model */
int ldm_gemm_plan(const ldm_gemm_params* p, int* tile, int* split_k);
/* The tile table of ldm_gemm (host only): tiles 1 .. ldm_gemm_tile_count() - 1 exist (0 = auto). */
#define LDM_TILE_PERSISTENT 1     /* persistent ping-pong kernel: bf16, N % bn == 0, no split-K */
#define LDM_TILE_HALO 2           /* halo-staged A operand: bf16 stride-1 3x3 convolutions whose 256-row M-tile is whole
                                     lines of one image, W = 16 or 32 */
#define LDM_TILE_BF16_ONLY 4
#define LDM_TILE_GEGLU 8          /* applies LDM_ACT_GEGLU ... */
#define LDM_TILE_GEGLU_VEC 16     /* ... but unsplit only through the 16-byte vector epilogue */
#define LDM_TILE_PHASE_F32 32     /* runs the phase form (upsample = 2) on float32 */
#define LDM_TILE_PHASE_BF16 64    /* ... on bf16 */
#define LDM_TILE_FORCED 128       /* the automatic plan never picks it: forced by the caller (plan tables) only */
#define LDM_TILE_FORCED_BF16 256  /* the automatic plan picks it on float32 only */
#define LDM_TILE_EXPERIMENTAL 512 /* not meant for plan tables either */
#define LDM_TILE_A2 1024          /* takes a second A operand (a2) */
#define LDM_TILE_WHOLE_N 2048     /* the automatic plan takes it only where N % bn == 0 (160/320-column tiles) */
typedef struct {
  int32_t bm, bn;        /* rows and columns of an output tile */
  int32_t resident;      /* workgroups per CU */
  uint32_t flags;        /* LDM_TILE_* */
} ldm_gemm_tile;
int ldm_gemm_tile_count(void);
/* LDM_OK, or LDM_ERR_ARG for a tile outside 1 .. count - 1 */
int ldm_gemm_tile_info(int tile, ldm_gemm_tile* out);
/* bytes of workspace ldm_gemm may need for these params with split_k = 0 (auto) */
size_t ldm_gemm_workspace_bytes(const ldm_gemm_params* p);

/*
 * Small direct 3x3 SAME convolution for tiny channel counts (Cin <= 8 or Cout <= 8):
 * conv_in 4->C (unet.py:71, autoencoder.py:275) and conv_out C->4/3 (unet.py:116,
 * autoencoder.py:289).  x [B][H][W][Cin] dtype in_dtype (pixel stride ldx), kernel
 * HWIO float32, bias float32, out dtype out_dtype (pixel stride ldo).
 */
int ldm_conv3x3_small(const void* x, int64_t ldx, int in_dtype, const float* kernel_hwio,
                      const float* bias, void* out, int64_t ldo, int out_dtype,
                      int B, int H, int W, int Cin, int Cout, void* stream);

/*
 * GroupNormalization over NHWC (Keras semantics: biased variance over (H,W,C/G)),
 * optionally followed by SiLU.  Two launches:
 *   ldm_groupnorm_partial : per (b, chunk, g) sums of x - K and (x - K)^2 -> partial[B][nchunks][G][2]
 *                           float, K = x[b, pixel 0, g * C/G] (a shift: the one-pass variance then
 *                           does not cancel on groups whose mean is large against their spread)
 *   ldm_groupnorm_apply   : finalises mean/rstd from the same K, writes (x-mu)*rstd*gamma+beta [silu]
 * nchunks is chosen by the caller (ldm_groupnorm_nchunks gives the library's choice).
 * Replaces GroupNormalization(+tf.nn.silu): unet.py:115,137,354,374,377,383,390;
 * autoencoder.py:31,33,68,237,288.
 */
int ldm_groupnorm_nchunks(int B, int HW, int C);
int ldm_groupnorm_partial(const void* x, int64_t ldx, float* partial, int B, int HW, int C,
                          int groups, int nchunks, int dtype, void* stream);
int ldm_groupnorm_apply(const void* x, int64_t ldx, const float* partial, const float* gamma,
                        const float* beta, void* out, int64_t ldo, int B, int HW, int C,
                        int groups, int nchunks, float eps, int silu, int dtype, void* stream);
/* Single-launch variant for small images (every U-Net GroupNorm): one workgroup owns whole
 * groups of one sample and keeps its slab in registers between the passes, so x is read once
 * and written once, and the variance is the two-pass (centred) form.  _supported is a pure
 * host query; ldm_groupnorm_fused fails (LDM_ERR_ARG) on an unsupported shape. */
int ldm_groupnorm_fused_supported(int B, int HW, int C, int groups, int dtype);
/* the launch form ldm_groupnorm_fused runs for this shape (host query, the plan of the launch itself):
 * form[4] = {GB, S, NT, MAXCH} as ldm_groupnorm_splitk_form; LDM_OK, or LDM_ERR_ARG when the shape is not
 * supported (form untouched) */
int ldm_groupnorm_fused_form(int B, int HW, int C, int groups, int dtype, int* form);
int ldm_groupnorm_fused(const void* x, int64_t ldx, const float* gamma, const float* beta, void* out,
                        int64_t ldo, int B, int HW, int C, int groups, float eps, int silu, int dtype,
                        void* stream);
/* LayerNormalization over the last axis (unet.py:304-306; transformer.py:165,170,209). */
int ldm_layernorm(const void* x, int64_t ldx, const float* gamma, const float* beta, void* out,
                  int64_t ldo, int rows, int C, float eps, int dtype, void* stream);

/* Row softmax of a [rows][cols] matrix after scaling by `scale` (autoencoder.py:86-90:
 * einsum * C**-0.5 then softmax).  out may alias x when the dtypes are equal. */
int ldm_softmax_rows(const void* x, int64_t ldx, int in_dtype, void* out, int64_t ldo,
                     int out_dtype, int rows, int cols, float scale, void* stream);

/*
 * Fused multi-head attention, logits never materialised:
 *   out[b][q][h][:] = softmax_c( scale * q[b][q][h][:] . k[b][c][h][:] ) @ v[b][c][h][:]
 * q: [batch][Tq] rows of heads*Sp elements (row stride ldq), k likewise [batch][Tk];
 * vt: V transposed per head: [batch][heads][Sp][ldvt] with ldvt >= Tk keys contiguous and ldvt a
 *     multiple of 16 bytes; the padding columns [Tk, ldvt) are read in whole 16-byte chunks but
 *     masked to zero in the kernel: they need not be initialised (NaN / Inf there are harmless);
 * out: [batch][Tq] rows of heads*Sp (row stride ldo).  Sp = head size padded to a
 * multiple of 32 with zeros (the padding lives in the re-laid-out projection weights).
 * Replaces unet.py:280-287 and transformer.py:107-116 (scale applied AFTER q.k^T).
 */
int ldm_attention(const void* q, int64_t ldq, int64_t q_bs, const void* k, int64_t ldk,
                  int64_t k_bs, const void* vt, int64_t ldvt, int64_t vt_bs, void* out,
                  int64_t ldo, int64_t o_bs, int batch, int heads, int Tq, int Tk, int Sp,
                  float scale, int dtype, void* stream);

/*
 * The same attention for bf16 heads of 40 dims padded to Sp = 48, with the softmax bookkeeping moved
 * onto the matrix cores ("matrix-side softmax"): the caller's projections put the padding to work --
 *   q : already in the exp2 domain: the query projection's weights carry scale * log2(e) (so the
 *       scale is applied BEFORE q.k^T here; for bf16 that is a rounding-order difference);
 *       q[..][h][40..47] = 0
 *   k : k[..][h][40] = 1.0, k[..][h][41..47] = 0
 *   vt: row 40 of every head = 1.0 (rows 41..47 = 0); padding COLUMNS [Tk, ldvt) as for ldm_attention
 * The kernel writes -m (each query's reference point, kept a bf16 number) into dim 40 of its Q
 * fragments, so K.Q^T returns logit - m, and row 40 of V^T.P^T accumulates the softmax denominator from
 * the same bf16 P as the numerator.  out[..][h][40..47] = 0.  Same result as ldm_attention up to bf16
 * rounding (tests/test_round3_gpu.py); 2 of the 5 VALU operations per logit remain.
 */
int ldm_attention_ms(const void* q, int64_t ldq, int64_t q_bs, const void* k, int64_t ldk,
                     int64_t k_bs, const void* vt, int64_t ldvt, int64_t vt_bs, void* out,
                     int64_t ldo, int64_t o_bs, int batch, int heads, int Tq, int Tk, int Sp,
                     int dtype, void* stream);

/*
 * Fused feed-forward of the BasicTransformerBlock (unet.py:313, :323-325, :335-338) for bf16 rows of C = 320:
 *     out[m] = x[m] + b2 + W2 . ( a * gelu(g) ),   (a | g) = W1 . LayerNorm(x[m]) + b1
 * as ONE launch per 128-row panel: the panel's input rows stay resident in LDS (A operand of all hidden
 * chunks, source of the LayerNorm statistics, residual), the [M, 4C] hidden activation never leaves the CU,
 * only weights stream.  x: [M][C] bf16 (row stride ldx); w1: [8C][C] bf16, gamma-folded and
 * GEGLU-interleaved (layout.ln_fold of layout.geglu_kernel); aux: float32 [8C / 128][256]: per 128 rows of
 * w1 their column sums (128) then their folded bias (128); w2: [C][4C] bf16; b2: [C]; out: [M][C] bf16.
 * Same arithmetic as ldm_gemm(ln_cs, GEGLU) followed by ldm_gemm(residual) except that the hidden
 * activation is rounded to bf16 in LDS instead of HBM (identical rounding points).
 */
/* The same with the neighbouring products folded in (one launch for the tail of a SpatialTransformer block):
 *     h   = r0 + bo + Wo . att        cross-attention output projection + residual (unet.py:312; att [M][K0], K0 = 384)
 *     y   = feed-forward(h)           as above (h and y live only in LDS)
 *     out = r1 + bp + Wp . y          proj_out + the block's input as residual (unet.py:363-365)
 * wo [C][K0], wp [C][C] bf16 (K contiguous); r0, r1, out [M][C] bf16. */
int ldm_st_tail(const void* att, int64_t lda, int K0, const void* wo, const float* bo, const void* r0,
                int64_t ldr0, const void* w1, const float* aux, const void* w2, const float* b2,
                const void* wp, const float* bp, const void* r1, int64_t ldr1, void* out, int64_t ldo,
                int M, int C, float eps, int dtype, void* stream);
/* ldm_st_tail with the cross-attention itself in front (unet.py:273-291, :311): the input rows are the QUERY
 * projection q [M][K0] in ldm_attention_ms's layout (exp2-domain logits, 8 heads of 40 padded to 48); ctx_k
 * [R][Tk][K0] / ctx_vt [R][K0][ldv] are the context keys / values^T of the M / T samples in the same layout (Tk <= 80:
 * one key tile, plain softmax; T query rows per sample, a multiple of 128).  The attention runs in place in the LDS
 * panel, its output never reaches HBM. */
int ldm_st_xtail(const void* q, int64_t ldq, int K0, const void* ctx_k, const void* ctx_vt, int Tk, int ldv, int T,
                 const void* wo, const float* bo, const void* r0, int64_t ldr0, const void* w1, const float* aux,
                 const void* w2, const float* b2, const void* wp, const float* bp, const void* r1, int64_t ldr1,
                 void* out, int64_t ldo, int M, int C, float eps, int dtype, void* stream);
/* ... and with the block's middle in front of that (unet.py:310-311): the input rows are the SELF-attention's output
 * att [M][K0]; h1 = r0 + bo1 + Wo1 . att and the LayerNorm-folded query projection q = Wq . LayerNorm(h1) + bq (wq
 * [K0][C] gamma-folded with the attention scale * log2(e) and the padded rows of ldm_attention_ms's layout, qcs its
 * column sums, qb the folded bias: layout.ln_fold) run first; h1 is the residual of the second o-projection.  One
 * launch from the self-attention's output to the SpatialTransformer's output; `out` doubles as scratch for h1 and
 * must not alias an input.
 * `in_rows` (0 or M: off; else M / 2): att, r0 and r1 hold only the first in_rows rows and output row m >= in_rows
 * reads input row m - in_rows -- the classifier-free-guidance pair of the DDIM loop (model_runners.py:449-452 runs
 * the U-Net on concat([xt, xt]): in front of the first cross-attention both halves of the batch are the same
 * numbers, so the launches that feed this one ran once, on half the rows; ctx_k / ctx_vt cover all M / T samples). */
int ldm_st_block(const void* att, int64_t lda, int K0, const void* wo1, const float* bo1, const void* r0, int64_t ldr0,
                 const void* wq, const float* qcs, const float* qb, const void* ctx_k, const void* ctx_vt, int Tk,
                 int ldv, int T, const void* wo2, const float* bo2, const void* w1, const float* aux, const void* w2,
                 const float* b2, const void* wp, const float* bp, const void* r1, int64_t ldr1, void* out, int64_t ldo,
                 int M, int in_rows, int C, float eps, int dtype, void* stream);
int ldm_ffn_geglu_supported(int M, int C, int dtype);
int ldm_ffn_geglu(const void* x, int64_t ldx, const void* w1, const float* aux, const void* w2,
                  const float* b2, void* out, int64_t ldo, int M, int C, float eps, int dtype, void* stream);

/* Sinusoidal timestep embedding, cos first (unet.py:401-422): out[r][0:half]=cos(t*f),
 * out[r][half:]=sin(t*f), f_k = exp(-ln(10000)*k/half), float32.  t is read from
 * steps[*index] when `index` != NULL (device-resident DDIM index, graph replay) else
 * from t_rows[r]. */
int ldm_time_embedding(const int32_t* t_rows, const int32_t* steps, const int32_t* index,
                       float* out, int rows, int channels, void* stream);

/* y[r][n] = act_out( sum_k act_in(x[r][k]) * Wt[n][k] + bias[n] ), all float32 except Wt
 * (dtype).  Skinny (rows <= 64) Dense used for the timestep MLP and the 22 ResBlock
 * temb projections (unet.py:72-73,127,386).  act_*: LDM_ACT_NONE / LDM_ACT_SILU. */
int ldm_gemv(const float* x, int64_t ldx, const void* wt, const float* bias, float* y,
             int64_t ldy, int rows, int N, int K, int act_in, int act_out, int dtype,
             void* stream);

/* out[0:cols] = table[i][0:cols] with i = *index, float32; `pre_decrement` != 0: i = --(*index) first.  The DDIM
 * loop (model_runners.py:484-502) evaluates the timestep embedding, its MLP and the 22 ResBlock temb projections
 * (unet.py:125-127, :386) -- functions of the step's t alone -- for ALL its steps once (a [N_steps][sum Cout] table)
 * and each replayed step selects its row here; the same launch moves the device-resident loop counter (one
 * workgroup: no launch may read *index while another moves it), so the step needs no decrement of its own. */
int ldm_select_row(const float* table, int64_t ld, int rows, int cols, int32_t* index, int pre_decrement, float* out,
                   void* stream);

/*
 * Classifier-free guidance + DDIM update, float32 (model_runners.py:451-468):
 *   eps = eps_u + s*(eps_c - eps_u); x0 = c1*xt - c2*eps; mean = sqrt(a_prev)*x0
 *   + sqrt(1 - a_prev - sigma^2)*eps; xt' = mean + noise*sigma.
 * eps_all [2B][n] (uncond rows first), xt/xt_out [B][n]; noise (may be NULL when
 * sigma = 0) is read at noise + (*index) * noise_index_stride, i.e. a [N_steps][B][n]
 * table indexed by the DDIM index (stride 0 = one [B][n] buffer).
 * coef = device table [N_steps][4] of float32 (c1, c2, a_prev, sigma) gathered at
 * *index (the `_extract` cast-then-gather, :41-44).  If `dec_index` != 0 *index is
 * decremented afterwards (device-side loop counter for graph replay).
 * pred_x0_out (optional) receives x0 (:455-460, `return_pred_x0`).
 * x_unet_out (optional, dtype x_dtype) receives concat([xt', xt']) for the next step
 * (:452) so the next U-Net call reads it directly.
 */
int ldm_cfg_ddim_update(const float* eps_all, const float* xt, const float* noise,
                        int64_t noise_index_stride, float* xt_out, float* pred_x0_out,
                        void* x_unet_out, int x_dtype, const float* coef, int32_t* index,
                        int dec_index, float guidance_scale, int clip_denoised, int B,
                        int64_t n_per_sample, void* stream);

/*
 * ldm_cfg_ddim_update + masked inpainting (img2img; CompVis DDIMSampler's mask / x0 convention, 1 = keep).
 * Same arguments and arithmetic as ldm_cfg_ddim_update; then, with idx = *index read like it and idx >= 1,
 * the output is blended for the NEXT step (DDIM index j = idx - 1) before it is written to xt_out and to both
 * halves of x_unet_out:
 *   o <- m * (q_coef[j][0] * z0 + q_coef[j][1] * Q[j]) + (1 - m) * o
 * i.e. m * q_sample(z0, steps[j], Q[j]) + (1 - m) * o (model_runners.py:580-600, LatentDiffusionModelTrainer.
 * q_sample).  At idx = 0 nothing is blended (that output is decoded as it is) and no table is read at -1.
 * z0 [B][n]; mask [B][n / channels] float32, broadcast over the channels; Q row j at q_noise + j * q_index_stride;
 * q_coef = device table [N_steps][2] of float32 (sqrt_ac, sqrt_1m_ac) at steps[j] (the `_extract` cast-then-
 * gather, :41-44).  One launch, like the unmasked entry: the blend adds no launch to a step.
 */
int ldm_cfg_ddim_update_masked(const float* eps_all, const float* xt, const float* noise,
                               int64_t noise_index_stride, float* xt_out, float* pred_x0_out,
                               void* x_unet_out, int x_dtype, const float* coef, int32_t* index,
                               int dec_index, float guidance_scale, int clip_denoised, int B,
                               int64_t n_per_sample, const float* z0, const float* mask,
                               const float* q_noise, int64_t q_index_stride, const float* q_coef,
                               int channels, void* stream);

/*
 * Classifier-free guidance + PLMS update (pseudo linear multistep, Liu et al. 2022), float32:
 * the sigma = 0 update of ldm_cfg_ddim_update with eps replaced by an Adams-Bashforth combination of the last
 * guided eps of THIS loop.  With idx = *index, st = *start (the DDIM index of the loop's first step) and
 * j = clamp(st - idx, 0, 3) earlier steps:
 *   e_i = eps_u + s*(eps_c - eps_u)                                  (what the ring stores)
 *   j=0: e' = e_i                     j=1: e' = (3 e_i - e_{i+1}) / 2
 *   j=2: e' = (23 e_i - 16 e_{i+1} + 5 e_{i+2}) / 12
 *   j=3: e' = (55 e_i - 59 e_{i+1} + 37 e_{i+2} - 9 e_{i+3}) / 24   (model_runners.PLMS_WEIGHTS)
 *   x0 = c1*xt - c2*e'; xt' = sqrt(a_prev)*x0 + sqrt(1 - a_prev)*e'; pred_x0_out (optional) receives x0.
 * ring = caller-owned [4][B][n] float32: e_i is stored to slot idx & 3 and slots (idx+1 .. idx+j) & 3 are read.
 * A slot beyond j is NOT read (not multiplied by zero): the ring may start uninitialised or hold another loop's
 * values.  The slot follows from idx alone, so a captured graph serves any start index.  ring must not alias
 * any other argument.  coef as in ldm_cfg_ddim_update (its sigma column is not read: PLMS is deterministic);
 * there is no clip_denoised.  eps_all, xt, xt_out, x_unet_out, dec_index as in ldm_cfg_ddim_update.
 * Masked blend (z0 != NULL; then mask, q_noise, q_coef are required): exactly that of
 * ldm_cfg_ddim_update_masked, applied to xt' for idx >= 1 and skipped at idx = 0; the ring and pred_x0_out keep
 * the unblended step's values.  z0 = NULL: no blend, the five blend arguments are ignored.
 * Every access is 16 bytes wide: n_per_sample must be a multiple of 4 (true for 4 latent channels) and every
 * float32 array 16-byte aligned (x_unet_out 8-byte when bf16); other calls are rejected with LDM_ERR_ARG,
 * there is no scalar path.
 */
int ldm_cfg_plms_update(const float* eps_all, const float* xt, float* ring, float* xt_out, float* pred_x0_out,
                        void* x_unet_out, int x_dtype, const float* coef, int32_t* index, const int32_t* start,
                        int dec_index, float guidance_scale, int B, int64_t n_per_sample, const float* z0,
                        const float* mask, const float* q_noise, int64_t q_index_stride, const float* q_coef,
                        int channels, void* stream);

/*
 * Forward diffusion (model_runners.py:580-600, LatentDiffusionModelTrainer.q_sample):
 *   xt[b] = sqrt_ac[t[b]] * x0[b] + sqrt_1m_ac[t[b]] * noise[b], float32.
 * x0 / noise / xt_out [B][n]; t int32 [B] on the device (DDPM timesteps, clamped to [0, num_steps)); the two
 * tables [num_steps] are the float32 casts of sqrt(abar) and sqrt(1 - abar) (:389-390, `_extract` casts then
 * gathers).  noise is read at noise + (*index) * noise_index_stride when `index` is non-NULL (a [N][B][n] table
 * indexed by a device-resident DDIM index), else at noise.  x_unet_out (optional, dtype x_dtype) receives
 * concat([xt, xt]), the U-Net input of an img2img loop's first step.
 */
int ldm_q_sample(const float* x0, const float* noise, int64_t noise_index_stride, const int32_t* index,
                 const int32_t* t, const float* sqrt_alphas_cumprod, const float* sqrt_one_minus_alphas_cumprod,
                 int num_steps, float* xt_out, void* x_unet_out, int x_dtype, int B, int64_t n_per_sample,
                 void* stream);

/*
 * Sampling noise drawn on the device.  Generator: Philox4x32-10 (Salmon et al., SC'11).
 * rng = uint32[4] on the device, {seed & 0xffffffff, seed >> 32, first_sample_index, 0}: the first two words are
 * the key, read through the pointer by every kernel below (a new seed or shard offset changes no kernel argument).
 * The words of elements 4q .. 4q+3 of sample b ([h][w][c] flattened) in stream s are Philox of the counter
 * (q, first_sample_index + b, s, 0).  Word x -> u = ((x >> 8) + 0.5) * 2^-24; the four normals are
 * r0 cos(2 pi u1), r0 sin(2 pi u1), r2 cos(2 pi u3), r2 sin(2 pi u3) with r = sqrt(-2 ln u): |z| <= 5.887.
 * Stream words (model_runners.XT_STREAM, ETA_STREAM, ENCODE_STREAM, Q_STREAM): x_T; eta noise of DDIM index i at
 * ETA + i; the posterior noise of get_latents; forward-diffusion noise Q[i] at Q + i.  Disjoint for i < 2^29.
 * Every access is 16 bytes wide: n_per_sample must be a multiple of 4 and every float32 / uint32 array 16-byte
 * aligned (x_unet_out 8-byte when bf16); other calls are rejected with LDM_ERR_ARG, there is no scalar path.
 */
#define LDM_RNG_XT_STREAM 0u
#define LDM_RNG_ETA_STREAM (1u << 29)
#define LDM_RNG_ENCODE_STREAM (1u << 30)
#define LDM_RNG_Q_STREAM ((1u << 30) + 1u)

/* out [B][n] uint32 = the raw Philox words of stream `stream_word` (the integer part of the generator, exact). */
int ldm_philox_u32(uint32_t* out, const uint32_t* rng, uint32_t stream_word, int B, int64_t n_per_sample,
                   void* stream);

/* out [B][n] float32 = the normals of stream `stream_word`; x_unet_out (optional, dtype x_dtype) receives
 * concat([out, out]).  x_T (LDM_RNG_XT_STREAM, with the first U-Net input), the posterior noise of get_latents
 * (LDM_RNG_ENCODE_STREAM), and one row of a noise table the entries above can read. */
int ldm_normal_fill(float* out, const uint32_t* rng, uint32_t stream_word, int B, int64_t n_per_sample,
                    void* x_unet_out, int x_dtype, void* stream);

/* ldm_q_sample with `noise` = the normals of stream `stream_word` (a host value: LDM_RNG_Q_STREAM + k - 1 for the
 * start latent of an img2img loop at DDIM index k - 1), drawn in the kernel.  Other arguments as in ldm_q_sample. */
int ldm_q_sample_rng(const float* x0, const uint32_t* rng, uint32_t stream_word, const int32_t* t,
                     const float* sqrt_alphas_cumprod, const float* sqrt_one_minus_alphas_cumprod, int num_steps,
                     float* xt_out, void* x_unet_out, int x_dtype, int B, int64_t n_per_sample, void* stream);

/*
 * ldm_cfg_ddim_update and ldm_cfg_ddim_update_masked behind one entry, without their tables: with idx = *index,
 * `noise` is the normals of stream LDM_RNG_ETA_STREAM + idx (not drawn when sigma = coef[idx][3] is 0) and the
 * blend's Q[idx - 1] those of stream LDM_RNG_Q_STREAM + idx - 1 (nothing is drawn at idx = 0), both formed in
 * registers by the one launch.  z0 = NULL: no blend, mask / q_coef / channels are ignored.  clip_denoised,
 * pred_x0_out, x_unet_out and dec_index as in ldm_cfg_ddim_update; same arithmetic, four elements per thread.
 */
int ldm_cfg_ddim_update_rng(const float* eps_all, const float* xt, const uint32_t* rng, float* xt_out,
                            float* pred_x0_out, void* x_unet_out, int x_dtype, const float* coef, int32_t* index,
                            int dec_index, float guidance_scale, int clip_denoised, int B, int64_t n_per_sample,
                            const float* z0, const float* mask, const float* q_coef, int channels, void* stream);

/* ldm_cfg_plms_update with the blend's Q[idx - 1] drawn like that (PLMS has no eta noise); z0 = NULL: no blend,
 * nothing is drawn.  The ring rules are those of ldm_cfg_plms_update. */
int ldm_cfg_plms_update_rng(const float* eps_all, const float* xt, float* ring, float* xt_out, float* pred_x0_out,
                            void* x_unet_out, int x_dtype, const float* coef, int32_t* index, const int32_t* start,
                            const uint32_t* rng, int dec_index, float guidance_scale, int B, int64_t n_per_sample,
                            const float* z0, const float* mask, const float* q_coef, int channels, void* stream);

/*
 * Classifier-free guidance + table-weighted multistep update (sampler="deis"), float32:
 * ldm_cfg_plms_update with the four Adams-Bashforth rows replaced by rows of a device table, so the weights can
 * follow the step table actually walked.  With idx = *index, st = *start and j = clamp(st - idx, 0, 3):
 *   w   = weights + idx * weights_pitch + 4 * j            (float32; entries 0 .. j are read, the others never)
 *   e'  = w[0] e_i, then e' = fma(w[m], e_{i+m}, e') for m = 1 .. j          (this order, explicit fmas)
 *   x0 = c1*xt - c2*e'; xt' = sqrt(a_prev)*x0 + sqrt(1 - a_prev)*e'; pred_x0_out (optional) receives x0.
 * weights = [N_steps][4][4] floats with weights_pitch (>= 16) floats between the rows of consecutive indices; the
 * kernel reads it through launch-uniform addresses.  Ring, start, blend, alignment and dec_index rules are those of
 * ldm_cfg_plms_update: slots beyond j are not read, n_per_sample % 4 != 0 or a misaligned array is LDM_ERR_ARG.
 */
int ldm_cfg_ms_update(const float* eps_all, const float* xt, float* ring, float* xt_out, float* pred_x0_out,
                      void* x_unet_out, int x_dtype, const float* coef, int32_t* index, const int32_t* start,
                      const float* weights, int64_t weights_pitch, int dec_index, float guidance_scale, int B,
                      int64_t n_per_sample, const float* z0, const float* mask, const float* q_noise,
                      int64_t q_index_stride, const float* q_coef, int channels, void* stream);

/* ldm_cfg_ms_update with the blend's Q[idx - 1] drawn from stream LDM_RNG_Q_STREAM + idx - 1, as
 * ldm_cfg_plms_update_rng does; z0 = NULL: no blend, nothing is drawn. */
int ldm_cfg_ms_update_rng(const float* eps_all, const float* xt, float* ring, float* xt_out, float* pred_x0_out,
                          void* x_unet_out, int x_dtype, const float* coef, int32_t* index, const int32_t* start,
                          const float* weights, int64_t weights_pitch, const uint32_t* rng, int dec_index,
                          float guidance_scale, int B, int64_t n_per_sample, const float* z0, const float* mask,
                          const float* q_coef, int channels, void* stream);

/*
 * Guidance schedule, float32: ldm_cfg_ms_update with the guidance scale read from a device
 * table and a conditional-only form.  With idx = *index:
 *   guided != 0:  e_i = eps_u + gtab[idx] * (eps_c - eps_u)      (gtab float32 [N_steps], a launch-uniform address:
 *                                                                 one captured launch serves every schedule)
 *   guided == 0:  e_i = eps_c, the second half of eps_all [2B][n]; the first half is NOT read (the conditional-only
 *                 U-Net evaluation leaves it unwritten) and gtab[idx] is not read either.
 * weights != NULL: e_i enters the ring and e' is the weighted sum of ldm_cfg_ms_update (ring, start, weights and
 * weights_pitch as there; the PLMS constants as a table give PLMS).  weights == NULL: e' = e_i, the DDIM step at
 * sigma = 0; ring and start may be NULL and are not touched.  x0 = c1*xt - c2*e'; xt' = sqrt(a_prev)*x0 +
 * sqrt(1 - a_prev)*e'.  x_unet_out (optional) always receives both halves concat([xt', xt']), whichever form ran, so
 * the next step may take either.  rng != NULL: the blend's Q[idx - 1] is drawn from stream LDM_RNG_Q_STREAM + idx - 1
 * (q_noise is ignored); rng == NULL: read from q_noise.  z0 = NULL: no blend.  Alignment, n_per_sample % 4 and
 * dec_index rules are those of ldm_cfg_ms_update.
 */
int ldm_cfg_sched_update(const float* eps_all, const float* xt, float* ring, float* xt_out, float* pred_x0_out,
                         void* x_unet_out, int x_dtype, const float* coef, const float* gtab, int32_t* index,
                         const int32_t* start, const float* weights, int64_t weights_pitch, const uint32_t* rng,
                         int guided, int dec_index, int B, int64_t n_per_sample, const float* z0, const float* mask,
                         const float* q_noise, int64_t q_index_stride, const float* q_coef, int channels,
                         void* stream);

/*
 * DDIM inversion, float32: the deterministic DDIM step run upwards.  coef row idx = *index is
 * (c1, c2, a_prev, sigma) as above; xt is on the level of a_prev and the result on the level of steps[idx]:
 *   guided != 0:  e = eps_u + guidance_scale * (eps_c - eps_u)
 *   guided == 0:  e = eps_c, the second half of eps_all [2B][n]; the first half is NOT read (the conditional-only
 *                 U-Net evaluation leaves it unwritten) and guidance_scale is ignored
 *   x0  = (xt - sqrtf(1 - a_prev) * e) / sqrtf(a_prev)
 *   xt' = (x0 + c2 * e) / c1
 * which undoes the sigma = 0 step of ldm_cfg_ddim_update given the same e.  sigma is not read: no noise, no clip, no
 * blend, no history.  xt_out (may be xt) receives xt', pred_x0_out (optional) x0, x_unet_out (optional) both halves
 * concat([xt', xt']) in x_dtype.  The entry does not know which way its caller walks the table: it reads row *index
 * and, with dec_index, decrements *index afterwards like every other update, so a caller that counts down hands in the
 * table reversed (model_runners.py does).  n_per_sample % 4 == 0 and 16-byte aligned arrays (8-byte for a bf16
 * x_unet_out), as ldm_cfg_ms_update.
 */
int ldm_cfg_ddim_invert_update(const float* eps_all, const float* xt, float* xt_out, float* pred_x0_out,
                               void* x_unet_out, int x_dtype, const float* coef, int32_t* index, int guided,
                               int dec_index, float guidance_scale, int B, int64_t n_per_sample, void* stream);

/*
 * Panorama sampling.  A canvas [B][H][W][c] float32 is covered by nW = nY * nX windows of
 * h x w at stride (sy, sx).  Along an axis of extent L with window l and stride s (1 <= l <= L, 1 <= s <= l):
 *   n = ceil((L - l) / s) + 1,  origin_i = min(i * s, L - l)    (the last window is clamped to the edge);
 * window k = ky * nX + kx has origin (oy[ky], ox[kx]).  Both entries compute the origins in the kernel from
 * (H, h, sy) and (W, w, sx): there is no device table.
 *
 * ldm_window_gather: x_win [2][B][nW][h][w][c] in x_dtype, x_win[half][b][k][y][x][:] =
 * canvas[b][oy + y][ox + x][:] for both halves (the U-Net's [uncond ; cond] rows carry the same x); a bf16 value is
 * the round-to-nearest-even conversion the update entries' x_unet_out takes.
 *
 * ldm_window_fold: eps_win [halves][B][nW][h][w][c] float32 -> eps_canvas [halves][B][H][W][c] float32, halves 1 or
 * 2: eps_canvas[..][y][x][ch] = (sum of eps_win over the windows covering (y, x)) / count, the sum in float32 in
 * ascending k starting from the first covering value, the division by (float)count correctly rounded.  A thread owns
 * a canvas pixel and reads its windows: no atomics, the result is deterministic; count = 1 copies the bits.
 *
 * c % 4 == 0 with 16-byte aligned pointers (8-byte for a bf16 x_win) moves one channel quad per thread in 16-byte
 * accesses; any other c >= 1, or a pointer aligned to its element only, takes an element-wise path with the same
 * results.  LDM_ERR_ARG: a null pointer, a bad dtype or halves, B, c < 1, h > H, w > W, or a stride outside [1, window].
 */
int ldm_window_gather(const float* canvas, void* x_win, int x_dtype, int B, int H, int W, int c, int h, int w, int sy,
                      int sx, void* stream);
int ldm_window_fold(const float* eps_win, float* eps_canvas, int halves, int B, int H, int W, int c, int h, int w,
                    int sy, int sx, void* stream);

/*
 * Seamless panoramas: the pair above with a wrap flag per axis (0 or 1) and a weighted fold.
 * An unwrapped axis is the grid above.  A wrapped axis of extent L with window l and stride s has
 *   n = ceil(L / s),  origin_i = i * s    (no clamp),
 * and window i covers the cells (origin_i + j) mod L, j = 0 .. l - 1: the windows near the end cross the edge and
 * come back on the other side.  Window order stays k = ky * nX + kx.
 *
 * ldm_window_gather_ex: ldm_window_gather with the source row and column taken modulo the extent on a wrapped axis;
 * with both flags 0 the same bits as ldm_window_gather.
 *
 * ldm_window_fold_ex: wy [h] and wx [w] are float32 device tables of positive window-profile weights, the window
 * element (jy, jx) weighing ww = wy[jy] * wx[jx].  Per canvas element, over the covering windows in ascending k and
 * starting from the first covering term: num += ww * v, den += ww, out = num / den -- every product, sum and the
 * division a float32 operation rounded once, nothing fused; no atomics.  Both tables NULL: uniform weights, the sum
 * of the values over the count (ldm_window_fold's arithmetic and, when no axis wraps, its bits); a table of ones gives
 * the bits of NULL.  One NULL and one non-NULL table is an error.  On a wrapped axis the windows covering position p
 * are the i with i s <= p < i s + l followed by the i < n with p + L < i s + l.
 *
 * Paths and rejections as ldm_window_gather / ldm_window_fold; also LDM_ERR_ARG: a wrap flag that is not 0 or 1.
 */
int ldm_window_gather_ex(const float* canvas, void* x_win, int x_dtype, int B, int H, int W, int c, int h, int w,
                         int sy, int sx, int wrap_y, int wrap_x, void* stream);
int ldm_window_fold_ex(const float* eps_win, float* eps_canvas, int halves, int B, int H, int W, int c, int h, int w,
                       int sy, int sx, int wrap_y, int wrap_x, const float* wy, const float* wx, void* stream);

/*
 * Circular padding for the wrapped decode: x [B][H][W][c] float32 -> out [B][H + 2 py]
 * [W + 2 px][c] float32, out[b][y][x][:] = x[b][(y - py) mod H][(x - px) mod W][:].  0 <= py <= H, 0 <= px <= W
 * (else LDM_ERR_ARG, as a null pointer or an extent, B or c below 1); py = px = 0 copies.  The two paths of the
 * entries above (channel quads when c % 4 == 0 and both pointers are 16-byte aligned, else element-wise).
 */
int ldm_wrap_pad_nhwc(const float* x, float* out, int B, int H, int W, int c, int py, int px, void* stream);

/*
 * Latent resize: x [B][H][W][c] float32 -> out [B][Ho][Wo][c] float32, enlarging or shrinking,
 * no antialiasing.  Per axis, with source extent L, output extent Lo and output index i:
 *   LDM_RESIZE_NEAREST:  the source index min((i * L) / Lo, L - 1) in integer arithmetic (i / 2 at 2x); the output is
 *                        a copy of the source bits.
 *   LDM_RESIZE_BILINEAR: s = max((i + 0.5) L / Lo - 0.5, 0), i0 = floor(s), f = s - i0; taps min(i0, L - 1) and
 *                        min(i0 + 1, L - 1) with the weights 1 - f and f.
 *   LDM_RESIZE_BICUBIC:  s = (i + 0.5) L / Lo - 0.5, i0 = floor(s), f = s - i0; taps clamp(i0 - 1 .. i0 + 2, 0, L - 1)
 *                        with the weights of Keys' kernel, a = -0.75, at the distances f + 1, f, 1 - f, 2 - f.
 * These are the align_corners = False rules.  s is formed exactly, as the integer (2 i + 1) L - Lo over 2 Lo, and f by
 * one correctly rounded float32 division; the weights and the sum over the tap grid of wy * wx * x (rows outermost,
 * acc = fma(wy * wx, x, acc) in both paths) are float32.  Taps and weights are computed in the kernel from (L, Lo, i): there is no device table.  A thread owns
 * an output pixel: no atomics, the result is deterministic.  Ho == H && Wo == W copies the bits in every mode.
 *
 * c % 4 == 0 with 16-byte aligned pointers moves one channel quad per thread in 16-byte accesses; any other c >= 1,
 * or a pointer aligned to its element only, takes an element-wise path with the same results.  LDM_ERR_ARG: a null
 * pointer, an unknown mode, or an extent, B or c below 1.
 */
#define LDM_RESIZE_NEAREST 0
#define LDM_RESIZE_BILINEAR 1
#define LDM_RESIZE_BICUBIC 2
int ldm_resize_nhwc(const float* x, float* out, int B, int H, int W, int c, int Ho, int Wo, int mode, void* stream);

/*
 * Antialiased resample: x [B][H][W][c] float32 -> out [B][Ho][Wo][c] float32 with a filter
 * whose footprint grows with the shrink factor (the rule of PIL's Image.resize and of torch's antialias=True), in two
 * launches: along W into tmp [B][H][Wo][c] float32 (scratch of the caller), then along H into out.  The caller hands
 * in one table per axis (ldm_tf2_amd/resample.py builds them on the host in float64, rounded once to float32): for
 * an axis of source extent L and output extent Lo, start int32 [Lo] and w float32 [Lo][taps]; output index i reads the
 * source indices start[i] .. start[i] + taps - 1 with the weights w[i][0 .. taps).  Every row must lie inside [0, L):
 * 0 <= start[i] <= L - taps; rows with fewer taps are zero-filled.  The kernels do not check the table's contents.
 * Per output element acc = fma(w[i][j], x_j, acc) for ascending j from acc = 0, float32, the same chain in both
 * paths below; taps == 1 (an identity table: every weight is 1) copies the source bits.  A thread owns an output
 * element: no atomics, the result is deterministic.
 *
 * c % 4 == 0 with x, tmp and out 16-byte aligned moves one channel quad per thread in 16-byte accesses; any other
 * c >= 1, or a pointer aligned to its element only, takes an element-wise path with the same bits.  LDM_ERR_ARG: a
 * null pointer, an extent, B or c below 1, or taps below 1 or above the axis's source extent; nothing is launched.
 */
int ldm_resample_nhwc(const float* x, float* tmp, float* out, int B, int H, int W, int c, int Ho, int Wo,
                      const int32_t* xstart, const float* xw, int xtaps, const int32_t* ystart, const float* yw,
                      int ytaps, void* stream);

/*
 * Latent previews: small RGB pictures of one or two latent tensors, written into a strip of
 * frames whose slot a device-resident index selects, so that the launch can sit inside a captured sampling step.
 *   lat_a, lat_b [B][h][w][c] float32 (lat_b may be NULL); proj [c + 1][3] float32: c weight rows, then the bias row;
 *   frames_a, frames_b [R][B][s h][s w][3] uint8, s = scale (frames_b NULL exactly when lat_b is).
 * Slot rule: idx = (index ? *index : 0) + index_bias.  idx < 0, idx % freq != 0 or idx / freq >= R: the launch writes
 * nothing at all.  Otherwise it writes slot r = idx / freq, and that slot alone, of every source present.
 * Per output byte k of pixel (y, x): for j = 0 .. c-1 in turn a_j = the latent channel j enlarged s times at (y, x) --
 * LDM_PREVIEW_NEAREST: lat[y / s][x / s][j]; LDM_PREVIEW_BILINEAR: the taps, clamps and fractions of LDM_RESIZE_BILINEAR
 * at Lo = s L, a_j = fma(wy wx, lat, a_j) from 0, rows outermost -- and v_k = fma(a_j, proj[j][k], v_k) from v_k =
 * proj[c][k]; t = fma(127.5, v_k, 127.5); the byte is floor(min(max(t, 0), 255) + 0.5), a NaN giving 0 through the max.
 * All float32.  scale 1 is the nearest rule in both modes (the weights are 1 and 0).
 *
 * A thread owns four consecutive pixels of the slot's flat pixel run (12 bytes): three dword stores where the slot's
 * first byte is 4-byte aligned, byte stores otherwise and for a last partial group, the same bytes either way.  No
 * atomics, no tables: the result is deterministic.  c = 4 and c = 3 keep proj in registers; any other c reads it in the
 * channel loop.  LDM_ERR_ARG, nothing launched: a null lat_a, proj or frames_a; one of lat_b and frames_b without the
 * other; an unknown mode; c or scale outside 1..16; freq or R below 1; B, h or w below 1.
 */
#define LDM_PREVIEW_NEAREST 0
#define LDM_PREVIEW_BILINEAR 1
int ldm_latent_preview(const float* lat_a, const float* lat_b, const float* proj, uint8_t* frames_a, uint8_t* frames_b,
                       const int32_t* index, int index_bias, int freq, int R, int B, int h, int w, int c, int scale,
                       int mode, void* stream);

/*
 * Cross-attention heat maps: the head-averaged softmax probabilities of the queries q against
 * the keys k, weighted and ADDED into acc, so that a captured sampling step can collect the maps the flash attention
 * kernels keep in registers.
 *   q [R][T][heads*sp] (row stride ldq, batch stride q_bs, elements), k [R][Tk][heads*sp] (ldk, k_bs), both `dtype`;
 *   acc [R][T][Tk] float32, contiguous, read-modify-write; S = the true head size, sp = the padded head stride.
 * Per (r, t), heads in ascending order: l[j] = log2_scale * sum_{d<S} q[r][t][h sp + d] k[r][j][h sp + d] (one fma
 * chain over d ascending; the dims d in [S, sp) never enter it, whatever they hold -- the matrix-softmax layout keeps a
 * 1 in k's dim 40), e[j] = exp2(l[j] - max_j l[j]), p[j] = e[j] * rcp(sum_j e[j]), hs[j] += p[j]; then
 * acc[r][t][j] = fma(w, hs[j] * (1 / heads), acc[r][t][j]).  All float32, hardware exp2 and reciprocal.  A query
 * projection already scaled into the exp2 domain passes log2_scale = 1, a plain one S^-1/2 log2(e).
 * The weight: idx = (index ? *index : 0) + index_bias; w = step_w ? step_w[idx] : 1.  With step_w given, idx outside
 * [0, n_w) or w == 0 makes the launch write nothing at all (acc stays bit for bit).  *index is only read.
 * One wave owns 64 consecutive queries of a row, one lane per query and one thread per acc element: no atomics, the
 * result is deterministic.  q is read with 16-byte loads where q, ldq and q_bs allow, else element by element; same
 * values.  Nothing is allocated or synchronised.  LDM_ERR_ARG, nothing launched: a null q, k or acc; a shape outside
 * ldm_xattn_map_supported (heads >= 1, 1 <= Tk <= 80, 1 <= S <= sp, sp one of 32/48/64/80/96/160, dtype float32 or
 * bf16); R or T below 1; ldq or ldk below heads*sp; step_w with n_w below 1.
 */
int ldm_xattn_map_supported(int heads, int Tk, int S, int sp, int dtype);
int ldm_xattn_map(const void* q, int64_t ldq, int64_t q_bs, const void* k, int64_t ldk, int64_t k_bs, float* acc, int R,
                  int heads, int T, int Tk, int S, int sp, float log2_scale, int dtype, const float* step_w, int n_w,
                  const int32_t* index, int index_bias, void* stream);

/*
 * DiffEdit.
 *
 * ldm_eps_contrast_accum: the contrast of the two halves of a paired U-Net output, ADDED into acc.
 *   eps_all [2B][cells][c] float32: rows 0 .. B-1 the source prompt's eps (e_src), rows B .. 2B-1 the target's (e_tgt);
 *   acc [B][cells] float32, read-modify-write.
 * Per cell, with d_j = e_tgt[j] - e_src[j]:  s = |d_0|;  s = s + |d_j| for j = 1 .. c-1 ascending;  acc = acc + s.
 * Plain float32 operations in exactly that order -- no multiply, so nothing can contract -- and a NumPy float32
 * restatement is bit-identical.  A NaN in one channel reaches its own cell only.  `counter` (may be NULL): *counter is
 * decremented by a one-thread launch after this one, so every block has read what it needed first; the next
 * ldm_q_sample reads its noise row through it.  c == 4: four cells per thread, 16-byte loads of both halves and one
 * 16-byte acc load and store; the cells % 4 tail and any other c in 1..16 take a scalar path.  Grid-stride.
 * LDM_ERR_ARG, nothing launched: a null eps_all or acc; B or cells below 1; c outside 1..16; eps_all or acc not
 * 16-byte aligned at c == 4 (4-byte at any other c).
 *
 * ldm_contrast_mask: acc [B][h][w] float32 -> mask_out [B][h][w] float32, 1 = keep.  Per sample b:
 *   mean_b = (sum_p acc[b][p]) / (h w);  thr_b = tau * mean_b;  edit[p] = acc[b][p] > thr_b, written exactly so (a NaN
 *   in the cell or in the sum keeps the cell; an all-zero sample edits nothing; no division by the mean);
 *   edit'[y][x] = OR of edit over the (2 dilate + 1)^2 neighbourhood clipped to the image;  mask = 1 - edit'.
 * mean_out, thr_out float32 [B] and count_out int32 [B] (the edited cells after dilation) may each be NULL.  The sum is
 * 256 strided float32 partial sums folded by a fixed tree: within h w 2^-24 relative of the exact sum for non-negative
 * terms, and the same bits on every run (no atomics).  One 256-thread workgroup per sample keeps the sample's
 * thresholded bytes in LDS, hence ldm_contrast_mask_supported: h, w >= 1, h w <= 65536, dilate in 0..3.
 * LDM_ERR_ARG, nothing launched: a null acc or mask_out, B below 1, a shape outside _supported.
 *
 * ldm_store_row: table[row][0 .. n) = src[0 .. n) for row = index_sign * (*index) + index_bias; a row outside [0, rows)
 * writes nothing at all.  The inverse of ldm_select_row: it keeps a step's output in the row a device-resident counter
 * selects, inside a captured step.  *index is only read.  16-byte copies: n % 4 == 0, row_stride % 4 == 0 and >= n, src
 * and table 16-byte aligned, index_sign 1 or -1; else LDM_ERR_ARG.
 */
int ldm_eps_contrast_accum(const float* eps_all, float* acc, int32_t* counter, int B, int64_t cells, int c,
                           void* stream);
int ldm_contrast_mask_supported(int h, int w, int dilate);
int ldm_contrast_mask(const float* acc, float* mask_out, float* mean_out, float* thr_out, int32_t* count_out, int B,
                      int h, int w, float tau, int dilate, void* stream);
int ldm_store_row(const float* src, float* table, int64_t row_stride, int rows, const int32_t* index, int index_sign,
                  int index_bias, int64_t n, void* stream);

/*
 * Push-pull hole filling: out [B][H][W][c] float32 = x [B][H][W][c] float32 with every cell the
 * keep mask m = keep [B][H][W] float32 (1 = keep) does not keep replaced by a smooth continuation of the kept ones: the
 * start of an outpainted border or of a regenerated region ("masked content: fill").
 *   Level 0: a_0 = x, w_0 = clamp(m, 0, 1), a NaN in m counting as 0.
 *   Pull, level l -> l+1 until the level is 1 x 1 (L = ceil(log2(max(H, W))) levels; none for a 1 x 1 image):
 *     H_{l+1} = ceil(H_l / 2), W_{l+1} = ceil(W_l / 2); coarse cell (i, j) reads its in-bounds children (2i + dy,
 *     2j + dx) in the order (0,0), (0,1), (1,0), (1,1): s += w, v = fma(w, a, v) per channel, a child of weight 0
 *     contributing nothing whatever its value (a select, not 0 * a: a NaN in a hole does not leak);
 *     a_{l+1} = s > 0 ? v / s : 0 (one correctly rounded division), w_{l+1} = min(s, 1).
 *   Push, from f_L = a_L (for a 1 x 1 image: x where w_0 > 0, else 0) down to f_0.  At fine cell (y, x): cy = y >> 1,
 *     ny = clamp(cy + (y & 1 ? +1 : -1), 0, H_{l+1} - 1), columns alike; top = fma(0.25, f[cy][nx], 0.75 f[cy][cx]),
 *     bot = fma(0.25, f[ny][nx], 0.75 f[ny][cx]), u = fma(0.25, bot, 0.75 top);
 *     f_l = a_l (the bits) where w_l == 1, u where w_l == 0, fma(w_l, a_l - u, u) otherwise.
 *   out = f_0.  Kept cells (m >= 1) come out bit for bit, an all-zero mask gives zeros, one kept cell a constant image.
 * All float32; a thread owns an output element of its level: no atomics, the result is deterministic.
 *
 * workspace: ldm_pushpull_workspace_bytes(B, H, W, c) bytes of the caller's (levels 1 .. L of a and w; 0 bytes and a
 * NULL pointer for a 1 x 1 image).  Every element read is written first, whatever the workspace held.  out == x is
 * allowed (level 0's push reads x at its own cell only); any other overlap is not.  Nothing is allocated or
 * synchronised.
 *
 * Launches: lds_tail = 0 gives every level its own pull and its own push launch (2 L in all).  lds_tail = 1 (the
 * product's setting) replaces, from the first level with H_l <= 32 and W_l <= 32 on, all remaining pulls and all
 * pushes back up to that level by ONE launch of one workgroup per sample that keeps those levels in LDS (under 28 KB
 * at c = 4; c > 10 would not fit 64 KB and runs as lds_tail = 0): 7 launches instead of 16 for a 256 x 256 image.  Both
 * settings run the same operations in the same order and give the same bits, as do the two paths of the launched
 * levels (channel quads when c % 4 == 0 and x, out and workspace are 16-byte aligned, else element-wise).
 * LDM_ERR_ARG, nothing launched: a null x, keep or out; a null workspace unless H == W == 1; B, H, W or c below 1;
 * H W c above 2^31 - 1; lds_tail other than 0 or 1.
 */
size_t ldm_pushpull_workspace_bytes(int B, int H, int W, int c);
int ldm_pushpull_fill(const float* x, const float* keep, float* out, float* workspace, int B, int H, int W, int c,
                      int lds_tail, void* stream);

/*
 * Pixel-space paste-back after a masked decode, float32.  Pixel p is kept, P(p) = 1, iff
 * keep(p) >= 1; anything else, a NaN included, is a hole.  keep is [B][H][W] with keep_bstride = H W, or one [H][W]
 * mask for every sample with keep_bstride = 0; w_bstride alike.
 *
 * ldm_mask_feather: out [B][H][W] = w, the weight of the source pixels, a ramp that lies inside the kept region.
 *   taps: g[0 .. 2r], r in [0, 48], the caller's (a Gaussian of sigma pixels, r = ceil(3 sigma), normalised to sum 1 in
 *     float64 and rounded to float32; r = 0: the single tap 1).
 *   e(p) = 1 iff every in-bounds pixel within Chebyshev distance r of p is kept (a row pass, then a column pass; pixels
 *     outside the image count as kept, so the picture's border does not fade); q = 1 - e.
 *   Hq(y, x) = sum_t g[t] q(y, x + t - r), V(y, x) = sum_t g[t] Hq(y + t - r, x): taps outside the image contribute
 *     nothing; each sum is one fma chain in ascending t from 0.
 *   w(p) = P(p) ? clamp(1 - V(p), 0, 1) : 0.  So w is exactly 0 on every hole, exactly 1 where no hole lies within
 *     Chebyshev distance 2r, and r = 0 returns P.
 *   lds_tile = 0 (the product's setting, the faster form where measured): four launches (erode rows, erode columns with the complement, blur rows, blur columns with the
 *     select) through workspace, ldm_mask_feather_workspace_bytes(B, H, W) bytes of the caller's; every element read is
 *     written first.  lds_tile = 1 with r <= 16: one launch, a workgroup per 32 x 32 output tile stages the (32 + 4r)^2
 *     neighbourhood of P in LDS (bytes for P, the row erosion and q, floats for Hq: 27 648 bytes at r = 16) and runs the
 *     same four passes there, the same taps in the same order; workspace is not touched and may be NULL.  lds_tile = 1
 *     with r > 16 runs as lds_tile = 0.  Both give the same bits.
 *   LDM_ERR_ARG, nothing launched: a null keep, taps or out; a null workspace on the four-launch path; B, H or W below
 *     1; H W above 2^31 - 1; r outside [0, 48]; keep_bstride neither 0 nor at least H W; lds_tile other than 0 or 1.
 *
 * ldm_keep_stats: o, d [B][H][W][c] (the source and the decoded images), c <= 4.  stats [B][c][5] float64 = n, sum o,
 *   sum o^2, sum d, sum d^2 over the pixels with P = 1; a pixel that is not kept is selected out, not multiplied by 0,
 *   so a NaN in a hole does not leak.  partial: B x ldm_keep_stats_partials(H, W) x c x 5 floats of the caller's, the
 *   float32 sums of one workgroup's chunk of pixels each (the chunk count depends on H W alone; thread stride, then
 *   wave, then LDS; no atomics); a finalise launch adds them in ascending order in float64 and writes gain, offset
 *   [B][c] float32: with var_x = (sum x^2 - (sum x)^2 / n) / n, a = sqrt(max(var_o, 0) / var_d) clamped to [0.5, 2],
 *   a = 1 if n < 2 or var_d <= 1e-12, b = mean_o - a mean_d; a = 1, b = 0 if n = 0.
 *   LDM_ERR_ARG: a null pointer; B (at most 65535), H, W or c below 1; c above 4; H W above 2^31 - 1; a bad stride.
 *
 * ldm_paste_back: d' = fma(a, d, b) per sample and channel with gain and offset (both or neither; NULL: d' = d, the
 *   bits); out = w >= 1 ? o : (w <= 0 ? d' : fma(w, o - d', d')), selects: o in a hole is never read into the result.
 *   out may be d.  Channel quads when c % 4 == 0 and o, d, out are 16-byte aligned, else element-wise; same bits.
 *   LDM_ERR_ARG: a null o, d, w or out; gain without offset; B, H, W or c below 1; H W c above 2^31 - 1; a bad stride.
 * Nothing is allocated or synchronised.
 */
size_t ldm_mask_feather_workspace_bytes(int B, int H, int W);
int ldm_mask_feather(const float* keep, int64_t keep_bstride, const float* taps, int r, float* out, float* workspace,
                     int B, int H, int W, int lds_tile, void* stream);
int ldm_keep_stats_partials(int H, int W);
int ldm_keep_stats(const float* o, const float* d, const float* keep, int64_t keep_bstride, float* partial,
                   double* stats, float* gain, float* offset, int B, int H, int W, int c, void* stream);
int ldm_paste_back(const float* o, const float* d, const float* w, int64_t w_bstride, const float* gain,
                   const float* offset, float* out, int B, int H, int W, int c, void* stream);

/* decode_first_stage prologue (model_runners.py:426 + autoencoder.py:362,434):
 * out = Dense_{C->C}(latents / scale_factor), C <= 8; float32 in, out_dtype out. */
int ldm_post_quant(const float* latents, float scale_factor, const float* kernel_io,
                   const float* bias, void* out, int out_dtype, int64_t pixels, int C,
                   void* stream);

/* DiagonalGaussian.sample / .mode (distribution.py:15-25,50): moments [pixels][2C] float32 =
 * (mean | logvar); out[p][c] = (mean + exp(0.5*logvar) * noise[p][c]) * out_scale, noise NULL
 * = mode.  The reference forms std from the UNCLIPPED logvar (:18); reproduced. */
int ldm_gaussian_sample(const float* moments, const float* noise, float* out, float out_scale,
                        int64_t pixels, int C, void* stream);

/* Nearest-codebook lookup (quantize.py:57-78): for each row z of [rows][C] (C <= 8):
 * idx = argmin_e |z|^2+|e|^2-2 z.e over codebook [V][C]; out = z + (e[idx]-z);
 * indices (int64) optional. */
int ldm_vq_nearest(const float* z, const float* codebook, float* out, int64_t* indices,
                   int64_t rows, int V, int C, void* stream);

/* tok_emb[ids] + pos_emb[0..T-1] (transformer.py:261-268); ids int64 [rows*T]. */
int ldm_embedding(const int64_t* ids, const float* tok_emb, const float* pos_emb, void* out,
                  int rows, int T, int D, int vocab, int out_dtype, void* stream);

/* tensor_to_image (run_ldm_sampler.py:18-25): per image (x-min)/(max-min)*255 -> uint8
 * (truncation).  scratch: 128 floats per image. */
int ldm_minmax_u8(const void* x, int in_dtype, uint8_t* out, float* scratch, int B,
                  int64_t n_per_image, void* stream);

/* dtype conversion / strided copy of [rows][cols] (cols contiguous). */
int ldm_cast(const void* x, int64_t ldx, int in_dtype, void* out, int64_t ldo, int out_dtype,
             int64_t rows, int cols, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LDM_HIP_H */
