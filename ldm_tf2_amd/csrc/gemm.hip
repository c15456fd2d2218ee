// MFMA GEMM + implicit-GEMM 3x3 convolution for gfx950 (MI355X).
//
// One kernel template serves Dense / 1x1 / attention projections (plain A rows)
// and 3x3 convolutions (A rows gathered from an NHWC image: no im2col buffer).
//
//   * A [M][K] and W^T [N][K] are both K-contiguous, so every MFMA operand
//     fragment is one 16-byte LDS read.  A K-tile is 128 BYTES of K per row
//     (64 bf16 or 32 f32); the tile is kept in LDS as rows of 8 x 16-byte
//     chunks with chunk' = chunk ^ ((row >> 1) & 7), which makes the
//     ds_read_b128 of 32 consecutive rows at one chunk conflict-free.
//   * bf16: v_mfma_f32_32x32x16_bf16 (lane = row (l&31), k = 8*(l>>5)+j).
//     f32 : v_mfma_f32_32x32x2_f32 issued 4x per 16-byte fragment; lane half h
//     then covers k = 4h..4h+3 of each 8-wide k group for A and B alike, a
//     permutation of the summation order only.
//   * staging is branch-free and asynchronous: every 16-byte piece is a
//     `buffer_load_dwordx4 ... lds` (LDS-DMA, no VGPR round trip) whose offset is
//     pushed out of range when the piece is padding (image border, M/N/K tails)
//     -- the hardware range check then writes zeros, so the conv's zero padding
//     costs one v_cndmask per piece and no divergent control flow.  An LDS-DMA
//     wave-instruction writes 64 x 16 B linearly, so the XOR swizzle is applied
//     to the SOURCE chunk each lane fetches.  Two LDS stages form a ring: tile
//     t+1 is issued while tile t is multiplied; s_waitcnt vmcnt(0) plus ONE raw
//     s_barrier per K-tile orders it.  The 256x128 tile (one workgroup per CU
//     either way) runs a 3-stage ring with a counted vmcnt instead; on the
//     smaller tiles a third stage would cost a resident workgroup per CU.
//   * the epilogue goes through LDS: accumulators are dropped as an f32 tile and
//     re-read row-wise so that bias / addend / residual / output all move as
//     16-byte vectors (the MFMA accumulator layout alone would give 2-byte
//     scattered stores).
//   * workgroup ids are remapped so that the tiles sharing an A row-panel run
//     on one XCD (its L2 then serves the panel's re-reads).
//   * stride-1 convolutions at the 32x32 / 16x16 levels can run with a HALO-STAGED A operand (tiles
//     15 / 16, gemm_kernel.h MODE 3): the (lines + 2) x (W + 2) input pixels of a 64-channel chunk are
//     staged once and serve all nine taps; only the weight tiles go through the stage ring.
//   * the 3x3 convolution over the nearest-2x upsampled image also runs as four 2x2 "phase" convolutions over
//     the image itself (upsample = 2, gemm_kernel.h MODE 4): output pixel (2i + a, 2j + b) only sees a 2x2
//     neighbourhood of the image, with weights summed beforehand (layout.upsample_phase_kernel) -- 16 instead
//     of 36 multiply-adds per pixel, channel pair and output phase.
//   * small-M layers (4x4 / 8x8 feature maps) stream their weights with split-K
//     over all CUs; partial sums go to an f32 workspace and a second kernel
//     reduces + applies the epilogue.
#include "gemm_kernel.h"
#include "gemm3_kernel.h"
#include "gemm_tiles.h"

using namespace ldm_gemm_detail;

namespace {

// split-K reduce + epilogue: one thread per output element
__global__ __launch_bounds__(256) void splitk_epilogue_kernel(GemmArgs p) {
  const int nout = p.act == LDM_ACT_GEGLU ? p.N / 2 : p.N;
  const int64_t total = (int64_t)p.M * nout;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * 256) {
    const int m = (int)(idx / nout), c = (int)(idx - (int64_t)m * nout);
    if (p.act == LDM_ACT_GEGLU) {
      const int nv = (c >> 5) * 64 + (c & 31), ng = nv + 32;
      float a = 0.f, g = 0.f;
      for (int s = 0; s < p.split_k; ++s) {
        const float* ws = p.ws + ((int64_t)s * p.M + m) * p.N;
        a += ws[nv]; g += ws[ng];
      }
      epi_store(p, 0, m, c, epi_pre(p, m, nv, a) * gelu_erf_f(epi_pre(p, m, ng, g)));
    } else {
      float a = 0.f;
      for (int s = 0; s < p.split_k; ++s) a += p.ws[((int64_t)s * p.M + m) * p.N + c];
      epi_store(p, 0, m, c, apply_act(p.act, epi_pre(p, m, c, a)));
    }
  }
}

// sum of the split slabs for 8 consecutive logical columns of row m, in split order
__device__ __forceinline__ void splitk_sum8(const GemmArgs& p, int m, int nlog, float (&v)[8]) {
  const float* src = p.ws + (int64_t)m * p.N + nlog;
  const int64_t slab = (int64_t)p.M * p.N;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = 0.f;
  int s = 0;
  for (; s + 4 <= p.split_k; s += 4) {          // 8 x 16-byte loads in flight, then ordered adds
    f32x4 t[4][2];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      t[u][0] = *(const f32x4*)(src + (s + u) * slab);
      t[u][1] = *(const f32x4*)(src + (s + u) * slab + 4);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[e] += t[u][0][e]; v[4 + e] += t[u][1][e]; }
  }
  for (; s < p.split_k; ++s) {
    const f32x4 t0 = *(const f32x4*)(src + s * slab), t1 = *(const f32x4*)(src + s * slab + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[e] += t0[e]; v[4 + e] += t1[e]; }
  }
  if (p.bias) {
    const f32x4 b0 = *(const f32x4*)(p.bias + nlog), b1 = *(const f32x4*)(p.bias + nlog + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[e] = v[e] * p.alpha + b0[e]; v[4 + e] = v[4 + e] * p.alpha + b1[e]; }
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] *= p.alpha;
  }
  if (p.addend) {
    const float* ad = p.addend + (int64_t)(m / p.add_rows) * p.add_ld + nlog;
    const f32x4 a0 = *(const f32x4*)ad, a1 = *(const f32x4*)(ad + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[e] += a0[e]; v[4 + e] += a1[e]; }
  }
}

// split-K reduce + epilogue for the row-major, 16-byte-aligned case: one thread per 8 output
// columns (the launches this serves are the 4x4 / 8x8 convolutions: it is pure slab traffic)
__global__ __launch_bounds__(256) void splitk_epilogue_vec_kernel(GemmArgs p) {
  const bool geglu = p.act == LDM_ACT_GEGLU;
  const int nout = geglu ? p.N / 2 : p.N;
  const int pcols = nout / 8;
  const int64_t total = (int64_t)p.M * pcols;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * 256) {
    const int m = (int)(idx / pcols), c = (int)(idx - (int64_t)m * pcols) * 8;
    const int nlog = geglu ? (c >> 5) * 64 + (c & 31) : c;
    float v[8];
    splitk_sum8(p, m, nlog, v);
    if (geglu) {
      float g[8];
      splitk_sum8(p, m, nlog + 32, g);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] *= gelu_erf_f(g[e]);
    } else if (p.act != LDM_ACT_NONE) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = apply_act(p.act, v[e]);
    }
    const int64_t ooff = (int64_t)m * p.ldc_m + c;
    const int64_t roff = (int64_t)m * p.ldr + c;
    if (p.out_dtype == LDM_BF16) {
      if (p.residual) {
        float rr[8];
        chunk_to_f32(*(const u32x4*)((const bf16_t*)p.residual + roff), rr, bf16_t());
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += rr[e];
      }
      *(u32x4*)((bf16_t*)p.out + ooff) = f32_to_chunk(v, bf16_t());
    } else {
      if (p.residual) {
        const f32x4 r0 = *(const f32x4*)((const float*)p.residual + roff);
        const f32x4 r1 = *(const f32x4*)((const float*)p.residual + roff + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[e] += r0[e]; v[4 + e] += r1[e]; }
      }
      f32x4 o0 = {v[0], v[1], v[2], v[3]}, o1 = {v[4], v[5], v[6], v[7]};
      *(f32x4*)((float*)p.out + ooff) = o0;
      *(f32x4*)((float*)p.out + ooff + 4) = o1;
    }
  }
}

// the two measured policies of choose() (everything below reads a tile's properties from its row of kTiles, gemm_tiles.h)
constexpr double kCoResidentPreference = 0.9;   // cost factor of a tile with `prefer_over` where that tile cannot fill the chip
constexpr int kHaloTwinMinKtiles = 27;          // K-tiles per split (three 64-channel chunks) from which a `halo_twin` wins

// MODE 3 geometry: stride 1, pad 1, no upsample, the 256-row M-tile = 256 / W whole lines of ONE image
bool halo_ring_ok(const ldm_gemm_params* p) {
  return p->conv && p->stride == 1 && !p->upsample && !p->no_lead_pad && p->dtype == LDM_BF16 && p->batch == 1 &&
         (p->W == 16 || p->W == 32) && 256 % p->W == 0 && p->H % (256 / p->W) == 0 && p->M % 256 == 0 &&
         p->OH == p->H && p->OW == p->W;
}

inline bool is_phase_form(const ldm_gemm_params* p) { return p->conv && p->upsample == 2; }
// M-tiles of a launch: the phase form tiles the rows of each of its four phases (M / 4) separately
inline int m_tiles(const ldm_gemm_params* p, int bm) {
  return is_phase_form(p) ? 4 * ((p->M / 4 + bm - 1) / bm) : (p->M + bm - 1) / bm;
}

inline int cdiv(int a, int b) { return (a + b - 1) / b; }
inline int elem_size(const ldm_gemm_params* p) { return p->dtype == LDM_BF16 ? 2 : 4; }

// vectorised epilogue: row-major output whose every 8-column piece is 16-byte addressable
bool vec_epilogue_ok(const ldm_gemm_params* p) {
  const int nout = p->act == LDM_ACT_GEGLU ? p->N / 2 : p->N;
  auto al = [](const void* q, int by) { return ((uintptr_t)q % by) == 0; };
  return p->ldc_n == 1 && nout % 8 == 0 && p->ldc_m % 8 == 0 && p->stride_c % 8 == 0 && al(p->out, 16) &&
         (!p->residual || (p->ldr % 8 == 0 && p->stride_r % 8 == 0 && al(p->residual, 16))) &&
         (!p->bias || al(p->bias, 16)) &&
         (!p->addend || (al(p->addend, 16) && p->add_ld % 4 == 0));
}

// Choose tile config + split-K jointly with a small cost model calibrated on MI355X
// (tools/gemm_bench.py): a launch runs in rounds of (256 CUs x resident workgroups)
// tiles; a round costs (K-tiles per split + a fixed prologue/epilogue overhead) x the
// measured time one CU needs for one K-tile of that configuration with its resident
// workgroups co-running.  Split-K adds the f32 partial round trip + one more launch.
struct Plan { int cfg, split, kps; };   // tile, slabs, K-tiles per slab
Plan choose(const ldm_gemm_params* p, int esize) {
  static const int kSplits[] = {1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 24, 32};
#ifdef LDM_TOOLS_BUILD
  static const bool no160 = getenv("LDM_GEMM_NO160") != nullptr;   // A/B switch, tools build only
  static const bool no_t2pref = getenv("LDM_GEMM_NO_T2PREF") != nullptr;
#else
  constexpr bool no160 = false, no_t2pref = false;
#endif
  const int ktiles = cdiv(p->K, 128 / esize);
  const bool geglu = p->act == LDM_ACT_GEGLU;
  const bool geglu_vec = geglu && vec_epilogue_ok(p);
  const double f32x = esize == 4 ? 8.0 : 1.0;   // f32 MFMA: 1/16 the rate at half the K per tile
  const bool tile_given = p->tile > 0 && p->tile < kNumTiles;
  double best = 1e30;
  int best_cfg = kFallbackTile, best_split = 1;
  for (int c = 1; c < kNumTiles; ++c) {
    const TileRow& t = kTiles[c];
    const bool forced = p->tile == c;
    if (tile_given && !forced) continue;
    if (!forced && has(c, esize == 2 ? tForced | tForcedBf16 : tForced)) continue;   // plan tables (bf16: a faster twin exists)
    if (has(c, tBf16) && esize != 2) continue;
    if (is_phase_form(p) && !phase_tile_ok(c, esize)) continue;   // phase form: its own few tiles
    if (p->a2 && !has(c, tA2) && !forced) continue;
    if (has(c, tWholeN) && !forced && (p->N % t.bn != 0 || no160)) continue;   // 160/320-column tiles: N = 160*k layers
    if (p->out2 && p->n_split % t.bn != 0) continue;                          // every tile on one side of n_split
    if (geglu && !has(c, tGeglu)) continue;
    const double tiles = (double)m_tiles(p, t.bm) * cdiv(p->N, t.bn) * p->batch;
    for (int split : kSplits) {
      if (p->split_k > 0 && split != p->split_k) continue;
      if (has(c, tPers) && split > 1) continue;   // the persistent kernel does not split K
      if (geglu && has(c, LDM_TILE_GEGLU_VEC) && split == 1 && !geglu_vec) continue;   // with split-K the reduce kernels apply it
      // split-K only rescues launches that cannot fill the machine once, and must fit
      // the caller's workspace
      if (split > 1 && (p->batch != 1 || ktiles / split < 4 || tiles >= 256.0 * t.resident ||
                        (p->split_k <= 0 && (!p->workspace || (size_t)split * p->M * p->N * 4 > p->workspace_bytes))))
        continue;
      const int kps = cdiv(ktiles, split);
      const double rounds = (double)(int64_t)((tiles * split + 256.0 * t.resident - 1) / (256.0 * t.resident));
      double us = rounds * (kps + t.overhead_steps) * t.step_us * f32x;
      // calibration (tools/splitk_sweep.py): when the 256x128 tiling cannot fill the chip once
      // (small-M convolutions: 4x4 / 8x8 / 16x16 maps), two co-resident 128x128 workgroups per
      // CU measure 5-14 % faster than one 256x128 at the same split
      if (!no_t2pref && t.prefer_over &&
          (double)m_tiles(p, kTiles[t.prefer_over].bm) * cdiv(p->N, kTiles[t.prefer_over].bn) * p->batch < 256.0)
        us *= kCoResidentPreference;
      if (split > 1) us += 3.0 + (double)p->M * p->N * 4.0 * (split + 1) / 3.0e6;   // bytes / (3 TB/s) in us
      if (us < best) { best = us; best_cfg = c; best_split = split; }
    }
  }
  if (p->split_k > 0 && p->batch == 1) best_split = p->split_k;
  const int twin = kTiles[best_cfg].halo_twin;
  if (tile_given) best_cfg = p->tile;
  // where the model picks the 256x160 ping-pong tile for a stride-1 convolution the halo-staged twin
  // measures 2-6 % faster from three channel chunks up (tools/conv_ring_probe.py)
  else if (twin && halo_ring_ok(p) && p->N % kTiles[twin].bn == 0 && !p->out2 && !p->ln_out && !p->a2 &&
           ktiles / best_split >= kHaloTwinMinKtiles)
    best_cfg = twin;
  return {best_cfg, best_split, 0};
}

// The (tile, split) ldm_gemm really launches for p: the cost model / forced plan of choose() plus the
// overrides of the launch forms that pin the tile, and the split as it comes out after whole K-tile
// ranges (empty trailing splits dropped).  One function, because ldm_gemm, ldm_gemm_splits,
// ldm_gemm_reduce and ldm_groupnorm_splitk must agree on the slab count.
Plan final_plan(const ldm_gemm_params* p) {
  const int esize = elem_size(p);
  auto [cfg, split, kps] = choose(p, esize);
  if (p->ln_out) { cfg = kLnTile; split = 1; }
  if (p->ln_cs && !has(cfg, tPers)) {
    // LayerNorm fold: the persistent kernel only (it derives the row statistics from its A tiles)
    const bool wide_ok = p->act != LDM_ACT_GEGLU && p->N % kTiles[kLnFoldWideTile].bn == 0;
    cfg = wide_ok && (p->N % kTiles[kLnFoldTile].bn != 0 || p->tile == kLnFoldWideTile) ? kLnFoldWideTile : kLnFoldTile;
    split = 1;
  }
  if (p->out2 || has(cfg, tPers)) split = 1;
  const int ktiles = cdiv(p->K, 128 / esize);
  kps = cdiv(ktiles, split < 1 ? 1 : split);
  if (has(cfg, tHalo)) kps = cdiv(kps, 9) * 9;   // splits at whole channel chunks (9 taps)
  return {cfg, cdiv(ktiles, kps), kps};             // (empty trailing splits dropped)
}

// addressable bytes from the (per-batch) base pointers of a and w (phase form: w of ONE phase's [N][K] block); plain
// rows of a hold `cols` columns: K, or the first K - Cin2 with a second operand
int64_t a_extent(const ldm_gemm_params* p, int cols) {
  return (p->conv ? ((int64_t)p->B * p->H * p->W - 1) * p->lda + p->Cin : ((int64_t)p->M - 1) * p->lda + cols) * elem_size(p);
}
int64_t w_extent(const ldm_gemm_params* p) { return (int64_t)p->N * p->K * elem_size(p); }

// the kernel arguments GemmArgs and Gemm3Args have in common
template <typename Args>
Args common_args(const ldm_gemm_params* p) {
  Args a;
  memset(&a, 0, sizeof(a));
  a.a = (const char*)p->a; a.w = (const char*)p->w; a.bias = p->bias; a.addend = p->addend;
  a.residual = (const char*)p->residual; a.out = (char*)p->out;
  a.lda = p->lda; a.ldr = p->ldr; a.add_ld = p->add_ld; a.M = p->M; a.N = p->N; a.K = p->K;
  a.a_bytes = (uint32_t)a_extent(p, p->K - (p->a2 ? p->Cin2 : 0)); a.w_bytes = (uint32_t)w_extent(p);
  a.add_rows = p->add_rows > 0 ? p->add_rows : 1;
  a.conv = p->conv; a.H = p->H; a.W = p->W; a.Cin = p->Cin; a.OH = p->OH; a.OW = p->OW;
  a.stride = p->stride; a.upsample = p->upsample; a.pad = p->no_lead_pad ? 0 : 1; a.act = p->act;
  return a;
}

// kernel arguments of the non-persistent path (main kernel and split-K reduce alike)
GemmArgs build_args(const ldm_gemm_params* p, Plan pl) {
  const int esize = elem_size(p), bke = 128 / esize;
  GemmArgs a = common_args<GemmArgs>(p);
  a.ws = (float*)p->workspace; a.ldc_m = p->ldc_m; a.ldc_n = p->ldc_n; a.batch = p->batch;
  a.stride_a = p->stride_a; a.stride_w = p->stride_w; a.stride_c = p->stride_c; a.stride_r = p->stride_r;
  a.out_dtype = p->out_dtype; a.alpha = p->alpha;
  a.ln_out = (char*)p->ln_out; a.ln_gamma = p->ln_gamma; a.ln_beta = p->ln_beta; a.ld_ln = p->ld_ln; a.ln_eps = p->ln_eps;
  a.out2 = (char*)p->out2; a.ld2 = p->ld2; a.stride2 = p->stride2; a.n_split = p->n_split; a.rows2 = p->rows2;
  a.ktiles = a.kt9 = cdiv(p->K, bke);               // no second operand: every K-tile belongs to the first
  if (p->a2) {
    a.a2 = (const char*)p->a2; a.lda2 = p->lda2; a.kt9 = (p->K - p->Cin2) / bke;
    a.a2_bytes = (uint32_t)((((int64_t)p->M - 1) * p->lda2 + p->Cin2) * esize);
  }
  a.vec_epilogue = vec_epilogue_ok(p);
  a.split_k = pl.split; a.ktiles_per_split = pl.kps;
  a.tiles_m = m_tiles(p, kTiles[pl.cfg].bm); a.tiles_n = cdiv(p->N, kTiles[pl.cfg].bn);
#ifdef LDM_TOOLS_BUILD
  { static const bool adj = getenv("LDM_UP2_PHASE_ADJACENT") != nullptr; a.phase_adjacent = adj; }   // tile-order A/B
#endif
  return a;
}

int launch_reduce(const ldm_gemm_params* p, const GemmArgs& a, hipStream_t s) {
  const int nout = p->act == LDM_ACT_GEGLU ? p->N / 2 : p->N;
  const bool vec = a.vec_epilogue && ((uintptr_t)p->workspace % 16) == 0 && p->N % 4 == 0;
  int64_t total = vec ? (int64_t)p->M * (nout / 8) : (int64_t)p->M * nout;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  if (vec) hipLaunchKernelGGL(splitk_epilogue_vec_kernel, dim3(blocks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(splitk_epilogue_kernel, dim3(blocks), dim3(256), 0, s, a);
  return ldm_launch_status("ldm_gemm(splitk epilogue)");
}

// ldm_gemm's checks that do not depend on the tile (every argument check precedes every launch)
int check_shape(const ldm_gemm_params* p) {
  LDM_CHECK_ARG(p && p->a && p->w && p->out, "ldm_gemm: null pointer");
  LDM_CHECK_ARG(p->dtype == LDM_F32 || p->dtype == LDM_BF16, "ldm_gemm: bad dtype %d", p->dtype);
  LDM_CHECK_ARG(p->out_dtype == LDM_F32 || p->out_dtype == LDM_BF16, "ldm_gemm: bad out_dtype");
  LDM_CHECK_ARG(p->M > 0 && p->N > 0 && p->K > 0 && p->batch > 0, "ldm_gemm: bad M/N/K/batch");
  const int esize = elem_size(p);
  const int epc = 16 / esize, bke = 8 * epc;
  LDM_CHECK_ARG(p->K % bke == 0, "ldm_gemm: K=%d must be a multiple of the K-tile (%d elements)", p->K, bke);
  LDM_CHECK_ARG(((uintptr_t)p->a % 16) == 0 && ((uintptr_t)p->w % 16) == 0,
                "ldm_gemm: a/w must be 16-byte aligned");
  LDM_CHECK_ARG(p->lda % epc == 0 && p->stride_a % epc == 0 && p->stride_w % epc == 0,
                "ldm_gemm: lda/stride_a/stride_w must be multiples of %d elements", epc);
  if (p->conv) {
    LDM_CHECK_ARG(p->Cin > 0 && p->Cin % bke == 0, "ldm_gemm(conv): Cin=%d must be a multiple of %d",
                  p->Cin, bke);
    if (p->upsample == 2) {
      // phase form: four 2x2 convolutions over the image, weights [4][N][4*Cin] (layout.upsample_phase_kernel)
      LDM_CHECK_ARG(p->K == 4 * p->Cin, "ldm_gemm(conv): the phase form (upsample = 2) needs K == 4*Cin (K=%d Cin=%d)", p->K, p->Cin);
      LDM_CHECK_ARG(p->stride == 1 && !p->no_lead_pad, "ldm_gemm(conv): the phase form (upsample = 2) needs stride 1 (stride=%d)", p->stride);
      LDM_CHECK_ARG(!p->a2 && !p->out2 && !p->ln_out && !p->ln_cs && p->act != LDM_ACT_GEGLU && p->ldc_n == 1,
                    "ldm_gemm(conv): the phase form (upsample = 2) takes no second operand (a2), out2, ln_out, ln_cs or GEGLU "
                    "and needs a row-major output");
      LDM_CHECK_ARG(4ll * p->N * p->K * esize < (1ll << 31), "ldm_gemm(conv): the phase form's weights must be < 2 GiB");
    } else
    LDM_CHECK_ARG(p->K == 9 * p->Cin + (p->a2 ? p->Cin2 : 0), "ldm_gemm(conv): K must be 9*Cin (+ Cin2 with a second operand)");
    if (p->a2)
      LDM_CHECK_ARG(p->stride == 1 && !p->upsample && !p->no_lead_pad && p->OH == p->H && p->OW == p->W,
                    "ldm_gemm(conv): the second operand (a2) needs a stride-1, pad-1, non-upsampled convolution");
    LDM_CHECK_ARG(p->stride == 1 || p->stride == 2, "ldm_gemm(conv): stride must be 1 or 2");
    LDM_CHECK_ARG(p->upsample >= 0 && p->upsample <= 2, "ldm_gemm(conv): upsample must be 0, 1 or 2 (the phase form)");
    LDM_CHECK_ARG(p->B > 0 && p->H > 0 && p->W > 0 && p->OH > 0 && p->OW > 0, "ldm_gemm(conv): dims");
    LDM_CHECK_ARG(p->H < 32768 && p->W < 32768, "ldm_gemm(conv): H/W too large");
    LDM_CHECK_ARG(!(p->upsample && p->stride != 1), "ldm_gemm(conv): upsample needs stride 1");
    // the upsampled form packs the tap origin in the UPSAMPLED image into 16 bits each (a_aux of gemm_kernel.h /
    // gemm3_kernel.h: (iy0 << 16) | (ix0 & 0xffff), ix0 read back as a short), so 2H and 2W must fit
    LDM_CHECK_ARG(!p->upsample || (2 * p->H < 32768 && 2 * p->W < 32768),
                  "ldm_gemm(conv): upsample needs 2*H and 2*W below 32768 (H=%d W=%d)", p->H, p->W);
    const int hs = p->upsample ? 2 * p->H : p->H, wsz = p->upsample ? 2 * p->W : p->W;
    LDM_CHECK_ARG(!p->no_lead_pad || p->stride == 2, "ldm_gemm(conv): no_lead_pad needs stride 2");
    const int padsum = p->no_lead_pad ? 1 : 2;
    LDM_CHECK_ARG(p->OH == (hs + padsum - 3) / p->stride + 1 && p->OW == (wsz + padsum - 3) / p->stride + 1,
                  "ldm_gemm(conv): OH/OW inconsistent with H/W/stride/upsample");
    LDM_CHECK_ARG(p->M == p->B * p->OH * p->OW, "ldm_gemm(conv): M != B*OH*OW");
    LDM_CHECK_ARG(p->batch == 1, "ldm_gemm(conv): batch must be 1");
  }
  const int64_t a_bytes = a_extent(p, p->K), w_bytes = w_extent(p);
  LDM_CHECK_ARG(a_bytes < (1ll << 31) && w_bytes < (1ll << 31),
                "ldm_gemm: operand extent must be < 2 GiB (a=%lld w=%lld bytes)", (long long)a_bytes,
                (long long)w_bytes);
  if (p->addend) LDM_CHECK_ARG(p->add_rows > 0, "ldm_gemm: add_rows must be > 0 with addend");
  if (p->act == LDM_ACT_GEGLU) {
    LDM_CHECK_ARG(p->N % 64 == 0, "ldm_gemm: GEGLU needs N %% 64 == 0");
    LDM_CHECK_ARG(p->ldc_n == 1, "ldm_gemm: GEGLU needs a row-major output");
    LDM_CHECK_ARG(!p->addend, "ldm_gemm: GEGLU takes no addend");
  }
  LDM_CHECK_ARG(p->ldc_n == 1 || p->ldc_m == 1, "ldm_gemm: one of ldc_m / ldc_n must be 1");

  if (p->a2) {   // second A operand for the last Cin2 columns of K: plain rows, or a 1x1 over the image a2
    LDM_CHECK_ARG(p->Cin2 > 0 && p->Cin2 % bke == 0 && p->lda2 % epc == 0 && p->lda2 >= p->Cin2 && ((uintptr_t)p->a2 % 16) == 0,
                  "ldm_gemm: a2 needs Cin2 %% %d == 0, lda2 %% %d == 0, lda2 >= Cin2 and 16-byte alignment", bke, epc);
    LDM_CHECK_ARG((((int64_t)p->M - 1) * p->lda2 + p->Cin2) * esize < (1ll << 31), "ldm_gemm: a2 extent must be < 2 GiB");
    LDM_CHECK_ARG(p->conv || (p->batch == 1 && p->Cin2 < p->K && (p->K - p->Cin2) % bke == 0 && !p->ln_cs && !p->ln_out && !p->out2),
                  "ldm_gemm: a2 on plain rows needs batch 1, whole K-tiles on both sides and a plain epilogue");
  }
  LDM_CHECK_ARG(!p->ln_cs || (p->dtype == LDM_BF16 && p->out_dtype == LDM_BF16 && !p->conv && p->batch == 1 && !p->ln_out),
                "ldm_gemm: ln_cs (LayerNorm fold) needs bf16 plain rows, batch 1 (the persistent tiles)");
  LDM_CHECK_ARG(p->tile >= 0 && p->tile < kNumTiles, "ldm_gemm: tile %d does not exist (0 = auto, 1-%d)", p->tile, kNumTiles - 1);
  return LDM_OK;
}

// MODE of gemm_kernel.h for a launch on tile cfg: 0 plain rows, 1 conv, 2 conv over the 2x-upsampled image, 3 halo-staged, 4 phase form
inline int gemm_mode(int conv, int upsample, int cfg) {
  return conv && upsample == 2 ? 4 : has(cfg, tHalo) ? 3 : !conv ? 0 : !upsample ? 1 : 2;
}

// what the planned tile `cfg` (its row t) asks of the arguments
int check_tile(const ldm_gemm_params* p, int cfg, int split) {
  const TileRow& t = kTiles[cfg];
  // out2 on a persistent tile: with n_split == 0 the WHOLE product is stored transposed per group of rows2 rows (V^T); with
  // n_split > 0 the n-tiles from n_split on, the ones below row-major (q | k | V^T as one launch; LayerNorm-folded form only)
  const bool trans = p->out2 != nullptr, ln = p->ln_cs != nullptr, nsplit_out = trans && p->n_split > 0;
  const int esize = elem_size(p);
  auto al16 = [](const void* q) { return ((uintptr_t)q % 16) == 0; };
  if (p->ln_out) {
    LDM_CHECK_ARG(!p->conv && p->batch == 1 && p->act != LDM_ACT_GEGLU && p->ldc_n == 1 &&
                      ldm_gemm_ln_supported(p->N, p->out_dtype) && p->ln_gamma && p->ln_beta,
                  "ldm_gemm: ln_out needs plain rows, batch 1, no GEGLU, N == %d and gamma/beta", kTiles[kLnTile].bn);
    LDM_CHECK_ARG(p->ld_ln % 8 == 0 && al16(p->ln_out) && al16(p->ln_gamma) && al16(p->ln_beta),
                  "ldm_gemm: ln_out / gamma / beta alignment");
  }
  if (trans && !has(cfg, tPers)) {
    LDM_CHECK_ARG(!p->conv && p->batch == 1 && p->act != LDM_ACT_GEGLU && p->ldc_n == 1 && !p->ln_out && !p->residual,
                  "ldm_gemm: out2 needs plain rows, batch 1, a row-major first output, no GEGLU / ln_out");
    LDM_CHECK_ARG(p->n_split > 0 && p->n_split < p->N && p->n_split % t.bn == 0,
                  "ldm_gemm: n_split=%d must be a multiple of the tile width %d", p->n_split, t.bn);
    LDM_CHECK_ARG(p->rows2 > 0 && p->rows2 % 4 == 0 && p->M % p->rows2 == 0 && p->ld2 % 4 == 0 && p->stride2 % 4 == 0 &&
                      al16(p->out2), "ldm_gemm: out2 geometry (rows2 %% 4, M %% rows2, ld2 / stride2 %% 4, alignment)");
  }
  if (p->act == LDM_ACT_GEGLU) {
    LDM_CHECK_ARG(has(cfg, tGeglu), "ldm_gemm: GEGLU needs a tile whose width is a multiple of 64 and that applies it "
                  "(the GEGLU flag of ldm_gemm_tile_info): not tile %d", cfg);
    if (has(cfg, LDM_TILE_GEGLU_VEC) && split <= 1)
      LDM_CHECK_ARG(vec_epilogue_ok(p), "ldm_gemm: GEGLU on tile %d without split-K needs the 16-byte alignment of the vector epilogue: "
                    "out, bias and residual 16-byte aligned, row pitches multiples of 8 elements", cfg);
  }
  LDM_CHECK_ARG(!has(cfg, tBf16) || esize == 2, "ldm_gemm: tile %d is bf16 only", cfg);
  if (is_phase_form(p))
    LDM_CHECK_ARG(phase_tile_ok(cfg, esize), "ldm_gemm: tile %d has no phase form (upsample = 2) for this dtype "
                  "(the phase flags of ldm_gemm_tile_info)", cfg);
  LDM_CHECK_ARG(!p->a2 || has(cfg, tA2), "ldm_gemm: tile %d cannot take a second A operand (a2): implicit-GEMM tiles only "
                "(the a2 flag of ldm_gemm_tile_info)", cfg);
  if (has(cfg, tHalo))
    LDM_CHECK_ARG(halo_ring_ok(p) && p->N % t.bn == 0 && !p->out2 && !p->ln_out,
                  "ldm_gemm: tile %d (halo-staged conv) needs a bf16 stride-1 3x3 convolution with W = 16 or 32, "
                  "H %% (256 / W) == 0, M %% 256 == 0 and N %% %d == 0", cfg, t.bn);
  if (has(cfg, tPers)) {   // persistent ping-pong kernel: bf16 in/out, row-major 16-byte-aligned output, whole n-tiles
    if (ln)
      LDM_CHECK_ARG(!p->conv && p->bias && al16(p->ln_cs) && p->ln_eps > 0.f && !p->addend && !p->residual,
                    "ldm_gemm: ln_cs (LayerNorm fold) needs plain rows, the folded bias, ln_eps > 0 and no addend / residual");
    if (trans)
      LDM_CHECK_ARG((p->n_split == 0 || (ln && p->n_split % t.bn == 0 && p->n_split < p->N)) && !p->conv && (!p->bias || ln) &&
                        !p->addend && !p->residual && p->act == LDM_ACT_NONE &&
                        p->rows2 > 0 && p->rows2 % 32 == 0 && p->M % p->rows2 == 0 && p->ld2 % 8 == 0 && p->stride2 % 8 == 0 &&
                        al16(p->out2),
                    "ldm_gemm: tile %d transposed output needs n_split 0 (or, LayerNorm-folded, whole n-tiles below it), a plain "
                    "product, rows2 %% 32 == 0, ld2 / stride2 %% 8 == 0", cfg);
    LDM_CHECK_ARG(p->dtype == LDM_BF16 && p->out_dtype == LDM_BF16 && p->batch == 1 && p->ldc_n == 1 &&
                      !p->ln_out && split <= 1 && p->N % t.bn == 0 && ((trans && !nsplit_out) || (p->ldc_m % 8 == 0 && al16(p->out))) &&
                      (!p->residual || (p->ldr % 4 == 0 && al16(p->residual))) && (!p->bias || al16(p->bias)) &&
                      (!p->addend || (al16(p->addend) && p->add_ld % 4 == 0)),
                  "ldm_gemm: tile %d (persistent) needs bf16 in/out, batch 1, a row-major 16-byte-aligned output, "
                  "N %% %d == 0, no split-K / out2 / ln_out", cfg, t.bn);
    LDM_CHECK_ARG(p->alpha == 1.0f, "ldm_gemm: tile %d (persistent) needs alpha == 1", cfg);
  } else {
    LDM_CHECK_ARG(!p->ln_out || vec_epilogue_ok(p), "ldm_gemm: ln_out needs the 16-byte-aligned row-major epilogue");
    // (implied by the bf16 / phase / halo checks above: it ties what is accepted here to what launch_tile instantiates)
    LDM_CHECK_ARG(tile_has_kernel(cfg, esize, gemm_mode(p->conv, p->upsample, cfg)), "ldm_gemm: tile %d has no kernel for this dtype and form", cfg);
  }
  return LDM_OK;
}

int launch_persistent(const ldm_gemm_params* p, int cfg, hipStream_t s) {
  const int bn = kTiles[cfg].bn;
  const bool trans = p->out2 != nullptr, ln = p->ln_cs != nullptr;
  Gemm3Args g = common_args<Gemm3Args>(p);   // (no a2 here: check_tile)
  g.ldc = p->ldc_m;
#ifdef LDM_TOOLS_BUILD
  { static const int dbg = getenv("LDM_G3_DEBUG") ? atoi(getenv("LDM_G3_DEBUG")) : 0; g.dbg = dbg; }   // timing ablations
#endif
  g.ktiles = p->K / 64; g.panels = cdiv(p->M, 256); g.ntiles = p->N / bn;
  // workgroups per panel: fill the 256 CUs about once, at most one workgroup per n-tile
  int nsplit = p->split_k < 0 ? -p->split_k : (256 + g.panels / 2) / g.panels;
  if (nsplit < 1) nsplit = 1;
  if (nsplit > g.ntiles) nsplit = g.ntiles;
  g.tiles_per_wg = cdiv(g.ntiles, nsplit);
  g.nsplit = cdiv(g.ntiles, g.tiles_per_wg);
  if (trans && p->n_split > 0) g.ntiles1 = p->n_split / bn;   // (a workgroup's range of n-tiles may straddle it)
  g.out_t = (char*)p->out2; g.ld_t = p->ld2; g.stride_t = p->stride2; g.rows_t = p->rows2; g.n_split = p->n_split;
  g.ln_cs = p->ln_cs; g.ln_eps = p->ln_eps;
  const dim3 grid((unsigned)(g.panels * g.nsplit));
  const int epi = (trans ? (ln ? (kEpiTrans | kEpiBias | (p->n_split > 0 ? kEpiSplit : 0)) : kEpiTrans)
                         : epi_code(p->bias != nullptr, p->addend != nullptr, p->residual != nullptr, p->act)) | (ln ? kEpiLn : 0);
  bool ok;
  if (ln) ok = launch_gemm3_ln(bn / 32, epi, g, grid, s);
  else if (!p->conv) ok = launch_gemm3<0>(bn / 32, epi, g, grid, s);
  else if (!p->upsample) ok = launch_gemm3<1>(bn / 32, epi, g, grid, s);
  else ok = launch_gemm3<2>(bn / 32, epi, g, grid, s);
  LDM_CHECK_ARG(ok, "ldm_gemm: tile %d (persistent) has no kernel for this epilogue (bias %d addend %d residual %d act %d)",
                cfg, p->bias != nullptr, p->addend != nullptr, p->residual != nullptr, p->act);
  return ldm_launch_status("ldm_gemm(persistent)");
}

int launch_ring(const ldm_gemm_params* p, Plan pl, hipStream_t s) {
  const int cfg = pl.cfg, split = pl.split;
  const GemmArgs a = build_args(p, pl);
  if (split > 1) {
    const size_t need = (size_t)split * p->M * p->N * 4;
    if (!p->workspace || p->workspace_bytes < need) {
      ldm_set_error("ldm_gemm: split_k=%d needs %zu workspace bytes, have %zu", split, need,
                    p->workspace ? p->workspace_bytes : (size_t)0);
      return LDM_ERR_WORKSPACE;
    }
  }
  const int64_t nblk = (int64_t)a.tiles_m * a.tiles_n * (split > 1 ? split : p->batch);
  LDM_CHECK_ARG(nblk < (1ll << 31), "ldm_gemm: grid too large");
  const dim3 grid((unsigned)nblk);
  auto launch = [&](auto elem) {   // the switch of the (element type, MODE) pair: gemm_launch.h, one gemm_inst_*.hip each
    using T = decltype(elem);
    switch (gemm_mode(p->conv, p->upsample, cfg)) {
      case 0: return launch_cfg<T, 0>(cfg, a, grid, s);
      case 1: return launch_cfg<T, 1>(cfg, a, grid, s);
      case 2: return launch_cfg<T, 2>(cfg, a, grid, s);
      case 3: if constexpr (sizeof(T) == 2) launch_cfg<T, 3>(cfg, a, grid, s); return;
      default: return launch_cfg<T, 4>(cfg, a, grid, s);
    }
  };
  if (p->dtype == LDM_BF16) launch(bf16_t()); else launch(float());
  int st = ldm_launch_status("ldm_gemm");
  if (st != LDM_OK) return st;
  // defer_reduce: the f32 slabs stay in the workspace; the caller completes the product with
  // ldm_gemm_reduce or fuses the reduction into the GroupNorm that follows (ldm_groupnorm_splitk)
  if (split > 1 && !p->defer_reduce) st = launch_reduce(p, a, s);
  return st;
}

}  // namespace

extern "C" int ldm_gemm_tile_count(void) { return kNumTiles; }

extern "C" int ldm_gemm_tile_info(int tile, ldm_gemm_tile* out) {
  LDM_CHECK_ARG(out && tile > 0 && tile < kNumTiles, "ldm_gemm_tile_info: tile %d does not exist (1-%d)", tile, kNumTiles - 1);
  const TileRow& t = kTiles[tile];
  out->bm = t.bm; out->bn = t.bn; out->resident = t.resident; out->flags = t.flags;
  return LDM_OK;
}

extern "C" int ldm_gemm_splits(const ldm_gemm_params* p) {
  if (!p || !(p->dtype == LDM_F32 || p->dtype == LDM_BF16) || p->K <= 0) return 0;
  return final_plan(p).split;
}

extern "C" int ldm_gemm_reduce(const ldm_gemm_params* p, void* stream) {
  LDM_CHECK_ARG(p && p->out && p->workspace, "ldm_gemm_reduce: null pointer");
  LDM_CHECK_ARG(!(p->act == LDM_ACT_GEGLU && p->addend), "ldm_gemm_reduce: GEGLU takes no addend");
  const Plan pl = final_plan(p);
  LDM_CHECK_ARG(pl.split > 1, "ldm_gemm_reduce: these parameters do not split K (nothing was deferred)");
  LDM_CHECK_ARG(p->workspace_bytes >= (size_t)pl.split * p->M * p->N * 4, "ldm_gemm_reduce: workspace too small");
  return launch_reduce(p, build_args(p, pl), (hipStream_t)stream);
}

extern "C" size_t ldm_gemm_workspace_bytes(const ldm_gemm_params* p) {
  if (!p) return 0;
  const int split = final_plan(p).split;
  return split > 1 ? (size_t)split * p->M * p->N * 4 : 0;
}

extern "C" int ldm_gemm_ln_supported(int N, int dtype) {
  return (N == kTiles[kLnTile].bn && (dtype == LDM_F32 || dtype == LDM_BF16)) ? 1 : 0;
}

extern "C" int ldm_gemm_plan(const ldm_gemm_params* p, int* tile, int* split_k) {
  LDM_CHECK_ARG(p && tile && split_k, "ldm_gemm_plan: null pointer");
  LDM_CHECK_ARG(p->dtype == LDM_F32 || p->dtype == LDM_BF16, "ldm_gemm_plan: bad dtype %d", p->dtype);
  const Plan pl = final_plan(p);
  *tile = pl.cfg; *split_k = pl.split;
  return LDM_OK;
}

extern "C" int ldm_gemm(const ldm_gemm_params* p, void* stream) {
  int st = check_shape(p);
  if (st != LDM_OK) return st;
  const Plan pl = final_plan(p);
  if ((st = check_tile(p, pl.cfg, pl.split)) != LDM_OK) return st;
  return has(pl.cfg, tPers) ? launch_persistent(p, pl.cfg, (hipStream_t)stream) : launch_ring(p, pl, (hipStream_t)stream);
}
