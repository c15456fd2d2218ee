// Pixel-space paste-back after a masked decode, float32: the feathered weight map of a keep
// mask, the statistics of the kept pixels that give a per-channel gain and offset, and the blend that puts the source
// pixels back.  Pixel p is kept, P(p) = 1, iff keep(p) >= 1 (a NaN is a hole).
//
// ldm_mask_feather: w = P ? clamp(1 - blur(1 - erode(P)), 0, 1) : 0 with a (2r+1)-tap separable box erosion and a
// (2r+1)-tap separable blur, so the ramp lies inside the kept region.  Two structures: four output-stationary launches
// through the caller's workspace (erode rows, erode columns with the complement, blur rows, blur columns with the
// select), or feather_tile_kernel, one workgroup per 32 x 32 output tile that stages the (32 + 4r)^2 neighbourhood of P
// in LDS and runs the same four passes there.  Both call blur_tap / feather_weight below with the same taps in the same
// order, so they hold the same bits.
// ldm_keep_stats: per sample and channel n, sum o, sum o^2, sum d, sum d^2 over the kept pixels: float32 partial sums
// per workgroup chunk (thread stride, then wave, then LDS; no atomics), added in float64 by a finalise launch that also
// writes the gain and offset.
// ldm_paste_back: out = w >= 1 ? o : (w <= 0 ? d' : fma(w, o - d', d')), d' = fma(a, d, b) or d itself.
#include "common.h"

namespace {

constexpr int kMaxRadius = 48;                   // r = ceil(3 sigma), sigma <= 16
constexpr int kTile = 32;                        // feather_tile_kernel's output tile
constexpr int kTileMaxRadius = 16;               // ... and the largest r it stages: (32 + 64)^2 cells of P
constexpr int kStatsChunkPixels = 4096;          // pixels a statistics workgroup walks
constexpr int kStatsMaxChunks = 1024;
constexpr int kStatsMaxC = 4;

__device__ __forceinline__ bool kept(float m) { return m >= 1.f; }

// one step of a blur chain: acc + g v, rounded once.  v = 0 leaves acc as it is (acc is never -0), so a tap that is
// skipped and a tap that reads a 0 give the same bits.
__device__ __forceinline__ float blur_tap(float acc, float g, float v) { return __builtin_fmaf(g, v, acc); }

__device__ __forceinline__ float feather_weight(bool p, float v) {
  return p ? fminf(fmaxf(1.f - v, 0.f), 1.f) : 0.f;
}

// ---- the four launches: a thread owns an output pixel ------------------------------------------------------
// er(y, x) = 1 iff every in-bounds pixel (y, x + dx), |dx| <= r, is kept
__global__ __launch_bounds__(256) void erode_rows_kernel(const float* keep, int64_t kb, float* er, int B, int H, int W,
                                                         int r) {
  const int64_t total = (int64_t)B * H * W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int x = (int)(i % W);
    const int64_t row = i / W;                    // b * H + y
    const float* kp = keep + (row / H) * kb + (row % H) * W;
    const int lo = x - r < 0 ? 0 : x - r, hi = x + r > W - 1 ? W - 1 : x + r;
    bool all = true;
    for (int xx = lo; xx <= hi; ++xx) all = all && kept(kp[xx]);
    er[i] = all ? 1.f : 0.f;
  }
}

// q(y, x) = 1 - e(y, x), e = 1 iff er(y + dy, x) = 1 for every in-bounds |dy| <= r
__global__ __launch_bounds__(256) void erode_cols_kernel(const float* er, float* q, int B, int H, int W, int r) {
  const int64_t total = (int64_t)B * H * W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int x = (int)(i % W);
    const int64_t row = i / W;
    const int y = (int)(row % H);
    const float* ep = er + (row / H) * H * W + x;
    const int lo = y - r < 0 ? 0 : y - r, hi = y + r > H - 1 ? H - 1 : y + r;
    bool all = true;
    for (int yy = lo; yy <= hi; ++yy) all = all && ep[(int64_t)yy * W] != 0.f;
    q[i] = all ? 0.f : 1.f;
  }
}

__global__ __launch_bounds__(256) void blur_rows_kernel(const float* q, const float* taps, float* hq, int B, int H,
                                                        int W, int r) {
  const int64_t total = (int64_t)B * H * W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int x = (int)(i % W);
    const float* qp = q + (i - x);
    float acc = 0.f;
    for (int t = 0; t <= 2 * r; ++t) {
      const int xx = x + t - r;
      if (xx >= 0 && xx < W) acc = blur_tap(acc, taps[t], qp[xx]);
    }
    hq[i] = acc;
  }
}

__global__ __launch_bounds__(256) void blur_cols_kernel(const float* hq, const float* taps, const float* keep,
                                                        int64_t kb, float* out, int B, int H, int W, int r) {
  const int64_t total = (int64_t)B * H * W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int x = (int)(i % W);
    const int64_t row = i / W;
    const int y = (int)(row % H);
    const int64_t b = row / H;
    const float* hp = hq + b * H * W + x;
    float acc = 0.f;
    for (int t = 0; t <= 2 * r; ++t) {
      const int yy = y + t - r;
      if (yy >= 0 && yy < H) acc = blur_tap(acc, taps[t], hp[(int64_t)yy * W]);
    }
    out[i] = feather_weight(kept(keep[b * kb + (int64_t)y * W + x]), acc);
  }
}

// ---- one launch: a workgroup owns a 32 x 32 output tile ----------------------------------------------------
// With S = 32 + 4r and S2 = 32 + 2r, in LDS: hq [S2][32] floats, then the bytes pk [S][S] (P over the tile's
// neighbourhood, 1 outside the image), er [S][S2] (row erosion) and qb [S2][S2] (1 - e, 0 outside the image, where q
// contributes nothing).  27 648 bytes at r = 16.  Index k of a narrower array lies r cells inside index k of the
// wider one, so tap t of output k reads input k + t.
__global__ __launch_bounds__(256) void feather_tile_kernel(const float* keep, int64_t kb, const float* taps, int r,
                                                           float* out, int B, int H, int W, int tiles_y, int tiles_x) {
  extern __shared__ float lds[];
  const int S = kTile + 4 * r, S2 = kTile + 2 * r, T = 2 * r + 1;
  float* hq = lds;
  uint8_t* pk = (uint8_t*)(hq + S2 * kTile);
  uint8_t* er = pk + S * S;
  uint8_t* qb = er + S * S2;
  const int tid = threadIdx.x;
  const int64_t total = (int64_t)B * tiles_y * tiles_x;
  for (int64_t tile = blockIdx.x; tile < total; tile += gridDim.x) {
    const int tx = (int)(tile % tiles_x), ty = (int)((tile / tiles_x) % tiles_y);
    const int64_t b = tile / ((int64_t)tiles_x * tiles_y);
    const int Y0 = ty * kTile - 2 * r, X0 = tx * kTile - 2 * r;   // the image position of pk[0][0]
    const float* kp = keep + b * kb;
    for (int e = tid; e < S * S; e += 256) {
      const int iy = Y0 + e / S, ix = X0 + e % S;
      const bool in = iy >= 0 && iy < H && ix >= 0 && ix < W;
      pk[e] = in ? (kept(kp[(int64_t)iy * W + ix]) ? 1 : 0) : 1;
    }
    __syncthreads();
    for (int e = tid; e < S * S2; e += 256) {
      const uint8_t* p = pk + (e / S2) * S + e % S2;
      int all = 1;
      for (int t = 0; t < T; ++t) all &= p[t];
      er[e] = (uint8_t)all;
    }
    __syncthreads();
    for (int e = tid; e < S2 * S2; e += 256) {
      const int y = e / S2, x = e % S2;
      const uint8_t* p = er + y * S2 + x;
      int all = 1;
      for (int t = 0; t < T; ++t) all &= p[t * S2];
      const int iy = Y0 + r + y, ix = X0 + r + x;
      const bool in = iy >= 0 && iy < H && ix >= 0 && ix < W;
      qb[e] = in ? (uint8_t)(1 - all) : 0;
    }
    __syncthreads();
    for (int e = tid; e < S2 * kTile; e += 256) {
      const uint8_t* p = qb + (e / kTile) * S2 + e % kTile;
      float acc = 0.f;
      for (int t = 0; t < T; ++t) acc = blur_tap(acc, taps[t], (float)p[t]);
      hq[e] = acc;
    }
    __syncthreads();
    for (int e = tid; e < kTile * kTile; e += 256) {
      const int y = e / kTile, x = e % kTile;
      const int iy = ty * kTile + y, ix = tx * kTile + x;
      if (iy < H && ix < W) {
        const float* p = hq + y * kTile + x;
        float acc = 0.f;
        for (int t = 0; t < T; ++t) acc = blur_tap(acc, taps[t], p[t * kTile]);
        out[b * H * W + (int64_t)iy * W + ix] = feather_weight(pk[(y + 2 * r) * S + x + 2 * r] != 0, acc);
      }
    }
    __syncthreads();                             // (the next tile writes pk)
  }
}

// ---- keep statistics -----------------------------------------------------------------------------------------
// Workgroup (chunk, b) walks the pixels [chunk * per, (chunk + 1) * per) of sample b, thread t the pixels t, t + 256,
// ...; a pixel that is not kept is selected out (its o and d are never added, so a NaN there does not leak).  Per
// channel sum o, sum o^2, sum d, sum d^2 and once n, reduced over the wave by the xor butterfly and over the four
// waves in ascending order through LDS: partial [B][chunks][C][5] = (n, so, so2, sd, sd2).
template <int C, bool kWide>
__global__ __launch_bounds__(256) void keep_stats_kernel(const float* o, const float* d, const float* keep, int64_t kb,
                                                         float* partial, int64_t HW, int per) {
  constexpr int kVals = 4 * C + 1;
  __shared__ float red[4][kVals];
  const int chunk = blockIdx.x, chunks = gridDim.x;
  const int64_t b = blockIdx.y;
  const int64_t p0 = (int64_t)chunk * per;
  const int64_t p1 = p0 + per < HW ? p0 + per : HW;
  float acc[kVals];
#pragma unroll
  for (int k = 0; k < kVals; ++k) acc[k] = 0.f;
  for (int64_t p = p0 + threadIdx.x; p < p1; p += 256) {
    const bool on = kept(keep[b * kb + p]);
    const float* op = o + (b * HW + p) * C;
    const float* dp = d + (b * HW + p) * C;
    float ov[C], dv[C];
    if constexpr (kWide) {
      const f32x4 qo = *(const f32x4*)op, qd = *(const f32x4*)dp;
#pragma unroll
      for (int k = 0; k < 4; ++k) { ov[k] = qo[k]; dv[k] = qd[k]; }
    } else {
#pragma unroll
      for (int k = 0; k < C; ++k) { ov[k] = op[k]; dv[k] = dp[k]; }
    }
    acc[0] += on ? 1.f : 0.f;
#pragma unroll
    for (int k = 0; k < C; ++k) {
      const float ok = on ? ov[k] : 0.f, dk = on ? dv[k] : 0.f;
      acc[1 + 4 * k] += ok;
      acc[2 + 4 * k] = __builtin_fmaf(ok, ok, acc[2 + 4 * k]);
      acc[3 + 4 * k] += dk;
      acc[4 + 4 * k] = __builtin_fmaf(dk, dk, acc[4 + 4 * k]);
    }
  }
#pragma unroll
  for (int k = 0; k < kVals; ++k) acc[k] = wave_sum(acc[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < kVals; ++k) red[threadIdx.x >> 6][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < 5 * C) {
    const int k = threadIdx.x / 5, j = threadIdx.x % 5;
    const int v = j == 0 ? 0 : 4 * k + j;
    partial[((b * chunks + chunk) * C + k) * 5 + j] = ((red[0][v] + red[1][v]) + red[2][v]) + red[3][v];
  }
}

// Thread (b, k): the chunk partials in ascending order in float64 -> stats [B][C][5]; then the gain a and the offset b
// that bring d's mean and variance over the kept pixels to o's: a = sqrt(var_o / var_d) clamped to [0.5, 2] (1 when
// n < 2 or var_d <= 1e-12), b = mean_o - a mean_d; a = 1, b = 0 when nothing is kept.
__global__ __launch_bounds__(64) void keep_stats_finalise_kernel(const float* partial, double* stats, float* gain,
                                                                 float* offset, int B, int chunks, int C) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= B * C) return;
  const int b = i / C, k = i % C;
  double s[5] = {0., 0., 0., 0., 0.};
  for (int ch = 0; ch < chunks; ++ch) {
    const float* p = partial + (((int64_t)b * chunks + ch) * C + k) * 5;
#pragma unroll
    for (int j = 0; j < 5; ++j) s[j] += (double)p[j];
  }
#pragma unroll
  for (int j = 0; j < 5; ++j) stats[(int64_t)i * 5 + j] = s[j];
  const double n = s[0];
  double a = 1., off = 0.;
  if (n >= 1.) {
    const double mo = s[1] / n, md = s[3] / n;
    const double vo = (s[2] - s[1] * s[1] / n) / n, vd = (s[4] - s[3] * s[3] / n) / n;
    if (n >= 2. && vd > 1e-12) {
      a = sqrt((vo > 0. ? vo : 0.) / vd);
      a = a < 0.5 ? 0.5 : (a > 2. ? 2. : a);
    }
    off = mo - a * md;
  }
  gain[i] = (float)a;
  offset[i] = (float)off;
}

// ---- paste-back ----------------------------------------------------------------------------------------------
// A thread owns one pixel's channel quad (V = 4) or element (V = 1).  Selects throughout: o is not used where w <= 0,
// d not where w >= 1.  out may be d: a thread reads d at its own element only.
template <int V, bool kGain>
__global__ __launch_bounds__(256) void paste_kernel(const float* o, const float* d, const float* w, int64_t wb,
                                                    const float* gain, const float* offset, float* out, int B,
                                                    int64_t HW, int c) {
  const int cv = c / V;
  const int64_t total = (int64_t)B * HW * cv;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int ch = (int)(i % cv) * V;
    const int64_t px = i / cv;                   // b * HW + p
    const int64_t b = px / HW;
    const float wt = w[b * wb + (px - b * HW)];
    float ov[V], dv[V], res[V];
    if constexpr (V == 4) {
      const f32x4 qo = *(const f32x4*)(o + i * 4), qd = *(const f32x4*)(d + i * 4);
#pragma unroll
      for (int k = 0; k < 4; ++k) { ov[k] = qo[k]; dv[k] = qd[k]; }
    } else {
      ov[0] = o[i]; dv[0] = d[i];
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      float dk = dv[k];
      if constexpr (kGain) dk = __builtin_fmaf(gain[b * c + ch + k], dk, offset[b * c + ch + k]);
      res[k] = wt >= 1.f ? ov[k] : (wt <= 0.f ? dk : __builtin_fmaf(wt, ov[k] - dk, dk));
    }
    if constexpr (V == 4) {
      const f32x4 q = {res[0], res[1], res[2], res[3]};
      *(f32x4*)(out + i * 4) = q;
    } else {
      out[i] = res[0];
    }
  }
}

inline bool al16(const void* p) { return (uintptr_t)p % 16 == 0; }
inline size_t round4(size_t n) { return (n + 3) & ~(size_t)3; }

inline size_t tile_lds_bytes(int r) {
  const size_t S = kTile + 4 * r, S2 = kTile + 2 * r;
  return S2 * kTile * sizeof(float) + S * S + S * S2 + S2 * S2;
}

inline int stats_chunks(int64_t hw) {
  const int64_t n = (hw + kStatsChunkPixels - 1) / kStatsChunkPixels;
  return (int)(n < 1 ? 1 : (n > kStatsMaxChunks ? kStatsMaxChunks : n));
}

template <int C>
void launch_keep_stats(bool wide, dim3 grid, hipStream_t s, const float* o, const float* d, const float* keep,
                       int64_t kb, float* partial, int64_t HW, int per) {
  if constexpr (C == 4) {
    if (wide) {
      hipLaunchKernelGGL((keep_stats_kernel<4, true>), grid, dim3(256), 0, s, o, d, keep, kb, partial, HW, per);
      return;
    }
  }
  hipLaunchKernelGGL((keep_stats_kernel<C, false>), grid, dim3(256), 0, s, o, d, keep, kb, partial, HW, per);
}

}  // namespace

extern "C" size_t ldm_mask_feather_workspace_bytes(int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1) return 0;
  return 2 * round4((size_t)B * H * W) * sizeof(float);
}

extern "C" int ldm_mask_feather(const float* keep, int64_t keep_bstride, const float* taps, int r, float* out,
                                float* workspace, int B, int H, int W, int lds_tile, void* stream) {
  LDM_CHECK_ARG(keep && taps && out, "ldm_mask_feather: null pointer");
  LDM_CHECK_ARG(B >= 1 && H >= 1 && W >= 1, "ldm_mask_feather: bad args (B=%d, H=%d, W=%d)", B, H, W);
  LDM_CHECK_ARG((int64_t)H * W <= INT32_MAX, "ldm_mask_feather: an image of %d x %d pixels is too large", H, W);
  LDM_CHECK_ARG(r >= 0 && r <= kMaxRadius, "ldm_mask_feather: r must lie in [0, %d], got %d", kMaxRadius, r);
  LDM_CHECK_ARG(keep_bstride == 0 || keep_bstride >= (int64_t)H * W,
                "ldm_mask_feather: keep_bstride must be 0 or at least H W, got %lld", (long long)keep_bstride);
  LDM_CHECK_ARG(lds_tile == 0 || lds_tile == 1, "ldm_mask_feather: lds_tile must be 0 or 1, got %d", lds_tile);
  hipStream_t s = (hipStream_t)stream;
  if (lds_tile && r <= kTileMaxRadius) {
    const int tiles_y = (H + kTile - 1) / kTile, tiles_x = (W + kTile - 1) / kTile;
    const int64_t tiles = (int64_t)B * tiles_y * tiles_x;
    hipLaunchKernelGGL(feather_tile_kernel, dim3(grid_for(tiles, 1, 1 << 16)), dim3(256), tile_lds_bytes(r), s, keep,
                       keep_bstride, taps, r, out, B, H, W, tiles_y, tiles_x);
    return ldm_launch_status("ldm_mask_feather");
  }
  LDM_CHECK_ARG(workspace, "ldm_mask_feather: null workspace");
  float* wa = workspace;
  float* wb = workspace + round4((size_t)B * H * W);
  const dim3 g(grid_for((int64_t)B * H * W, 256, 4096));
  hipLaunchKernelGGL(erode_rows_kernel, g, dim3(256), 0, s, keep, keep_bstride, wa, B, H, W, r);
  hipLaunchKernelGGL(erode_cols_kernel, g, dim3(256), 0, s, wa, wb, B, H, W, r);
  hipLaunchKernelGGL(blur_rows_kernel, g, dim3(256), 0, s, wb, taps, wa, B, H, W, r);
  hipLaunchKernelGGL(blur_cols_kernel, g, dim3(256), 0, s, wa, taps, keep, keep_bstride, out, B, H, W, r);
  return ldm_launch_status("ldm_mask_feather");
}

extern "C" int ldm_keep_stats_partials(int H, int W) {
  if (H < 1 || W < 1) return 0;
  return stats_chunks((int64_t)H * W);
}

extern "C" int ldm_keep_stats(const float* o, const float* d, const float* keep, int64_t keep_bstride, float* partial,
                              double* stats, float* gain, float* offset, int B, int H, int W, int c, void* stream) {
  LDM_CHECK_ARG(o && d && keep && partial && stats && gain && offset, "ldm_keep_stats: null pointer");
  LDM_CHECK_ARG(B >= 1 && B <= 65535 && H >= 1 && W >= 1 && c >= 1, "ldm_keep_stats: bad args (B=%d, H=%d, W=%d, c=%d)",
                B, H, W, c);
  LDM_CHECK_ARG(c <= kStatsMaxC, "ldm_keep_stats: at most %d channels, got %d", kStatsMaxC, c);
  LDM_CHECK_ARG((int64_t)H * W <= INT32_MAX, "ldm_keep_stats: an image of %d x %d pixels is too large", H, W);
  LDM_CHECK_ARG(keep_bstride == 0 || keep_bstride >= (int64_t)H * W,
                "ldm_keep_stats: keep_bstride must be 0 or at least H W, got %lld", (long long)keep_bstride);
  hipStream_t s = (hipStream_t)stream;
  const int64_t HW = (int64_t)H * W;
  const int chunks = stats_chunks(HW);
  const int per = (int)((HW + chunks - 1) / chunks);
  const dim3 grid(chunks, B);
  const bool wide = al16(o) && al16(d);
  switch (c) {
    case 1: launch_keep_stats<1>(wide, grid, s, o, d, keep, keep_bstride, partial, HW, per); break;
    case 2: launch_keep_stats<2>(wide, grid, s, o, d, keep, keep_bstride, partial, HW, per); break;
    case 3: launch_keep_stats<3>(wide, grid, s, o, d, keep, keep_bstride, partial, HW, per); break;
    default: launch_keep_stats<4>(wide, grid, s, o, d, keep, keep_bstride, partial, HW, per); break;
  }
  hipLaunchKernelGGL(keep_stats_finalise_kernel, dim3((B * c + 63) / 64), dim3(64), 0, s, partial, stats, gain, offset,
                     B, chunks, c);
  return ldm_launch_status("ldm_keep_stats");
}

extern "C" int ldm_paste_back(const float* o, const float* d, const float* w, int64_t w_bstride, const float* gain,
                              const float* offset, float* out, int B, int H, int W, int c, void* stream) {
  LDM_CHECK_ARG(o && d && w && out, "ldm_paste_back: null pointer");
  LDM_CHECK_ARG((gain == nullptr) == (offset == nullptr), "ldm_paste_back: gain and offset go together");
  LDM_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && c >= 1, "ldm_paste_back: bad args (B=%d, H=%d, W=%d, c=%d)", B, H, W, c);
  LDM_CHECK_ARG((int64_t)H * W * c <= INT32_MAX && (int64_t)B * c <= INT32_MAX,
                "ldm_paste_back: a sample of %d x %d x %d elements is too large", H, W, c);
  LDM_CHECK_ARG(w_bstride == 0 || w_bstride >= (int64_t)H * W,
                "ldm_paste_back: w_bstride must be 0 or at least H W, got %lld", (long long)w_bstride);
  hipStream_t s = (hipStream_t)stream;
  const int64_t HW = (int64_t)H * W;
  const bool wide = c % 4 == 0 && al16(o) && al16(d) && al16(out);
  const int64_t total = (int64_t)B * HW * c;
  const dim3 g(grid_for(wide ? total / 4 : total, 256, 4096));
  if (wide && gain)
    hipLaunchKernelGGL((paste_kernel<4, true>), g, dim3(256), 0, s, o, d, w, w_bstride, gain, offset, out, B, HW, c);
  else if (wide)
    hipLaunchKernelGGL((paste_kernel<4, false>), g, dim3(256), 0, s, o, d, w, w_bstride, gain, offset, out, B, HW, c);
  else if (gain)
    hipLaunchKernelGGL((paste_kernel<1, true>), g, dim3(256), 0, s, o, d, w, w_bstride, gain, offset, out, B, HW, c);
  else
    hipLaunchKernelGGL((paste_kernel<1, false>), g, dim3(256), 0, s, o, d, w, w_bstride, gain, offset, out, B, HW, c);
  return ldm_launch_status("ldm_paste_back");
}
