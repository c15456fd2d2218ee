// Push-pull hole filling: out [B][H][W][c] = x [B][H][W][c] with the cells the keep mask
// m [B][H][W] does not keep replaced by a smooth continuation of the kept ones, float32.  A weighted image pyramid is
// pulled down to 1 x 1 (level l+1 has ceil(H_l / 2) x ceil(W_l / 2) cells, each the weighted mean of its up to four
// children) and pushed back up (each level is the bilinear enlargement of the coarser one wherever it has no weight
// of its own).  Levels 1 .. L of the values a and the weights w live in the caller's workspace; level 0 is x and m.
//
// Three kernels.  pull_kernel and push_kernel are output-stationary, one launch per level.  tail_kernel takes over at
// the first level of at most 32 x 32 cells: one workgroup per sample runs every remaining pull and every push back up
// to that level in LDS.  All three call pull_cell / push_cell below, so a level computed in LDS and the same level
// computed by its own launch hold the same bits.
#include "common.h"

namespace {

constexpr int kTailExtent = 32;                  // the tail starts at the first level with H_l, W_l <= this
constexpr size_t kTailLdsMax = 64 * 1024;        // dynamic LDS a launch gets without asking for more

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// clamp(m, 0, 1), a NaN counting as 0.  Idempotent, so the weights of the levels above 0 pass through it unchanged.
__device__ __forceinline__ float keep_weight(float m) { return m > 0.f ? (m < 1.f ? m : 1.f) : 0.f; }

// Coarse cell (i, j), channels ch .. ch+V-1, from the fine level (a, w) of Hf x Wf cells.  The in-bounds children in
// the order (0,0), (0,1), (1,0), (1,1): s += w, v = fma(w, a, v), where a child of weight 0 enters as the value 0 by a
// select (s and v are never -0, so adding its +0 changes no bit, and a NaN in a hole cannot leak).  val = v / s by one
// correctly rounded division, 0 where s == 0; wsum = min(s, 1).
template <int V>
__device__ __forceinline__ void pull_cell(const float* a, const float* w, int Hf, int Wf, int c, int i, int j, int ch,
                                          float (&val)[V], float& wsum) {
  float s = 0.f;
  float v[V];
#pragma unroll
  for (int k = 0; k < V; ++k) v[k] = 0.f;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const int y = 2 * i + (d >> 1), x = 2 * j + (d & 1);
    if (y < Hf && x < Wf) {
      const int cell = y * Wf + x;
      const float wt = keep_weight(w[cell]);
      const bool on = wt > 0.f;
      const float* src = a + (int64_t)cell * c + ch;
      float av[V];
      if constexpr (V == 4) {
        const f32x4 q = *(const f32x4*)src;
#pragma unroll
        for (int k = 0; k < 4; ++k) av[k] = q[k];
      } else {
        av[0] = *src;
      }
      s += wt;
#pragma unroll
      for (int k = 0; k < V; ++k) v[k] = __builtin_fmaf(wt, on ? av[k] : 0.f, v[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < V; ++k) val[k] = s > 0.f ? __fdiv_rn(v[k], s) : 0.f;
  wsum = s < 1.f ? s : 1.f;
}

// Fine cell (y, x), channels ch .. ch+V-1: u = the bilinear enlargement of the coarse level fc (Hc x Wc cells) at the
// cell's centre -- the coarse cell it lies in and its nearer neighbour per axis, weights 3/4 and 1/4, clamped at the
// border -- as explicit multiplies and fmas in one order; then the cell's own value a where its weight is 1 (the
// bits), u where it is 0 (a select: the hole's own value is never used), fma(w, a - u, u) between.
template <int V>
__device__ __forceinline__ void push_cell(const float* fc, int Hc, int Wc, const float* a, const float* w, int Wf,
                                          int c, int y, int x, int ch, float (&out)[V]) {
  const int cy = y >> 1, cx = x >> 1;
  const int ny = clampi(cy + ((y & 1) ? 1 : -1), Hc - 1), nx = clampi(cx + ((x & 1) ? 1 : -1), Wc - 1);
  const float* p00 = fc + ((int64_t)cy * Wc + cx) * c + ch;
  const float* p01 = fc + ((int64_t)cy * Wc + nx) * c + ch;
  const float* p10 = fc + ((int64_t)ny * Wc + cx) * c + ch;
  const float* p11 = fc + ((int64_t)ny * Wc + nx) * c + ch;
  const int cell = y * Wf + x;
  const float wt = keep_weight(w[cell]);
  const float* pa = a + (int64_t)cell * c + ch;
  float f00[V], f01[V], f10[V], f11[V], av[V];
  if constexpr (V == 4) {
    const f32x4 q00 = *(const f32x4*)p00, q01 = *(const f32x4*)p01, q10 = *(const f32x4*)p10,
                q11 = *(const f32x4*)p11, qa = *(const f32x4*)pa;
#pragma unroll
    for (int k = 0; k < 4; ++k) { f00[k] = q00[k]; f01[k] = q01[k]; f10[k] = q10[k]; f11[k] = q11[k]; av[k] = qa[k]; }
  } else {
    f00[0] = *p00; f01[0] = *p01; f10[0] = *p10; f11[0] = *p11; av[0] = *pa;
  }
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const float top = __builtin_fmaf(0.25f, f01[k], 0.75f * f00[k]);
    const float bot = __builtin_fmaf(0.25f, f11[k], 0.75f * f10[k]);
    const float u = __builtin_fmaf(0.25f, bot, 0.75f * top);
    out[k] = wt == 1.f ? av[k] : (wt == 0.f ? u : __builtin_fmaf(wt, av[k] - u, u));
  }
}

// Level (Hf x Wf) -> (Hc x Wc): a thread owns one coarse cell's channel quad (V = 4) or element (V = 1); the thread of
// channel 0 also writes the cell's weight.
template <int V>
__global__ __launch_bounds__(256) void pull_kernel(const float* a, const float* w, float* a_out, float* w_out, int B,
                                                   int Hf, int Wf, int Hc, int Wc, int c) {
  const int cv = c / V;
  const int64_t total = (int64_t)B * Hc * Wc * cv;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    int64_t r = i;
    const int ch = (int)(r % cv) * V; r /= cv;
    const int xo = (int)(r % Wc); r /= Wc;
    const int yo = (int)(r % Hc); r /= Hc;              // r = b
    float val[V], s;
    pull_cell<V>(a + r * Hf * Wf * c, w + r * Hf * Wf, Hf, Wf, c, yo, xo, ch, val, s);
    if constexpr (V == 4) {
      const f32x4 q = {val[0], val[1], val[2], val[3]};
      *(f32x4*)(a_out + i * 4) = q;
    } else {
      a_out[i] = val[0];
    }
    if (ch == 0) w_out[i / cv] = s;
  }
}

// Level (Hc x Wc) -> (Hf x Wf): a thread owns one fine cell's channel quad or element.  dst may be a (the levels above
// 0 are filled in place, and out may be x): a thread reads a at its own cell only.
template <int V>
__global__ __launch_bounds__(256) void push_kernel(const float* fc, const float* a, const float* w, float* dst, int B,
                                                   int Hf, int Wf, int Hc, int Wc, int c) {
  const int cv = c / V;
  const int64_t total = (int64_t)B * Hf * Wf * cv;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    int64_t r = i;
    const int ch = (int)(r % cv) * V; r /= cv;
    const int xo = (int)(r % Wf); r /= Wf;
    const int yo = (int)(r % Hf); r /= Hf;              // r = b
    float val[V];
    push_cell<V>(fc + r * Hc * Wc * c, Hc, Wc, a + r * Hf * Wf * c, w + r * Hf * Wf, Wf, c, yo, xo, ch, val);
    if constexpr (V == 4) {
      const f32x4 q = {val[0], val[1], val[2], val[3]};
      *(f32x4*)(dst + i * 4) = q;
    } else {
      dst[i] = val[0];
    }
  }
}

// A 1 x 1 image has no level above it: the top of the pyramid is the image, kept where it has weight.
__global__ __launch_bounds__(256) void top_kernel(const float* x, const float* m, float* out, int B, int c) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < B * c) out[i] = keep_weight(m[i / c]) > 0.f ? x[i] : 0.f;
}

// Extents and LDS offsets (in floats) of the tail's level t, counted from the level it starts at (H x W).
__device__ __forceinline__ void tail_level(int H, int W, int c, int t, int& h, int& w, int& oa, int& ow) {
  h = H; w = W; oa = 0;
  for (int k = 0; k < t; ++k) {
    oa += h * w * (c + 1);
    h = (h + 1) >> 1; w = (w + 1) >> 1;
  }
  ow = oa + h * w * c;
}

// One workgroup per sample, from a level of H x W <= 32 x 32 cells with at least one level above it: the level's
// values and weights are read into LDS, every pull up to 1 x 1 and every push back down run there, a thread per
// element as in the V = 1 launches, a barrier between levels; the last push writes the level to dst.  dst may be a:
// every global read is made before the first barrier.
__global__ __launch_bounds__(256) void tail_kernel(const float* a, const float* w, float* dst, int H, int W, int c,
                                                   int levels) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  a += b * H * W * c; w += b * H * W; dst += b * H * W * c;
  for (int e = tid; e < H * W * c; e += 256) lds[e] = a[e];
  for (int e = tid; e < H * W; e += 256) lds[H * W * c + e] = keep_weight(w[e]);
  __syncthreads();
  for (int t = 0; t < levels; ++t) {
    int hf, wf, oaf, owf, hc, wc, oac, owc;
    tail_level(H, W, c, t, hf, wf, oaf, owf);
    tail_level(H, W, c, t + 1, hc, wc, oac, owc);
    for (int e = tid; e < hc * wc * c; e += 256) {
      const int ch = e % c, cell = e / c;
      float val[1], s;
      pull_cell<1>(lds + oaf, lds + owf, hf, wf, c, cell / wc, cell % wc, ch, val, s);
      lds[oac + e] = val[0];
      if (ch == 0) lds[owc + cell] = s;
    }
    __syncthreads();
  }
  for (int t = levels - 1; t >= 0; --t) {
    int hf, wf, oaf, owf, hc, wc, oac, owc;
    tail_level(H, W, c, t, hf, wf, oaf, owf);
    tail_level(H, W, c, t + 1, hc, wc, oac, owc);
    for (int e = tid; e < hf * wf * c; e += 256) {
      const int ch = e % c, cell = e / c;
      float val[1];
      push_cell<1>(lds + oac, hc, wc, lds + oaf, lds + owf, wf, c, cell / wf, cell % wf, ch, val);
      if (t == 0) dst[e] = val[0];
      else lds[oaf + e] = val[0];                // (in place: a thread reads a at its own element only)
    }
    __syncthreads();
  }
}

inline bool al16(const void* p) { return (uintptr_t)p % 16 == 0; }

inline int levels_of(int H, int W) {
  int L = 0;
  while (H > 1 || W > 1) { H = (H + 1) / 2; W = (W + 1) / 2; ++L; }
  return L;
}

// The workspace: for l = 1 .. L the values a_l [B][H_l][W_l][c], then the weights w_l [B][H_l][W_l], every array
// starting at a multiple of four floats.  Returns the floats in all; off_a / off_w (may be NULL) get the offsets.
inline size_t round4(size_t n) { return (n + 3) & ~(size_t)3; }
size_t layout(int B, int H, int W, int c, size_t* off_a, size_t* off_w) {
  size_t off = 0;
  const int L = levels_of(H, W);
  for (int l = 1; l <= L; ++l) {
    H = (H + 1) / 2; W = (W + 1) / 2;
    if (off_a) off_a[l] = off;
    off += round4((size_t)B * H * W * c);
    if (off_w) off_w[l] = off;
    off += round4((size_t)B * H * W);
  }
  return off;
}

// LDS floats of a tail that starts at H x W cells
size_t tail_floats(int H, int W, int c) {
  size_t n = 0;
  for (;;) {
    n += (size_t)H * W * (c + 1);
    if (H == 1 && W == 1) return n;
    H = (H + 1) / 2; W = (W + 1) / 2;
  }
}

}  // namespace

extern "C" size_t ldm_pushpull_workspace_bytes(int B, int H, int W, int c) {
  if (B < 1 || H < 1 || W < 1 || c < 1) return 0;
  return layout(B, H, W, c, nullptr, nullptr) * sizeof(float);
}

extern "C" int ldm_pushpull_fill(const float* x, const float* keep, float* out, float* workspace, int B, int H, int W,
                                 int c, int lds_tail, void* stream) {
  LDM_CHECK_ARG(x && keep && out, "ldm_pushpull_fill: null pointer");
  LDM_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && c >= 1, "ldm_pushpull_fill: bad args (B=%d, H=%d, W=%d, c=%d)", B, H, W,
                c);
  LDM_CHECK_ARG((int64_t)H * W * c <= INT32_MAX && (int64_t)B * c <= INT32_MAX,
                "ldm_pushpull_fill: a sample of %d x %d x %d elements is too large", H, W, c);
  LDM_CHECK_ARG(lds_tail == 0 || lds_tail == 1, "ldm_pushpull_fill: lds_tail must be 0 or 1, got %d", lds_tail);
  const int L = levels_of(H, W);
  LDM_CHECK_ARG(workspace || L == 0, "ldm_pushpull_fill: null workspace");
  hipStream_t s = (hipStream_t)stream;
  if (L == 0) {
    hipLaunchKernelGGL(top_kernel, dim3(grid_for((int64_t)B * c, 256, 1 << 23)), dim3(256), 0, s, x, keep, out, B, c);
    return ldm_launch_status("ldm_pushpull_fill");
  }
  size_t off_a[34], off_w[34];                   // (L <= 31)
  layout(B, H, W, c, off_a, off_w);
  int hs[34], ws[34];
  hs[0] = H; ws[0] = W;
  for (int l = 1; l <= L; ++l) { hs[l] = (hs[l - 1] + 1) / 2; ws[l] = (ws[l - 1] + 1) / 2; }
  // T: the level the tail starts at (L: no tail).  A tail needs a level above it and its pyramid in LDS.
  int T = L;
  if (lds_tail) {
    for (int l = 0; l < L; ++l) {
      if (hs[l] <= kTailExtent && ws[l] <= kTailExtent) {
        if (tail_floats(hs[l], ws[l], c) * sizeof(float) <= kTailLdsMax) T = l;
        break;
      }
    }
  }
  const bool wide = c % 4 == 0 && al16(x) && al16(out) && al16(workspace);
  auto lvl_a = [&](int l) -> const float* { return l == 0 ? x : workspace + off_a[l]; };
  auto lvl_w = [&](int l) -> const float* { return l == 0 ? keep : workspace + off_w[l]; };
  auto lvl_f = [&](int l) -> float* { return l == 0 ? out : workspace + off_a[l]; };
  for (int l = 0; l < T; ++l) {
    const int64_t total = (int64_t)B * hs[l + 1] * ws[l + 1] * c;
    const dim3 g(grid_for(wide ? total / 4 : total, 256, 1024));
    if (wide)
      hipLaunchKernelGGL((pull_kernel<4>), g, dim3(256), 0, s, lvl_a(l), lvl_w(l), workspace + off_a[l + 1],
                         workspace + off_w[l + 1], B, hs[l], ws[l], hs[l + 1], ws[l + 1], c);
    else
      hipLaunchKernelGGL((pull_kernel<1>), g, dim3(256), 0, s, lvl_a(l), lvl_w(l), workspace + off_a[l + 1],
                         workspace + off_w[l + 1], B, hs[l], ws[l], hs[l + 1], ws[l + 1], c);
  }
  if (T < L) {
    const size_t lds = tail_floats(hs[T], ws[T], c) * sizeof(float);
    hipLaunchKernelGGL(tail_kernel, dim3(B), dim3(256), lds, s, lvl_a(T), lvl_w(T), lvl_f(T), hs[T], ws[T], c, L - T);
  }
  for (int l = T - 1; l >= 0; --l) {
    const int64_t total = (int64_t)B * hs[l] * ws[l] * c;
    const dim3 g(grid_for(wide ? total / 4 : total, 256, 1024));
    if (wide)
      hipLaunchKernelGGL((push_kernel<4>), g, dim3(256), 0, s, workspace + off_a[l + 1], lvl_a(l), lvl_w(l), lvl_f(l), B,
                         hs[l], ws[l], hs[l + 1], ws[l + 1], c);
    else
      hipLaunchKernelGGL((push_kernel<1>), g, dim3(256), 0, s, workspace + off_a[l + 1], lvl_a(l), lvl_w(l), lvl_f(l), B,
                         hs[l], ws[l], hs[l + 1], ws[l + 1], c);
  }
  return ldm_launch_status("ldm_pushpull_fill");
}
