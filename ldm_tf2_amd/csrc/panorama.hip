// Panorama sampling: the two kernels a step adds around the U-Net.  A canvas [B][H][W][c] is
// covered by nY x nX windows of h x w at stride (sy, sx), the last one of an axis clamped to the edge:
//   n = ceil((L - l) / s) + 1,  origin_i = min(i * s, L - l).
// ldm_window_gather crops the canvas into the U-Net's window batch, ldm_window_fold averages the windows' eps back
// onto the canvas.  Origins are recomputed in the kernels: no table, nothing a captured graph could find stale.
//
// Seamless panoramas: ldm_window_gather_ex / ldm_window_fold_ex take a wrap flag per axis and
// fold with a separable window profile wy[h] x wx[w]; ldm_wrap_pad_nhwc pads a canvas circularly for the decoder.  A
// wrapped axis has n = ceil(L / s) windows at origin_i = i * s (no clamp), window i covering (origin_i + j) mod L.
#include "common.h"

namespace {

struct Grid1 {
  int L, l, s, n;      // canvas extent, window extent, stride, windows
};
inline Grid1 grid1(int L, int l, int s) { return Grid1{L, l, s, (L - l + s - 1) / s + 1}; }
__device__ __forceinline__ int origin(const Grid1& g, int i) {
  const int o = i * g.s, last = g.L - g.l;
  return o < last ? o : last;
}
// The windows covering position p: indices lo .. hi.  Unclamped windows i cover p iff i*s <= p < i*s + l; the clamped
// last one starts at L - l <= (n-1)*s, so it covers every p >= L - l, and no p below that reaches index n - 1.
__device__ __forceinline__ void covering(const Grid1& g, int p, int& lo, int& hi) {
  lo = p < g.l ? 0 : (p - g.l) / g.s + 1;
  hi = p >= g.L - g.l ? g.n - 1 : p / g.s;
}

__device__ __forceinline__ void st4(float* p, const f32x4& v) { *(f32x4*)p = v; }
__device__ __forceinline__ void st4(bf16_t* p, const f32x4& v) {
  u32x2 c;
  c[0] = pack_bf2(v[0], v[1]);
  c[1] = pack_bf2(v[2], v[3]);
  *(u32x2*)p = c;
}

// x_win[half][b][k][y][x][:] = canvas[b][oy(k) + y][ox(k) + x][:] for both halves.  V = 4: a thread moves one channel
// quad (c % 4 == 0, aligned pointers); V = 1: one element.
template <typename TX, int V>
__global__ __launch_bounds__(256) void window_gather_kernel(const float* __restrict__ canvas, TX* __restrict__ x_win,
                                                            int B, int c, Grid1 gy, Grid1 gx) {
  const int cv = c / V;
  const int64_t half = (int64_t)B * gy.n * gx.n * gy.l * gx.l * c;
  const int64_t total = half / V;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    int64_t r = i;
    const int ch = (int)(r % cv) * V; r /= cv;
    const int x = (int)(r % gx.l); r /= gx.l;
    const int y = (int)(r % gy.l); r /= gy.l;
    const int kx = (int)(r % gx.n); r /= gx.n;
    const int ky = (int)(r % gy.n); r /= gy.n;          // r = b
    const int64_t src = ((r * gy.L + origin(gy, ky) + y) * gx.L + origin(gx, kx) + x) * c + ch;
    if constexpr (V == 4) {
      const f32x4 v = *(const f32x4*)(canvas + src);
      st4(x_win + i * 4, v);
      st4(x_win + half + i * 4, v);
    } else {
      const float v = canvas[src];
      Elem<TX>::st(x_win + i, v);
      Elem<TX>::st(x_win + half + i, v);
    }
  }
}

// eps_canvas[b][y][x][:] = (sum over the windows covering (y, x), ascending k = ky * nX + kx, starting from the first
// covering value) / count, in float32 with a correctly rounded division.  b runs over halves * B canvases.  A thread
// owns a canvas pixel's channel quad (V = 4) or element (V = 1) and reads the windows: no atomics.
template <int V>
__global__ __launch_bounds__(256) void window_fold_kernel(const float* __restrict__ eps_win,
                                                          float* __restrict__ eps_canvas, int BB, int c, Grid1 gy,
                                                          Grid1 gx) {
  const int cv = c / V;
  const int64_t total = (int64_t)BB * gy.L * gx.L * cv;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    int64_t r = i;
    const int ch = (int)(r % cv) * V; r /= cv;
    const int x = (int)(r % gx.L); r /= gx.L;
    const int y = (int)(r % gy.L); r /= gy.L;           // r = b
    int ky0, ky1, kx0, kx1;
    covering(gy, y, ky0, ky1);
    covering(gx, x, kx0, kx1);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    bool first = true;
    for (int ky = ky0; ky <= ky1; ++ky) {
      const int wy = y - origin(gy, ky);
      for (int kx = kx0; kx <= kx1; ++kx) {
        const int wx = x - origin(gx, kx);
        const int64_t src = ((((r * gy.n + ky) * gx.n + kx) * gy.l + wy) * gx.l + wx) * c + ch;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if constexpr (V == 4) v = *(const f32x4*)(eps_win + src);
        else v[0] = eps_win[src];
        acc = first ? v : acc + v;
        first = false;
      }
    }
    const float count = (float)((ky1 - ky0 + 1) * (kx1 - kx0 + 1));
    if constexpr (V == 4) {
      f32x4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = __fdiv_rn(acc[k], count);
      *(f32x4*)(eps_canvas + i * 4) = o;
    } else {
      eps_canvas[i] = __fdiv_rn(acc[0], count);
    }
  }
}

// ---- wrap-around windows and weighted folds --------------------------------------------
struct GridW {
  int L, l, s, n, wrap;  // as Grid1; wrap: windows cross the edge and come back on the other side
};
inline GridW gridw(int L, int l, int s, int wrap) {
  return wrap ? GridW{L, l, s, (L + s - 1) / s, 1} : GridW{L, l, s, (L - l + s - 1) / s + 1, 0};
}
// Canvas position of element j of window i.  Wrapped: i * s < L and j < l <= L, so one subtraction folds it back.
__device__ __forceinline__ int position(const GridW& g, int i, int j) {
  if (g.wrap) {
    const int p = i * g.s + j;
    return p < g.L ? p : p - g.L;
  }
  const int o = i * g.s, last = g.L - g.l;
  return (o < last ? o : last) + j;
}
// The windows covering position p, as two ascending index ranges lo[r] .. hi[r].  Unwrapped: covering() and an empty
// second range.  Wrapped: window i holds p at element p - i*s (range 0: i*s <= p < i*s + l) or, across the edge, at
// element p + L - i*s (range 1: i*s <= p + L < i*s + l, whose left half holds for every i < n); hi[0] = p / s <=
// (L - 1) / s = n - 1 and lo[1] = (p + L - l) / s + 1 > p / s, so the ranges are disjoint and range 0 lies below.
struct Cover {
  int lo[2], hi[2];
};
__device__ __forceinline__ Cover covering_ex(const GridW& g, int p) {
  Cover c;
  c.lo[0] = p < g.l ? 0 : (p - g.l) / g.s + 1;
  if (g.wrap) {
    c.hi[0] = p / g.s;
    c.lo[1] = (p + g.L - g.l) / g.s + 1;
    c.hi[1] = g.n - 1;
  } else {
    c.hi[0] = p >= g.L - g.l ? g.n - 1 : p / g.s;
    c.lo[1] = 1;
    c.hi[1] = 0;
  }
  return c;
}
// Element of window i (of range r) that lies on position p.
__device__ __forceinline__ int element(const GridW& g, int i, int p, int r) {
  if (g.wrap) return p + (r ? g.L : 0) - i * g.s;
  const int o = i * g.s, last = g.L - g.l;
  return p - (o < last ? o : last);
}

// The fold's arithmetic is one rounding per operation: -ffp-contract=fast would fuse a product into the sum that
// follows it (__fmul_rn / __fadd_rn are a plain * and + to the compiler), so contraction is off in these two.
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

// window_gather_kernel with the source row and column taken modulo the extent on a wrapped axis.  The wrap is over
// pixels and a quad lies within one pixel's channels: a four-wide access never straddles it.
template <typename TX, int V>
__global__ __launch_bounds__(256) void window_gather_ex_kernel(const float* __restrict__ canvas,
                                                               TX* __restrict__ x_win, int B, int c, GridW gy,
                                                               GridW gx) {
  const int cv = c / V;
  const int64_t half = (int64_t)B * gy.n * gx.n * gy.l * gx.l * c;
  const int64_t total = half / V;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    int64_t r = i;
    const int ch = (int)(r % cv) * V; r /= cv;
    const int x = (int)(r % gx.l); r /= gx.l;
    const int y = (int)(r % gy.l); r /= gy.l;
    const int kx = (int)(r % gx.n); r /= gx.n;
    const int ky = (int)(r % gy.n); r /= gy.n;          // r = b
    const int64_t src = ((r * gy.L + position(gy, ky, y)) * gx.L + position(gx, kx, x)) * c + ch;
    if constexpr (V == 4) {
      const f32x4 v = *(const f32x4*)(canvas + src);
      st4(x_win + i * 4, v);
      st4(x_win + half + i * 4, v);
    } else {
      const float v = canvas[src];
      Elem<TX>::st(x_win + i, v);
      Elem<TX>::st(x_win + half + i, v);
    }
  }
}

// eps_canvas[b][y][x][:] = (sum_k ww_k v_k) / (sum_k ww_k) over the windows covering (y, x) in ascending k = ky * nX
// + kx (per axis: range 0, then range 1), ww = wy[jy] * wx[jx] at the window element (jy, jx) on the cell; both sums
// start from their first term; every product, sum and the division round once.  WT = false (no tables): the sum of
// the values over the count, window_fold_kernel's arithmetic.  Thread ownership as there: no atomics.
template <int V, bool WT>
__global__ __launch_bounds__(256) void window_fold_ex_kernel(const float* __restrict__ eps_win,
                                                             float* __restrict__ eps_canvas, int BB, int c, GridW gy,
                                                             GridW gx, const float* __restrict__ wy,
                                                             const float* __restrict__ wx) {
  const int cv = c / V;
  const int64_t total = (int64_t)BB * gy.L * gx.L * cv;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    int64_t r = i;
    const int ch = (int)(r % cv) * V; r /= cv;
    const int x = (int)(r % gx.L); r /= gx.L;
    const int y = (int)(r % gy.L); r /= gy.L;           // r = b
    const Cover cy = covering_ex(gy, y), cx = covering_ex(gx, x);
    f32x4 num = {0.f, 0.f, 0.f, 0.f};
    float den = 0.f;
    int count = 0;
#pragma unroll
    for (int ry = 0; ry < 2; ++ry) {
      for (int ky = cy.lo[ry]; ky <= cy.hi[ry]; ++ky) {
        const int jy = element(gy, ky, y, ry);
#pragma unroll
        for (int rx = 0; rx < 2; ++rx) {
          for (int kx = cx.lo[rx]; kx <= cx.hi[rx]; ++kx) {
            const int jx = element(gx, kx, x, rx);
            const int64_t src = ((((r * gy.n + ky) * gx.n + kx) * gy.l + jy) * gx.l + jx) * c + ch;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if constexpr (V == 4) v = *(const f32x4*)(eps_win + src);
            else v[0] = eps_win[src];
            if constexpr (WT) {
              const float ww = mul_rn(wy[jy], wx[jx]);
#pragma unroll
              for (int k = 0; k < V; ++k) num[k] = count ? add_rn(num[k], mul_rn(ww, v[k])) : mul_rn(ww, v[k]);
              den = count ? add_rn(den, ww) : ww;
            } else {
              num = count ? num + v : v;
            }
            ++count;
          }
        }
      }
    }
    if constexpr (!WT) den = (float)count;
    if constexpr (V == 4) {
      f32x4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = __fdiv_rn(num[k], den);
      *(f32x4*)(eps_canvas + i * 4) = o;
    } else {
      eps_canvas[i] = __fdiv_rn(num[0], den);
    }
  }
}

// out[b][y][x][:] = x[b][(y - py) mod H][(x - px) mod W][:], out [B][H + 2 py][W + 2 px][c]; py <= H, px <= W.
template <int V>
__global__ __launch_bounds__(256) void wrap_pad_kernel(const float* __restrict__ in, float* __restrict__ out, int B,
                                                       int H, int W, int c, int py, int px) {
  const int cv = c / V, Ho = H + 2 * py, Wo = W + 2 * px;
  const int64_t total = (int64_t)B * Ho * Wo * cv;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    int64_t r = i;
    const int ch = (int)(r % cv) * V; r /= cv;
    const int x = (int)(r % Wo); r /= Wo;
    const int y = (int)(r % Ho); r /= Ho;               // r = b
    const int sy = (y - py + H) % H, sx = (x - px + W) % W;          // (y - py + H >= 0: py <= H)
    const int64_t src = ((r * H + sy) * W + sx) * c + ch;
    if constexpr (V == 4) *(f32x4*)(out + i * 4) = *(const f32x4*)(in + src);
    else out[i] = in[src];
  }
}

inline bool al(const void* p, int bytes) { return (uintptr_t)p % bytes == 0; }

int grid_check(const char* what, int B, int H, int W, int c, int h, int w, int sy, int sx) {
  LDM_CHECK_ARG(B > 0 && c > 0 && H > 0 && W > 0, "%s: bad args (B=%d, H=%d, W=%d, c=%d)", what, B, H, W, c);
  LDM_CHECK_ARG(h >= 1 && h <= H && w >= 1 && w <= W, "%s: window %dx%d must lie within the canvas %dx%d", what, h, w,
                H, W);
  LDM_CHECK_ARG(sy >= 1 && sy <= h && sx >= 1 && sx <= w,
                "%s: stride (%d, %d) must be at least 1 and at most the window (%d, %d)", what, sy, sx, h, w);
  return LDM_OK;
}

}  // namespace

extern "C" int ldm_window_gather(const float* canvas, void* x_win, int x_dtype, int B, int H, int W, int c, int h,
                                 int w, int sy, int sx, void* stream) {
  LDM_CHECK_ARG(canvas && x_win, "ldm_window_gather: null pointer");
  LDM_CHECK_ARG(DT_OK(x_dtype), "ldm_window_gather: bad x_dtype %d", x_dtype);
  const int st = grid_check("ldm_window_gather", B, H, W, c, h, w, sy, sx);
  if (st != LDM_OK) return st;
  const Grid1 gy = grid1(H, h, sy), gx = grid1(W, w, sx);
  const int64_t half = (int64_t)B * gy.n * gx.n * h * w * c;
  // four-wide: the canvas is read and a float32 batch written in 16-byte accesses, a bf16 batch in 8-byte ones
  const bool wide = c % 4 == 0 && al(canvas, 16) && al(x_win, x_dtype == LDM_BF16 ? 8 : 16);
  hipStream_t s = (hipStream_t)stream;
  const dim3 g(grid_for(wide ? half / 4 : half, 256, 1024));
#define GATHER(TX, V) \
  hipLaunchKernelGGL((window_gather_kernel<TX, V>), g, dim3(256), 0, s, canvas, (TX*)x_win, B, c, gy, gx)
  if (x_dtype == LDM_BF16) {
    if (wide) GATHER(bf16_t, 4); else GATHER(bf16_t, 1);
  } else {
    if (wide) GATHER(float, 4); else GATHER(float, 1);
  }
#undef GATHER
  return ldm_launch_status("ldm_window_gather");
}

extern "C" int ldm_window_fold(const float* eps_win, float* eps_canvas, int halves, int B, int H, int W, int c, int h,
                               int w, int sy, int sx, void* stream) {
  LDM_CHECK_ARG(eps_win && eps_canvas, "ldm_window_fold: null pointer");
  LDM_CHECK_ARG(halves == 1 || halves == 2, "ldm_window_fold: halves=%d must be 1 or 2", halves);
  const int st = grid_check("ldm_window_fold", B, H, W, c, h, w, sy, sx);
  if (st != LDM_OK) return st;
  const Grid1 gy = grid1(H, h, sy), gx = grid1(W, w, sx);
  const bool wide = c % 4 == 0 && al(eps_win, 16) && al(eps_canvas, 16);
  const int64_t total = (int64_t)halves * B * H * W * c;
  hipStream_t s = (hipStream_t)stream;
  const dim3 g(grid_for(wide ? total / 4 : total, 256, 1024));
  if (wide) hipLaunchKernelGGL(window_fold_kernel<4>, g, dim3(256), 0, s, eps_win, eps_canvas, halves * B, c, gy, gx);
  else hipLaunchKernelGGL(window_fold_kernel<1>, g, dim3(256), 0, s, eps_win, eps_canvas, halves * B, c, gy, gx);
  return ldm_launch_status("ldm_window_fold");
}

extern "C" int ldm_window_gather_ex(const float* canvas, void* x_win, int x_dtype, int B, int H, int W, int c, int h,
                                    int w, int sy, int sx, int wrap_y, int wrap_x, void* stream) {
  LDM_CHECK_ARG(canvas && x_win, "ldm_window_gather_ex: null pointer");
  LDM_CHECK_ARG(DT_OK(x_dtype), "ldm_window_gather_ex: bad x_dtype %d", x_dtype);
  LDM_CHECK_ARG((wrap_y == 0 || wrap_y == 1) && (wrap_x == 0 || wrap_x == 1),
                "ldm_window_gather_ex: wrap flags (%d, %d) must be 0 or 1", wrap_y, wrap_x);
  const int st = grid_check("ldm_window_gather_ex", B, H, W, c, h, w, sy, sx);
  if (st != LDM_OK) return st;
  const GridW gy = gridw(H, h, sy, wrap_y), gx = gridw(W, w, sx, wrap_x);
  const int64_t half = (int64_t)B * gy.n * gx.n * h * w * c;
  const bool wide = c % 4 == 0 && al(canvas, 16) && al(x_win, x_dtype == LDM_BF16 ? 8 : 16);
  hipStream_t s = (hipStream_t)stream;
  const dim3 g(grid_for(wide ? half / 4 : half, 256, 1024));
#define GATHER(TX, V) \
  hipLaunchKernelGGL((window_gather_ex_kernel<TX, V>), g, dim3(256), 0, s, canvas, (TX*)x_win, B, c, gy, gx)
  if (x_dtype == LDM_BF16) {
    if (wide) GATHER(bf16_t, 4); else GATHER(bf16_t, 1);
  } else {
    if (wide) GATHER(float, 4); else GATHER(float, 1);
  }
#undef GATHER
  return ldm_launch_status("ldm_window_gather_ex");
}

extern "C" int ldm_window_fold_ex(const float* eps_win, float* eps_canvas, int halves, int B, int H, int W, int c,
                                  int h, int w, int sy, int sx, int wrap_y, int wrap_x, const float* wy,
                                  const float* wx, void* stream) {
  LDM_CHECK_ARG(eps_win && eps_canvas, "ldm_window_fold_ex: null pointer");
  LDM_CHECK_ARG(halves == 1 || halves == 2, "ldm_window_fold_ex: halves=%d must be 1 or 2", halves);
  LDM_CHECK_ARG((wrap_y == 0 || wrap_y == 1) && (wrap_x == 0 || wrap_x == 1),
                "ldm_window_fold_ex: wrap flags (%d, %d) must be 0 or 1", wrap_y, wrap_x);
  LDM_CHECK_ARG((wy == nullptr) == (wx == nullptr),
                "ldm_window_fold_ex: the weight tables wy and wx must both be given or both be null");
  const int st = grid_check("ldm_window_fold_ex", B, H, W, c, h, w, sy, sx);
  if (st != LDM_OK) return st;
  const GridW gy = gridw(H, h, sy, wrap_y), gx = gridw(W, w, sx, wrap_x);
  const bool wide = c % 4 == 0 && al(eps_win, 16) && al(eps_canvas, 16);
  const int64_t total = (int64_t)halves * B * H * W * c;
  hipStream_t s = (hipStream_t)stream;
  const dim3 g(grid_for(wide ? total / 4 : total, 256, 1024));
#define FOLD(V, WT)                                                                                              \
  hipLaunchKernelGGL((window_fold_ex_kernel<V, WT>), g, dim3(256), 0, s, eps_win, eps_canvas, halves * B, c, gy, \
                     gx, wy, wx)
  if (wy) {
    if (wide) FOLD(4, true); else FOLD(1, true);
  } else {
    if (wide) FOLD(4, false); else FOLD(1, false);
  }
#undef FOLD
  return ldm_launch_status("ldm_window_fold_ex");
}

extern "C" int ldm_wrap_pad_nhwc(const float* x, float* out, int B, int H, int W, int c, int py, int px,
                                 void* stream) {
  LDM_CHECK_ARG(x && out, "ldm_wrap_pad_nhwc: null pointer");
  LDM_CHECK_ARG(B > 0 && c > 0 && H > 0 && W > 0, "ldm_wrap_pad_nhwc: bad args (B=%d, H=%d, W=%d, c=%d)", B, H, W, c);
  LDM_CHECK_ARG(py >= 0 && py <= H && px >= 0 && px <= W,
                "ldm_wrap_pad_nhwc: margin (%d, %d) must lie in [0, %d] x [0, %d] (the extents)", py, px, H, W);
  const bool wide = c % 4 == 0 && al(x, 16) && al(out, 16);
  const int64_t total = (int64_t)B * (H + 2 * py) * (W + 2 * px) * c;
  hipStream_t s = (hipStream_t)stream;
  const dim3 g(grid_for(wide ? total / 4 : total, 256, 1024));
  if (wide) hipLaunchKernelGGL(wrap_pad_kernel<4>, g, dim3(256), 0, s, x, out, B, H, W, c, py, px);
  else hipLaunchKernelGGL(wrap_pad_kernel<1>, g, dim3(256), 0, s, x, out, B, H, W, c, py, px);
  return ldm_launch_status("ldm_wrap_pad_nhwc");
}
