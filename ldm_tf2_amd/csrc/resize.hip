// Latent resize: out [B][Ho][Wo][c] = x [B][H][W][c] resampled, float32, enlarging or shrinking,
// no antialiasing.  Per axis (source extent L, output extent Lo, output index i) the source coordinate is
//   s = (i + 0.5) L / Lo - 0.5 = ((2 i + 1) L - Lo) / (2 Lo),
// kept as an integer numerator over the denominator 2 Lo: floor(s) is an integer division and the fraction
// f = s - floor(s) ONE correctly rounded float division of two integers.  Nothing is tabulated: a thread computes the
// taps and weights of its output pixel from (L, Lo, i), so a captured graph holds no address that could go stale.
#include "common.h"

namespace {

template <int MODE> struct Taps {
  static constexpr int N = MODE == LDM_RESIZE_NEAREST ? 1 : MODE == LDM_RESIZE_BILINEAR ? 2 : 4;
  int idx[N];
  float w[N];
};

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// Keys' cubic convolution kernel, a = -0.75.  |d| <= 1: (a + 2) d^3 - (a + 3) d^2 + 1 in Horner form.  1 < |d| < 2:
// a (d^3 - 5 d^2 + 8 d - 4) = a (d - 1) (d - 2)^2, written in its factors: at d = 1 + f that is a f (1 - f)^2 with no
// cancellation, where the expanded polynomial subtracts terms of size 6 to leave 0.1.
__device__ __forceinline__ float keys_near(float d) {
  return __builtin_fmaf(__builtin_fmaf(1.25f, d, -2.25f) * d, d, 1.0f);
}
__device__ __forceinline__ float keys_far(float dm1, float dm2) { return -0.75f * dm1 * (dm2 * dm2); }

template <int MODE>
__device__ __forceinline__ Taps<MODE> taps(int L, int Lo, int i) {
  Taps<MODE> t;
  if constexpr (MODE == LDM_RESIZE_NEAREST) {
    t.idx[0] = clampi((int)(((int64_t)i * L) / Lo), L - 1);
    t.w[0] = 1.0f;
  } else {
    const int64_t den = 2 * (int64_t)Lo;
    const int64_t num = (2 * (int64_t)i + 1) * L - Lo;          // > -den: floor(s) >= -1
    const int64_t q = (num + den) / den;                         // floor(s) + 1
    const int i0 = (int)q - 1;
    const float f = __fdiv_rn((float)(num + den - q * den), (float)den);
    if constexpr (MODE == LDM_RESIZE_BILINEAR) {
      const float fb = num < 0 ? 0.0f : f;                       // s = max(s, 0)
      const int ib = num < 0 ? 0 : i0;
      t.idx[0] = clampi(ib, L - 1);
      t.idx[1] = clampi(ib + 1, L - 1);
      t.w[0] = 1.0f - fb;
      t.w[1] = fb;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) t.idx[k] = clampi(i0 - 1 + k, L - 1);
      const float g = 1.0f - f;                                  // distances f + 1, f, 1 - f, 2 - f
      t.w[0] = keys_far(f, g);
      t.w[1] = keys_near(f);
      t.w[2] = keys_near(g);
      t.w[3] = keys_far(g, f);
    }
  }
  return t;
}

// A thread owns one output pixel's channel quad (V = 4: c % 4 == 0, 16-byte aligned pointers) or element (V = 1) and
// sums wy * wx * x over its tap grid, rows outermost, in float32: acc = fma(wy * wx, x, acc), the same instruction
// sequence per element in both paths.  Nearest copies the source bits.
template <int MODE, int V>
__global__ __launch_bounds__(256) void resize_kernel(const float* __restrict__ x, float* __restrict__ out, int B, int H,
                                                     int W, int c, int Ho, int Wo) {
  const int cv = c / V;
  const int64_t total = (int64_t)B * Ho * Wo * cv;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    int64_t r = i;
    const int ch = (int)(r % cv) * V; r /= cv;
    const int xo = (int)(r % Wo); r /= Wo;
    const int yo = (int)(r % Ho); r /= Ho;              // r = b
    const Taps<MODE> ty = taps<MODE>(H, Ho, yo), tx = taps<MODE>(W, Wo, xo);
    const float* img = x + r * H * W * c + ch;
    if constexpr (MODE == LDM_RESIZE_NEAREST) {
      const float* src = img + ((int64_t)ty.idx[0] * W + tx.idx[0]) * c;
      if constexpr (V == 4) *(f32x4*)(out + i * 4) = *(const f32x4*)src;
      else out[i] = *src;
    } else {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int a = 0; a < Taps<MODE>::N; ++a) {
#pragma unroll
        for (int b = 0; b < Taps<MODE>::N; ++b) {
          const float* src = img + ((int64_t)ty.idx[a] * W + tx.idx[b]) * c;
          const float w = ty.w[a] * tx.w[b];
          // explicit fused multiply-adds: left to contraction, the two paths were compiled to different roundings
          if constexpr (V == 4) {
            const f32x4 v = *(const f32x4*)src;
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = __builtin_fmaf(w, v[k], acc[k]);
          } else {
            acc[0] = __builtin_fmaf(w, *src, acc[0]);
          }
        }
      }
      if constexpr (V == 4) *(f32x4*)(out + i * 4) = acc;
      else out[i] = acc[0];
    }
  }
}

inline bool al16(const void* p) { return (uintptr_t)p % 16 == 0; }

template <int MODE>
void launch(const float* x, float* out, int B, int H, int W, int c, int Ho, int Wo, hipStream_t s) {
  const bool wide = c % 4 == 0 && al16(x) && al16(out);
  const int64_t total = (int64_t)B * Ho * Wo * c;
  const dim3 g(grid_for(wide ? total / 4 : total, 256, 1024));
  if (wide) hipLaunchKernelGGL((resize_kernel<MODE, 4>), g, dim3(256), 0, s, x, out, B, H, W, c, Ho, Wo);
  else hipLaunchKernelGGL((resize_kernel<MODE, 1>), g, dim3(256), 0, s, x, out, B, H, W, c, Ho, Wo);
}

}  // namespace

extern "C" int ldm_resize_nhwc(const float* x, float* out, int B, int H, int W, int c, int Ho, int Wo, int mode,
                               void* stream) {
  LDM_CHECK_ARG(x && out, "ldm_resize_nhwc: null pointer");
  LDM_CHECK_ARG(mode == LDM_RESIZE_NEAREST || mode == LDM_RESIZE_BILINEAR || mode == LDM_RESIZE_BICUBIC,
                "ldm_resize_nhwc: unknown mode %d", mode);
  LDM_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && c >= 1 && Ho >= 1 && Wo >= 1,
                "ldm_resize_nhwc: bad args (B=%d, H=%d, W=%d, c=%d, Ho=%d, Wo=%d)", B, H, W, c, Ho, Wo);
  // the same size: every source coordinate is an integer and every mode's weights are (1, 0 ..); the copy keeps the
  // bits of a -0.0 or a NaN, which 1 * x + 0 * y would not
  if (Ho == H && Wo == W) mode = LDM_RESIZE_NEAREST;
  hipStream_t s = (hipStream_t)stream;
  if (mode == LDM_RESIZE_NEAREST) launch<LDM_RESIZE_NEAREST>(x, out, B, H, W, c, Ho, Wo, s);
  else if (mode == LDM_RESIZE_BILINEAR) launch<LDM_RESIZE_BILINEAR>(x, out, B, H, W, c, Ho, Wo, s);
  else launch<LDM_RESIZE_BICUBIC>(x, out, B, H, W, c, Ho, Wo, s);
  return ldm_launch_status("ldm_resize_nhwc");
}
