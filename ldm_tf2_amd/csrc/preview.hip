// Latent previews: frames [R][B][s h][s w][3] uint8 <- lat [B][h][w][c] float32 through an affine
// map of the latent channels to RGB, an integer upscale and an 8-bit quantisation, for up to two sources in one launch.
// The slot r of the frame strips comes from a device-resident index, so the launch sits inside a captured step: it
// writes slot idx / freq when idx = *index + index_bias is a multiple of freq (and the slot exists), else nothing.
//
// Per output pixel, for every latent channel j in turn: a_j = the upscaled latent (nearest: a copy; bilinear: the taps
// and weights of resize.hip's LDM_RESIZE_BILINEAR at Lo = s L, acc = fma(wy * wx, lat, acc) from 0, rows outermost), then
// v_k = fma(a_j, proj[j][k], v_k) from v_k = bias[k]; t = fma(127.5, v, 127.5); byte = floor(min(max(t, 0), 255) + 0.5).
// The upscale comes first because it is the cheaper order (4 c + 3 c multiply-adds against 12 c + 12); both orders are
// the same affine map.
//
// Thread map: the B s h s w pixels of a slot are one flat run of 3-byte pixels; a work item is four consecutive
// pixels, 12 contiguous bytes, so that a wave's stores cover 768 contiguous bytes.  Where the slot's first byte is
// 4-byte aligned an item goes out as three dwords, else (and for the last, partial item) as bytes; the values are
// computed before the path is chosen, so both paths store the same bytes.
#include "common.h"

namespace {

constexpr int kMaxC = 16;
constexpr int kPix = 4;          // pixels per work item: 12 bytes, three dwords

struct Tap2 {
  int i0, i1;
  float w0, w1;
};

__device__ __forceinline__ int clamp_hi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// One axis of source extent L enlarged `scale` times, output index i: resize.hip's taps<> at Lo = scale L.  There
// s = ((2 i + 1) L - Lo) / (2 Lo); at Lo = scale L the extent cancels, s = ((2 i + 1) - scale) / (2 scale), and with
// i = m scale + r it is m + e / (2 scale), e = 2 r + 1 - scale in (-scale, scale): floor(s) = m - (e < 0) and the
// fraction ONE correctly rounded division of the remainder by 2 scale -- the same quotient as resize.hip's, whose
// numerator and denominator are these times L.  One 32-bit division per axis instead of 64-bit ones.
template <int MODE>
__device__ __forceinline__ Tap2 axis_tap(int L, int scale, int i) {
  Tap2 t;
  const int m = i / scale;
  if constexpr (MODE == LDM_PREVIEW_NEAREST) {
    t.i0 = t.i1 = clamp_hi(m, L - 1);                            // (i L) / (scale L)
    t.w0 = 1.0f;
    t.w1 = 0.0f;
  } else {
    const int e = 2 * (i - m * scale) + 1 - scale;
    const int i0 = e < 0 ? m - 1 : m;                            // floor(s) >= -1
    const float f = __fdiv_rn((float)(e < 0 ? e + 2 * scale : e), (float)(2 * scale));
    const float fb = i0 < 0 ? 0.0f : f;                          // s = max(s, 0)
    const int ib = i0 < 0 ? 0 : i0;
    t.i0 = clamp_hi(ib, L - 1);
    t.i1 = clamp_hi(ib + 1, L - 1);
    t.w0 = 1.0f - fb;
    t.w1 = fb;
  }
  return t;
}

__device__ __forceinline__ uint32_t quantise(float v) {
  const float t = __builtin_fmaf(127.5f, v, 127.5f);
  // fmaxf(NaN, 0) = 0: a NaN never reaches the conversion
  return (uint32_t)floorf(fminf(fmaxf(t, 0.0f), 255.0f) + 0.5f);
}

struct Src {
  const float* lat;
  uint8_t* frames;
};

// C > 0: the channel count at compile time, proj in registers; C == 0: any c <= kMaxC, proj read through the scalar
// cache inside the channel loop.  The arithmetic per byte is the same chain in every instance.
template <int MODE, int C>
__global__ __launch_bounds__(256) void preview_kernel(Src a, Src b, const float* __restrict__ proj,
                                                      const int32_t* __restrict__ index, int index_bias, int freq,
                                                      int R, int B, int h, int w, int c_rt, int scale) {
  const int64_t idx = (int64_t)(index ? *index : 0) + index_bias;
  if (idx < 0 || idx % freq != 0 || idx / freq >= R) return;     // uniform: the whole launch writes nothing
  const int c = C > 0 ? C : c_rt;
  const int sh = scale * h, sw = scale * w;
  const int64_t npix = (int64_t)B * sh * sw;                     // pixels of a slot
  const int64_t slot_bytes = npix * 3;
  const int64_t items = (npix + kPix - 1) / kPix;                // per source
  const int64_t total = items * (b.lat ? 2 : 1);
  float pw[C > 0 ? (C + 1) * 3 : 1];
  if constexpr (C > 0) {
#pragma unroll
    for (int i = 0; i < (C + 1) * 3; ++i) pw[i] = proj[i];
  }
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < total; it += (int64_t)gridDim.x * 256) {
    const bool second = it >= items;
    const int64_t g = second ? it - items : it;
    const float* __restrict__ lat = second ? b.lat : a.lat;
    uint8_t* out = (second ? b.frames : a.frames) + (idx / freq) * slot_bytes;
    const int64_t p0 = g * kPix;
    int xo, yo, bi;
    if (npix <= INT32_MAX) {                                     // uniform: 32-bit divisions where the slot allows
      const uint32_t row = (uint32_t)p0 / (uint32_t)sw;
      xo = (int)((uint32_t)p0 - row * (uint32_t)sw);
      bi = (int)(row / (uint32_t)sh);
      yo = (int)(row - (uint32_t)bi * (uint32_t)sh);
    } else {
      int64_t r = p0;
      xo = (int)(r % sw); r /= sw;
      yo = (int)(r % sh);
      bi = (int)(r / sh);
    }
    const int n = (int)(npix - p0 < kPix ? npix - p0 : kPix);
    Tap2 ty = axis_tap<MODE>(h, scale, yo);                      // (again below when the item crosses a row end)
    uint32_t bytes[kPix * 3];
#pragma unroll
    for (int p = 0; p < kPix; ++p) {
      bytes[3 * p] = bytes[3 * p + 1] = bytes[3 * p + 2] = 0;
      if (p < n) {
        const Tap2 tx = axis_tap<MODE>(w, scale, xo);
        const float* img = lat + (int64_t)bi * h * w * c;
        const float* s00 = img + ((int64_t)ty.i0 * w + tx.i0) * c;
        float v0, v1, v2;
        if constexpr (C > 0) {
          v0 = pw[3 * C]; v1 = pw[3 * C + 1]; v2 = pw[3 * C + 2];
        } else {
          v0 = proj[3 * c]; v1 = proj[3 * c + 1]; v2 = proj[3 * c + 2];
        }
        if constexpr (MODE == LDM_PREVIEW_NEAREST) {
#pragma unroll
          for (int j = 0; j < (C > 0 ? C : kMaxC); ++j) {
            if (C == 0 && j >= c) break;
            const float aj = s00[j];
            const float* pj = C > 0 ? pw + 3 * j : proj + 3 * j;
            v0 = __builtin_fmaf(aj, pj[0], v0);
            v1 = __builtin_fmaf(aj, pj[1], v1);
            v2 = __builtin_fmaf(aj, pj[2], v2);
          }
        } else {
          const float* s01 = img + ((int64_t)ty.i0 * w + tx.i1) * c;
          const float* s10 = img + ((int64_t)ty.i1 * w + tx.i0) * c;
          const float* s11 = img + ((int64_t)ty.i1 * w + tx.i1) * c;
          const float w00 = ty.w0 * tx.w0, w01 = ty.w0 * tx.w1, w10 = ty.w1 * tx.w0, w11 = ty.w1 * tx.w1;
#pragma unroll
          for (int j = 0; j < (C > 0 ? C : kMaxC); ++j) {
            if (C == 0 && j >= c) break;
            float aj = __builtin_fmaf(w00, s00[j], 0.0f);
            aj = __builtin_fmaf(w01, s01[j], aj);
            aj = __builtin_fmaf(w10, s10[j], aj);
            aj = __builtin_fmaf(w11, s11[j], aj);
            const float* pj = C > 0 ? pw + 3 * j : proj + 3 * j;
            v0 = __builtin_fmaf(aj, pj[0], v0);
            v1 = __builtin_fmaf(aj, pj[1], v1);
            v2 = __builtin_fmaf(aj, pj[2], v2);
          }
        }
        bytes[3 * p] = quantise(v0);
        bytes[3 * p + 1] = quantise(v1);
        bytes[3 * p + 2] = quantise(v2);
        if (++xo == sw) {
          xo = 0;
          if (++yo == sh) { yo = 0; ++bi; }
          ty = axis_tap<MODE>(h, scale, yo);
        }
      }
    }
    uint8_t* dst = out + p0 * 3;
    if (n == kPix && (uintptr_t)out % 4 == 0) {                  // p0 * 3 is a multiple of 12
      uint32_t* d = (uint32_t*)dst;
#pragma unroll
      for (int k = 0; k < 3; ++k)
        d[k] = bytes[4 * k] | (bytes[4 * k + 1] << 8) | (bytes[4 * k + 2] << 16) | (bytes[4 * k + 3] << 24);
    } else {
#pragma unroll
      for (int k = 0; k < kPix * 3; ++k)
        if (k < 3 * n) dst[k] = (uint8_t)bytes[k];
    }
  }
}

template <int MODE>
void launch(Src a, Src b, const float* proj, const int32_t* index, int index_bias, int freq, int R, int B, int h, int w,
            int c, int scale, hipStream_t s) {
  const int64_t items = ((int64_t)B * scale * h * scale * w + kPix - 1) / kPix * (b.lat ? 2 : 1);
  const dim3 g(grid_for(items, 256, 4096));
#define LDM_PREVIEW_LAUNCH(C) \
  hipLaunchKernelGGL((preview_kernel<MODE, C>), g, dim3(256), 0, s, a, b, proj, index, index_bias, freq, R, B, h, w, c, scale)
  if (c == 4) LDM_PREVIEW_LAUNCH(4);
  else if (c == 3) LDM_PREVIEW_LAUNCH(3);
  else LDM_PREVIEW_LAUNCH(0);
#undef LDM_PREVIEW_LAUNCH
}

}  // namespace

extern "C" int ldm_latent_preview(const float* lat_a, const float* lat_b, const float* proj, uint8_t* frames_a,
                                  uint8_t* frames_b, const int32_t* index, int index_bias, int freq, int R, int B,
                                  int h, int w, int c, int scale, int mode, void* stream) {
  LDM_CHECK_ARG(lat_a && proj && frames_a, "ldm_latent_preview: null pointer");
  LDM_CHECK_ARG((lat_b != nullptr) == (frames_b != nullptr),
                "ldm_latent_preview: lat_b and frames_b must be given together (lat_b=%p, frames_b=%p)", (const void*)lat_b,
                (void*)frames_b);
  LDM_CHECK_ARG(mode == LDM_PREVIEW_NEAREST || mode == LDM_PREVIEW_BILINEAR, "ldm_latent_preview: unknown mode %d", mode);
  LDM_CHECK_ARG(c >= 1 && c <= kMaxC, "ldm_latent_preview: c=%d outside 1..%d", c, kMaxC);
  LDM_CHECK_ARG(scale >= 1 && scale <= 16, "ldm_latent_preview: scale=%d outside 1..16", scale);
  LDM_CHECK_ARG(freq >= 1 && R >= 1, "ldm_latent_preview: bad args (freq=%d, R=%d)", freq, R);
  LDM_CHECK_ARG(B >= 1 && h >= 1 && w >= 1, "ldm_latent_preview: bad args (B=%d, h=%d, w=%d)", B, h, w);
  LDM_CHECK_ARG((int64_t)scale * h <= INT32_MAX && (int64_t)scale * w <= INT32_MAX,
                "ldm_latent_preview: frame extents %lld x %lld exceed int32", (long long)scale * h, (long long)scale * w);
  // scale 1: every source coordinate is an integer and the bilinear weights are (1, 0); the copy keeps an infinity
  // times the zero weight from becoming a NaN
  if (scale == 1) mode = LDM_PREVIEW_NEAREST;
  const Src a = {lat_a, frames_a}, b = {lat_b, frames_b};
  hipStream_t s = (hipStream_t)stream;
  if (mode == LDM_PREVIEW_NEAREST) launch<LDM_PREVIEW_NEAREST>(a, b, proj, index, index_bias, freq, R, B, h, w, c, scale, s);
  else launch<LDM_PREVIEW_BILINEAR>(a, b, proj, index, index_bias, freq, R, B, h, w, c, scale, s);
  return ldm_launch_status("ldm_latent_preview");
}
