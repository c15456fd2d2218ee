// Antialiased resample: out [B][Ho][Wo][c] = x [B][H][W][c] resampled with a filter whose
// footprint grows with the shrink factor, float32, in two separable launches: along W into tmp [B][H][Wo][c], then
// along H into out.  The taps and weights of an axis come from a host-built table (ldm_tf2_amd/resample.py): output
// index i reads the `taps` consecutive source indices start[i] .. start[i] + taps - 1 with the weights w[i][0 .. taps),
// zero-filled, and the table keeps every row inside [0, L), so the kernels have no bounds branch.
//
// Nothing is staged in LDS.  A thread owns one output element (or channel quad), channel fastest: in the H pass the
// lanes of a wave read consecutive addresses of one source row per tap (fully coalesced) and in the W pass consecutive
// lanes read the channels of one pixel and then the pixels next to it, whose tap windows overlap, so a line fetched
// once serves the neighbouring lanes.  The weight row of a thread is shared by every lane with the same output index
// (all of a wave in the H pass unless Wo * c < 64) and comes from the cache as a broadcast.
#include "common.h"

namespace {

// One axis.  x is seen as [outer][L][inner] (W pass: outer = B * H, inner = c; H pass: outer = B, inner = Wo * c) and
// out as [outer][Lo][inner]; V = 4 moves a quad of `inner` per thread.  acc = fma(w_j, x_j, acc) for ascending j from
// 0, written as explicit fused multiply-adds: the same instruction chain per element in both paths.  taps == 1 is a
// table whose weights are all exactly 1 (a row of one tap is normalised to 1): the source bits are copied, which
// keeps a -0.0 and a NaN's payload where 1 * x + 0 would not.
template <int V>
__global__ __launch_bounds__(256) void resample_axis_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                            int64_t outer, int L, int Lo, int64_t inner,
                                                            const int32_t* __restrict__ start,
                                                            const float* __restrict__ w, int taps) {
  const int64_t iv = inner / V;
  const int64_t total = outer * Lo * iv;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    int64_t r = i;
    const int64_t e = (r % iv) * V; r /= iv;
    const int o = (int)(r % Lo); r /= Lo;                 // r = the outer index
    const float* src = x + (r * L + start[o]) * inner + e;
    const float* wr = w + (int64_t)o * taps;
    if (taps == 1) {
      if constexpr (V == 4) *(f32x4*)(out + i * 4) = *(const f32x4*)src;
      else out[i] = *src;
      continue;
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < taps; ++j, src += inner) {
      const float wj = wr[j];
      if constexpr (V == 4) {
        const f32x4 v = *(const f32x4*)src;
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = __builtin_fmaf(wj, v[k], acc[k]);
      } else {
        acc[0] = __builtin_fmaf(wj, *src, acc[0]);
      }
    }
    if constexpr (V == 4) *(f32x4*)(out + i * 4) = acc;
    else out[i] = acc[0];
  }
}

inline bool al16(const void* p) { return (uintptr_t)p % 16 == 0; }

void launch_axis(bool wide, const float* x, float* out, int64_t outer, int L, int Lo, int64_t inner,
                 const int32_t* start, const float* w, int taps, hipStream_t s) {
  const int64_t total = outer * Lo * inner;
  const dim3 g(grid_for(wide ? total / 4 : total, 256, 4096));
  if (wide) hipLaunchKernelGGL(resample_axis_kernel<4>, g, dim3(256), 0, s, x, out, outer, L, Lo, inner, start, w, taps);
  else hipLaunchKernelGGL(resample_axis_kernel<1>, g, dim3(256), 0, s, x, out, outer, L, Lo, inner, start, w, taps);
}

}  // namespace

extern "C" int ldm_resample_nhwc(const float* x, float* tmp, float* out, int B, int H, int W, int c, int Ho, int Wo,
                                 const int32_t* xstart, const float* xw, int xtaps, const int32_t* ystart,
                                 const float* yw, int ytaps, void* stream) {
  LDM_CHECK_ARG(x && tmp && out && xstart && xw && ystart && yw, "ldm_resample_nhwc: null pointer");
  LDM_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && c >= 1 && Ho >= 1 && Wo >= 1,
                "ldm_resample_nhwc: bad args (B=%d, H=%d, W=%d, c=%d, Ho=%d, Wo=%d)", B, H, W, c, Ho, Wo);
  LDM_CHECK_ARG(xtaps >= 1 && xtaps <= W && ytaps >= 1 && ytaps <= H,
                "ldm_resample_nhwc: bad taps (xtaps=%d of W=%d, ytaps=%d of H=%d)", xtaps, W, ytaps, H);
  hipStream_t s = (hipStream_t)stream;
  // one decision for both launches: a quad of channels never straddles a pixel, and with c % 4 == 0 every row,
  // pixel and quad of the three buffers is 16-byte aligned when their bases are
  const bool wide = c % 4 == 0 && al16(x) && al16(tmp) && al16(out);
  launch_axis(wide, x, tmp, (int64_t)B * H, W, Wo, c, xstart, xw, xtaps, s);
  launch_axis(wide, tmp, out, B, H, Ho, (int64_t)Wo * c, ystart, yw, ytaps, s);
  return ldm_launch_status("ldm_resample_nhwc");
}
