// Cross-attention heat maps: acc [R][T][Tk] float32 += w * the head-averaged softmax
// probabilities of q [R][T][heads*sp] against k [R][Tk][heads*sp], the tensor the flash kernels never write.  The weight
// w comes from a device-resident step index, so the launch sits inside a captured sampling step.
//
// Per (row r, query t): for each head h in ascending order l[j] = log2_scale * sum_{d<S} q[h*sp+d] k[j][h*sp+d] (fma
// chain over d ascending from 0), m = max_j l[j], e[j] = exp2(l[j] - m), p[j] = e[j] * rcp(sum_j e[j]) (sum ascending),
// hs[j] += p[j]; then acc[j] = fma(w, hs[j] * (1/heads), acc[j]).  All float32; the dims d in [S, sp) are never read
// into a product.
//
// Thread map: a workgroup is one wave and owns kRows = 64 consecutive queries of one row r, one lane per query, with
// the Tk logits and the Tk head sums of its query in registers (every index below is a compile-time constant after
// unrolling).  The key slice of (r, h) is the same for all lanes: it is staged in LDS as float32 [Tk8][S8] (both
// rounded up to 8, the padding zero) and read as broadcast 16-byte loads, eight keys per uniform branch.  The lane's
// query values come as 16-byte loads of eight dims, the next chunk's issued ahead of the current one's products.  At
// the end the tile's 64 x Tk block of acc, which is one contiguous run, is read-modified-written through LDS (row
// stride Tk | 1, odd, so the lanes' column writes spread over the banks), consecutive lanes on consecutive floats.
// One thread owns each acc element: no atomics.
#include "common.h"

namespace {

constexpr int kRows = 64;        // queries per workgroup (one wave)
constexpr int kMaxTk = 80;
constexpr int kGroups = kMaxTk / 8;

// Eight dims d0 .. d0+7 of one head, as they lie in memory: 16-byte loads (VEC; d0 + 8 <= S8 <= sp, so the chunk lies
// inside the head's padded slice) or element loads of the dims below S.  `raw8` is the load, issued ahead of its use;
// `to_f32` unpacks it and zeroes the dims from S on, whatever they hold (a NaN too).
template <typename T> struct Raw8 { u32x4 a, b; };

template <typename T, bool VEC>
__device__ __forceinline__ Raw8<T> raw8(const T* __restrict__ p, int d0, int S) {
  Raw8<T> r;
  r.a = r.b = u32x4{0u, 0u, 0u, 0u};
  if constexpr (VEC) {
    r.a = *(const u32x4*)(p + d0);
    if constexpr (sizeof(T) == 4) r.b = *(const u32x4*)(p + d0 + 4);
  } else if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (d0 + i < S) r.a[i] = *(const uint32_t*)(p + d0 + i);
      if (d0 + 4 + i < S) r.b[i] = *(const uint32_t*)(p + d0 + 4 + i);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t lo = d0 + 2 * i < S ? p[d0 + 2 * i] : 0u, hi = d0 + 2 * i + 1 < S ? p[d0 + 2 * i + 1] : 0u;
      r.a[i] = lo | (hi << 16);
    }
  }
  return r;
}

template <typename T>
__device__ __forceinline__ void to_f32(const Raw8<T>& r, int d0, int S, float (&v)[8]) {
  if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[i] = __uint_as_float(r.a[i]);
      v[4 + i] = __uint_as_float(r.b[i]);
    }
  } else {
    chunk_to_f32(r.a, v, bf16_t());
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = d0 + i < S ? v[i] : 0.0f;
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kRows) void xattn_map_kernel(const T* __restrict__ q, int64_t ldq, int64_t q_bs,
                                                          const T* __restrict__ k, int64_t ldk, int64_t k_bs,
                                                          float* __restrict__ acc, int heads, int Tq, int Tk, int S,
                                                          int sp, int tiles, float log2_scale, float inv_heads,
                                                          const float* __restrict__ step_w, int n_w,
                                                          const int32_t* __restrict__ index, int index_bias) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float w = 1.0f;
  if (step_w) {                                                  // uniform: the whole launch writes nothing
    const int64_t idx = (int64_t)(index ? *index : 0) + index_bias;
    if (idx < 0 || idx >= n_w) return;
    w = step_w[idx];
    if (w == 0.0f) return;
  }
  const int lane = threadIdx.x;
  const int r = blockIdx.x / tiles;
  const int t0 = (blockIdx.x - r * tiles) * kRows;
  const int nrows = Tq - t0 < kRows ? Tq - t0 : kRows;
  const int t = t0 + (lane < nrows ? lane : nrows - 1);          // (lanes past the end repeat the last query, unstored)
  const int S8 = (S + 7) & ~7, Tk8 = (Tk + 7) & ~7;
  const T* __restrict__ qrow = q + (int64_t)r * q_bs + (int64_t)t * ldq;
  const T* __restrict__ kb = k + (int64_t)r * k_bs;

  float hs[kMaxTk];
#pragma unroll
  for (int j = 0; j < kMaxTk; ++j) hs[j] = 0.0f;

  for (int h = 0; h < heads; ++h) {
    // the key slice of (r, h) as float32 [Tk8][S8], zero where j >= Tk or d >= S: chunks of eight dims, four loads
    // of a lane in flight
    const uint32_t cpr = (uint32_t)S8 >> 3, nc = (uint32_t)Tk8 * cpr;
    for (uint32_t c0 = lane; c0 < nc; c0 += 4 * kRows) {
      Raw8<T> raw[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t c = c0 + u * kRows, j = c / cpr, d0 = (c - j * cpr) << 3;
        raw[u].a = raw[u].b = u32x4{0u, 0u, 0u, 0u};
        if (c < nc && (int)j < Tk) raw[u] = raw8<T, VEC>(kb + (int64_t)j * ldk + h * sp, (int)d0, S);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t c = c0 + u * kRows, j = c / cpr, d0 = (c - j * cpr) << 3;
        if (c < nc) {
          float v[8];
          to_f32<T>(raw[u], (int)d0, S, v);
          *(f32x4*)(smem + c * 8) = f32x4{v[0], v[1], v[2], v[3]};
          *(f32x4*)(smem + c * 8 + 4) = f32x4{v[4], v[5], v[6], v[7]};
        }
      }
    }
    __syncthreads();
    float l[kMaxTk];
#pragma unroll
    for (int j = 0; j < kMaxTk; ++j) l[j] = 0.0f;
    Raw8<T> qnext = raw8<T, VEC>(qrow + h * sp, 0, S);
    for (int d0 = 0; d0 < S8; d0 += 8) {
      float qv[8];
      to_f32<T>(qnext, d0, S, qv);
      if (d0 + 8 < S8) qnext = raw8<T, VEC>(qrow + h * sp, d0 + 8, S);      // (ahead of this chunk's products)
#pragma unroll
      for (int g = 0; g < kGroups; ++g) {
        if (g * 8 < Tk) {                                        // uniform
#pragma unroll
          for (int jj = 0; jj < 8; ++jj) {
            const int j = g * 8 + jj;
            const f32x4 ka = *(const f32x4*)(smem + j * S8 + d0), kc = *(const f32x4*)(smem + j * S8 + d0 + 4);
            float a = l[j];
#pragma unroll
            for (int i = 0; i < 4; ++i) a = __builtin_fmaf(qv[i], ka[i], a);
#pragma unroll
            for (int i = 0; i < 4; ++i) a = __builtin_fmaf(qv[4 + i], kc[i], a);
            l[j] = a;
          }
        }
      }
    }
    float m = -INFINITY;
#pragma unroll
    for (int g = 0; g < kGroups; ++g) {
      if (g * 8 < Tk) {
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
          const int j = g * 8 + jj;
          l[j] *= log2_scale;
          m = j < Tk ? fmaxf(m, l[j]) : m;
        }
      }
    }
    float sum = 0.0f;
#pragma unroll
    for (int g = 0; g < kGroups; ++g) {
      if (g * 8 < Tk) {
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
          const int j = g * 8 + jj;
          const float e = j < Tk ? __builtin_amdgcn_exp2f(l[j] - m) : 0.0f;
          l[j] = e;
          sum += e;
        }
      }
    }
    const float inv = __builtin_amdgcn_rcpf(sum);
#pragma unroll
    for (int g = 0; g < kGroups; ++g) {
      if (g * 8 < Tk) {
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
          const int j = g * 8 + jj;
          hs[j] += l[j] * inv;
        }
      }
    }
    __syncthreads();                                             // (the next head's keys, or the tile, overwrite smem)
  }

  // the tile's [nrows][Tk] block of acc through LDS
  const int ldt = Tk | 1;
#pragma unroll
  for (int g = 0; g < kGroups; ++g) {
    if (g * 8 < Tk) {
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const int j = g * 8 + jj;
        if (j < Tk) smem[lane * ldt + j] = hs[j] * inv_heads;
      }
    }
  }
  __syncthreads();
  float* __restrict__ tile = acc + ((int64_t)r * Tq + t0) * Tk;
  const uint32_t n = (uint32_t)(nrows * Tk);
  for (uint32_t e = lane; e < n; e += kRows) {
    const uint32_t row = e / (uint32_t)Tk, j = e - row * (uint32_t)Tk;
    tile[e] = __builtin_fmaf(w, smem[row * ldt + j], tile[e]);
  }
}

bool sp_ok(int sp) { return sp == 32 || sp == 48 || sp == 64 || sp == 80 || sp == 96 || sp == 160; }

template <typename T>
void launch(const void* q, int64_t ldq, int64_t q_bs, const void* k, int64_t ldk, int64_t k_bs, float* acc, int R,
            int heads, int Tq, int Tk, int S, int sp, float log2_scale, const float* step_w, int n_w,
            const int32_t* index, int index_bias, hipStream_t s) {
  const int tiles = (Tq + kRows - 1) / kRows;
  const int S8 = (S + 7) & ~7, Tk8 = (Tk + 7) & ~7;
  const int keys = Tk8 * S8, tile = kRows * (Tk | 1);
  const size_t lds = sizeof(float) * (size_t)(keys > tile ? keys : tile);          // at most 80 * 160 * 4 = 51200 bytes
  const bool vec = (uintptr_t)q % 16 == 0 && ldq * sizeof(T) % 16 == 0 && q_bs * sizeof(T) % 16 == 0 &&
                   (uintptr_t)k % 16 == 0 && ldk * sizeof(T) % 16 == 0 && k_bs * sizeof(T) % 16 == 0;
  const dim3 g((unsigned)((int64_t)R * tiles));
  const float inv_heads = 1.0f / (float)heads;
#define LDM_XMAP_LAUNCH(VEC)                                                                                        \
  hipLaunchKernelGGL((xattn_map_kernel<T, VEC>), g, dim3(kRows), lds, s, (const T*)q, ldq, q_bs, (const T*)k, ldk,  \
                     k_bs, acc, heads, Tq, Tk, S, sp, tiles, log2_scale, inv_heads, step_w, n_w, index, index_bias)
  if (vec) LDM_XMAP_LAUNCH(true);
  else LDM_XMAP_LAUNCH(false);
#undef LDM_XMAP_LAUNCH
}

}  // namespace

extern "C" int ldm_xattn_map_supported(int heads, int Tk, int S, int sp, int dtype) {
  return heads >= 1 && Tk >= 1 && Tk <= kMaxTk && S >= 1 && S <= sp && sp_ok(sp) && DT_OK(dtype);
}

extern "C" int ldm_xattn_map(const void* q, int64_t ldq, int64_t q_bs, const void* k, int64_t ldk, int64_t k_bs,
                             float* acc, int R, int heads, int T, int Tk, int S, int sp, float log2_scale, int dtype,
                             const float* step_w, int n_w, const int32_t* index, int index_bias, void* stream) {
  LDM_CHECK_ARG(q && k && acc, "ldm_xattn_map: null pointer");
  LDM_CHECK_ARG(ldm_xattn_map_supported(heads, Tk, S, sp, dtype),
                "ldm_xattn_map: unsupported shape (heads=%d, Tk=%d, S=%d, sp=%d, dtype=%d): Tk in 1..%d, S <= sp, sp one "
                "of 32/48/64/80/96/160", heads, Tk, S, sp, dtype, kMaxTk);
  LDM_CHECK_ARG(R >= 1 && T >= 1, "ldm_xattn_map: bad args (R=%d, T=%d)", R, T);
  LDM_CHECK_ARG(ldq >= (int64_t)heads * sp && ldk >= (int64_t)heads * sp,
                "ldm_xattn_map: row strides (ldq=%lld, ldk=%lld) below heads*sp=%lld", (long long)ldq, (long long)ldk,
                (long long)heads * sp);
  LDM_CHECK_ARG(!step_w || n_w >= 1, "ldm_xattn_map: step_w with n_w=%d", n_w);
  LDM_CHECK_ARG((int64_t)R * ((T + kRows - 1) / kRows) <= INT32_MAX, "ldm_xattn_map: R=%d x T=%d exceeds the grid", R, T);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == LDM_F32)
    launch<float>(q, ldq, q_bs, k, ldk, k_bs, acc, R, heads, T, Tk, S, sp, log2_scale, step_w, n_w, index, index_bias, s);
  else
    launch<bf16_t>(q, ldq, q_bs, k, ldk, k_bs, acc, R, heads, T, Tk, S, sp, log2_scale, step_w, n_w, index, index_bias, s);
  return ldm_launch_status("ldm_xattn_map");
}
