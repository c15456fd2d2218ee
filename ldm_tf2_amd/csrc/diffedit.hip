// DiffEdit: the prompt-contrast accumulator, the mask derived from it, and the row store that
// keeps the inversion trajectory inside the captured inversion step.
//
// ldm_eps_contrast_accum: per cell s = |d_0|, s = s + |d_j| for j = 1 .. c-1 (d_j = e_tgt[j] - e_src[j]), acc = acc + s:
// float32 subtractions, absolute values and additions in that order, no multiply, so nothing contracts and a NumPy
// float32 restatement gives the same bits.  c == 4: a work item is four consecutive cells -- 64 contiguous bytes of
// either half as four 16-byte loads, one 16-byte acc load and store; the cells % 4 tail and every other c take one
// cell per item with scalar accesses.  Both item kinds run the same chain per cell.
//
// ldm_contrast_mask: one 256-thread workgroup per sample.  Strided partial sums, a fixed LDS tree (the same bits on
// every run), the thresholded bytes of the sample in LDS, the dilation read from LDS, then the stores.  The tree's 256
// floats and, at the end, the count's 256 ints alias the first KiB of the byte array: a barrier separates each use, and
// the workgroup's LDS stays at 64 KiB for h w = 65536.
#include "common.h"

namespace {

constexpr int kMaxC = 16;
constexpr int kMaskCells = 65536;      // bytes of LDS a sample's thresholded cells may take
constexpr int kMaxDilate = 3;

inline bool al16(const void* p) { return (uintptr_t)p % 16 == 0; }
inline bool al4(const void* p) { return (uintptr_t)p % 4 == 0; }

// after the launch that read through *counter (stream order): every block of it has read the counter first
__global__ void dec_counter_kernel(int32_t* counter) { *counter = *counter - 1; }

__device__ __forceinline__ float cell_contrast(const float* __restrict__ src, const float* __restrict__ tgt, int c) {
  float s = fabsf(tgt[0] - src[0]);
  for (int j = 1; j < c; ++j) s = s + fabsf(tgt[j] - src[j]);
  return s;
}

__device__ __forceinline__ float cell_contrast4(const f32x4& src, const f32x4& tgt) {
  float s = fabsf(tgt[0] - src[0]);
#pragma unroll
  for (int j = 1; j < 4; ++j) s = s + fabsf(tgt[j] - src[j]);
  return s;
}

// cells = B * cells per sample: the two halves and acc are flat runs over it
__global__ __launch_bounds__(256) void contrast4_kernel(const float* __restrict__ src, const float* __restrict__ tgt,
                                                        float* __restrict__ acc, int64_t cells) {
  const int64_t quads = cells >> 2, items = quads + (cells & 3);
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
    if (it < quads) {
      const int64_t g = it * 4;
      const f32x4 a = *(const f32x4*)(acc + g);
      f32x4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const f32x4 s = *(const f32x4*)(src + (g + k) * 4);
        const f32x4 t = *(const f32x4*)(tgt + (g + k) * 4);
        o[k] = a[k] + cell_contrast4(s, t);
      }
      *(f32x4*)(acc + g) = o;
    } else {
      const int64_t g = quads * 4 + (it - quads);
      acc[g] = acc[g] + cell_contrast(src + g * 4, tgt + g * 4, 4);
    }
  }
}

__global__ __launch_bounds__(256) void contrast_kernel(const float* __restrict__ src, const float* __restrict__ tgt,
                                                       float* __restrict__ acc, int64_t cells, int c) {
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < cells; g += (int64_t)gridDim.x * 256)
    acc[g] = acc[g] + cell_contrast(src + g * c, tgt + g * c, c);
}

__global__ __launch_bounds__(256) void contrast_mask_kernel(const float* __restrict__ acc, float* __restrict__ mask_out,
                                                            float* __restrict__ mean_out, float* __restrict__ thr_out,
                                                            int32_t* __restrict__ count_out, int h, int w, float tau,
                                                            int r) {
  __shared__ __attribute__((aligned(16))) unsigned char cell[kMaskCells];
  float* red = (float*)cell;
  int* ired = (int*)cell;
  const int n = h * w, tid = threadIdx.x;
  const float* a = acc + (int64_t)blockIdx.x * n;
  float* m = mask_out + (int64_t)blockIdx.x * n;

  float s = 0.f;
  for (int p = tid; p < n; p += 256) s += a[p];
  red[tid] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] = red[tid] + red[tid + o];
    __syncthreads();
  }
  const float mean = __fdiv_rn(red[0], (float)n);
  const float thr = tau * mean;
  __syncthreads();                                     // red[0] is read by all before the bytes take its place

  // written exactly so: a NaN (in the cell or in thr) compares false and keeps the cell; an all-zero map has thr = 0
  // and 0 > 0 edits nothing
  for (int p = tid; p < n; p += 256) cell[p] = a[p] > thr ? 1 : 0;
  __syncthreads();

  int cnt = 0;
  for (int p = tid; p < n; p += 256) {
    unsigned e = cell[p];
    if (r > 0) {
      const int y = p / w, x = p - y * w;
      const int y0 = y - r < 0 ? 0 : y - r, y1 = y + r > h - 1 ? h - 1 : y + r;
      const int x0 = x - r < 0 ? 0 : x - r, x1 = x + r > w - 1 ? w - 1 : x + r;
      for (int yy = y0; yy <= y1; ++yy)
        for (int xx = x0; xx <= x1; ++xx) e |= cell[yy * w + xx];
    }
    m[p] = e ? 0.f : 1.f;
    cnt += (int)e;
  }
  __syncthreads();                                     // the last byte is read before the ints take their place
  ired[tid] = cnt;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) ired[tid] = ired[tid] + ired[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    if (mean_out) mean_out[blockIdx.x] = mean;
    if (thr_out) thr_out[blockIdx.x] = thr;
    if (count_out) count_out[blockIdx.x] = ired[0];
  }
}

__global__ __launch_bounds__(256) void store_row_kernel(const float* __restrict__ src, float* __restrict__ table,
                                                        int64_t row_stride, int rows, const int32_t* __restrict__ index,
                                                        int index_sign, int index_bias, int64_t n) {
  const int64_t row = (int64_t)index_sign * (int64_t)(*index) + index_bias;
  if (row < 0 || row >= rows) return;                  // uniform: the whole launch writes nothing
  float* dst = table + row * row_stride;
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (int64_t)gridDim.x * 256 * 4)
    *(f32x4*)(dst + i) = *(const f32x4*)(src + i);
}

}  // namespace

extern "C" int ldm_eps_contrast_accum(const float* eps_all, float* acc, int32_t* counter, int B, int64_t cells, int c,
                                      void* stream) {
  LDM_CHECK_ARG(eps_all && acc, "ldm_eps_contrast_accum: null pointer");
  LDM_CHECK_ARG(B >= 1 && cells >= 1 && c >= 1 && c <= kMaxC,
                "ldm_eps_contrast_accum: bad args (B=%d, cells=%lld, c=%d outside 1..%d)", B, (long long)cells, c, kMaxC);
  LDM_CHECK_ARG(c == 4 ? al16(eps_all) && al16(acc) : al4(eps_all) && al4(acc),
                "ldm_eps_contrast_accum: eps_all and acc must be 16-byte aligned at c = 4 (4-byte at any other c)");
  LDM_CHECK_ARG(!counter || al4(counter), "ldm_eps_contrast_accum: counter must be 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int64_t total = (int64_t)B * cells;
  const float* tgt = eps_all + total * c;              // (c = 4: total * 16 bytes on, still 16-byte aligned)
  if (c == 4)
    hipLaunchKernelGGL(contrast4_kernel, dim3(grid_for((total >> 2) + (total & 3), 256, 4096)), dim3(256), 0, s,
                       eps_all, tgt, acc, total);
  else
    hipLaunchKernelGGL(contrast_kernel, dim3(grid_for(total, 256, 4096)), dim3(256), 0, s, eps_all, tgt, acc, total, c);
  int status = ldm_launch_status("ldm_eps_contrast_accum");
  if (status == LDM_OK && counter) {
    hipLaunchKernelGGL(dec_counter_kernel, dim3(1), dim3(1), 0, s, counter);
    status = ldm_launch_status("ldm_eps_contrast_accum");
  }
  return status;
}

extern "C" int ldm_contrast_mask_supported(int h, int w, int dilate) {
  return h >= 1 && w >= 1 && (int64_t)h * w <= kMaskCells && dilate >= 0 && dilate <= kMaxDilate;
}

extern "C" int ldm_contrast_mask(const float* acc, float* mask_out, float* mean_out, float* thr_out, int32_t* count_out,
                                 int B, int h, int w, float tau, int dilate, void* stream) {
  LDM_CHECK_ARG(acc && mask_out, "ldm_contrast_mask: null pointer");
  LDM_CHECK_ARG(al4(acc) && al4(mask_out) && al4(mean_out) && al4(thr_out) && al4(count_out),
                "ldm_contrast_mask: arrays must be 4-byte aligned");
  LDM_CHECK_ARG(B >= 1, "ldm_contrast_mask: bad args (B=%d)", B);
  LDM_CHECK_ARG(ldm_contrast_mask_supported(h, w, dilate),
                "ldm_contrast_mask: h=%d, w=%d, dilate=%d outside ldm_contrast_mask_supported (h w <= %d, dilate 0..%d)", h,
                w, dilate, kMaskCells, kMaxDilate);
  hipLaunchKernelGGL(contrast_mask_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, acc, mask_out, mean_out, thr_out,
                     count_out, h, w, tau, dilate);
  return ldm_launch_status("ldm_contrast_mask");
}

extern "C" int ldm_store_row(const float* src, float* table, int64_t row_stride, int rows, const int32_t* index,
                             int index_sign, int index_bias, int64_t n, void* stream) {
  LDM_CHECK_ARG(src && table && index, "ldm_store_row: null pointer");
  LDM_CHECK_ARG(n >= 1 && n % 4 == 0 && rows >= 1 && row_stride >= n && row_stride % 4 == 0,
                "ldm_store_row: bad args (n=%lld must be a positive multiple of 4, row_stride=%lld a multiple of 4 of "
                "at least n, rows=%d)", (long long)n, (long long)row_stride, rows);
  LDM_CHECK_ARG(index_sign == 1 || index_sign == -1, "ldm_store_row: index_sign=%d must be 1 or -1", index_sign);
  LDM_CHECK_ARG(al16(src) && al16(table) && al4(index), "ldm_store_row: src and table must be 16-byte aligned");
  hipLaunchKernelGGL(store_row_kernel, dim3(grid_for(n / 4, 256, 1024)), dim3(256), 0, (hipStream_t)stream, src, table,
                     row_stride, rows, index, index_sign, index_bias, n);
  return ldm_launch_status("ldm_store_row");
}
