// Small / HBM-bound kernels of the sampling path: tiny-channel 3x3 convs, timestep
// embedding + skinny Dense, CFG + DDIM update, first-stage prologue, VQ lookup,
// token embedding, per-image min-max -> uint8, casts.
#include "common.h"

namespace {

template <typename T> __device__ __forceinline__ float ldf(const T* p);
template <> __device__ __forceinline__ float ldf<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float ldf<bf16_t>(const bf16_t* p) { return bf2f(*p); }
template <typename T> __device__ __forceinline__ void stf(T* p, float v);
template <> __device__ __forceinline__ void stf<float>(float* p, float v) { *p = v; }
template <> __device__ __forceinline__ void stf<bf16_t>(bf16_t* p, float v) { *p = f2bf(v); }

// ---- conv_in, LDS-resident weights: Cin = 4, Cout % 8 == 0, 9*Cin*Cout floats <= 64 KB --------
// Persistent workgroups keep the whole HWIO kernel in LDS; a work item is (4 consecutive pixels
// of a row, 8 consecutive couts): per input row 6 pixel loads (a 4-channel float pixel is one
// 16-byte load) serve the 3 x 4 taps, every weight pair (2 ds_read_b128) is used for 4 pixels,
// one 16-byte store per pixel.  Same accumulation order per output as the kernel below.
template <typename TI, typename TO, int CIN>
__global__ __launch_bounds__(256, 2) void conv_in_lds_kernel(const TI* __restrict__ x, int64_t ldx,
                                                          const float* __restrict__ w,
                                                          const float* __restrict__ bias,
                                                          TO* __restrict__ out, int64_t ldo, int B, int H,
                                                          int W, int Cout) {
  extern __shared__ __attribute__((aligned(16))) float sw[];      // [9*CIN][Cout]
  const int nw = 9 * CIN * Cout;
  for (int i = threadIdx.x * 4; i < nw; i += 256 * 4) *(f32x4*)(sw + i) = *(const f32x4*)(w + i);
  __syncthreads();
  const int c8n = Cout >> 3, wg4 = (W + 3) >> 2;
  const int64_t total = (int64_t)B * H * wg4 * c8n;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int c8 = (int)(idx % c8n) * 8;
    const int64_t g = idx / c8n;
    const int ox0 = (int)(g % wg4) * 4, oy = (int)((g / wg4) % H), b = (int)(g / ((int64_t)wg4 * H));
    float acc[4][8];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[j][e] = bias ? bias[c8 + e] : 0.f;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int iy = oy + kh - 1;
      if ((unsigned)iy >= (unsigned)H) continue;
      float xr[6][CIN];
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        const int ix = ox0 + q - 1;
        const bool ok = (unsigned)ix < (unsigned)W;
        const TI* xp = x + ((int64_t)(b * H + iy) * W + (ok ? ix : 0)) * ldx;
        if constexpr (CIN == 4 && sizeof(TI) == 4) {
          const f32x4 v = *(const f32x4*)xp;
#pragma unroll
          for (int ci = 0; ci < 4; ++ci) xr[q][ci] = ok ? v[ci] : 0.f;
        } else {
#pragma unroll
          for (int ci = 0; ci < CIN; ++ci) xr[q][ci] = ok ? ldf<TI>(xp + ci) : 0.f;
        }
      }
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const float* wp = sw + (kh * 3 + kw) * CIN * Cout + c8;
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci) {
          const f32x4 w0 = *(const f32x4*)(wp + ci * Cout), w1 = *(const f32x4*)(wp + ci * Cout + 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float xv = xr[j + kw][ci];
#pragma unroll
            for (int e = 0; e < 4; ++e) { acc[j][e] += xv * w0[e]; acc[j][4 + e] += xv * w1[e]; }
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (ox0 + j >= W) break;
      TO* op = out + ((int64_t)(b * H + oy) * W + ox0 + j) * ldo + c8;
      if constexpr (sizeof(TO) == 2) {
        *(u32x4*)op = f32_to_chunk(acc[j], bf16_t());
      } else {
        f32x4 o0 = {acc[j][0], acc[j][1], acc[j][2], acc[j][3]}, o1 = {acc[j][4], acc[j][5], acc[j][6], acc[j][7]};
        *(f32x4*)op = o0;
        *(f32x4*)(op + 4) = o1;
      }
    }
  }
}

// ---- conv_in: Cin <= 8, any Cout.  thread = (pixel, 4 consecutive couts) -------
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void conv_small_in_kernel(const TI* __restrict__ x, int64_t ldx,
                                                            const float* __restrict__ w,
                                                            const float* __restrict__ bias,
                                                            TO* __restrict__ out, int64_t ldo, int B,
                                                            int H, int W, int Cin, int Cout) {
  const int cq = Cout >> 2;
  const int64_t total = (int64_t)B * H * W * cq;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * 256) {
    const int c4 = (int)(idx % cq) * 4;
    const int64_t pix = idx / cq;
    const int ox = (int)(pix % W), oy = (int)((pix / W) % H), b = (int)(pix / ((int64_t)W * H));
    float acc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = bias ? bias[c4 + e] : 0.f;
    for (int kh = 0; kh < 3; ++kh) {
      const int iy = oy + kh - 1;
      if ((unsigned)iy >= (unsigned)H) continue;
      for (int kw = 0; kw < 3; ++kw) {
        const int ix = ox + kw - 1;
        if ((unsigned)ix >= (unsigned)W) continue;
        const TI* xp = x + ((int64_t)(b * H + iy) * W + ix) * ldx;
        const float* wp = w + (int64_t)((kh * 3 + kw) * Cin) * Cout + c4;
        for (int ci = 0; ci < Cin; ++ci) {
          const float xv = ldf<TI>(xp + ci);
          const f32x4 wv = *(const f32x4*)(wp + (int64_t)ci * Cout);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] += xv * wv[e];
        }
      }
    }
    TO* op = out + pix * ldo + c4;
#pragma unroll
    for (int e = 0; e < 4; ++e) stf<TO>(op + e, acc[e]);
  }
}

// ---- conv_out: Cout <= 4, Cin multiple of 16-byte chunks.  One wave = 8 pixels,
// 8 lanes split the 9*Cin reduction of one pixel; weights [9*Cin][Cout] f32 in LDS.
template <typename TI, typename TO, int COUT>
__global__ __launch_bounds__(256) void conv_small_out_kernel(const TI* __restrict__ x, int64_t ldx,
                                                             const float* __restrict__ w,
                                                             const float* __restrict__ bias,
                                                             TO* __restrict__ out, int64_t ldo,
                                                             int B, int H, int W, int Cin) {
  constexpr int EPC = Elem<TI>::kPerChunk;
  extern __shared__ __attribute__((aligned(16))) float sw[];  // [9*Cin][COUT]
  const int nw = 9 * Cin * COUT;
  for (int i = threadIdx.x; i < nw; i += 256) sw[i] = w[i];
  __syncthreads();
  const int sub = threadIdx.x & 7;
  const int64_t npix = (int64_t)B * H * W;
  const int nvec = Cin / EPC;
  for (int64_t pix = (int64_t)blockIdx.x * 32 + (threadIdx.x >> 3); pix < npix;
       pix += (int64_t)gridDim.x * 32) {
    const int ox = (int)(pix % W), oy = (int)((pix / W) % H), b = (int)(pix / ((int64_t)W * H));
    float acc[COUT];
#pragma unroll
    for (int e = 0; e < COUT; ++e) acc[e] = 0.f;
    for (int kh = 0; kh < 3; ++kh) {
      const int iy = oy + kh - 1;
      if ((unsigned)iy >= (unsigned)H) continue;
      for (int kw = 0; kw < 3; ++kw) {
        const int ix = ox + kw - 1;
        if ((unsigned)ix >= (unsigned)W) continue;
        const TI* xp = x + ((int64_t)(b * H + iy) * W + ix) * ldx;
        const float* wp = sw + (kh * 3 + kw) * Cin * COUT;
        for (int v = sub; v < nvec; v += 8) {
          const u32x4 c = *(const u32x4*)(xp + v * EPC);
          float f[EPC];
          chunk_to_f32(c, f, TI());
#pragma unroll
          for (int e = 0; e < EPC; ++e) {
            const float* wr = wp + (v * EPC + e) * COUT;
#pragma unroll
            for (int co = 0; co < COUT; ++co) acc[co] += f[e] * wr[co];
          }
        }
      }
    }
#pragma unroll
    for (int co = 0; co < COUT; ++co) {
      float v = acc[co];
      v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64);
      acc[co] = v;
    }
    if (sub == 0) {
      TO* op = out + pix * ldo;
#pragma unroll
      for (int co = 0; co < COUT; ++co) stf<TO>(op + co, acc[co] + (bias ? bias[co] : 0.f));
    }
  }
}

// ---- timestep embedding -------------------------------------------------------
__global__ void time_embedding_kernel(const int32_t* __restrict__ t_rows,
                                      const int32_t* __restrict__ steps,
                                      const int32_t* __restrict__ index, float* __restrict__ out,
                                      int rows, int channels) {
  const int half = channels / 2;
  const int total = rows * half;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int r = i / half, k = i - r * half;
    const int t = index ? steps[*index] : t_rows[r];
    // freqs = exp(-ln(10000) * k / half) in float32 (unet.py:413-416)
    const float f = expf(-logf(10000.0f) * (float)k / (float)half);
    const float a = (float)t * f;
    out[(int64_t)r * channels + k] = cosf(a);
    out[(int64_t)r * channels + half + k] = sinf(a);
    if ((channels & 1) && k == 0) out[(int64_t)r * channels + channels - 1] = 0.f;
  }
}

// ---- skinny Dense: one wave per output column n, all rows at once (rows <= 64) ---
template <typename T, int RT>
__global__ __launch_bounds__(256) void gemv_kernel(const float* __restrict__ x, int64_t ldx,
                                                   const T* __restrict__ wt,
                                                   const float* __restrict__ bias,
                                                   float* __restrict__ y, int64_t ldy, int rows, int N,
                                                   int K, int act_in, int act_out) {
  constexpr int EPC = Elem<T>::kPerChunk;
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const int r0 = blockIdx.y * RT;
  float acc[RT];
#pragma unroll
  for (int r = 0; r < RT; ++r) acc[r] = 0.f;
  const T* wr = wt + (int64_t)n * K;
  for (int k = lane * EPC; k < K; k += 64 * EPC) {
    const u32x4 c = *(const u32x4*)(wr + k);
    float wv[EPC];
    chunk_to_f32(c, wv, T());
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      if (r0 + r < rows) {
        const float* xr = x + (int64_t)(r0 + r) * ldx + k;
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
          float xv = xr[e];
          if (act_in == LDM_ACT_SILU) xv = silu_f(xv);
          acc[r] += xv * wv[e];
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    const float s = wave_sum(acc[r]);
    if (lane == 0 && r0 + r < rows) {
      float v = s + (bias ? bias[n] : 0.f);
      if (act_out == LDM_ACT_SILU) v = silu_f(v);
      y[(int64_t)(r0 + r) * ldy + n] = v;
    }
  }
}

// ---- forward diffusion q(x_t | x_0) -------------------------------------------------
// model_runners.py:580-600: xt = _extract(sqrt_ac, t) * x0 + _extract(sqrt_1m_ac, t) * eps, the coefficients
// float32 (cast, then gathered).  One inline body serves ldm_q_sample and the blend of the masked DDIM update, so
// a kept latent cell is bit for bit the q_sample of its init latent.
__device__ __forceinline__ float q_sample_f(float sa, float sb, float x0, float eps) { return sa * x0 + sb * eps; }

template <typename TX>
__global__ __launch_bounds__(256) void q_sample_kernel(const float* __restrict__ x0, const float* __restrict__ noise,
                                                       int64_t noise_stride, const int32_t* index,
                                                       const int32_t* __restrict__ t,
                                                       const float* __restrict__ sqrt_ac,
                                                       const float* __restrict__ sqrt_1m_ac, int num_steps,
                                                       float* __restrict__ xt_out, TX* __restrict__ x_unet, int B,
                                                       int64_t n) {
  if (index) noise += (int64_t)(*index) * noise_stride;
  const int64_t total = (int64_t)B * n;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    int ti = t[i / n];
    ti = ti < 0 ? 0 : (ti >= num_steps ? num_steps - 1 : ti);      // (a stray t reads a valid row)
    const float o = q_sample_f(sqrt_ac[ti], sqrt_1m_ac[ti], x0[i], noise[i]);
    xt_out[i] = o;
    if (x_unet) { stf<TX>(x_unet + i, o); stf<TX>(x_unet + total + i, o); }
  }
}

// ---- CFG + DDIM update (+ inpainting blend) -----------------------------------------------
// Blend = false is ldm_cfg_ddim_update.  Blend = true (ldm_cfg_ddim_update_masked) pins the kept cells to the
// init latent before the NEXT step (index idx - 1) reads them: o <- m * q_sample(z0, steps[idx-1], Q[idx-1])
// + (1 - m) * o, skipped at idx = 0 (its output goes to the decoder as it is).
struct BlendArgs {
  const float* z0;        // [B][n]
  const float* mask;      // [B][n / channels]
  const float* q_noise;   // Q table, row j at q_noise + j * q_stride
  int64_t q_stride;
  const float* q_coef;    // [N_steps][2]: (sqrt_ac, sqrt_1m_ac) at steps[j], float32
  int channels;
};

template <typename TX, bool Blend>
__global__ __launch_bounds__(256) void cfg_ddim_kernel(const float* __restrict__ eps_all,
                                                       const float* __restrict__ xt,
                                                       const float* __restrict__ noise,
                                                       int64_t noise_stride,
                                                       float* __restrict__ xt_out,
                                                       float* __restrict__ pred_x0_out,
                                                       TX* __restrict__ x_unet, const float* coef,
                                                       int32_t* index, int dec_index, float gs,
                                                       int clip, int B, int64_t n, BlendArgs bl) {
  const int idx = *index;
  if (noise) noise += (int64_t)idx * noise_stride;
  const float c1 = coef[idx * 4 + 0], c2 = coef[idx * 4 + 1];
  const float a_prev = coef[idx * 4 + 2], sigma = coef[idx * 4 + 3];
  const float sa = sqrtf(a_prev);
  const float sb = sqrtf(1.0f - a_prev - sigma * sigma);
  bool blend = false;
  float qa = 0.f, qb = 0.f;
  const float* qn = nullptr;
  if constexpr (Blend) {
    blend = idx >= 1;                                // never reads a table at -1
    if (blend) {
      qa = bl.q_coef[(idx - 1) * 2 + 0];
      qb = bl.q_coef[(idx - 1) * 2 + 1];
      qn = bl.q_noise + (int64_t)(idx - 1) * bl.q_stride;
    }
  }
  const int64_t total = (int64_t)B * n;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const float eu = eps_all[i], ec = eps_all[total + i];
    const float eps = eu + gs * (ec - eu);
    const float x = xt[i];
    float x0 = c1 * x - c2 * eps;
    if (clip) x0 = fminf(fmaxf(x0, -1.f), 1.f);
    const float mean = sa * x0 + sb * eps;
    float o = mean + (noise ? noise[i] : 0.f) * sigma;
    if constexpr (Blend) {
      if (blend) {
        const float m = bl.mask[i / bl.channels];    // i = (b * n + pixel * channels + c) -> b * (n / channels) + pixel
        const float q = q_sample_f(qa, qb, bl.z0[i], qn[i]);
        o = m * q + (1.f - m) * o;
      }
    }
    xt_out[i] = o;
    if (pred_x0_out) pred_x0_out[i] = x0;
    if (x_unet) { stf<TX>(x_unet + i, o); stf<TX>(x_unet + total + i, o); }
  }
}
// decrement happens in its own 1-thread kernel AFTER the update so that every block
// of the update kernel has read *index first
__global__ void dec_index_kernel(int32_t* index) { *index = *index - 1; }

// ---- CFG + PLMS update (+ inpainting blend) -----------------------------------------------
// The sigma = 0 update above with eps replaced by e', the Adams-Bashforth combination of this step's guided eps
// and the j = clamp(*start - idx, 0, 3) before it (rows of model_runners.PLMS_WEIGHTS: (1), (3,-1)/2,
// (23,-16,5)/12, (55,-59,37,-9)/24).  ring [4][B][n]: e_i goes to slot idx & 3, slots (idx+1 .. idx+j) & 3 are
// read; j is uniform over the launch, so a slot beyond j is never loaded (it may hold NaN).  Four elements per
// thread, 16-byte accesses (the launcher checks n % 4 and the alignments).  xt_out may be xt.
__device__ __forceinline__ void st4(float* p, const f32x4& v) { *(f32x4*)p = v; }
__device__ __forceinline__ void st4(bf16_t* p, const f32x4& v) {
  u32x2 c;
  c[0] = pack_bf2(v[0], v[1]);
  c[1] = pack_bf2(v[2], v[3]);
  *(u32x2*)p = c;
}

template <typename TX, bool Blend>
__global__ __launch_bounds__(256) void cfg_plms_kernel(const float* __restrict__ eps_all, const float* xt,
                                                       float* __restrict__ ring, float* xt_out,
                                                       float* __restrict__ pred_x0_out, TX* __restrict__ x_unet,
                                                       const float* coef, const int32_t* index,
                                                       const int32_t* start, float gs, int B, int64_t n,
                                                       BlendArgs bl) {
  const int idx = *index;
  const int d = *start - idx;
  const int j = d < 0 ? 0 : (d > 3 ? 3 : d);
  const float c1 = coef[idx * 4 + 0], c2 = coef[idx * 4 + 1], a_prev = coef[idx * 4 + 2];
  const float sa = sqrtf(a_prev);
  const float sb = sqrtf(1.0f - a_prev);
  const int64_t total = (int64_t)B * n;
  float* e_out = ring + (int64_t)(idx & 3) * total;
  const float* e1 = ring + (int64_t)((idx + 1) & 3) * total;
  const float* e2 = ring + (int64_t)((idx + 2) & 3) * total;
  const float* e3 = ring + (int64_t)((idx + 3) & 3) * total;
  bool blend = false;
  float qa = 0.f, qb = 0.f;
  const float* qn = nullptr;
  if constexpr (Blend) {
    blend = idx >= 1;                                // never reads a table at -1
    if (blend) {
      qa = bl.q_coef[(idx - 1) * 2 + 0];
      qb = bl.q_coef[(idx - 1) * 2 + 1];
      qn = bl.q_noise + (int64_t)(idx - 1) * bl.q_stride;
    }
  }
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < total; i += (int64_t)gridDim.x * 256 * 4) {
    const f32x4 eu = *(const f32x4*)(eps_all + i), ec = *(const f32x4*)(eps_all + total + i);
    const f32x4 x = *(const f32x4*)(xt + i);
    const f32x4 e0 = eu + gs * (ec - eu);
    f32x4 ep = e0;
    if (j == 1) {
      ep = (3.f * e0 - *(const f32x4*)(e1 + i)) / 2.f;
    } else if (j == 2) {
      ep = (23.f * e0 - 16.f * *(const f32x4*)(e1 + i) + 5.f * *(const f32x4*)(e2 + i)) / 12.f;
    } else if (j == 3) {
      ep = (55.f * e0 - 59.f * *(const f32x4*)(e1 + i) + 37.f * *(const f32x4*)(e2 + i) -
            9.f * *(const f32x4*)(e3 + i)) / 24.f;
    }
    const f32x4 x0 = c1 * x - c2 * ep;
    f32x4 o = sa * x0 + sb * ep;
    if constexpr (Blend) {
      if (blend) {
        const f32x4 z = *(const f32x4*)(bl.z0 + i), qe = *(const f32x4*)(qn + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float m = bl.mask[(i + k) / bl.channels];
          const float q = q_sample_f(qa, qb, z[k], qe[k]);
          o[k] = m * q + (1.f - m) * o[k];
        }
      }
    }
    *(f32x4*)(e_out + i) = e0;
    *(f32x4*)(xt_out + i) = o;
    if (pred_x0_out) *(f32x4*)(pred_x0_out + i) = x0;
    if (x_unet) { st4(x_unet + i, o); st4(x_unet + total + i, o); }
  }
}

// ---- sampling noise drawn in the kernels ------------------------------------------------
// Philox4x32-10 (Salmon et al., SC'11): counter (c0..c3), key (k0, k1) -> four 32-bit words.  Plain integer code.
__device__ __forceinline__ u32x4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                               uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  u32x4 o = {c0, c1, c2, c3};
  return o;
}

// rng = {seed_lo, seed_hi, first_sample_index, 0} on the device.  The words of elements 4q .. 4q+3 of sample b in
// stream `s`: key (seed_lo, seed_hi), counter (q, first_sample_index + b, s, 0).
__device__ __forceinline__ u32x4 rng_words(const uint32_t* __restrict__ rng, uint32_t q, uint32_t b, uint32_t s) {
  return philox4x32_10(q, rng[2] + b, s, 0u, rng[0], rng[1]);
}

// u = ((x >> 8) + 0.5) * 2^-24 in one rounding: never 0; above 1/2 the half is rounded to even.
__device__ __forceinline__ float rng_uniform(uint32_t x) { return fmaf((float)(x >> 8), 0x1p-24f, 0x1p-25f); }

// Box-Muller on the word pairs (x0, x1) and (x2, x3): the normals of elements 4q .. 4q+3.
__device__ __forceinline__ f32x4 rng_normal4(const uint32_t* __restrict__ rng, uint32_t q, uint32_t b, uint32_t s) {
  const u32x4 w = rng_words(rng, q, b, s);
  const float r0 = sqrtf(-2.0f * logf(rng_uniform(w[0]))), r1 = sqrtf(-2.0f * logf(rng_uniform(w[2])));
  float s0, c0, s1, c1;
  sincospif(2.0f * rng_uniform(w[1]), &s0, &c0);
  sincospif(2.0f * rng_uniform(w[3]), &s1, &c1);
  f32x4 z = {r0 * c0, r0 * s0, r1 * c1, r1 * s1};
  return z;
}

__global__ __launch_bounds__(256) void philox_u32_kernel(uint32_t* __restrict__ out, const uint32_t* __restrict__ rng,
                                                         uint32_t stream_word, int B, int64_t n) {
  const int64_t total = (int64_t)B * n;
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < total; i += (int64_t)gridDim.x * 256 * 4) {
    const int64_t b = i / n;
    *(u32x4*)(out + i) = rng_words(rng, (uint32_t)((i - b * n) >> 2), (uint32_t)b, stream_word);
  }
}

template <typename TX>
__global__ __launch_bounds__(256) void normal_fill_kernel(float* __restrict__ out, const uint32_t* __restrict__ rng,
                                                          uint32_t stream_word, int B, int64_t n,
                                                          TX* __restrict__ x_unet) {
  const int64_t total = (int64_t)B * n;
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < total; i += (int64_t)gridDim.x * 256 * 4) {
    const int64_t b = i / n;
    const f32x4 z = rng_normal4(rng, (uint32_t)((i - b * n) >> 2), (uint32_t)b, stream_word);
    *(f32x4*)(out + i) = z;
    if (x_unet) { st4(x_unet + i, z); st4(x_unet + total + i, z); }
  }
}

// ldm_q_sample with the noise of stream `stream_word` drawn here.
template <typename TX>
__global__ __launch_bounds__(256) void q_sample_rng_kernel(const float* __restrict__ x0,
                                                           const uint32_t* __restrict__ rng, uint32_t stream_word,
                                                           const int32_t* __restrict__ t,
                                                           const float* __restrict__ sqrt_ac,
                                                           const float* __restrict__ sqrt_1m_ac, int num_steps,
                                                           float* __restrict__ xt_out, TX* __restrict__ x_unet, int B,
                                                           int64_t n) {
  const int64_t total = (int64_t)B * n;
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < total; i += (int64_t)gridDim.x * 256 * 4) {
    const int64_t b = i / n;
    int ti = t[b];
    ti = ti < 0 ? 0 : (ti >= num_steps ? num_steps - 1 : ti);      // (a stray t reads a valid row)
    const float sa = sqrt_ac[ti], sb = sqrt_1m_ac[ti];
    const f32x4 x = *(const f32x4*)(x0 + i);
    const f32x4 z = rng_normal4(rng, (uint32_t)((i - b * n) >> 2), (uint32_t)b, stream_word);
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = q_sample_f(sa, sb, x[k], z[k]);
    *(f32x4*)(xt_out + i) = o;
    if (x_unet) { st4(x_unet + i, o); st4(x_unet + total + i, o); }
  }
}

// cfg_ddim_kernel (Plms = false) and cfg_plms_kernel (Plms = true) with their tables drawn here: the eta noise of
// stream eta_stream + idx (DDIM, skipped when sigma == 0: uniform over the launch) and the blend's Q[idx-1] of
// stream q_stream + idx - 1 (bl.z0 != NULL and idx >= 1; nothing is drawn at idx = 0).  bl.q_noise is not read.
// Four elements per thread, the arithmetic of the table kernels expression for expression.
template <typename TX, bool Plms>
__global__ __launch_bounds__(256) void cfg_update_rng_kernel(const float* __restrict__ eps_all, const float* xt,
                                                             float* __restrict__ ring, float* xt_out,
                                                             float* __restrict__ pred_x0_out, TX* __restrict__ x_unet,
                                                             const float* coef, const int32_t* index,
                                                             const int32_t* start, const uint32_t* __restrict__ rng,
                                                             uint32_t eta_stream, uint32_t q_stream, float gs,
                                                             int clip, int B, int64_t n, BlendArgs bl) {
  const int idx = *index;
  int j = 0;
  if constexpr (Plms) {
    const int d = *start - idx;
    j = d < 0 ? 0 : (d > 3 ? 3 : d);
  }
  const float c1 = coef[idx * 4 + 0], c2 = coef[idx * 4 + 1], a_prev = coef[idx * 4 + 2];
  const float sigma = Plms ? 0.f : coef[idx * 4 + 3];
  const float sa = sqrtf(a_prev);
  const float sb = Plms ? sqrtf(1.0f - a_prev) : sqrtf(1.0f - a_prev - sigma * sigma);
  const int64_t total = (int64_t)B * n;
  float* e_out = nullptr;
  const float *e1 = nullptr, *e2 = nullptr, *e3 = nullptr;
  if constexpr (Plms) {
    e_out = ring + (int64_t)(idx & 3) * total;
    e1 = ring + (int64_t)((idx + 1) & 3) * total;
    e2 = ring + (int64_t)((idx + 2) & 3) * total;
    e3 = ring + (int64_t)((idx + 3) & 3) * total;
  }
  const bool blend = bl.z0 != nullptr && idx >= 1;   // never draws a row at -1
  float qa = 0.f, qb = 0.f;
  if (blend) {
    qa = bl.q_coef[(idx - 1) * 2 + 0];
    qb = bl.q_coef[(idx - 1) * 2 + 1];
  }
  const bool draw_eta = !Plms && sigma != 0.f;
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < total; i += (int64_t)gridDim.x * 256 * 4) {
    const f32x4 eu = *(const f32x4*)(eps_all + i), ec = *(const f32x4*)(eps_all + total + i);
    const f32x4 x = *(const f32x4*)(xt + i);
    const f32x4 e0 = eu + gs * (ec - eu);
    f32x4 ep = e0;
    if constexpr (Plms) {
      if (j == 1) {
        ep = (3.f * e0 - *(const f32x4*)(e1 + i)) / 2.f;
      } else if (j == 2) {
        ep = (23.f * e0 - 16.f * *(const f32x4*)(e1 + i) + 5.f * *(const f32x4*)(e2 + i)) / 12.f;
      } else if (j == 3) {
        ep = (55.f * e0 - 59.f * *(const f32x4*)(e1 + i) + 37.f * *(const f32x4*)(e2 + i) -
              9.f * *(const f32x4*)(e3 + i)) / 24.f;
      }
    }
    f32x4 x0 = c1 * x - c2 * ep;
    if constexpr (!Plms) {
      if (clip) {
#pragma unroll
        for (int k = 0; k < 4; ++k) x0[k] = fminf(fmaxf(x0[k], -1.f), 1.f);
      }
    }
    f32x4 o = sa * x0 + sb * ep;
    const int64_t b = i / n;
    const uint32_t q = (uint32_t)((i - b * n) >> 2);
    if (draw_eta) {
      const f32x4 nz = rng_normal4(rng, q, (uint32_t)b, eta_stream + (uint32_t)idx);
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = o[k] + nz[k] * sigma;
    }
    if (blend) {
      const f32x4 z = *(const f32x4*)(bl.z0 + i);
      const f32x4 qe = rng_normal4(rng, q, (uint32_t)b, q_stream + (uint32_t)(idx - 1));
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float m = bl.mask[(i + k) / bl.channels];
        const float qs = q_sample_f(qa, qb, z[k], qe[k]);
        o[k] = m * qs + (1.f - m) * o[k];
      }
    }
    if constexpr (Plms) *(f32x4*)(e_out + i) = e0;
    *(f32x4*)(xt_out + i) = o;
    if (pred_x0_out) *(f32x4*)(pred_x0_out + i) = x0;
    if (x_unet) { st4(x_unet + i, o); st4(x_unet + total + i, o); }
  }
}

// ---- CFG + table-weighted multistep update ---------------------------------------------
// cfg_plms_kernel with the Adams-Bashforth constants replaced by a row of a device table: with idx = *index and
// j = clamp(*start - idx, 0, 3), e' = sum_{m <= j} w[m] * e_{idx+m}, w = weights + idx * w_pitch + 4 * j.  idx and j
// are uniform over the launch, so the row is read through a uniform address (scalar loads) and only its j + 1 entries
// are read; only ring slots (idx+1 .. idx+j) & 3 are loaded (the others may hold NaN).  e' is accumulated with
// explicit fused multiply-adds in the order m = 0 .. j.  Rng: the blend's Q[idx-1] is drawn from stream
// q_stream + idx - 1 instead of read from bl.q_noise.  The blend runs when bl.z0 != NULL and idx >= 1.
template <typename TX, bool Rng>
__global__ __launch_bounds__(256) void cfg_ms_kernel(const float* __restrict__ eps_all, const float* xt,
                                                     float* __restrict__ ring, float* xt_out,
                                                     float* __restrict__ pred_x0_out, TX* __restrict__ x_unet,
                                                     const float* coef, const int32_t* index, const int32_t* start,
                                                     const float* __restrict__ weights, int64_t w_pitch,
                                                     const uint32_t* __restrict__ rng, uint32_t q_stream, float gs,
                                                     int B, int64_t n, BlendArgs bl) {
  const int idx = *index;
  const int d = *start - idx;
  const int j = d < 0 ? 0 : (d > 3 ? 3 : d);
  const float c1 = coef[idx * 4 + 0], c2 = coef[idx * 4 + 1], a_prev = coef[idx * 4 + 2];
  const float sa = sqrtf(a_prev);
  const float sb = sqrtf(1.0f - a_prev);
  const float* wr = weights + (int64_t)idx * w_pitch + 4 * j;
  const float w0 = wr[0];
  const float w1 = j >= 1 ? wr[1] : 0.f;
  const float w2 = j >= 2 ? wr[2] : 0.f;
  const float w3 = j >= 3 ? wr[3] : 0.f;
  const int64_t total = (int64_t)B * n;
  float* e_out = ring + (int64_t)(idx & 3) * total;
  const float* e1 = ring + (int64_t)((idx + 1) & 3) * total;
  const float* e2 = ring + (int64_t)((idx + 2) & 3) * total;
  const float* e3 = ring + (int64_t)((idx + 3) & 3) * total;
  const bool blend = bl.z0 != nullptr && idx >= 1;   // never reads or draws a row at -1
  float qa = 0.f, qb = 0.f;
  const float* qn = nullptr;
  if (blend) {
    qa = bl.q_coef[(idx - 1) * 2 + 0];
    qb = bl.q_coef[(idx - 1) * 2 + 1];
    if constexpr (!Rng) qn = bl.q_noise + (int64_t)(idx - 1) * bl.q_stride;
  }
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < total; i += (int64_t)gridDim.x * 256 * 4) {
    const f32x4 eu = *(const f32x4*)(eps_all + i), ec = *(const f32x4*)(eps_all + total + i);
    const f32x4 x = *(const f32x4*)(xt + i);
    const f32x4 e0 = eu + gs * (ec - eu);
    f32x4 ep;
#pragma unroll
    for (int k = 0; k < 4; ++k) ep[k] = w0 * e0[k];
    if (j >= 1) {
      const f32x4 h = *(const f32x4*)(e1 + i);
#pragma unroll
      for (int k = 0; k < 4; ++k) ep[k] = __builtin_fmaf(w1, h[k], ep[k]);
    }
    if (j >= 2) {
      const f32x4 h = *(const f32x4*)(e2 + i);
#pragma unroll
      for (int k = 0; k < 4; ++k) ep[k] = __builtin_fmaf(w2, h[k], ep[k]);
    }
    if (j >= 3) {
      const f32x4 h = *(const f32x4*)(e3 + i);
#pragma unroll
      for (int k = 0; k < 4; ++k) ep[k] = __builtin_fmaf(w3, h[k], ep[k]);
    }
    const f32x4 x0 = c1 * x - c2 * ep;
    f32x4 o = sa * x0 + sb * ep;
    if (blend) {
      const f32x4 z = *(const f32x4*)(bl.z0 + i);
      f32x4 qe;
      if constexpr (Rng) {
        const int64_t b = i / n;
        qe = rng_normal4(rng, (uint32_t)((i - b * n) >> 2), (uint32_t)b, q_stream + (uint32_t)(idx - 1));
      } else {
        qe = *(const f32x4*)(qn + i);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float m = bl.mask[(i + k) / bl.channels];
        const float q = q_sample_f(qa, qb, z[k], qe[k]);
        o[k] = m * q + (1.f - m) * o[k];
      }
    }
    *(f32x4*)(e_out + i) = e0;
    *(f32x4*)(xt_out + i) = o;
    if (pred_x0_out) *(f32x4*)(pred_x0_out + i) = x0;
    if (x_unet) { st4(x_unet + i, o); st4(x_unet + total + i, o); }
  }
}

// ---- guidance schedule: CFG by a device table / conditional-only steps -----------------
// cfg_ms_kernel with the scale read from a device table, gs = gtab[idx] (a launch-uniform address, like coef: one
// captured launch serves every schedule), and a second form of the same body.  Guided: e0 = eu + gs * (ec - eu), the
// expression of the kernels above.  !Guided: e0 = ec, the conditional half of eps_all [2B][n]; the unconditional
// half is never loaded (the conditional-only U-Net evaluation does not write it: it may hold NaN).  weights == NULL:
// no history (j = 0, e' = e0: the DDIM step at sigma = 0), ring and start are not touched.  Both halves of x_unet
// are always written, so the next step may take either form.  Rng and the blend as in cfg_ms_kernel.
template <typename TX, bool Guided, bool Rng>
__global__ __launch_bounds__(256) void cfg_sched_kernel(const float* __restrict__ eps_all, const float* xt,
                                                        float* __restrict__ ring, float* xt_out,
                                                        float* __restrict__ pred_x0_out, TX* __restrict__ x_unet,
                                                        const float* coef, const float* __restrict__ gtab,
                                                        const int32_t* index, const int32_t* start,
                                                        const float* __restrict__ weights, int64_t w_pitch,
                                                        const uint32_t* __restrict__ rng, uint32_t q_stream, int B,
                                                        int64_t n, BlendArgs bl) {
  const int idx = *index;
  int j = 0;
  float w0 = 1.f, w1 = 0.f, w2 = 0.f, w3 = 0.f;
  if (weights) {
    const int d = *start - idx;
    j = d < 0 ? 0 : (d > 3 ? 3 : d);
    const float* wr = weights + (int64_t)idx * w_pitch + 4 * j;
    w0 = wr[0];
    w1 = j >= 1 ? wr[1] : 0.f;
    w2 = j >= 2 ? wr[2] : 0.f;
    w3 = j >= 3 ? wr[3] : 0.f;
  }
  float gs = 1.f;
  if constexpr (Guided) gs = gtab[idx];
  const float c1 = coef[idx * 4 + 0], c2 = coef[idx * 4 + 1], a_prev = coef[idx * 4 + 2];
  const float sa = sqrtf(a_prev);
  const float sb = sqrtf(1.0f - a_prev);
  const int64_t total = (int64_t)B * n;
  float* e_out = weights ? ring + (int64_t)(idx & 3) * total : nullptr;
  const float *e1 = nullptr, *e2 = nullptr, *e3 = nullptr;
  if (weights) {
    e1 = ring + (int64_t)((idx + 1) & 3) * total;
    e2 = ring + (int64_t)((idx + 2) & 3) * total;
    e3 = ring + (int64_t)((idx + 3) & 3) * total;
  }
  const bool blend = bl.z0 != nullptr && idx >= 1;   // never reads or draws a row at -1
  float qa = 0.f, qb = 0.f;
  const float* qn = nullptr;
  if (blend) {
    qa = bl.q_coef[(idx - 1) * 2 + 0];
    qb = bl.q_coef[(idx - 1) * 2 + 1];
    if constexpr (!Rng) qn = bl.q_noise + (int64_t)(idx - 1) * bl.q_stride;
  }
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < total; i += (int64_t)gridDim.x * 256 * 4) {
    const f32x4 ec = *(const f32x4*)(eps_all + total + i);
    const f32x4 x = *(const f32x4*)(xt + i);
    f32x4 e0 = ec;
    if constexpr (Guided) {
      const f32x4 eu = *(const f32x4*)(eps_all + i);
      e0 = eu + gs * (ec - eu);
    }
    f32x4 ep;
#pragma unroll
    for (int k = 0; k < 4; ++k) ep[k] = w0 * e0[k];
    if (j >= 1) {
      const f32x4 h = *(const f32x4*)(e1 + i);
#pragma unroll
      for (int k = 0; k < 4; ++k) ep[k] = __builtin_fmaf(w1, h[k], ep[k]);
    }
    if (j >= 2) {
      const f32x4 h = *(const f32x4*)(e2 + i);
#pragma unroll
      for (int k = 0; k < 4; ++k) ep[k] = __builtin_fmaf(w2, h[k], ep[k]);
    }
    if (j >= 3) {
      const f32x4 h = *(const f32x4*)(e3 + i);
#pragma unroll
      for (int k = 0; k < 4; ++k) ep[k] = __builtin_fmaf(w3, h[k], ep[k]);
    }
    const f32x4 x0 = c1 * x - c2 * ep;
    f32x4 o = sa * x0 + sb * ep;
    if (blend) {
      const f32x4 z = *(const f32x4*)(bl.z0 + i);
      f32x4 qe;
      if constexpr (Rng) {
        const int64_t b = i / n;
        qe = rng_normal4(rng, (uint32_t)((i - b * n) >> 2), (uint32_t)b, q_stream + (uint32_t)(idx - 1));
      } else {
        qe = *(const f32x4*)(qn + i);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float m = bl.mask[(i + k) / bl.channels];
        const float q = q_sample_f(qa, qb, z[k], qe[k]);
        o[k] = m * q + (1.f - m) * o[k];
      }
    }
    if (e_out) *(f32x4*)(e_out + i) = e0;
    *(f32x4*)(xt_out + i) = o;
    if (pred_x0_out) *(f32x4*)(pred_x0_out + i) = x0;
    if (x_unet) { st4(x_unet + i, o); st4(x_unet + total + i, o); }
  }
}

// ---- out[:] = table[i][:], i = *index (pre_decrement: i = --*index first) --------------------------
// ONE workgroup: the thread that moves the loop counter is in the same workgroup as every reader of it, so the
// decrement needs no launch of its own, and every later launch of the step sees the new value.
__global__ __launch_bounds__(1024) void select_row_kernel(const float* __restrict__ table, int64_t ld, int rows,
                                                          int cols, int32_t* __restrict__ index, int pre_decrement,
                                                          float* __restrict__ out) {
  __shared__ int si;
  if (threadIdx.x == 0) {
    int i = *index;
    if (pre_decrement) { i -= 1; *index = i; }
    si = i < 0 ? 0 : (i >= rows ? rows - 1 : i);      // (a stray index reads a valid row; the loop never leaves the table)
  }
  __syncthreads();
  const float* src = table + (int64_t)si * ld;
  for (int c = threadIdx.x * 4; c < cols; c += 1024 * 4) *(f32x4*)(out + c) = *(const f32x4*)(src + c);
}

// ---- post_quant: out = Dense(latents / sf) ----------------------------------------
template <typename TO>
__global__ __launch_bounds__(256) void post_quant_kernel(const float* __restrict__ z, float sf,
                                                         const float* __restrict__ kio,
                                                         const float* __restrict__ bias,
                                                         TO* __restrict__ out, int64_t pixels, int C) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < pixels; p += (int64_t)gridDim.x * 256) {
    float zi[8];
    for (int i = 0; i < C; ++i) zi[i] = z[p * C + i] / sf;
    for (int o = 0; o < C; ++o) {
      float a = 0.f;
      for (int i = 0; i < C; ++i) a += zi[i] * kio[i * C + o];
      stf<TO>(out + p * C + o, a + (bias ? bias[o] : 0.f));
    }
  }
}

// ---- DiagonalGaussian sample / mode ------------------------------------------------------
__global__ __launch_bounds__(256) void gaussian_sample_kernel(const float* __restrict__ mom,
                                                              const float* __restrict__ noise,
                                                              float* __restrict__ out, float scale,
                                                              int64_t total, int C) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t p = i / C;
    const int c = (int)(i - p * C);
    const float mean = mom[p * 2 * C + c];
    float v = mean;
    if (noise) v = mean + expf(0.5f * mom[p * 2 * C + C + c]) * noise[i];
    out[i] = v * scale;
  }
}

// ---- VQ nearest: one wave per row, lanes stride the codebook ------------------------
__global__ __launch_bounds__(256) void vq_nearest_kernel(const float* __restrict__ z,
                                                         const float* __restrict__ cb,
                                                         float* __restrict__ out,
                                                         int64_t* __restrict__ indices, int64_t rows,
                                                         int V, int C) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float zi[8];
  float zz = 0.f;
  for (int i = 0; i < C; ++i) { zi[i] = z[row * C + i]; zz += zi[i] * zi[i]; }
  float best = INFINITY;
  int bidx = 0x7fffffff;
  for (int v = lane; v < V; v += 64) {
    float ee = 0.f, ze = 0.f;
    for (int i = 0; i < C; ++i) { const float e = cb[(int64_t)v * C + i]; ee += e * e; ze += zi[i] * e; }
    const float d = zz + ee - 2.0f * ze;   // quantize.py:66-70
    if (d < best) { best = d; bidx = v; }
  }
  // argmin with lowest-index tie break (tf.argmin returns the first minimum)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bidx, o, 64);
    if (ob < best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
  }
  if (lane < C) {
    const float zv = z[row * C + lane];
    const float q = cb[(int64_t)bidx * C + lane];
    out[row * C + lane] = zv + (q - zv);   // quantize.py:87 straight-through form
  }
  if (lane == 0 && indices) indices[row] = bidx;
}

// ---- token + positional embedding ---------------------------------------------------
template <typename TO>
__global__ __launch_bounds__(256) void embedding_kernel(const int64_t* __restrict__ ids,
                                                        const float* __restrict__ tok,
                                                        const float* __restrict__ pos,
                                                        TO* __restrict__ out, int rows, int T, int D,
                                                        int vocab) {
  const int64_t total = (int64_t)rows * T * D;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int d = (int)(i % D);
    const int64_t rt = i / D;
    const int t = (int)(rt % T);
    int64_t id = ids[rt];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    stf<TO>(out + i, tok[id * D + d] + pos[(int64_t)t * D + d]);
  }
}

// ---- min-max -> uint8 ------------------------------------------------------------------
template <typename TI>
__global__ __launch_bounds__(256) void minmax_kernel(const TI* __restrict__ x, float* scratch,
                                                     int64_t n) {
  // grid (nblk, B); scratch[b][nblk][2]
  __shared__ float smin[4], smax[4];
  const int b = blockIdx.y;
  const TI* xb = x + (int64_t)b * n;
  float mn = INFINITY, mx = -INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float v = ldf<TI>(xb + i);
    mn = fminf(mn, v); mx = fmaxf(mx, v);
  }
  mn = wave_min(mn); mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) { smin[threadIdx.x >> 6] = mn; smax[threadIdx.x >> 6] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float* o = scratch + ((int64_t)b * gridDim.x + blockIdx.x) * 2;
    o[0] = fminf(fminf(smin[0], smin[1]), fminf(smin[2], smin[3]));
    o[1] = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
  }
}
template <typename TI>
__global__ __launch_bounds__(256) void to_u8_kernel(const TI* __restrict__ x, const float* scratch,
                                                    int nblk, uint8_t* __restrict__ out, int64_t n) {
  const int b = blockIdx.y;
  float mn = INFINITY, mx = -INFINITY;
  for (int i = 0; i < nblk; ++i) {
    mn = fminf(mn, scratch[((int64_t)b * nblk + i) * 2]);
    mx = fmaxf(mx, scratch[((int64_t)b * nblk + i) * 2 + 1]);
  }
  const float range = mx - mn;
  const TI* xb = x + (int64_t)b * n;
  uint8_t* ob = out + (int64_t)b * n;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    float v = (ldf<TI>(xb + i) - mn) / range;   // run_ldm_sampler.py:21-22
    v *= 255.0f;                                  // :23
    ob[i] = (uint8_t)v;                           // :24 astype(uint8): truncation
  }
}

template <typename TI, typename TO>
__global__ __launch_bounds__(256) void cast_kernel(const TI* __restrict__ x, int64_t ldx,
                                                   TO* __restrict__ out, int64_t ldo, int64_t rows,
                                                   int cols) {
  const int64_t total = rows * cols;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / cols;
    const int c = (int)(i - r * cols);
    stf<TO>(out + r * ldo + c, ldf<TI>(x + r * ldx + c));
  }
}

inline int grid_for(int64_t total, int per_block = 256, int cap = 4096) {
  int64_t g = (total + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (int)g;
}
constexpr int kMinmaxBlocks = 64;

}  // namespace

#define DT_OK(d) ((d) == LDM_F32 || (d) == LDM_BF16)

extern "C" int ldm_conv3x3_small(const void* x, int64_t ldx, int in_dtype, const float* kernel_hwio,
                                 const float* bias, void* out, int64_t ldo, int out_dtype, int B,
                                 int H, int W, int Cin, int Cout, void* stream) {
  LDM_CHECK_ARG(x && kernel_hwio && out, "ldm_conv3x3_small: null pointer");
  LDM_CHECK_ARG(DT_OK(in_dtype) && DT_OK(out_dtype), "ldm_conv3x3_small: bad dtype");
  LDM_CHECK_ARG(B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "ldm_conv3x3_small: bad dims");
  hipStream_t s = (hipStream_t)stream;
  const int64_t npix = (int64_t)B * H * W;
  if (Cin == 4 && Cout % 8 == 0 && (size_t)9 * Cin * Cout * sizeof(float) <= 64 * 1024 &&
      ldo % 8 == 0 && ((uintptr_t)out % 16) == 0 && ((uintptr_t)kernel_hwio % 16) == 0 &&
      (in_dtype != LDM_F32 || Cin != 4 || (ldx % 4 == 0 && ((uintptr_t)x % 16) == 0))) {
    const size_t shm = (size_t)9 * Cin * Cout * sizeof(float);
    dim3 g(grid_for(((npix + 3) / 4) * (Cout / 8), 256, 768));
#define LAUNCH_INL(TI, TO, CI)                                                                     \
  hipLaunchKernelGGL((conv_in_lds_kernel<TI, TO, CI>), g, dim3(256), shm, s, (const TI*)x, ldx,    \
                     kernel_hwio, bias, (TO*)out, ldo, B, H, W, Cout)
#define LAUNCH_INL_T(TI, TO) LAUNCH_INL(TI, TO, 4)   /* CIN = 3 spills in this form: it takes the kernel below */
    if (in_dtype == LDM_F32 && out_dtype == LDM_F32) { LAUNCH_INL_T(float, float); }
    else if (in_dtype == LDM_F32) { LAUNCH_INL_T(float, bf16_t); }
    else if (out_dtype == LDM_F32) { LAUNCH_INL_T(bf16_t, float); }
    else { LAUNCH_INL_T(bf16_t, bf16_t); }
#undef LAUNCH_INL_T
#undef LAUNCH_INL
    return ldm_launch_status("ldm_conv3x3_small(in, lds)");
  }
  if (Cin <= 8) {
    LDM_CHECK_ARG(Cout % 4 == 0, "ldm_conv3x3_small: Cout must be a multiple of 4 when Cin <= 8");
    dim3 g(grid_for(npix * (Cout / 4), 256, 8192));
#define LAUNCH_IN(TI, TO)                                                                          \
  hipLaunchKernelGGL((conv_small_in_kernel<TI, TO>), g, dim3(256), 0, s, (const TI*)x, ldx,        \
                     kernel_hwio, bias, (TO*)out, ldo, B, H, W, Cin, Cout)
    if (in_dtype == LDM_F32 && out_dtype == LDM_F32) LAUNCH_IN(float, float);
    else if (in_dtype == LDM_F32) LAUNCH_IN(float, bf16_t);
    else if (out_dtype == LDM_F32) LAUNCH_IN(bf16_t, float);
    else LAUNCH_IN(bf16_t, bf16_t);
#undef LAUNCH_IN
    return ldm_launch_status("ldm_conv3x3_small(in)");
  }
  LDM_CHECK_ARG(Cout <= 4, "ldm_conv3x3_small: needs Cin <= 8 or Cout <= 4 (got %d -> %d)", Cin, Cout);
  const int epc = in_dtype == LDM_BF16 ? 8 : 4;
  LDM_CHECK_ARG(Cin % epc == 0 && ldx % epc == 0 && ((uintptr_t)x % 16) == 0,
                "ldm_conv3x3_small: Cin/ldx/x alignment");
  const size_t shm = (size_t)9 * Cin * Cout * sizeof(float);
  LDM_CHECK_ARG(shm <= 64 * 1024, "ldm_conv3x3_small: Cin*Cout too large for LDS");
  dim3 g(grid_for(npix, 32, 4096));
#define LAUNCH_OUT(TI, TO, CO)                                                                     \
  hipLaunchKernelGGL((conv_small_out_kernel<TI, TO, CO>), g, dim3(256), shm, s, (const TI*)x, ldx, \
                     kernel_hwio, bias, (TO*)out, ldo, B, H, W, Cin)
#define LAUNCH_OUT_T(TI, TO)                        \
  switch (Cout) {                                   \
    case 1: LAUNCH_OUT(TI, TO, 1); break;           \
    case 2: LAUNCH_OUT(TI, TO, 2); break;           \
    case 3: LAUNCH_OUT(TI, TO, 3); break;           \
    default: LAUNCH_OUT(TI, TO, 4); break;          \
  }
  if (in_dtype == LDM_F32 && out_dtype == LDM_F32) { LAUNCH_OUT_T(float, float) }
  else if (in_dtype == LDM_F32) { LAUNCH_OUT_T(float, bf16_t) }
  else if (out_dtype == LDM_F32) { LAUNCH_OUT_T(bf16_t, float) }
  else { LAUNCH_OUT_T(bf16_t, bf16_t) }
#undef LAUNCH_OUT_T
#undef LAUNCH_OUT
  return ldm_launch_status("ldm_conv3x3_small(out)");
}

extern "C" int ldm_time_embedding(const int32_t* t_rows, const int32_t* steps, const int32_t* index,
                                  float* out, int rows, int channels, void* stream) {
  LDM_CHECK_ARG(out && rows > 0 && channels > 1, "ldm_time_embedding: bad args");
  LDM_CHECK_ARG((index && steps) || t_rows, "ldm_time_embedding: need t_rows or (steps, index)");
  hipLaunchKernelGGL(time_embedding_kernel, dim3(grid_for((int64_t)rows * (channels / 2))), dim3(256),
                     0, (hipStream_t)stream, t_rows, steps, index, out, rows, channels);
  return ldm_launch_status("ldm_time_embedding");
}

extern "C" int ldm_gemv(const float* x, int64_t ldx, const void* wt, const float* bias, float* y,
                        int64_t ldy, int rows, int N, int K, int act_in, int act_out, int dtype,
                        void* stream) {
  LDM_CHECK_ARG(x && wt && y, "ldm_gemv: null pointer");
  LDM_CHECK_ARG(DT_OK(dtype), "ldm_gemv: bad dtype");
  const int epc = dtype == LDM_BF16 ? 8 : 4;
  LDM_CHECK_ARG(rows > 0 && N > 0 && K > 0 && K % epc == 0 && ((uintptr_t)wt % 16) == 0,
                "ldm_gemv: K=%d must be a multiple of %d", K, epc);
  hipStream_t s = (hipStream_t)stream;
  constexpr int RT = 4;
  dim3 g((N + 3) / 4, (rows + RT - 1) / RT);
  if (dtype == LDM_BF16)
    hipLaunchKernelGGL((gemv_kernel<bf16_t, RT>), g, dim3(256), 0, s, x, ldx, (const bf16_t*)wt, bias,
                       y, ldy, rows, N, K, act_in, act_out);
  else
    hipLaunchKernelGGL((gemv_kernel<float, RT>), g, dim3(256), 0, s, x, ldx, (const float*)wt, bias, y,
                       ldy, rows, N, K, act_in, act_out);
  return ldm_launch_status("ldm_gemv");
}

template <bool Blend>
static int cfg_ddim_launch(const char* what, const float* eps_all, const float* xt, const float* noise,
                           int64_t noise_index_stride, float* xt_out, float* pred_x0_out, void* x_unet_out,
                           int x_dtype, const float* coef, int32_t* index, int dec_index, float guidance_scale,
                           int clip_denoised, int B, int64_t n_per_sample, const BlendArgs& bl, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  dim3 g(grid_for((int64_t)B * n_per_sample, 256, 1024));
  if (x_dtype == LDM_BF16)
    hipLaunchKernelGGL((cfg_ddim_kernel<bf16_t, Blend>), g, dim3(256), 0, s, eps_all, xt, noise, noise_index_stride,
                       xt_out, pred_x0_out, (bf16_t*)x_unet_out, coef, index, dec_index, guidance_scale,
                       clip_denoised, B, n_per_sample, bl);
  else
    hipLaunchKernelGGL((cfg_ddim_kernel<float, Blend>), g, dim3(256), 0, s, eps_all, xt, noise, noise_index_stride,
                       xt_out, pred_x0_out, (float*)x_unet_out, coef, index, dec_index, guidance_scale,
                       clip_denoised, B, n_per_sample, bl);
  int st = ldm_launch_status(what);
  if (st != LDM_OK) return st;
  if (dec_index) {
    hipLaunchKernelGGL(dec_index_kernel, dim3(1), dim3(1), 0, s, index);
    st = ldm_launch_status(what);
  }
  return st;
}

extern "C" int ldm_cfg_ddim_update(const float* eps_all, const float* xt, const float* noise,
                                   int64_t noise_index_stride, float* xt_out, float* pred_x0_out,
                                   void* x_unet_out, int x_dtype, const float* coef,
                                   int32_t* index, int dec_index, float guidance_scale,
                                   int clip_denoised, int B, int64_t n_per_sample, void* stream) {
  LDM_CHECK_ARG(eps_all && xt && xt_out && coef && index, "ldm_cfg_ddim_update: null pointer");
  LDM_CHECK_ARG(DT_OK(x_dtype) && B > 0 && n_per_sample > 0, "ldm_cfg_ddim_update: bad args");
  return cfg_ddim_launch<false>("ldm_cfg_ddim_update", eps_all, xt, noise, noise_index_stride, xt_out, pred_x0_out,
                                x_unet_out, x_dtype, coef, index, dec_index, guidance_scale, clip_denoised, B,
                                n_per_sample, BlendArgs{}, stream);
}

extern "C" int ldm_cfg_ddim_update_masked(const float* eps_all, const float* xt, const float* noise,
                                          int64_t noise_index_stride, float* xt_out, float* pred_x0_out,
                                          void* x_unet_out, int x_dtype, const float* coef, int32_t* index,
                                          int dec_index, float guidance_scale, int clip_denoised, int B,
                                          int64_t n_per_sample, const float* z0, const float* mask,
                                          const float* q_noise, int64_t q_index_stride, const float* q_coef,
                                          int channels, void* stream) {
  LDM_CHECK_ARG(eps_all && xt && xt_out && coef && index && z0 && mask && q_noise && q_coef,
                "ldm_cfg_ddim_update_masked: null pointer");
  LDM_CHECK_ARG(DT_OK(x_dtype) && B > 0 && n_per_sample > 0 && channels > 0 && n_per_sample % channels == 0 &&
                    q_index_stride >= 0,
                "ldm_cfg_ddim_update_masked: bad args (n_per_sample=%lld, channels=%d)", (long long)n_per_sample,
                channels);
  const BlendArgs bl{z0, mask, q_noise, q_index_stride, q_coef, channels};
  return cfg_ddim_launch<true>("ldm_cfg_ddim_update_masked", eps_all, xt, noise, noise_index_stride, xt_out,
                               pred_x0_out, x_unet_out, x_dtype, coef, index, dec_index, guidance_scale,
                               clip_denoised, B, n_per_sample, bl, stream);
}

template <bool Blend>
static int cfg_plms_launch(const float* eps_all, const float* xt, float* ring, float* xt_out, float* pred_x0_out,
                           void* x_unet_out, int x_dtype, const float* coef, int32_t* index, const int32_t* start,
                           int dec_index, float guidance_scale, int B, int64_t n_per_sample, const BlendArgs& bl,
                           void* stream) {
  hipStream_t s = (hipStream_t)stream;
  dim3 g(grid_for((int64_t)B * n_per_sample / 4, 256, 1024));
  if (x_dtype == LDM_BF16)
    hipLaunchKernelGGL((cfg_plms_kernel<bf16_t, Blend>), g, dim3(256), 0, s, eps_all, xt, ring, xt_out, pred_x0_out,
                       (bf16_t*)x_unet_out, coef, index, start, guidance_scale, B, n_per_sample, bl);
  else
    hipLaunchKernelGGL((cfg_plms_kernel<float, Blend>), g, dim3(256), 0, s, eps_all, xt, ring, xt_out, pred_x0_out,
                       (float*)x_unet_out, coef, index, start, guidance_scale, B, n_per_sample, bl);
  int st = ldm_launch_status("ldm_cfg_plms_update");
  if (st != LDM_OK) return st;
  if (dec_index) {
    hipLaunchKernelGGL(dec_index_kernel, dim3(1), dim3(1), 0, s, index);
    st = ldm_launch_status("ldm_cfg_plms_update");
  }
  return st;
}

extern "C" int ldm_cfg_plms_update(const float* eps_all, const float* xt, float* ring, float* xt_out,
                                   float* pred_x0_out, void* x_unet_out, int x_dtype, const float* coef,
                                   int32_t* index, const int32_t* start, int dec_index, float guidance_scale, int B,
                                   int64_t n_per_sample, const float* z0, const float* mask, const float* q_noise,
                                   int64_t q_index_stride, const float* q_coef, int channels, void* stream) {
  LDM_CHECK_ARG(eps_all && xt && ring && xt_out && coef && index && start, "ldm_cfg_plms_update: null pointer");
  LDM_CHECK_ARG(DT_OK(x_dtype) && B > 0 && n_per_sample > 0 && n_per_sample % 4 == 0,
                "ldm_cfg_plms_update: bad args (n_per_sample=%lld must be a positive multiple of 4)",
                (long long)n_per_sample);
  const uintptr_t al = (uintptr_t)eps_all | (uintptr_t)xt | (uintptr_t)ring | (uintptr_t)xt_out |
                       (uintptr_t)pred_x0_out | (uintptr_t)z0 | (uintptr_t)q_noise;
  LDM_CHECK_ARG(al % 16 == 0 && (uintptr_t)x_unet_out % (x_dtype == LDM_BF16 ? 8 : 16) == 0 &&
                    (!z0 || q_index_stride % 4 == 0),
                "ldm_cfg_plms_update: arrays must be 16-byte aligned (q_index_stride a multiple of 4)");
  if (!z0)
    return cfg_plms_launch<false>(eps_all, xt, ring, xt_out, pred_x0_out, x_unet_out, x_dtype, coef, index, start,
                                  dec_index, guidance_scale, B, n_per_sample, BlendArgs{}, stream);
  LDM_CHECK_ARG(mask && q_noise && q_coef, "ldm_cfg_plms_update: z0 without mask / q_noise / q_coef");
  LDM_CHECK_ARG(channels > 0 && n_per_sample % channels == 0 && q_index_stride >= 0,
                "ldm_cfg_plms_update: bad args (n_per_sample=%lld, channels=%d)", (long long)n_per_sample, channels);
  const BlendArgs bl{z0, mask, q_noise, q_index_stride, q_coef, channels};
  return cfg_plms_launch<true>(eps_all, xt, ring, xt_out, pred_x0_out, x_unet_out, x_dtype, coef, index, start,
                               dec_index, guidance_scale, B, n_per_sample, bl, stream);
}

extern "C" int ldm_q_sample(const float* x0, const float* noise, int64_t noise_index_stride, const int32_t* index,
                            const int32_t* t, const float* sqrt_alphas_cumprod,
                            const float* sqrt_one_minus_alphas_cumprod, int num_steps, float* xt_out,
                            void* x_unet_out, int x_dtype, int B, int64_t n_per_sample, void* stream) {
  LDM_CHECK_ARG(x0 && noise && t && sqrt_alphas_cumprod && sqrt_one_minus_alphas_cumprod && xt_out,
                "ldm_q_sample: null pointer");
  LDM_CHECK_ARG(DT_OK(x_dtype) && B > 0 && n_per_sample > 0 && num_steps > 0 && noise_index_stride >= 0,
                "ldm_q_sample: bad args");
  hipStream_t s = (hipStream_t)stream;
  dim3 g(grid_for((int64_t)B * n_per_sample, 256, 1024));
  if (x_dtype == LDM_BF16)
    hipLaunchKernelGGL(q_sample_kernel<bf16_t>, g, dim3(256), 0, s, x0, noise, noise_index_stride, index, t,
                       sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod, num_steps, xt_out, (bf16_t*)x_unet_out,
                       B, n_per_sample);
  else
    hipLaunchKernelGGL(q_sample_kernel<float>, g, dim3(256), 0, s, x0, noise, noise_index_stride, index, t,
                       sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod, num_steps, xt_out, (float*)x_unet_out,
                       B, n_per_sample);
  return ldm_launch_status("ldm_q_sample");
}

#define AL16(p) (((uintptr_t)(p) % 16) == 0)
#define XU_OK(p, d) (((uintptr_t)(p) % ((d) == LDM_BF16 ? 8 : 16)) == 0)

extern "C" int ldm_philox_u32(uint32_t* out, const uint32_t* rng, uint32_t stream_word, int B, int64_t n_per_sample,
                              void* stream) {
  LDM_CHECK_ARG(out && rng, "ldm_philox_u32: null pointer");
  LDM_CHECK_ARG(B > 0 && n_per_sample > 0 && n_per_sample % 4 == 0 && AL16(out),
                "ldm_philox_u32: n_per_sample=%lld must be a positive multiple of 4, out 16-byte aligned",
                (long long)n_per_sample);
  dim3 g(grid_for((int64_t)B * n_per_sample / 4, 256, 1024));
  hipLaunchKernelGGL(philox_u32_kernel, g, dim3(256), 0, (hipStream_t)stream, out, rng, stream_word, B, n_per_sample);
  return ldm_launch_status("ldm_philox_u32");
}

extern "C" int ldm_normal_fill(float* out, const uint32_t* rng, uint32_t stream_word, int B, int64_t n_per_sample,
                               void* x_unet_out, int x_dtype, void* stream) {
  LDM_CHECK_ARG(out && rng, "ldm_normal_fill: null pointer");
  LDM_CHECK_ARG(DT_OK(x_dtype) && B > 0 && n_per_sample > 0 && n_per_sample % 4 == 0 && AL16(out) &&
                    XU_OK(x_unet_out, x_dtype),
                "ldm_normal_fill: n_per_sample=%lld must be a positive multiple of 4, arrays 16-byte aligned",
                (long long)n_per_sample);
  hipStream_t s = (hipStream_t)stream;
  dim3 g(grid_for((int64_t)B * n_per_sample / 4, 256, 1024));
  if (x_dtype == LDM_BF16)
    hipLaunchKernelGGL(normal_fill_kernel<bf16_t>, g, dim3(256), 0, s, out, rng, stream_word, B, n_per_sample,
                       (bf16_t*)x_unet_out);
  else
    hipLaunchKernelGGL(normal_fill_kernel<float>, g, dim3(256), 0, s, out, rng, stream_word, B, n_per_sample,
                       (float*)x_unet_out);
  return ldm_launch_status("ldm_normal_fill");
}

extern "C" int ldm_q_sample_rng(const float* x0, const uint32_t* rng, uint32_t stream_word, const int32_t* t,
                                const float* sqrt_alphas_cumprod, const float* sqrt_one_minus_alphas_cumprod,
                                int num_steps, float* xt_out, void* x_unet_out, int x_dtype, int B,
                                int64_t n_per_sample, void* stream) {
  LDM_CHECK_ARG(x0 && rng && t && sqrt_alphas_cumprod && sqrt_one_minus_alphas_cumprod && xt_out,
                "ldm_q_sample_rng: null pointer");
  LDM_CHECK_ARG(DT_OK(x_dtype) && B > 0 && n_per_sample > 0 && num_steps > 0 && n_per_sample % 4 == 0 && AL16(x0) &&
                    AL16(xt_out) && XU_OK(x_unet_out, x_dtype),
                "ldm_q_sample_rng: n_per_sample=%lld must be a positive multiple of 4, arrays 16-byte aligned",
                (long long)n_per_sample);
  hipStream_t s = (hipStream_t)stream;
  dim3 g(grid_for((int64_t)B * n_per_sample / 4, 256, 1024));
  if (x_dtype == LDM_BF16)
    hipLaunchKernelGGL(q_sample_rng_kernel<bf16_t>, g, dim3(256), 0, s, x0, rng, stream_word, t, sqrt_alphas_cumprod,
                       sqrt_one_minus_alphas_cumprod, num_steps, xt_out, (bf16_t*)x_unet_out, B, n_per_sample);
  else
    hipLaunchKernelGGL(q_sample_rng_kernel<float>, g, dim3(256), 0, s, x0, rng, stream_word, t, sqrt_alphas_cumprod,
                       sqrt_one_minus_alphas_cumprod, num_steps, xt_out, (float*)x_unet_out, B, n_per_sample);
  return ldm_launch_status("ldm_q_sample_rng");
}

// checks and launch shared by ldm_cfg_ddim_update_rng (ring = start = NULL) and ldm_cfg_plms_update_rng
static int cfg_update_rng_launch(const char* what, bool plms, const float* eps_all, const float* xt, float* ring,
                                 float* xt_out, float* pred_x0_out, void* x_unet_out, int x_dtype, const float* coef,
                                 int32_t* index, const int32_t* start, const uint32_t* rng, int dec_index,
                                 float guidance_scale, int clip_denoised, int B, int64_t n_per_sample, const float* z0,
                                 const float* mask, const float* q_coef, int channels, void* stream) {
  LDM_CHECK_ARG(eps_all && xt && xt_out && coef && index && rng && (!plms || (ring && start)), "%s: null pointer",
                what);
  LDM_CHECK_ARG(DT_OK(x_dtype) && B > 0 && n_per_sample > 0 && n_per_sample % 4 == 0,
                "%s: bad args (n_per_sample=%lld must be a positive multiple of 4)", what, (long long)n_per_sample);
  LDM_CHECK_ARG(AL16(eps_all) && AL16(xt) && AL16(ring) && AL16(xt_out) && AL16(pred_x0_out) && AL16(z0) &&
                    XU_OK(x_unet_out, x_dtype),
                "%s: arrays must be 16-byte aligned", what);
  BlendArgs bl{};
  if (z0) {
    LDM_CHECK_ARG(mask && q_coef, "%s: z0 without mask / q_coef", what);
    LDM_CHECK_ARG(channels > 0 && n_per_sample % channels == 0, "%s: bad args (n_per_sample=%lld, channels=%d)", what,
                  (long long)n_per_sample, channels);
    bl = BlendArgs{z0, mask, nullptr, 0, q_coef, channels};
  }
  hipStream_t s = (hipStream_t)stream;
  dim3 g(grid_for((int64_t)B * n_per_sample / 4, 256, 1024));
#define LAUNCH_RNG(TX, PLMS)                                                                                        \
  hipLaunchKernelGGL((cfg_update_rng_kernel<TX, PLMS>), g, dim3(256), 0, s, eps_all, xt, ring, xt_out, pred_x0_out, \
                     (TX*)x_unet_out, coef, index, start, rng, (uint32_t)LDM_RNG_ETA_STREAM,                       \
                     (uint32_t)LDM_RNG_Q_STREAM, guidance_scale, clip_denoised, B, n_per_sample, bl)
  if (plms) {
    if (x_dtype == LDM_BF16) LAUNCH_RNG(bf16_t, true); else LAUNCH_RNG(float, true);
  } else {
    if (x_dtype == LDM_BF16) LAUNCH_RNG(bf16_t, false); else LAUNCH_RNG(float, false);
  }
#undef LAUNCH_RNG
  int st = ldm_launch_status(what);
  if (st != LDM_OK) return st;
  if (dec_index) {
    hipLaunchKernelGGL(dec_index_kernel, dim3(1), dim3(1), 0, s, index);
    st = ldm_launch_status(what);
  }
  return st;
}

extern "C" int ldm_cfg_ddim_update_rng(const float* eps_all, const float* xt, const uint32_t* rng, float* xt_out,
                                       float* pred_x0_out, void* x_unet_out, int x_dtype, const float* coef,
                                       int32_t* index, int dec_index, float guidance_scale, int clip_denoised, int B,
                                       int64_t n_per_sample, const float* z0, const float* mask, const float* q_coef,
                                       int channels, void* stream) {
  return cfg_update_rng_launch("ldm_cfg_ddim_update_rng", false, eps_all, xt, nullptr, xt_out, pred_x0_out, x_unet_out,
                               x_dtype, coef, index, nullptr, rng, dec_index, guidance_scale, clip_denoised, B,
                               n_per_sample, z0, mask, q_coef, channels, stream);
}

extern "C" int ldm_cfg_plms_update_rng(const float* eps_all, const float* xt, float* ring, float* xt_out,
                                       float* pred_x0_out, void* x_unet_out, int x_dtype, const float* coef,
                                       int32_t* index, const int32_t* start, const uint32_t* rng, int dec_index,
                                       float guidance_scale, int B, int64_t n_per_sample, const float* z0,
                                       const float* mask, const float* q_coef, int channels, void* stream) {
  return cfg_update_rng_launch("ldm_cfg_plms_update_rng", true, eps_all, xt, ring, xt_out, pred_x0_out, x_unet_out,
                               x_dtype, coef, index, start, rng, dec_index, guidance_scale, 0, B, n_per_sample, z0,
                               mask, q_coef, channels, stream);
}
// checks and launch shared by ldm_cfg_ms_update (rng = NULL: Q from the table) and ldm_cfg_ms_update_rng
static int cfg_ms_launch(const char* what, bool draws, const float* eps_all, const float* xt, float* ring,
                         float* xt_out, float* pred_x0_out, void* x_unet_out, int x_dtype, const float* coef,
                         int32_t* index, const int32_t* start, const float* weights, int64_t weights_pitch,
                         const uint32_t* rng, int dec_index, float guidance_scale, int B, int64_t n_per_sample,
                         const float* z0, const float* mask, const float* q_noise, int64_t q_index_stride,
                         const float* q_coef, int channels, void* stream) {
  LDM_CHECK_ARG(eps_all && xt && ring && xt_out && coef && index && start && weights && (!draws || rng),
                "%s: null pointer", what);
  LDM_CHECK_ARG(DT_OK(x_dtype) && B > 0 && n_per_sample > 0 && n_per_sample % 4 == 0,
                "%s: bad args (n_per_sample=%lld must be a positive multiple of 4)", what, (long long)n_per_sample);
  LDM_CHECK_ARG(weights_pitch >= 16, "%s: weights_pitch=%lld, a row holds 4 x 4 floats", what,
                (long long)weights_pitch);
  LDM_CHECK_ARG(AL16(eps_all) && AL16(xt) && AL16(ring) && AL16(xt_out) && AL16(pred_x0_out) && AL16(z0) &&
                    XU_OK(x_unet_out, x_dtype) && (draws || !z0 || (AL16(q_noise) && q_index_stride % 4 == 0)),
                "%s: arrays must be 16-byte aligned (q_index_stride a multiple of 4)", what);
  BlendArgs bl{};
  if (z0) {
    LDM_CHECK_ARG(mask && q_coef && (draws || q_noise), "%s: z0 without mask / q_noise / q_coef", what);
    LDM_CHECK_ARG(channels > 0 && n_per_sample % channels == 0 && q_index_stride >= 0,
                  "%s: bad args (n_per_sample=%lld, channels=%d)", what, (long long)n_per_sample, channels);
    bl = BlendArgs{z0, mask, draws ? nullptr : q_noise, draws ? 0 : q_index_stride, q_coef, channels};
  }
  hipStream_t s = (hipStream_t)stream;
  dim3 g(grid_for((int64_t)B * n_per_sample / 4, 256, 1024));
#define LAUNCH_MS(TX, RNG)                                                                                       \
  hipLaunchKernelGGL((cfg_ms_kernel<TX, RNG>), g, dim3(256), 0, s, eps_all, xt, ring, xt_out, pred_x0_out,       \
                     (TX*)x_unet_out, coef, index, start, weights, weights_pitch, rng, (uint32_t)LDM_RNG_Q_STREAM, \
                     guidance_scale, B, n_per_sample, bl)
  if (draws) {
    if (x_dtype == LDM_BF16) LAUNCH_MS(bf16_t, true); else LAUNCH_MS(float, true);
  } else {
    if (x_dtype == LDM_BF16) LAUNCH_MS(bf16_t, false); else LAUNCH_MS(float, false);
  }
#undef LAUNCH_MS
  int st = ldm_launch_status(what);
  if (st != LDM_OK) return st;
  if (dec_index) {
    hipLaunchKernelGGL(dec_index_kernel, dim3(1), dim3(1), 0, s, index);
    st = ldm_launch_status(what);
  }
  return st;
}

extern "C" int ldm_cfg_ms_update(const float* eps_all, const float* xt, float* ring, float* xt_out,
                                 float* pred_x0_out, void* x_unet_out, int x_dtype, const float* coef,
                                 int32_t* index, const int32_t* start, const float* weights, int64_t weights_pitch,
                                 int dec_index, float guidance_scale, int B, int64_t n_per_sample, const float* z0,
                                 const float* mask, const float* q_noise, int64_t q_index_stride, const float* q_coef,
                                 int channels, void* stream) {
  return cfg_ms_launch("ldm_cfg_ms_update", false, eps_all, xt, ring, xt_out, pred_x0_out, x_unet_out, x_dtype, coef,
                       index, start, weights, weights_pitch, nullptr, dec_index, guidance_scale, B, n_per_sample, z0,
                       mask, q_noise, q_index_stride, q_coef, channels, stream);
}

extern "C" int ldm_cfg_ms_update_rng(const float* eps_all, const float* xt, float* ring, float* xt_out,
                                     float* pred_x0_out, void* x_unet_out, int x_dtype, const float* coef,
                                     int32_t* index, const int32_t* start, const float* weights,
                                     int64_t weights_pitch, const uint32_t* rng, int dec_index, float guidance_scale,
                                     int B, int64_t n_per_sample, const float* z0, const float* mask,
                                     const float* q_coef, int channels, void* stream) {
  return cfg_ms_launch("ldm_cfg_ms_update_rng", true, eps_all, xt, ring, xt_out, pred_x0_out, x_unet_out, x_dtype,
                       coef, index, start, weights, weights_pitch, rng, dec_index, guidance_scale, B, n_per_sample, z0,
                       mask, nullptr, 0, q_coef, channels, stream);
}
extern "C" int ldm_cfg_sched_update(const float* eps_all, const float* xt, float* ring, float* xt_out,
                                    float* pred_x0_out, void* x_unet_out, int x_dtype, const float* coef,
                                    const float* gtab, int32_t* index, const int32_t* start, const float* weights,
                                    int64_t weights_pitch, const uint32_t* rng, int guided, int dec_index, int B,
                                    int64_t n_per_sample, const float* z0, const float* mask, const float* q_noise,
                                    int64_t q_index_stride, const float* q_coef, int channels, void* stream) {
  const char* what = "ldm_cfg_sched_update";
  const bool draws = rng != nullptr;
  LDM_CHECK_ARG(eps_all && xt && xt_out && coef && gtab && index, "%s: null pointer", what);
  LDM_CHECK_ARG(!weights || (ring && start), "%s: weights without ring / start", what);
  LDM_CHECK_ARG(DT_OK(x_dtype) && B > 0 && n_per_sample > 0 && n_per_sample % 4 == 0,
                "%s: bad args (n_per_sample=%lld must be a positive multiple of 4)", what, (long long)n_per_sample);
  LDM_CHECK_ARG(!weights || weights_pitch >= 16, "%s: weights_pitch=%lld, a row holds 4 x 4 floats", what,
                (long long)weights_pitch);
  LDM_CHECK_ARG(AL16(eps_all) && AL16(xt) && AL16(ring) && AL16(xt_out) && AL16(pred_x0_out) && AL16(z0) &&
                    XU_OK(x_unet_out, x_dtype) && (draws || !z0 || (AL16(q_noise) && q_index_stride % 4 == 0)),
                "%s: arrays must be 16-byte aligned (q_index_stride a multiple of 4)", what);
  BlendArgs bl{};
  if (z0) {
    LDM_CHECK_ARG(mask && q_coef && (draws || q_noise), "%s: z0 without mask / q_noise / q_coef", what);
    LDM_CHECK_ARG(channels > 0 && n_per_sample % channels == 0 && q_index_stride >= 0,
                  "%s: bad args (n_per_sample=%lld, channels=%d)", what, (long long)n_per_sample, channels);
    bl = BlendArgs{z0, mask, draws ? nullptr : q_noise, draws ? 0 : q_index_stride, q_coef, channels};
  }
  if (!weights) ring = nullptr;                      // (no history: the ring is neither read nor written)
  hipStream_t s = (hipStream_t)stream;
  dim3 g(grid_for((int64_t)B * n_per_sample / 4, 256, 1024));
#define LAUNCH_SCHED(TX, GUIDED, RNG)                                                                              \
  hipLaunchKernelGGL((cfg_sched_kernel<TX, GUIDED, RNG>), g, dim3(256), 0, s, eps_all, xt, ring, xt_out,           \
                     pred_x0_out, (TX*)x_unet_out, coef, gtab, index, start, weights, weights_pitch, rng,           \
                     (uint32_t)LDM_RNG_Q_STREAM, B, n_per_sample, bl)
#define LAUNCH_SCHED_TX(GUIDED, RNG) \
  do { if (x_dtype == LDM_BF16) LAUNCH_SCHED(bf16_t, GUIDED, RNG); else LAUNCH_SCHED(float, GUIDED, RNG); } while (0)
  if (guided) {
    if (draws) LAUNCH_SCHED_TX(true, true); else LAUNCH_SCHED_TX(true, false);
  } else {
    if (draws) LAUNCH_SCHED_TX(false, true); else LAUNCH_SCHED_TX(false, false);
  }
#undef LAUNCH_SCHED_TX
#undef LAUNCH_SCHED
  int st = ldm_launch_status(what);
  if (st != LDM_OK) return st;
  if (dec_index) {
    hipLaunchKernelGGL(dec_index_kernel, dim3(1), dim3(1), 0, s, index);
    st = ldm_launch_status(what);
  }
  return st;
}
#undef AL16
#undef XU_OK

extern "C" int ldm_select_row(const float* table, int64_t ld, int rows, int cols, int32_t* index, int pre_decrement,
                              float* out, void* stream) {
  LDM_CHECK_ARG(table && index && out && rows > 0 && cols > 0, "ldm_select_row: bad args");
  LDM_CHECK_ARG(cols % 4 == 0 && ld % 4 == 0 && ((uintptr_t)table % 16) == 0 && ((uintptr_t)out % 16) == 0,
                "ldm_select_row: cols / ld must be multiples of 4 floats, table / out 16-byte aligned");
  hipLaunchKernelGGL(select_row_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, table, ld, rows, cols, index,
                     pre_decrement, out);
  return ldm_launch_status("ldm_select_row");
}

extern "C" int ldm_post_quant(const float* latents, float scale_factor, const float* kernel_io,
                              const float* bias, void* out, int out_dtype, int64_t pixels, int C,
                              void* stream) {
  LDM_CHECK_ARG(latents && kernel_io && out && pixels > 0 && C > 0 && C <= 8 && DT_OK(out_dtype),
                "ldm_post_quant: bad args");
  hipStream_t s = (hipStream_t)stream;
  dim3 g(grid_for(pixels));
  if (out_dtype == LDM_BF16)
    hipLaunchKernelGGL(post_quant_kernel<bf16_t>, g, dim3(256), 0, s, latents, scale_factor, kernel_io,
                       bias, (bf16_t*)out, pixels, C);
  else
    hipLaunchKernelGGL(post_quant_kernel<float>, g, dim3(256), 0, s, latents, scale_factor, kernel_io,
                       bias, (float*)out, pixels, C);
  return ldm_launch_status("ldm_post_quant");
}

extern "C" int ldm_gaussian_sample(const float* moments, const float* noise, float* out,
                                   float out_scale, int64_t pixels, int C, void* stream) {
  LDM_CHECK_ARG(moments && out && pixels > 0 && C > 0, "ldm_gaussian_sample: bad args");
  dim3 g(grid_for(pixels * C, 256, 4096));
  hipLaunchKernelGGL(gaussian_sample_kernel, g, dim3(256), 0, (hipStream_t)stream, moments, noise, out,
                     out_scale, pixels * C, C);
  return ldm_launch_status("ldm_gaussian_sample");
}

extern "C" int ldm_vq_nearest(const float* z, const float* codebook, float* out, int64_t* indices,
                              int64_t rows, int V, int C, void* stream) {
  LDM_CHECK_ARG(z && codebook && out && rows > 0 && V > 0 && C > 0 && C <= 8, "ldm_vq_nearest: bad args");
  LDM_CHECK_ARG((rows + 3) / 4 < (1ll << 31), "ldm_vq_nearest: too many rows");
  hipLaunchKernelGGL(vq_nearest_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0,
                     (hipStream_t)stream, z, codebook, out, indices, rows, V, C);
  return ldm_launch_status("ldm_vq_nearest");
}

extern "C" int ldm_embedding(const int64_t* ids, const float* tok_emb, const float* pos_emb, void* out,
                             int rows, int T, int D, int vocab, int out_dtype, void* stream) {
  LDM_CHECK_ARG(ids && tok_emb && pos_emb && out && rows > 0 && T > 0 && D > 0 && vocab > 0 &&
                    DT_OK(out_dtype), "ldm_embedding: bad args");
  hipStream_t s = (hipStream_t)stream;
  dim3 g(grid_for((int64_t)rows * T * D));
  if (out_dtype == LDM_BF16)
    hipLaunchKernelGGL(embedding_kernel<bf16_t>, g, dim3(256), 0, s, ids, tok_emb, pos_emb,
                       (bf16_t*)out, rows, T, D, vocab);
  else
    hipLaunchKernelGGL(embedding_kernel<float>, g, dim3(256), 0, s, ids, tok_emb, pos_emb, (float*)out,
                       rows, T, D, vocab);
  return ldm_launch_status("ldm_embedding");
}

extern "C" int ldm_minmax_u8(const void* x, int in_dtype, uint8_t* out, float* scratch, int B,
                             int64_t n_per_image, void* stream) {
  LDM_CHECK_ARG(x && out && scratch && B > 0 && n_per_image > 0 && DT_OK(in_dtype),
                "ldm_minmax_u8: bad args (scratch needs %d floats per image)", 2 * kMinmaxBlocks);
  hipStream_t s = (hipStream_t)stream;
  dim3 g1(kMinmaxBlocks, B), g2(grid_for(n_per_image, 256, 256), B);
  if (in_dtype == LDM_BF16) {
    hipLaunchKernelGGL(minmax_kernel<bf16_t>, g1, dim3(256), 0, s, (const bf16_t*)x, scratch, n_per_image);
    hipLaunchKernelGGL(to_u8_kernel<bf16_t>, g2, dim3(256), 0, s, (const bf16_t*)x, scratch,
                       kMinmaxBlocks, out, n_per_image);
  } else {
    hipLaunchKernelGGL(minmax_kernel<float>, g1, dim3(256), 0, s, (const float*)x, scratch, n_per_image);
    hipLaunchKernelGGL(to_u8_kernel<float>, g2, dim3(256), 0, s, (const float*)x, scratch,
                       kMinmaxBlocks, out, n_per_image);
  }
  return ldm_launch_status("ldm_minmax_u8");
}

extern "C" int ldm_cast(const void* x, int64_t ldx, int in_dtype, void* out, int64_t ldo,
                        int out_dtype, int64_t rows, int cols, void* stream) {
  LDM_CHECK_ARG(x && out && rows > 0 && cols > 0 && DT_OK(in_dtype) && DT_OK(out_dtype),
                "ldm_cast: bad args");
  hipStream_t s = (hipStream_t)stream;
  dim3 g(grid_for(rows * cols));
  if (in_dtype == LDM_F32 && out_dtype == LDM_F32)
    hipLaunchKernelGGL((cast_kernel<float, float>), g, dim3(256), 0, s, (const float*)x, ldx, (float*)out, ldo, rows, cols);
  else if (in_dtype == LDM_F32)
    hipLaunchKernelGGL((cast_kernel<float, bf16_t>), g, dim3(256), 0, s, (const float*)x, ldx, (bf16_t*)out, ldo, rows, cols);
  else if (out_dtype == LDM_F32)
    hipLaunchKernelGGL((cast_kernel<bf16_t, float>), g, dim3(256), 0, s, (const bf16_t*)x, ldx, (float*)out, ldo, rows, cols);
  else
    hipLaunchKernelGGL((cast_kernel<bf16_t, bf16_t>), g, dim3(256), 0, s, (const bf16_t*)x, ldx, (bf16_t*)out, ldo, rows, cols);
  return ldm_launch_status("ldm_cast");
}
