// Sampler kernels: forward diffusion q(x_t | x_0), the Philox noise source, and the update of a sampling step (CFG,
// then DDIM / PLMS / a table-weighted multistep rule, then the inpainting blend): one scalar DDIM kernel and one
// four-wide body for every other form, behind one host launcher.
#include "common.h"

namespace {

// ---- forward diffusion q(x_t | x_0) -------------------------------------------------
// model_runners.py:580-600: xt = _extract(sqrt_ac, t) * x0 + _extract(sqrt_1m_ac, t) * eps, the coefficients
// float32 (cast, then gathered).  One inline body serves ldm_q_sample and the blend of the masked updates, so
// a kept latent cell is bit for bit the q_sample of its init latent.
__device__ __forceinline__ float q_sample_f(float sa, float sb, float x0, float eps) { return sa * x0 + sb * eps; }

__device__ __forceinline__ void st4(float* p, const f32x4& v) { *(f32x4*)p = v; }
__device__ __forceinline__ void st4(bf16_t* p, const f32x4& v) {
  u32x2 c;
  c[0] = pack_bf2(v[0], v[1]);
  c[1] = pack_bf2(v[2], v[3]);
  *(u32x2*)p = c;
}

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
    if (x_unet) { Elem<TX>::st(x_unet + i, o); Elem<TX>::st(x_unet + total + i, o); }
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

// ---- the update of a sampling step ----------------------------------------------------------------------------
// The inpainting blend pins the kept cells to the init latent before the NEXT step (index idx - 1) reads them:
// o <- m * q_sample(z0, steps[idx-1], Q[idx-1]) + (1 - m) * o, skipped at idx = 0 (its output goes to the decoder as
// it is).  z0 == NULL: no blend.
struct BlendArgs {
  const float* z0;        // [B][n]
  const float* mask;      // [B][n / channels]
  const float* q_noise;   // Q table, row j at q_noise + j * q_stride; NULL when Q is drawn
  int64_t q_stride;
  const float* q_coef;    // [N_steps][2]: (sqrt_ac, sqrt_1m_ac) at steps[j], float32
  int channels;
};

// Every update kernel takes this struct by value; an entry fills what its form reads (update_base, the entries below).
struct UpdateArgs {
  const float* eps_all;   // [2B][n]: unconditional half, conditional half
  const float* xt;
  float* xt_out;          // may be xt
  float* pred_x0_out;     // may be NULL
  void* x_unet;           // [2B][n] in TX, both halves written; may be NULL
  const float* coef;      // [N][4]: c1, c2, a_prev, sigma
  const int32_t* index;
  float gs;
  int B;
  int64_t n;
  const float* noise;     // DDIM, tables: eta noise, row idx at noise + idx * noise_stride; may be NULL
  int64_t noise_stride;
  int clip;               // DDIM
  float* ring;            // [4][B][n] guided eps by idx & 3
  const int32_t* start;   // DDIM index of the loop's first step
  const float* weights;   // kTable: row of step idx with j earlier steps at weights + idx * w_pitch + 4 * j
  int64_t w_pitch;
  const float* gtab;      // kScaleTable: [N]
  const uint32_t* rng;    // drawn noise: the generator state
  BlendArgs bl;
};

// The blend's row of the launch: whether it runs, q_coef[idx-1] and (tables) Q[idx-1].  Never reads a row at -1.
struct BlendRow {
  bool on;
  float qa, qb;
  const float* qn;
};
__device__ __forceinline__ BlendRow blend_row(const BlendArgs& bl, int idx, bool table) {
  BlendRow r{bl.z0 != nullptr && idx >= 1, 0.f, 0.f, nullptr};
  if (r.on) {
    r.qa = bl.q_coef[(idx - 1) * 2 + 0];
    r.qb = bl.q_coef[(idx - 1) * 2 + 1];
    if (table) r.qn = bl.q_noise + (int64_t)(idx - 1) * bl.q_stride;
  }
  return r;
}

// CFG + DDIM update, one element per thread, any n: ldm_cfg_ddim_update (Blend = false) and _masked (Blend = true).
template <typename TX, bool Blend>
__global__ __launch_bounds__(256) void cfg_ddim_kernel(UpdateArgs a) {
  const int idx = *a.index;
  const float* noise = a.noise ? a.noise + (int64_t)idx * a.noise_stride : nullptr;
  const float c1 = a.coef[idx * 4 + 0], c2 = a.coef[idx * 4 + 1];
  const float a_prev = a.coef[idx * 4 + 2], sigma = a.coef[idx * 4 + 3];
  const float sa = sqrtf(a_prev);
  const float sb = sqrtf(1.0f - a_prev - sigma * sigma);
  BlendRow br{};
  if constexpr (Blend) br = blend_row(a.bl, idx, true);
  TX* x_unet = (TX*)a.x_unet;
  const int64_t total = (int64_t)a.B * a.n;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const float eu = a.eps_all[i], ec = a.eps_all[total + i];
    const float eps = eu + a.gs * (ec - eu);
    const float x = a.xt[i];
    float x0 = c1 * x - c2 * eps;
    if (a.clip) x0 = fminf(fmaxf(x0, -1.f), 1.f);
    const float mean = sa * x0 + sb * eps;
    float o = mean + (noise ? noise[i] : 0.f) * sigma;
    if constexpr (Blend) {
      if (br.on) {
        // i = (b * n + pixel * channels + c) -> b * (n / channels) + pixel
        const float m = a.bl.mask[i / a.bl.channels];
        const float q = q_sample_f(br.qa, br.qb, a.bl.z0[i], br.qn[i]);
        o = m * q + (1.f - m) * o;
      }
    }
    a.xt_out[i] = o;
    if (a.pred_x0_out) a.pred_x0_out[i] = x0;
    if (x_unet) { Elem<TX>::st(x_unet + i, o); Elem<TX>::st(x_unet + total + i, o); }
  }
}
// decrement happens in its own 1-thread kernel AFTER the update so that every block
// of the update kernel has read *index first
__global__ void dec_index_kernel(int32_t* index) { *index = *index - 1; }

// How e', which takes the place of eps in the sigma = 0 update, is formed from this step's e0 and the j =
// clamp(*start - idx, 0, 3) steps before it (ring slots (idx+1 .. idx+j) & 3; e0 goes to slot idx & 3):
//   kDdim            no history, and the rest of the DDIM step: sigma, clip, eta noise of stream eta_stream + idx
//                    (skipped when sigma == 0).  Instantiated with drawn noise only; tables take cfg_ddim_kernel.
//   kAdamsBashforth  the constants of model_runners.PLMS_WEIGHTS as (numerators) / denominator
//   kTable           e' = sum_{m <= j} w[m] * e_{idx+m} by explicit fused multiply-adds in the order m = 0 .. j
//                    (DESIGN.md section 10); weights == NULL: no history, ring and start are not touched
//   kInvert          no history, and the step runs the other way: xt is on the level of a_prev,
//                    x0 = (xt - sqrt(1 - a_prev) * e0) / sqrt(a_prev), xt' = (x0 + c2 * e0) / c1 is on the level of
//                    steps[idx]; no sigma, noise, clip or blend.  Tables only (it draws nothing).
// j is uniform over the launch, so a slot or a weight beyond j is never loaded (it may hold NaN).
enum Hist { kDdim, kAdamsBashforth, kTable, kInvert };
// Where the scale of e0 = eu + gs * (ec - eu) comes from: the argument, gtab[idx], or none at all: e0 = ec and the
// unconditional half of eps_all is never loaded.
enum Scale { kScaleArg, kScaleTable, kCondOnly };

// Four elements per thread, 16-byte accesses (update_check: n % 4 and the alignments).  Rng: the blend's Q[idx-1] is
// drawn from stream q_stream + idx - 1 instead of read from bl.q_noise.  Blend = false leaves the blend out at compile
// time (PLMS from tables without z0: three registers fewer); every other form decides by bl.z0 at run time.
template <typename TX, Hist H, Scale S, bool Rng, bool Blend>
__global__ __launch_bounds__(256) void cfg_update4_kernel(UpdateArgs a) {
  static_assert(H != kDdim || Rng, "DDIM from tables is cfg_ddim_kernel");
  static_assert(H != kInvert || (!Rng && !Blend && S != kScaleTable), "the inversion draws and blends nothing");
  const int idx = *a.index;
  const bool hist = H == kAdamsBashforth || (H == kTable && a.weights);
  int j = 0;
  if (hist) {
    const int d = *a.start - idx;
    j = d < 0 ? 0 : (d > 3 ? 3 : d);
  }
  float w0 = 1.f, w1 = 0.f, w2 = 0.f, w3 = 0.f;
  if (H == kTable && a.weights) {
    const float* wr = a.weights + (int64_t)idx * a.w_pitch + 4 * j;
    w0 = wr[0];
    w1 = j >= 1 ? wr[1] : 0.f;
    w2 = j >= 2 ? wr[2] : 0.f;
    w3 = j >= 3 ? wr[3] : 0.f;
  }
  float gs = a.gs;
  if constexpr (S == kScaleTable) gs = a.gtab[idx];
  const float c1 = a.coef[idx * 4 + 0], c2 = a.coef[idx * 4 + 1], a_prev = a.coef[idx * 4 + 2];
  const float sigma = H == kDdim ? a.coef[idx * 4 + 3] : 0.f;
  const float sa = sqrtf(a_prev);
  const float sb = H == kDdim ? sqrtf(1.0f - a_prev - sigma * sigma) : sqrtf(1.0f - a_prev);
  const bool draw_eta = H == kDdim && sigma != 0.f;
  const int64_t total = (int64_t)a.B * a.n;
  float* e_out = hist ? a.ring + (int64_t)(idx & 3) * total : nullptr;
  const float *e1 = nullptr, *e2 = nullptr, *e3 = nullptr;
  if (hist) {
    e1 = a.ring + (int64_t)((idx + 1) & 3) * total;
    e2 = a.ring + (int64_t)((idx + 2) & 3) * total;
    e3 = a.ring + (int64_t)((idx + 3) & 3) * total;
  }
  BlendRow br{};
  if constexpr (Blend) br = blend_row(a.bl, idx, !Rng);
  TX* x_unet = (TX*)a.x_unet;
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < total; i += (int64_t)gridDim.x * 256 * 4) {
    const f32x4 ec = *(const f32x4*)(a.eps_all + total + i);
    const f32x4 x = *(const f32x4*)(a.xt + i);
    f32x4 e0 = ec;
    if constexpr (S != kCondOnly) {
      const f32x4 eu = *(const f32x4*)(a.eps_all + i);
      e0 = eu + gs * (ec - eu);
    }
    f32x4 ep = e0;
    if constexpr (H == kAdamsBashforth) {
      if (j == 1) {
        ep = (3.f * e0 - *(const f32x4*)(e1 + i)) / 2.f;
      } else if (j == 2) {
        ep = (23.f * e0 - 16.f * *(const f32x4*)(e1 + i) + 5.f * *(const f32x4*)(e2 + i)) / 12.f;
      } else if (j == 3) {
        ep = (55.f * e0 - 59.f * *(const f32x4*)(e1 + i) + 37.f * *(const f32x4*)(e2 + i) -
              9.f * *(const f32x4*)(e3 + i)) / 24.f;
      }
    } else if constexpr (H == kTable) {
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
    }
    f32x4 x0;
    if constexpr (H == kInvert) x0 = (x - sb * ep) / sa;
    else x0 = c1 * x - c2 * ep;
    if constexpr (H == kDdim) {
      if (a.clip) {
#pragma unroll
        for (int k = 0; k < 4; ++k) x0[k] = fminf(fmaxf(x0[k], -1.f), 1.f);
      }
    }
    f32x4 o;
    if constexpr (H == kInvert) o = (x0 + c2 * ep) / c1;
    else o = sa * x0 + sb * ep;
    const int64_t b = i / a.n;                         // (drawn noise: sample b, quad q of it)
    const uint32_t q = (uint32_t)((i - b * a.n) >> 2);
    if (draw_eta) {
      const f32x4 nz = rng_normal4(a.rng, q, (uint32_t)b, (uint32_t)LDM_RNG_ETA_STREAM + (uint32_t)idx);
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = o[k] + nz[k] * sigma;
    }
    if (br.on) {
      const f32x4 z = *(const f32x4*)(a.bl.z0 + i);
      f32x4 qe;
      if constexpr (Rng) qe = rng_normal4(a.rng, q, (uint32_t)b, (uint32_t)LDM_RNG_Q_STREAM + (uint32_t)(idx - 1));
      else qe = *(const f32x4*)(br.qn + i);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float m = a.bl.mask[(i + k) / a.bl.channels];
        const float qs = q_sample_f(br.qa, br.qb, z[k], qe[k]);
        o[k] = m * qs + (1.f - m) * o[k];
      }
    }
    if (e_out) *(f32x4*)(e_out + i) = e0;
    *(f32x4*)(a.xt_out + i) = o;
    if (a.pred_x0_out) *(f32x4*)(a.pred_x0_out + i) = x0;
    if (x_unet) { st4(x_unet + i, o); st4(x_unet + total + i, o); }
  }
}

// ---- host side ------------------------------------------------------------------------------------------------
inline bool al16(const void* p) { return (uintptr_t)p % 16 == 0; }
inline bool xu_ok(const void* p, int d) { return (uintptr_t)p % (d == LDM_BF16 ? 8 : 16) == 0; }

// what an entry requires besides eps_all, xt, xt_out, coef and index
// (kQNoiseAligned: q_noise must be 16-byte aligned even without z0)
enum : unsigned {
  kWide = 1, kNeedRing = 2, kNeedWeights = 4, kNeedRng = 8, kNeedGtab = 16, kNeedBlend = 32, kQNoiseAligned = 64
};

UpdateArgs update_base(const float* eps_all, const float* xt, float* xt_out, float* pred_x0_out, void* x_unet_out,
                       const float* coef, const int32_t* index, float guidance_scale, int B, int64_t n_per_sample) {
  UpdateArgs a{};
  a.eps_all = eps_all, a.xt = xt, a.xt_out = xt_out, a.pred_x0_out = pred_x0_out, a.x_unet = x_unet_out;
  a.coef = coef, a.index = index, a.gs = guidance_scale, a.B = B, a.n = n_per_sample;
  return a;
}

// Validates the arguments of any update entry (kWide: the four-wide body's n % 4 and alignments) and settles a.bl:
// empty without z0, without a Q table when Q is drawn (a.rng).
int update_check(const char* what, unsigned need, UpdateArgs& a, int x_dtype) {
  const bool draws = a.rng != nullptr;
  BlendArgs& bl = a.bl;
  LDM_CHECK_ARG(a.eps_all && a.xt && a.xt_out && a.coef && a.index && (!(need & kNeedRing) || (a.ring && a.start)) &&
                    (!(need & kNeedWeights) || a.weights) && (!(need & kNeedRng) || a.rng) &&
                    (!(need & kNeedGtab) || a.gtab) &&
                    (!(need & kNeedBlend) || (bl.z0 && bl.mask && bl.q_noise && bl.q_coef)),
                "%s: null pointer", what);
  LDM_CHECK_ARG(!a.weights || (a.ring && a.start), "%s: weights without ring / start", what);
  LDM_CHECK_ARG(DT_OK(x_dtype) && a.B > 0 && a.n > 0 && (!(need & kWide) || a.n % 4 == 0),
                need & kWide ? "%s: bad args (n_per_sample=%lld must be a positive multiple of 4)" : "%s: bad args",
                what, (long long)a.n);
  LDM_CHECK_ARG(!a.weights || a.w_pitch >= 16, "%s: weights_pitch=%lld, a row holds 4 x 4 floats", what,
                (long long)a.w_pitch);
  LDM_CHECK_ARG(!(need & kWide) ||
                    (al16(a.eps_all) && al16(a.xt) && al16(a.ring) && al16(a.xt_out) && al16(a.pred_x0_out) &&
                     al16(bl.z0) && xu_ok(a.x_unet, x_dtype) && (!(need & kQNoiseAligned) || al16(bl.q_noise)) &&
                     (draws || !bl.z0 || (al16(bl.q_noise) && bl.q_stride % 4 == 0))),
                "%s: arrays must be 16-byte aligned (q_index_stride a multiple of 4)", what);
  if (!bl.z0) {
    bl = BlendArgs{};
    return LDM_OK;
  }
  LDM_CHECK_ARG(bl.mask && bl.q_coef && (draws || bl.q_noise),
                need & kNeedRng ? "%s: z0 without mask / q_coef" : "%s: z0 without mask / q_noise / q_coef", what);
  LDM_CHECK_ARG(bl.channels > 0 && a.n % bl.channels == 0 && bl.q_stride >= 0,
                "%s: bad args (n_per_sample=%lld, channels=%d)", what, (long long)a.n, bl.channels);
  if (draws) bl.q_noise = nullptr, bl.q_stride = 0;
  return LDM_OK;
}

// Checks, then the instantiation of (hist, scale, whether noise is drawn, x_dtype), then the decrement of *index.
int update_launch(const char* what, unsigned need, Hist hist, Scale scale, UpdateArgs a, int x_dtype, int32_t* index,
                  int dec_index, void* stream) {
  const int st = update_check(what, need, a, x_dtype);
  if (st != LDM_OK) return st;
  hipStream_t s = (hipStream_t)stream;
  const bool wide = need & kWide;
  const dim3 g(grid_for(wide ? (int64_t)a.B * a.n / 4 : (int64_t)a.B * a.n, 256, 1024));
#define LAUNCH(KERNEL, ...)                                                                         \
  do {                                                                                              \
    if (x_dtype == LDM_BF16) hipLaunchKernelGGL((KERNEL<bf16_t, __VA_ARGS__>), g, dim3(256), 0, s, a); \
    else hipLaunchKernelGGL((KERNEL<float, __VA_ARGS__>), g, dim3(256), 0, s, a);                   \
  } while (0)
#define FORM(H, S, DRAWS) ((H) | (S) << 2 | (DRAWS) << 4)
  switch (FORM(hist, scale, a.rng != nullptr) | (wide ? 0 : 32)) {
    case FORM(kDdim, kScaleArg, 0) | 32:                                  // ldm_cfg_ddim_update, _masked
      if (a.bl.z0) LAUNCH(cfg_ddim_kernel, true); else LAUNCH(cfg_ddim_kernel, false);
      break;
    case FORM(kDdim, kScaleArg, 1): LAUNCH(cfg_update4_kernel, kDdim, kScaleArg, true, true); break;   // _ddim_.._rng
    case FORM(kAdamsBashforth, kScaleArg, 0):                             // ldm_cfg_plms_update
      if (a.bl.z0) LAUNCH(cfg_update4_kernel, kAdamsBashforth, kScaleArg, false, true);
      else LAUNCH(cfg_update4_kernel, kAdamsBashforth, kScaleArg, false, false);
      break;
    case FORM(kAdamsBashforth, kScaleArg, 1):                             // ldm_cfg_plms_update_rng
      LAUNCH(cfg_update4_kernel, kAdamsBashforth, kScaleArg, true, true);
      break;
    case FORM(kTable, kScaleArg, 0): LAUNCH(cfg_update4_kernel, kTable, kScaleArg, false, true); break;   // _ms_update
    case FORM(kTable, kScaleArg, 1): LAUNCH(cfg_update4_kernel, kTable, kScaleArg, true, true); break;    // _ms_.._rng
    // ldm_cfg_sched_update
    case FORM(kTable, kScaleTable, 0): LAUNCH(cfg_update4_kernel, kTable, kScaleTable, false, true); break;
    case FORM(kTable, kScaleTable, 1): LAUNCH(cfg_update4_kernel, kTable, kScaleTable, true, true); break;
    case FORM(kTable, kCondOnly, 0): LAUNCH(cfg_update4_kernel, kTable, kCondOnly, false, true); break;
    case FORM(kTable, kCondOnly, 1): LAUNCH(cfg_update4_kernel, kTable, kCondOnly, true, true); break;
    case FORM(kInvert, kScaleArg, 0): LAUNCH(cfg_update4_kernel, kInvert, kScaleArg, false, false); break;   // _invert
    case FORM(kInvert, kCondOnly, 0): LAUNCH(cfg_update4_kernel, kInvert, kCondOnly, false, false); break;
    default: LDM_CHECK_ARG(false, "%s: no kernel for this form", what);
  }
#undef FORM
#undef LAUNCH
  int status = ldm_launch_status(what);
  if (status == LDM_OK && dec_index) {
    hipLaunchKernelGGL(dec_index_kernel, dim3(1), dim3(1), 0, s, index);
    status = ldm_launch_status(what);
  }
  return status;
}

}  // namespace

extern "C" int ldm_cfg_ddim_update(const float* eps_all, const float* xt, const float* noise,
                                   int64_t noise_index_stride, float* xt_out, float* pred_x0_out,
                                   void* x_unet_out, int x_dtype, const float* coef,
                                   int32_t* index, int dec_index, float guidance_scale,
                                   int clip_denoised, int B, int64_t n_per_sample, void* stream) {
  UpdateArgs a =
      update_base(eps_all, xt, xt_out, pred_x0_out, x_unet_out, coef, index, guidance_scale, B, n_per_sample);
  a.noise = noise, a.noise_stride = noise_index_stride, a.clip = clip_denoised;
  return update_launch("ldm_cfg_ddim_update", 0, kDdim, kScaleArg, a, x_dtype, index, dec_index, stream);
}

extern "C" int ldm_cfg_ddim_update_masked(const float* eps_all, const float* xt, const float* noise,
                                          int64_t noise_index_stride, float* xt_out, float* pred_x0_out,
                                          void* x_unet_out, int x_dtype, const float* coef, int32_t* index,
                                          int dec_index, float guidance_scale, int clip_denoised, int B,
                                          int64_t n_per_sample, const float* z0, const float* mask,
                                          const float* q_noise, int64_t q_index_stride, const float* q_coef,
                                          int channels, void* stream) {
  UpdateArgs a =
      update_base(eps_all, xt, xt_out, pred_x0_out, x_unet_out, coef, index, guidance_scale, B, n_per_sample);
  a.noise = noise, a.noise_stride = noise_index_stride, a.clip = clip_denoised;
  a.bl = BlendArgs{z0, mask, q_noise, q_index_stride, q_coef, channels};
  return update_launch("ldm_cfg_ddim_update_masked", kNeedBlend, kDdim, kScaleArg, a, x_dtype, index, dec_index,
                       stream);
}

extern "C" int ldm_cfg_plms_update(const float* eps_all, const float* xt, float* ring, float* xt_out,
                                   float* pred_x0_out, void* x_unet_out, int x_dtype, const float* coef,
                                   int32_t* index, const int32_t* start, int dec_index, float guidance_scale, int B,
                                   int64_t n_per_sample, const float* z0, const float* mask, const float* q_noise,
                                   int64_t q_index_stride, const float* q_coef, int channels, void* stream) {
  UpdateArgs a =
      update_base(eps_all, xt, xt_out, pred_x0_out, x_unet_out, coef, index, guidance_scale, B, n_per_sample);
  a.ring = ring, a.start = start, a.bl = BlendArgs{z0, mask, q_noise, q_index_stride, q_coef, channels};
  return update_launch("ldm_cfg_plms_update", kWide | kNeedRing | kQNoiseAligned, kAdamsBashforth, kScaleArg, a,
                       x_dtype, index, dec_index, stream);
}

extern "C" int ldm_cfg_ddim_update_rng(const float* eps_all, const float* xt, const uint32_t* rng, float* xt_out,
                                       float* pred_x0_out, void* x_unet_out, int x_dtype, const float* coef,
                                       int32_t* index, int dec_index, float guidance_scale, int clip_denoised, int B,
                                       int64_t n_per_sample, const float* z0, const float* mask, const float* q_coef,
                                       int channels, void* stream) {
  UpdateArgs a =
      update_base(eps_all, xt, xt_out, pred_x0_out, x_unet_out, coef, index, guidance_scale, B, n_per_sample);
  a.rng = rng, a.clip = clip_denoised, a.bl = BlendArgs{z0, mask, nullptr, 0, q_coef, channels};
  return update_launch("ldm_cfg_ddim_update_rng", kWide | kNeedRng, kDdim, kScaleArg, a, x_dtype, index, dec_index,
                       stream);
}

extern "C" int ldm_cfg_plms_update_rng(const float* eps_all, const float* xt, float* ring, float* xt_out,
                                       float* pred_x0_out, void* x_unet_out, int x_dtype, const float* coef,
                                       int32_t* index, const int32_t* start, const uint32_t* rng, int dec_index,
                                       float guidance_scale, int B, int64_t n_per_sample, const float* z0,
                                       const float* mask, const float* q_coef, int channels, void* stream) {
  UpdateArgs a =
      update_base(eps_all, xt, xt_out, pred_x0_out, x_unet_out, coef, index, guidance_scale, B, n_per_sample);
  a.ring = ring, a.start = start, a.rng = rng, a.bl = BlendArgs{z0, mask, nullptr, 0, q_coef, channels};
  return update_launch("ldm_cfg_plms_update_rng", kWide | kNeedRing | kNeedRng, kAdamsBashforth, kScaleArg, a, x_dtype,
                       index, dec_index, stream);
}

extern "C" int ldm_cfg_ms_update(const float* eps_all, const float* xt, float* ring, float* xt_out,
                                 float* pred_x0_out, void* x_unet_out, int x_dtype, const float* coef,
                                 int32_t* index, const int32_t* start, const float* weights, int64_t weights_pitch,
                                 int dec_index, float guidance_scale, int B, int64_t n_per_sample, const float* z0,
                                 const float* mask, const float* q_noise, int64_t q_index_stride, const float* q_coef,
                                 int channels, void* stream) {
  UpdateArgs a =
      update_base(eps_all, xt, xt_out, pred_x0_out, x_unet_out, coef, index, guidance_scale, B, n_per_sample);
  a.ring = ring, a.start = start, a.weights = weights, a.w_pitch = weights_pitch;
  a.bl = BlendArgs{z0, mask, q_noise, q_index_stride, q_coef, channels};
  return update_launch("ldm_cfg_ms_update", kWide | kNeedRing | kNeedWeights, kTable, kScaleArg, a, x_dtype, index,
                       dec_index, stream);
}

extern "C" int ldm_cfg_ms_update_rng(const float* eps_all, const float* xt, float* ring, float* xt_out,
                                     float* pred_x0_out, void* x_unet_out, int x_dtype, const float* coef,
                                     int32_t* index, const int32_t* start, const float* weights,
                                     int64_t weights_pitch, const uint32_t* rng, int dec_index, float guidance_scale,
                                     int B, int64_t n_per_sample, const float* z0, const float* mask,
                                     const float* q_coef, int channels, void* stream) {
  UpdateArgs a =
      update_base(eps_all, xt, xt_out, pred_x0_out, x_unet_out, coef, index, guidance_scale, B, n_per_sample);
  a.ring = ring, a.start = start, a.weights = weights, a.w_pitch = weights_pitch, a.rng = rng;
  a.bl = BlendArgs{z0, mask, nullptr, 0, q_coef, channels};
  return update_launch("ldm_cfg_ms_update_rng", kWide | kNeedRing | kNeedWeights | kNeedRng, kTable, kScaleArg, a,
                       x_dtype, index, dec_index, stream);
}

extern "C" int ldm_cfg_sched_update(const float* eps_all, const float* xt, float* ring, float* xt_out,
                                    float* pred_x0_out, void* x_unet_out, int x_dtype, const float* coef,
                                    const float* gtab, int32_t* index, const int32_t* start, const float* weights,
                                    int64_t weights_pitch, const uint32_t* rng, int guided, int dec_index, int B,
                                    int64_t n_per_sample, const float* z0, const float* mask, const float* q_noise,
                                    int64_t q_index_stride, const float* q_coef, int channels, void* stream) {
  UpdateArgs a = update_base(eps_all, xt, xt_out, pred_x0_out, x_unet_out, coef, index, 1.f, B, n_per_sample);
  a.ring = ring, a.start = start, a.weights = weights, a.w_pitch = weights_pitch, a.gtab = gtab, a.rng = rng;
  a.bl = BlendArgs{z0, mask, q_noise, q_index_stride, q_coef, channels};
  return update_launch("ldm_cfg_sched_update", kWide | kNeedGtab, kTable, guided ? kScaleTable : kCondOnly, a, x_dtype,
                       index, dec_index, stream);
}

extern "C" int ldm_cfg_ddim_invert_update(const float* eps_all, const float* xt, float* xt_out, float* pred_x0_out,
                                          void* x_unet_out, int x_dtype, const float* coef, int32_t* index,
                                          int guided, int dec_index, float guidance_scale, int B,
                                          int64_t n_per_sample, void* stream) {
  UpdateArgs a =
      update_base(eps_all, xt, xt_out, pred_x0_out, x_unet_out, coef, index, guidance_scale, B, n_per_sample);
  return update_launch("ldm_cfg_ddim_invert_update", kWide, kInvert, guided ? kScaleArg : kCondOnly, a, x_dtype, index,
                       dec_index, stream);
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
  const dim3 g(grid_for((int64_t)B * n_per_sample, 256, 1024));
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

extern "C" int ldm_philox_u32(uint32_t* out, const uint32_t* rng, uint32_t stream_word, int B, int64_t n_per_sample,
                              void* stream) {
  LDM_CHECK_ARG(out && rng, "ldm_philox_u32: null pointer");
  LDM_CHECK_ARG(B > 0 && n_per_sample > 0 && n_per_sample % 4 == 0 && al16(out),
                "ldm_philox_u32: n_per_sample=%lld must be a positive multiple of 4, out 16-byte aligned",
                (long long)n_per_sample);
  hipLaunchKernelGGL(philox_u32_kernel, dim3(grid_for((int64_t)B * n_per_sample / 4, 256, 1024)), dim3(256), 0,
                     (hipStream_t)stream, out, rng, stream_word, B, n_per_sample);
  return ldm_launch_status("ldm_philox_u32");
}

extern "C" int ldm_normal_fill(float* out, const uint32_t* rng, uint32_t stream_word, int B, int64_t n_per_sample,
                               void* x_unet_out, int x_dtype, void* stream) {
  LDM_CHECK_ARG(out && rng, "ldm_normal_fill: null pointer");
  LDM_CHECK_ARG(DT_OK(x_dtype) && B > 0 && n_per_sample > 0 && n_per_sample % 4 == 0 && al16(out) &&
                    xu_ok(x_unet_out, x_dtype),
                "ldm_normal_fill: n_per_sample=%lld must be a positive multiple of 4, arrays 16-byte aligned",
                (long long)n_per_sample);
  hipStream_t s = (hipStream_t)stream;
  const dim3 g(grid_for((int64_t)B * n_per_sample / 4, 256, 1024));
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
  LDM_CHECK_ARG(DT_OK(x_dtype) && B > 0 && n_per_sample > 0 && num_steps > 0 && n_per_sample % 4 == 0 && al16(x0) &&
                    al16(xt_out) && xu_ok(x_unet_out, x_dtype),
                "ldm_q_sample_rng: n_per_sample=%lld must be a positive multiple of 4, arrays 16-byte aligned",
                (long long)n_per_sample);
  hipStream_t s = (hipStream_t)stream;
  const dim3 g(grid_for((int64_t)B * n_per_sample / 4, 256, 1024));
  if (x_dtype == LDM_BF16)
    hipLaunchKernelGGL(q_sample_rng_kernel<bf16_t>, g, dim3(256), 0, s, x0, rng, stream_word, t, sqrt_alphas_cumprod,
                       sqrt_one_minus_alphas_cumprod, num_steps, xt_out, (bf16_t*)x_unet_out, B, n_per_sample);
  else
    hipLaunchKernelGGL(q_sample_rng_kernel<float>, g, dim3(256), 0, s, x0, rng, stream_word, t, sqrt_alphas_cumprod,
                       sqrt_one_minus_alphas_cumprod, num_steps, xt_out, (float*)x_unet_out, B, n_per_sample);
  return ldm_launch_status("ldm_q_sample_rng");
}
