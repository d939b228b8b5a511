// Per-step kernels of the sampling loops behind LatentDiffusion.log_images: the masked re-noise
// of inpainting, the ancestral (p_sample) update, the quantised-x0 forms of the DDIM and the
// ancestral update, and the DDIM inversion step (DDIMSamplerAttn.next_step).  fp32 NCHW latents; all of it is latency-bound at the sampling shapes
// (2 048 pixels at N = 8), so each is one launch per step that a captured step graph replays:
// timesteps and coefficient rows are read from device memory at execution time.
//
// The quantised forms are pixel-major: the lanes of a pixel form pred_x0 for all e_dim channels
// (every lane of the row computes the same values), search the codebook with vq_search.h (the
// search of the VQ decode head) and lane 0 of the row finishes the update with the code itself.
#include "vq_search.h"

namespace {

enum { STEP_DDIM = 0, STEP_ANCESTRAL = 1, STEP_INVERT = 2 };

__global__ void renoise_kernel(float* img, const float* x0, const float* z, const float* mask, const int mask_c,
                               const long long* t, const float* sa, const float* s1a, const int batch, const int c,
                               const int hw) {
  const long per = (long)c * hw;
  const long n = (long)batch * per;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int b = (int)(i / per);
    const long r = i - b * per;
    const float m = mask[mask_c == 1 ? (long)b * hw + r % hw : i];
    if (m == 0.f) continue;  // img kept as it is (bitwise)
    const long long tt = t[b];
    // q_sample with qsample_kernel's rounding: both products rounded, then one add.  The empty asm
    // makes the products opaque, so -ffp-contract=fast cannot fuse either into the add.
    float qa = sa[tt] * x0[i], qb = s1a[tt] * z[i];
    asm volatile("" : "+v"(qa), "+v"(qb));
    const float q = qa + qb;
    img[i] = m == 1.f ? q : m * q + (1.f - m) * img[i];
  }
}

struct Coef {
  float v[5];
};

// coefficient row of this step: the device table at *index, or the scalars of the call
template <int KIND>
ED_DEV Coef load_coef(const EncdiffSamplerStepArgs& p, int& row) {
  constexpr int N = KIND == STEP_DDIM ? 4 : (KIND == STEP_INVERT ? 2 : 5);
  Coef k;
  row = p.index ? *p.index : -1;
#pragma unroll
  for (int i = 0; i < N; ++i) k.v[i] = p.index ? p.coef[(long)N * row + i] : p.coef_host[i];
  return k;
}

// DDIM (ddim.py:197-206), k = {a_t, a_prev, sigma, sqrt(1 - a_t)}
struct DdimMath {
  float s1, rs, sap, dcoef, sigma;
  ED_DEV DdimMath(const Coef& k, int) {
    s1 = k.v[3];
    rs = 1.f / sqrtf(k.v[0]);
    sap = sqrtf(k.v[1]);
    sigma = k.v[2];
    dcoef = sqrtf(1.f - k.v[1] - sigma * sigma);
  }
  ED_DEV float x0(float x, float e, int) const { return (x - s1 * e) * rs; }
  ED_DEV float next(float x0v, float, float e, const float* z, long i) const {
    return sap * x0v + dcoef * e + (z ? sigma * z[i] : 0.f);
  }
};

// ancestral step (ddpm_enc.py:234-247, 1255-1315), k = {sqrt_recip_ac, sqrt_recipm1_ac,
// posterior_mean_coef1, posterior_mean_coef2, posterior_log_variance_clipped} at t = row
struct AncestralMath {
  float c0, c1, m1, m2, sd;
  bool noisy;
  ED_DEV AncestralMath(const Coef& k, int row) {
    c0 = k.v[0]; c1 = k.v[1]; m1 = k.v[2]; m2 = k.v[3];
    sd = expf(0.5f * k.v[4]);
    noisy = row != 0;  // no noise at t == 0
  }
  ED_DEV float x0(float x, float e, int clamp) const {
    const float r = c0 * x - c1 * e;
    return clamp ? fminf(fmaxf(r, -1.f), 1.f) : r;
  }
  ED_DEV float next(float x0v, float x, float, const float* z, long i) const {
    const float mean = m1 * x0v + m2 * x;
    return (noisy && z) ? mean + sd * z[i] : mean;
  }
};

// DDIM inversion (ddim.py:469-482 next_step), k = {a_t, a_next}: the deterministic step upwards in t
struct InvertMath {
  float s1, sa, san, dn;
  ED_DEV InvertMath(const Coef& k, int) {
    s1 = sqrtf(1.f - k.v[0]);
    sa = sqrtf(k.v[0]);
    san = sqrtf(k.v[1]);
    dn = sqrtf(1.f - k.v[1]);
  }
  ED_DEV float x0(float x, float e, int) const { return (x - s1 * e) / sa; }
  ED_DEV float next(float x0v, float, float e, const float*, long) const { return san * x0v + dn * e; }
};

template <int KIND>
struct MathOf {
  typedef DdimMath type;
};
template <>
struct MathOf<STEP_ANCESTRAL> {
  typedef AncestralMath type;
};
template <>
struct MathOf<STEP_INVERT> {
  typedef InvertMath type;
};

template <int KIND>
__global__ void step_kernel(const EncdiffSamplerStepArgs p) {
  int row;
  const Coef k = load_coef<KIND>(p, row);
  const typename MathOf<KIND>::type mth(k, row);
  const long n = (long)p.batch * p.c * p.hw;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float x = p.x[i], e = p.e[i];
    const float x0v = mth.x0(x, e, p.clamp);
    if (p.x0_out) p.x0_out[i] = x0v;
    p.x_out[i] = mth.next(x0v, x, e, p.noise, i);
  }
}

template <int ED, int KIND>
__global__ __launch_bounds__(VQ_T) void step_quant_kernel(const EncdiffSamplerStepArgs p, const int split,
                                                          const int chunk) {
  __shared__ float cb[VQ_LDS_FLOATS];
  int crow;
  const Coef k = load_coef<KIND>(p, crow);
  const typename MathOf<KIND>::type mth(k, crow);
  const long total = (long)p.batch * p.hw;
  const int rows_per_block = VQ_T / split;
  const int sub = threadIdx.x % split;
  const long row_raw = (long)blockIdx.x * rows_per_block + threadIdx.x / split;
  const bool live = row_raw < total;
  const long row = live ? row_raw : total - 1;  // dead lanes keep the barriers / shuffles uniform
  const long b = row / p.hw, px = row - b * p.hw;

  float x[ED], e[ED], q[ED];
#pragma unroll
  for (int c = 0; c < ED; ++c) {
    const long i = (b * ED + c) * p.hw + px;
    x[c] = p.x[i];
    e[c] = p.e[i];
    q[c] = mth.x0(x[c], e[c], p.clamp);
  }
  const int best = vq_search<ED>(q, cb, p.codebook, p.n_e, split, sub, chunk);
  if (!live || sub) return;  // every read of the row is done: x_out may alias x

  if (p.idx_out) p.idx_out[row] = best;
#pragma unroll
  for (int c = 0; c < ED; ++c) {
    const long i = (b * ED + c) * p.hw + px;
    const float code = p.codebook[(long)best * ED + c];
    if (p.x0_out) p.x0_out[i] = code;
    p.x_out[i] = mth.next(code, x[c], e[c], p.noise, i);
  }
}

__global__ void step_index_dec_kernel(int* index) { *index -= 1; }
__global__ void step_index_inc_kernel(int* index) { *index += 1; }  // inversion walks upwards in t

inline int grid_of(long n) {
  const long g = (n + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

template <int ED, int KIND>
void quant_launch(const EncdiffSamplerStepArgs& a, hipStream_t s) {
  const long total = (long)a.batch * a.hw;
  const int split = vq_split(total, a.n_e);
  const int rows_per_block = VQ_T / split;
  const long grid = (total + rows_per_block - 1) / rows_per_block;
  hipLaunchKernelGGL((step_quant_kernel<ED, KIND>), dim3((unsigned)grid), dim3(VQ_T), 0, s, a, split,
                     VQ_LDS_FLOATS / ED);
}

template <int KIND>
int step_launch(const EncdiffSamplerStepArgs* a, void* stream) {
  if (!a || !a->x || !a->e || !a->x_out) return ENCDIFF_ERR_ARG;
  // inversion adds no noise and quantises nothing
  if (KIND == STEP_INVERT && (a->noise || a->codebook || a->n_e != 0 || a->clamp || a->idx_out))
    return ENCDIFF_ERR_ARG;
  if ((a->index != nullptr) != (a->coef != nullptr)) return ENCDIFF_ERR_ARG;
  if (KIND == STEP_ANCESTRAL && !a->index) return ENCDIFF_ERR_ARG;  // t is the table row
  if (a->advance && !a->index) return ENCDIFF_ERR_ARG;
  if (a->batch <= 0 || a->c <= 0 || a->hw <= 0) return ENCDIFF_ERR_SHAPE;
  if (KIND != STEP_INVERT && (long)a->batch * a->hw * VQ_MAX_DIM >= (1L << 31)) return ENCDIFF_ERR_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  if constexpr (KIND == STEP_INVERT) {
    if ((long)a->batch * a->c * a->hw >= (1L << 31)) return ENCDIFF_ERR_SHAPE;
    hipLaunchKernelGGL(step_kernel<KIND>, dim3(grid_of((long)a->batch * a->c * a->hw)), dim3(256), 0, s, *a);
  } else if (a->n_e != 0 || a->codebook) {
    if (a->c > VQ_MAX_DIM || a->n_e < 1 || a->n_e > VQ_MAX_CODES) return ENCDIFF_ERR_SHAPE;
    if (!a->codebook) return ENCDIFF_ERR_ARG;
    switch (a->c) {
      case 1: quant_launch<1, KIND>(*a, s); break;
      case 2: quant_launch<2, KIND>(*a, s); break;
      case 3: quant_launch<3, KIND>(*a, s); break;
      case 4: quant_launch<4, KIND>(*a, s); break;
      case 5: quant_launch<5, KIND>(*a, s); break;
      case 6: quant_launch<6, KIND>(*a, s); break;
      case 7: quant_launch<7, KIND>(*a, s); break;
      default: quant_launch<8, KIND>(*a, s); break;
    }
  } else {
    if (a->idx_out) return ENCDIFF_ERR_ARG;  // nothing was looked up
    if ((long)a->batch * a->c * a->hw >= (1L << 31)) return ENCDIFF_ERR_SHAPE;
    hipLaunchKernelGGL(step_kernel<KIND>, dim3(grid_of((long)a->batch * a->c * a->hw)), dim3(256), 0, s, *a);
  }
  ED_CHECK_LAUNCH();
  if (a->advance) {
    if (KIND == STEP_INVERT) {
      hipLaunchKernelGGL(step_index_inc_kernel, dim3(1), dim3(1), 0, s, a->index);
    } else {
      hipLaunchKernelGGL(step_index_dec_kernel, dim3(1), dim3(1), 0, s, a->index);
    }
    ED_CHECK_LAUNCH();
  }
  return ENCDIFF_OK;
}

}  // namespace

extern "C" int encdiff_masked_renoise(float* img, const float* x0, const float* z, const float* mask, int mask_c,
                                      const long long* t, const float* sqrt_ac, const float* sqrt_1mac, int batch,
                                      int c, int hw, void* stream) {
  if (!img || !x0 || !z || !mask || !t || !sqrt_ac || !sqrt_1mac) return ENCDIFF_ERR_ARG;
  if (batch <= 0 || c <= 0 || hw <= 0 || (mask_c != 1 && mask_c != c)) return ENCDIFF_ERR_SHAPE;
  if ((long)batch * c * hw >= (1L << 31)) return ENCDIFF_ERR_SHAPE;
  hipLaunchKernelGGL(renoise_kernel, dim3(grid_of((long)batch * c * hw)), dim3(256), 0, (hipStream_t)stream, img, x0,
                     z, mask, mask_c, t, sqrt_ac, sqrt_1mac, batch, c, hw);
  ED_CHECK_LAUNCH();
  return ENCDIFF_OK;
}

extern "C" int encdiff_ddim_step_quantized(const EncdiffSamplerStepArgs* a, void* stream) {
  if (a && !a->codebook) return ENCDIFF_ERR_ARG;
  return step_launch<STEP_DDIM>(a, stream);
}

extern "C" int encdiff_ancestral_step(const EncdiffSamplerStepArgs* a, void* stream) {
  return step_launch<STEP_ANCESTRAL>(a, stream);
}

extern "C" int encdiff_ddim_invert_step(const EncdiffSamplerStepArgs* a, void* stream) {
  return step_launch<STEP_INVERT>(a, stream);
}
