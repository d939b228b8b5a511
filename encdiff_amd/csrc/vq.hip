// VQ first-stage decode head: nearest codebook entry per latent pixel (taming VectorQuantizer2,
// autoencoder.py VQModelInterface.decode), the quantised latent, and the decoder's input rows
// post_quant_conv(cat(z_q, s_b)) in one launch.
//
// The search (direct fp32 distance, channel-major LDS chunks, lanes split per row, ties to the
// lowest index) is vq_search.h, shared with the quantised-x0 sampling steps.  The 1x1
// post_quant_conv is linear: rows = T[idx] + Wd s_b + b with T = E Wpq[:, :e_dim]^T composed by
// the caller.
#include "vq_search.h"

namespace {

template <int ED>
__global__ __launch_bounds__(VQ_T) void vq_lookup_kernel(const EncdiffVqArgs p, const int split, const int chunk) {
  __shared__ float cb[VQ_LDS_FLOATS];
  const long total = (long)p.batch * p.hw;
  const int rows_per_block = VQ_T / split;
  const int sub = threadIdx.x % split;
  const long row_raw = (long)blockIdx.x * rows_per_block + threadIdx.x / split;
  const bool live = row_raw < total;
  const long row = live ? row_raw : total - 1;  // dead lanes keep the barriers / shuffles uniform
  const long b = row / p.hw, px = row - b * p.hw;

  float z[ED];
#pragma unroll
  for (int c = 0; c < ED; ++c) z[c] = p.z[(b * ED + c) * p.hw + px];

  const int best = p.quantize ? vq_search<ED>(z, cb, p.codebook, p.n_e, split, sub, chunk) : 0;
  if (!live || sub) return;

  if (p.idx) p.idx[row] = best;
  if (p.zq) {
#pragma unroll
    for (int c = 0; c < ED; ++c) p.zq[(b * ED + c) * p.hw + px] = p.codebook[(long)best * ED + c];
  }
  if (p.rows) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float acc = 0.f;
      if (k < p.z_ch) {
        if (p.quantize) {
          acc = p.table[(long)best * p.z_ch + k];
        } else {
#pragma unroll
          for (int c = 0; c < ED; ++c) acc += p.wq[k * ED + c] * z[c];
        }
        if (p.repr)
          for (int d = 0; d < p.dis_dim; ++d) acc += p.wd[k * p.dis_dim + d] * p.repr[b * p.dis_dim + d];
        acc += p.bias[k];
      }
      v[k] = acc;
    }
    *(uint4*)((bf16_t*)p.rows + row * p.ld_rows) = pack8(v);
  }
}

template <int ED>
int vq_launch(const EncdiffVqArgs& a, int split, hipStream_t s) {
  const long total = (long)a.batch * a.hw;
  const int rows_per_block = VQ_T / split;
  const long grid = (total + rows_per_block - 1) / rows_per_block;
  const int chunk = VQ_LDS_FLOATS / ED;
  hipLaunchKernelGGL(vq_lookup_kernel<ED>, dim3((unsigned)grid), dim3(VQ_T), 0, s, a, split, chunk);
  ED_CHECK_LAUNCH();
  return ENCDIFF_OK;
}

}  // namespace

extern "C" int encdiff_vq_lookup(const EncdiffVqArgs* a, void* stream) {
  if (!a || !a->z) return ENCDIFF_ERR_ARG;
  if (a->batch <= 0 || a->hw <= 0 || a->e_dim < 1 || a->e_dim > VQ_MAX_DIM) return ENCDIFF_ERR_SHAPE;
  const long total = (long)a->batch * a->hw;
  if (total * VQ_MAX_DIM >= (1L << 31)) return ENCDIFF_ERR_SHAPE;
  if (a->quantize) {
    if (!a->codebook) return ENCDIFF_ERR_ARG;
    if (a->n_e < 1 || a->n_e > VQ_MAX_CODES) return ENCDIFF_ERR_SHAPE;
    if (a->rows && !a->table) return ENCDIFF_ERR_ARG;
  } else {
    if (a->idx || a->zq) return ENCDIFF_ERR_ARG;  // nothing was looked up
    if (a->rows && !a->wq) return ENCDIFF_ERR_ARG;
  }
  if (a->rows) {
    if (a->z_ch < 1 || a->z_ch > 8 || a->dis_dim < 0) return ENCDIFF_ERR_SHAPE;
    if (!a->bias || (a->dis_dim > 0 && a->repr && !a->wd)) return ENCDIFF_ERR_ARG;
    if (a->ld_rows < 8 || a->ld_rows % 8 || ((uintptr_t)a->rows % 16)) return ENCDIFF_ERR_ARG;  // one 16-byte store
  }
  const int split = a->quantize ? vq_split(total, a->n_e) : 1;
  hipStream_t s = (hipStream_t)stream;
  switch (a->e_dim) {
    case 1: return vq_launch<1>(*a, split, s);
    case 2: return vq_launch<2>(*a, split, s);
    case 3: return vq_launch<3>(*a, split, s);
    case 4: return vq_launch<4>(*a, split, s);
    case 5: return vq_launch<5>(*a, split, s);
    case 6: return vq_launch<6>(*a, split, s);
    case 7: return vq_launch<7>(*a, split, s);
    default: return vq_launch<8>(*a, split, s);
  }
}
