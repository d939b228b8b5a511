#pragma once
// gemm_finalize.h -- the split-K finalize pass: gemm_finalize() (also the riding finalize blocks of
// the paired and weight-gradient grids) and its two kernels.  Builds on gemm_common.h.
#include "gemm_common.h"

namespace {
// split-K finalize: C = alpha * sum_z slab[z] (+bias)(+resid).  Each lane owns 4
// consecutive outputs (float4 slab loads).  Up to 8 slabs one lane sums them all in z order
// (a workgroup covers 1024 outputs); deeper splits (e.g. 128 slabs of a 64x64 weight
// gradient) give 4 wave-rows every 4th slab and add the 4 partials in a fixed order.  Either
// way bitwise reproducible, no atomics.  The first version (one scalar load per lane,
// 64 outputs per workgroup) spent ~9 us on a 2048x256 split-4 GEMM in workgroup turnover.
constexpr int FIN_ZG = 4;
__host__ __device__ inline int fin_zgroups(const EncdiffGemmArgs& p) { return p.split_k > 8 ? FIN_ZG : 1; }
__host__ __device__ inline bool fin_vec(const EncdiffGemmArgs& p) {
  return (p.N & 3) == 0 && ((uintptr_t)p.workspace & 15) == 0;
}
// outputs one workgroup covers per grid-stride iteration
__host__ __device__ inline int fin_per_block(const EncdiffGemmArgs& p) {
  return (fin_vec(p) ? 4 : 1) * 256 / fin_zgroups(p);
}

// output row of GEMM row m (K4S2_TP: parity-major rows -> their pixel; plain division, the
// finalize is not on a hot path)
__device__ __forceinline__ long fin_row(const EncdiffGemmArgs& p, int m) {
  if (p.a_mode != ENCDIFF_OPA_IM2COL || p.conv.resample != ENCDIFF_RESAMPLE_K4S2_TP) return m;
  const int mq = p.M >> 2, q = m / mq, hh = p.conv.h >> 1, wh = p.conv.w >> 1;
  const int mm = m - q * mq, b = mm / (hh * wh), r = mm - b * hh * wh, y = r / wh, x = r - y * wh;
  return ((long)b * p.conv.h + 2 * y + (q >> 1)) * p.conv.w + 2 * x + (q & 1);
}

__device__ __forceinline__ void fin_store(const EncdiffGemmArgs& p, const bf16_t* R, const long i, float v) {
  const int row0 = (int)(i / p.N), col = (int)(i - (long)row0 * p.N);
  const long row = fin_row(p, row0);
  v = splitk_scale(v, p.alpha, p.bias ? p.bias[col] : 0.f);
  if (R) v += bf2f(R[(long)row * p.ld_resid + col]);
  if (p.c_mode == ENCDIFF_OUT_BF16) ((bf16_t*)p.c)[(long)row * p.ldc + col] = f2bf(v);
  else if (p.c_mode == ENCDIFF_OUT_F32_ACCUM) ((float*)p.c)[(long)row * p.ldc + col] += v;
  else ((float*)p.c)[(long)row * p.ldc + col] = v;
}

__device__ __forceinline__ void gemm_finalize(const EncdiffGemmArgs& p, const int bid, const int nblk) {
  // alpha / bias through splitk_scale: norm.hip's gn_slab_row restates this combine bitwise
  __shared__ float4 part[FIN_ZG][64];
  const long total = (long)p.M * p.N;
  const bf16_t* R = (const bf16_t*)p.resid;
  const int zgn = fin_zgroups(p);
  const int tpo = 256 / zgn;  // lanes per z-group
  const int o = threadIdx.x % tpo, zg = threadIdx.x / tpo;
  const long per = fin_per_block(p);
  if (fin_vec(p)) {
    for (long t0 = (long)bid * per; t0 < total; t0 += (long)nblk * per) {
      const long i = t0 + 4L * o;  // total % 4 == 0: the 4 outputs are in range together
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      if (i < total) {
        const float* w = p.workspace + i;
#pragma unroll 8
        for (int z = zg; z < p.split_k; z += zgn) {
          const float4 v = *(const float4*)(w + (long)z * total);
          acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
      }
      if (zgn > 1) {  // block-uniform branch
        part[zg][o] = acc;
        __syncthreads();
        if (zg == 0) {
          const float4 a0 = part[0][o], a1 = part[1][o], a2 = part[2][o], a3 = part[3][o];
          acc.x = ((a0.x + a1.x) + a2.x) + a3.x;
          acc.y = ((a0.y + a1.y) + a2.y) + a3.y;
          acc.z = ((a0.z + a1.z) + a2.z) + a3.z;
          acc.w = ((a0.w + a1.w) + a2.w) + a3.w;
        }
      }
      if (zg == 0 && i < total) {
        // N % 4 == 0: one row.  32-bit division whenever the problem fits (uniform branch)
        const int row0 = total < (1L << 31) ? (int)i / p.N : (int)(i / p.N);
        const int col = (int)(i - (long)row0 * p.N);
        const long row = fin_row(p, row0);
        float v[4];
        {
          const float4 bb = p.bias ? make_float4(p.bias[col], p.bias[col + 1], p.bias[col + 2], p.bias[col + 3])
                                   : make_float4(0.f, 0.f, 0.f, 0.f);
          v[0] = splitk_scale(acc.x, p.alpha, bb.x);
          v[1] = splitk_scale(acc.y, p.alpha, bb.y);
          v[2] = splitk_scale(acc.z, p.alpha, bb.z);
          v[3] = splitk_scale(acc.w, p.alpha, bb.w);
        }
        if (R) {
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] += bf2f(R[(long)row * p.ld_resid + col + k]);
        }
        const long co = (long)row * p.ldc + col;
        if (p.c_mode == ENCDIFF_OUT_BF16) {
          bf16_t* c = (bf16_t*)p.c + co;
          if (((uintptr_t)c & 7) == 0) {  // one 8-byte store
            *(uint2*)c = make_uint2(pack2(v[0], v[1]), pack2(v[2], v[3]));
          } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) c[k] = f2bf(v[k]);
          }
        } else {
          float* c = (float*)p.c + co;
#pragma unroll
          for (int k = 0; k < 4; ++k) c[k] = p.c_mode == ENCDIFF_OUT_F32_ACCUM ? c[k] + v[k] : v[k];
        }
      }
      if (zgn > 1) __syncthreads();
    }
  } else {
    float* pz = (float*)part;
    for (long t0 = (long)bid * per; t0 < total; t0 += (long)nblk * per) {
      const long i = t0 + o;
      float acc = 0.f;
      if (i < total) {
        const float* w = p.workspace + i;
#pragma unroll 8
        for (int z = zg; z < p.split_k; z += zgn) acc += w[(long)z * total];
      }
      if (zgn > 1) {
        pz[zg * 64 + o] = acc;
        __syncthreads();
        if (zg == 0) acc = ((pz[o] + pz[64 + o]) + pz[128 + o]) + pz[192 + o];
      }
      if (zg == 0 && i < total) fin_store(p, R, i, acc);
      if (zgn > 1) __syncthreads();
    }
  }
  if (p.bias_grad) {  // bias-gradient slabs [split][M] behind the C slabs: 4 z-groups, fixed order
    float* pz = (float*)part;
    const int bo = threadIdx.x & 63, bz = threadIdx.x >> 6;
    const float* bs = p.workspace + (long)p.split_k * total;
    for (long t0 = (long)bid * 64; t0 < p.M; t0 += (long)nblk * 64) {
      const long m = t0 + bo;
      float acc = 0.f;
      if (m < p.M) {
#pragma unroll 8
        for (int z = bz; z < p.split_k; z += 4) acc += bs[(long)z * p.M + m];
      }
      __syncthreads();  // part may still be read by the C loop above
      pz[bz * 64 + bo] = acc;
      __syncthreads();
      if (bz == 0 && m < p.M) p.bias_grad[m] += ((pz[bo] + pz[64 + bo]) + pz[128 + bo]) + pz[192 + bo];
    }
  }
}

__global__ __launch_bounds__(256) void gemm_finalize_kernel(const EncdiffGemmArgs p) {
  gemm_finalize(p, blockIdx.x, gridDim.x);
}

// finalize of two split-K GEMMs in one launch (blocks [0, g1) for p1, the rest for p2)
__global__ __launch_bounds__(256) void gemm_finalize2_kernel(const EncdiffGemmArgs p1, const EncdiffGemmArgs p2,
                                                             int g1) {
  if ((int)blockIdx.x < g1) gemm_finalize(p1, blockIdx.x, g1);
  else gemm_finalize(p2, blockIdx.x - g1, gridDim.x - g1);
}
}  // namespace
