// Nearest-codebook-entry search shared by the VQ decode head (vq.hip) and the quantised-x0
// sampling steps (sampler.hip).
//
// The distance is evaluated directly, sum_c (z_c - E_jc)^2 in fp32 (not the expanded
// |z|^2 + |e|^2 - 2 z.e form: its cancellation costs digits exactly where two codes are close).
// The codebook is staged in LDS channel-major ([c][code]) in chunks of VQ_LDS_FLOATS: with one
// lane per row all lanes read one address (a broadcast), with `split` lanes per row the lanes of a
// row read consecutive dwords (no bank conflict).  A row's lanes scan codes sub, sub + split, ...
// in ascending order with a strict <, and are reduced by (distance, index) order, so ties go to
// the lowest index.  A row with no finite distance (NaN input) takes entry 0.
#pragma once
#include "common.h"

constexpr int VQ_T = 256;
constexpr int VQ_LDS_FLOATS = 8192;  // 32 KB: the 2048 x 3 codebook in one chunk
constexpr int VQ_MAX_DIM = 8;
constexpr int VQ_MAX_CODES = 8192;

// Every thread of the VQ_T-thread block calls this (it holds barriers); cb: VQ_LDS_FLOATS floats
// of LDS; split (a power of two <= 64) lanes share a row, sub = threadIdx.x % split; chunk =
// VQ_LDS_FLOATS / ED.  All lanes of a row return the same index.
template <int ED>
ED_DEV int vq_search(const float (&z)[ED], float* cb, const float* __restrict__ codebook, const int n_e,
                     const int split, const int sub, const int chunk) {
  float bd = __builtin_inff();
  int bj = 0x7fffffff;
  for (int j0 = 0; j0 < n_e; j0 += chunk) {
    const int n = min(chunk, n_e - j0);
    if (j0) __syncthreads();  // the previous chunk is consumed
    for (int i = threadIdx.x; i < n * ED; i += VQ_T) {
      const int j = i / ED, c = i - j * ED;
      cb[c * chunk + j] = codebook[(long)j0 * ED + i];
    }
    __syncthreads();
    for (int j = sub; j < n; j += split) {
      float d = 0.f;
#pragma unroll
      for (int c = 0; c < ED; ++c) {
        const float t = z[c] - cb[c * chunk + j];
        d += t * t;
      }
      if (d < bd) { bd = d; bj = j0 + j; }
    }
  }
  for (int o = split >> 1; o > 0; o >>= 1) {
    const float od = __shfl_xor(bd, o, 64);
    const int oj = __shfl_xor(bj, o, 64);
    if (od < bd || (od == bd && oj < bj)) { bd = od; bj = oj; }
  }
  return (bj >= 0 && bj < n_e) ? bj : 0;  // no finite distance (NaN input): entry 0
}

// lanes per row: a workgroup per CU at small batches (B = 4 at 16 x 16 is 1024 rows: 64 lanes
// per row, 256 workgroups), never more lanes than a wave or than codes
static inline int vq_split(long total, int n_e) {
  int split = 1;
  while (split < 64 && 2 * split <= n_e && total * split < 256L * VQ_T) split *= 2;
  return split;
}
