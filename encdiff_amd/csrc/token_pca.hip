// The per-unit PCA(n_components=1) that eval_func (main_val.py:38-96) applies to a 3-D token array
// tokens fp32 [N][U][d], U <= 64 units of d <= 64 numbers: the moments and the projection.  The d x d
// eigenproblem of every unit is host work between the two (encdiff_amd/metrics.py token_pca).
//
// Moments: one streaming pass, shifted by row 0 so that the sums of squares do not cancel:
//   S1[u][i] = sum_n (x[n][u][i] - x[0][u][i]),  S2[u][i][j] = sum_n (..i..) (..j..)   in fp64,
//   mean = x[0] + S1 / N,  cov = (S2 - S1 S1^T / N) / (N - 1).
// The differences are exact in fp64.  Block (chunk c, unit u) stages up to 2048 numbers of its chunk
// at a time in LDS (128 rows at d = 16; 16-byte non-temporal loads where d is a multiple of 4: the
// table is read once, and the loads of the next two tiles are in flight while one is consumed).
// The d x d sums are cut into 4 x 4 blocks and only the T = nb (nb + 1) / 2 blocks of the upper
// triangle are computed (nb = ceil(d / 4)); thread (g, block) keeps its 16 sums (and, on a diagonal
// block, 4 of S1) in registers and takes the rows r = g, g + G, ... of every tile, G = max(1, 256 /
// T): 8 LDS reads per 16 products.  At the end the G partials of a block are added in the order g =
// 0..G-1, the per-block results go to the workspace and token_fold_kernel adds them in chunk order,
// reading the lower triangle from its mirror.  No floating-point atomics: a second launch gives the
// same bits.
//
// Projection: out[n][u] = sum_i (x[n][u][i] - mean[u][i]) v[u][i] in fp64, rounded to fp32.  A group
// of L = pow2 >= d / 4 lanes takes one (n, u): each lane loads 4 consecutive numbers (the wave reads
// contiguous memory), adds its products in ascending order, and the L partials are folded by a xor
// shuffle tree.
#include "common.h"

namespace {

constexpr int TP_MAX = ENCDIFF_TOKEN_MAX;  // 64 units, 64 numbers per unit
constexpr int TP_TILE = 2048;               // numbers staged per pass (16 KB as doubles)
constexpr int TP_T = 256;
typedef float f4 __attribute__((ext_vector_type(4)));

// chunk length of the moments pass: about 2560 blocks over the units (two rounds of the 1280 blocks
// the chip holds at five per CU), at least 64 rows each
inline long chunk_rows(long n, int units) {
  const long target = (2560 + units - 1) / units;
  const long len = (n + target - 1) / target;
  return len < 64 ? 64 : len;
}

__global__ __launch_bounds__(TP_T) void token_moments_kernel(const float* __restrict__ tok, const long n,
                                                             const int U, const int d, const long len,
                                                             double* __restrict__ part) {
  __shared__ double tile[TP_TILE];
  __shared__ double x0[TP_MAX];
  const int t = threadIdx.x, u = blockIdx.y, dd = d * d;
  const int nb = (d + 3) >> 2, dp = nb * 4, T = nb * (nb + 1) / 2, G = T >= TP_T ? 1 : TP_T / T;
  const int tile_rows = TP_TILE / dp;
  const long c = blockIdx.x, r_lo = c * len, r_hi = r_lo + len < n ? r_lo + len : n;
  const bool vec = (d & 3) == 0;
  if (t < TP_MAX) x0[t] = t < d ? (double)tok[(long)u * d + t] : 0.0;
  for (int i = t; i < TP_TILE; i += TP_T) tile[i] = 0.0;  // the padding columns d..dp-1 stay zero
  // this thread's block (bi <= bj) of the upper triangle and its row group
  const int g = t / T, blk = t - g * T;
  const bool worker = g < G;
  int bi = 0, rem = blk;
  while (rem >= nb - bi) rem -= nb - bi, ++bi;
  const int bj = bi + rem;
  double acc[16], s1[4];
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) s1[q] = 0.0;
  // vector path: a tile is at most 512 16-byte loads, two per thread, held in registers
  const int d4 = d >> 2;
  f4 pre[2], pre2[2];
  auto prefetch = [&](f4* dst, const long r0, const int rows) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int i = t + k * TP_T;
      if (i < rows * d4) {
        const int r = i / d4, c4 = (i - r * d4) * 4;
        dst[k] = __builtin_nontemporal_load((const f4*)(tok + ((r0 + r) * U + u) * d + c4));
      }
    }
  };
  auto tile_len = [&](const long r0) { return r0 >= r_hi ? 0 : (r_hi - r0 < tile_rows ? (int)(r_hi - r0) : tile_rows); };
  // two tiles are in flight while one is consumed: pre holds the next tile, pre2 the one after it
  long r0 = r_lo;
  int rows = tile_len(r0), rows1 = tile_len(r0 + rows);
  if (vec) {
    prefetch(pre, r0, rows);
    if (rows1) prefetch(pre2, r0 + rows, rows1);
  }
  while (r0 < r_hi) {
    __syncthreads();  // x0 and the zeros are written; the previous tile is consumed
    if (vec) {
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int i = t + k * TP_T;
        if (i < rows * d4) {
          const int r = i / d4, c4 = (i - r * d4) * 4;
          double* dst = tile + r * dp + c4;
          dst[0] = (double)pre[k].x - x0[c4], dst[1] = (double)pre[k].y - x0[c4 + 1];
          dst[2] = (double)pre[k].z - x0[c4 + 2], dst[3] = (double)pre[k].w - x0[c4 + 3];
        }
      }
    } else {
      for (int i = t; i < rows * d; i += TP_T) {
        const int r = i / d, col = i - r * d;
        tile[r * dp + col] = (double)__builtin_nontemporal_load(tok + ((r0 + r) * U + u) * d + col) - x0[col];
      }
    }
    __syncthreads();
    const long r_next = r0 + rows, r_next2 = r_next + rows1;
    const int rows2 = tile_len(r_next2);
    if (vec) {
      pre[0] = pre2[0], pre[1] = pre2[1];
      if (rows2) prefetch(pre2, r_next2, rows2);
    }
    if (worker) {
      for (int r = g; r < rows; r += G) {
        const double* row = tile + r * dp;
        double ai[4], aj[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) ai[q] = row[bi * 4 + q], aj[q] = row[bj * 4 + q];
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
          for (int y = 0; y < 4; ++y) acc[x * 4 + y] += ai[x] * aj[y];
        if (bi == bj) {
#pragma unroll
          for (int q = 0; q < 4; ++q) s1[q] += ai[q];
        }
      }
    }
    r0 = r_next, rows = rows1, rows1 = rows2;
  }
  // the G partials of every sum, added in the order g = 0..G-1 by the block's g == 0 thread; the
  // tile holds 8 sums of every thread at a time: acc[0..7], acc[8..15], then s1
  double* out = part + (c * U + u) * (long)(dd + d);
#pragma unroll
  for (int pass = 0; pass < 3; ++pass) {
    __syncthreads();
    if (worker) {
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (pass < 2) tile[k * TP_T + t] = acc[pass * 8 + k];
        else if (k < 4) tile[k * TP_T + t] = s1[k];
    }
    __syncthreads();
    if (worker && g == 0 && (pass < 2 || bi == bj)) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (pass == 2 && k >= 4) break;
        double sum = 0.0;
        for (int h = 0; h < G; ++h) sum += tile[k * TP_T + h * T + blk];
        if (pass < 2) {
          const int q = pass * 8 + k, i = bi * 4 + (q >> 2), j = bj * 4 + (q & 3);
          if (i < d && j < d) out[i * d + j] = sum;
        } else {
          const int i = bi * 4 + k;
          if (i < d) out[dd + i] = sum;
        }
      }
    }
  }
}

// thread (u, e): the partials of S2[u][e] (of its mirror where e lies in a block below the diagonal)
// and of the two S1 entries it needs, added in chunk order
__global__ __launch_bounds__(TP_T) void token_fold_kernel(const float* __restrict__ tok, const double* __restrict__ part,
                                                          const long n, const int U, const int d, const int chunks,
                                                          double* __restrict__ mean, double* __restrict__ cov) {
  const int dd = d * d, u = blockIdx.y, e = blockIdx.x * TP_T + threadIdx.x;
  if (e >= dd) return;
  const int i = e / d, j = e - i * d;
  const int src = (i >> 2) > (j >> 2) ? j * d + i : e;
  double s2 = 0.0, si = 0.0, sj = 0.0;
  for (int c = 0; c < chunks; ++c) {
    const double* p = part + ((long)c * U + u) * (long)(dd + d);
    s2 += p[src], si += p[dd + i], sj += p[dd + j];
  }
  const double nn = (double)n;
  cov[(long)u * dd + e] = (s2 - si * sj / nn) / (nn - 1.0);
  if (i == 0) mean[u * d + j] = (double)tok[(long)u * d + j] + sj / nn;
}

__global__ __launch_bounds__(TP_T) void token_project_kernel(const float* __restrict__ tok, const long outputs,
                                                             const int U, const int d, const int lanes,
                                                             const double* __restrict__ mean,
                                                             const double* __restrict__ comp, float* __restrict__ out) {
  const int t = threadIdx.x, l = t & (lanes - 1), per_block = TP_T / lanes;
  const long o = (long)blockIdx.x * per_block + t / lanes;
  const bool live = o < outputs;
  const int c0 = l * 4;
  double acc = 0.0;
  if (live && c0 < d) {
    const int u = (int)(o % U);
    const float* x = tok + o * d + c0;
    const double* m = mean + u * d + c0;
    const double* v = comp + u * d + c0;
    if ((d & 3) == 0) {
      const f4 q = __builtin_nontemporal_load((const f4*)x);
      acc += ((double)q.x - m[0]) * v[0];
      acc += ((double)q.y - m[1]) * v[1];
      acc += ((double)q.z - m[2]) * v[2];
      acc += ((double)q.w - m[3]) * v[3];
    } else {
      for (int i = 0; i < 4 && c0 + i < d; ++i) acc += ((double)__builtin_nontemporal_load(x + i) - m[i]) * v[i];
    }
  }
  for (int s = lanes >> 1; s > 0; s >>= 1) acc += __shfl_xor(acc, s, 64);
  if (live && l == 0) out[o] = (float)acc;
}

bool token_shape_ok(long long n, int units, int dim) {
  return n >= 2 && n < (1LL << 31) && units >= 1 && units <= TP_MAX && dim >= 1 && dim <= TP_MAX;
}

}  // namespace

extern "C" int encdiff_token_workspace(long long n, int units, int dim, long long* bytes) {
  if (!bytes) return ENCDIFF_ERR_ARG;
  if (!token_shape_ok(n, units, dim)) return ENCDIFF_ERR_SHAPE;
  const long len = chunk_rows(n, units), chunks = (n + len - 1) / len;
  *bytes = 8LL * chunks * units * (dim * dim + dim);
  return ENCDIFF_OK;
}

extern "C" int encdiff_token_moments(const float* tokens, long long n, int units, int dim, void* workspace,
                                     double* mean, double* cov, void* stream) {
  if (!tokens || !workspace || !mean || !cov) return ENCDIFF_ERR_ARG;
  if (((unsigned long long)workspace & 7) != 0 || ((unsigned long long)tokens & 15) != 0) return ENCDIFF_ERR_ARG;
  if (!token_shape_ok(n, units, dim)) return ENCDIFF_ERR_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  const long len = chunk_rows(n, units), chunks = (n + len - 1) / len;
  const int dd = dim * dim;
  const dim3 grid((unsigned)chunks, (unsigned)units);
  double* part = (double*)workspace;
  hipLaunchKernelGGL(token_moments_kernel, grid, dim3(TP_T), 0, s, tokens, (long)n, units, dim, len, part);
  ED_CHECK_LAUNCH();
  hipLaunchKernelGGL(token_fold_kernel, dim3((dd + TP_T - 1) / TP_T, units), dim3(TP_T), 0, s, tokens, part, (long)n,
                     units, dim, (int)chunks, mean, cov);
  ED_CHECK_LAUNCH();
  return ENCDIFF_OK;
}

extern "C" int encdiff_token_project(const float* tokens, long long n, int units, int dim, const double* mean,
                                     const double* components, float* out, void* stream) {
  if (!tokens || !mean || !components || !out) return ENCDIFF_ERR_ARG;
  if (((unsigned long long)tokens & 15) != 0) return ENCDIFF_ERR_ARG;
  if (n < 1 || n >= (1LL << 31) || units < 1 || units > TP_MAX || dim < 1 || dim > TP_MAX) return ENCDIFF_ERR_SHAPE;
  int lanes = 1;
  while (lanes * 4 < dim) lanes <<= 1;
  const long outputs = (long)n * units, per_block = TP_T / lanes;
  const long blocks = (outputs + per_block - 1) / per_block;
  if (blocks >= (1L << 31)) return ENCDIFF_ERR_SHAPE;
  hipLaunchKernelGGL(token_project_kernel, dim3((unsigned)blocks), dim3(TP_T), 0, (hipStream_t)stream, tokens, outputs,
                     units, dim, lanes, mean, components, out);
  ED_CHECK_LAUNCH();
  return ENCDIFF_OK;
}
