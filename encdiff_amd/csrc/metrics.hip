// Disentanglement metrics over a device-resident code table codes fp32 [n_rows][dims], dims <= 64:
// the array work of the FactorVAE score (evaluation/metrics/factor_vae.py) and of the mutual
// information gap (mig.py, utils.py's histogram discretiser and discrete mutual information).  The
// "representation function" of the reference is a row lookup and its observations are row indices,
// so every kernel gathers rows through an int32 index table that the host sampled
// (encdiff_amd/metrics.py).
//
// Everything floating-point that is summed is summed in fp64 in a fixed order (per-thread strided
// partials, then a fixed LDS reduction): no floating-point atomics, so a launch repeats bitwise.
// Integer atomics (votes, joint counts) commute exactly.  No kernel reads back to the host or
// allocates: the ops are graph-capturable.  Row indices are clamped to [0, n_rows) and factor values
// outside [0, V_k) are not counted, so a bad table cannot address outside the buffers.
#include "common.h"

namespace {

constexpr int MT_MAXD = ENCDIFF_METRICS_MAX_DIMS;        // 64: one lane per dimension
constexpr int MT_BINS = ENCDIFF_METRICS_BINS;            // 20, utils.py's discretizer.num_bins
constexpr int MT_MAXV = ENCDIFF_METRICS_MAX_VALUES;      // 256 values of one factor
constexpr int MT_MAXK = ENCDIFF_METRICS_MAX_FACTORS;     // 16
constexpr int MT_CHUNK = 1024;                           // gathered rows per histogram block

struct Sizes {
  int v[MT_MAXK];
};

ED_DEV long row_of(const int* idx, long i, int n_rows) {
  const int r = idx[i];
  return r < 0 ? 0 : (r >= n_rows ? n_rows - 1 : r);
}

// next power of two >= d (d in 1..64)
inline int pow2_dims(int d) {
  int p = 1;
  while (p < d) p <<= 1;
  return p;
}

// Zeroes the integer outputs that the atomics then add into.  A kernel of our own, not a memset node:
// every op here may be captured into a graph, and the replayed ops must start from zeros.
__global__ __launch_bounds__(256) void zero_i32_kernel(int* __restrict__ p, const long n) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) p[i] = 0;
}

void zero_i32(int* p, long n, hipStream_t s) {
  const long blocks = (n + 255) / 256;
  hipLaunchKernelGGL(zero_i32_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, s, p, n);
}

// ------------------------------------------------------------------ column variances
// One block of 1024 threads, thread = (row lane rl, dimension d) with dp = pow2 >= dims columns:
// each thread sums the rows rl, rl + R, ... of its column, the R partials of a column are added in
// the order rl = 0 .. R-1 by one thread.  Two passes: mean, then sum of squared deviations.
__global__ __launch_bounds__(1024) void colvar_kernel(const float* __restrict__ codes, const int n_rows,
                                                      const int dims, const int dp, const int* __restrict__ idx,
                                                      const int n, double* __restrict__ out) {
  __shared__ double part[1024];
  __shared__ double mean_s[MT_MAXD];
  const int t = threadIdx.x, d = t & (dp - 1), rl = t / dp, R = 1024 / dp;
  double acc = 0.0;
  if (d < dims)
    for (int i = rl; i < n; i += R) acc += (double)codes[row_of(idx, i, n_rows) * dims + d];
  part[t] = acc;
  __syncthreads();
  if (t < dims) {
    double s = 0.0;
    for (int r = 0; r < R; ++r) s += part[r * dp + t];
    mean_s[t] = s / (double)n;
  }
  __syncthreads();
  acc = 0.0;
  if (d < dims) {
    const double m = mean_s[d];
    for (int i = rl; i < n; i += R) {
      const double x = (double)codes[row_of(idx, i, n_rows) * dims + d] - m;
      acc += x * x;
    }
  }
  part[t] = acc;
  __syncthreads();
  if (t < dims) {
    double s = 0.0;
    for (int r = 0; r < R; ++r) s += part[r * dp + t];
    out[t] = s / (double)(n - 1);
  }
}

// ------------------------------------------------------------------ FactorVAE votes
// A wave holds G = 64 / dp points, lane = (point g, dimension d): the lane reads its column of the
// point's `batch` gathered rows into registers (the dp lanes of a row read consecutive floats), and
// forms mean and variance alone, rows in index order -- no cross-lane sum.  Lane d == 0 of a point
// then walks the dims ratios in LDS for the argmin over the active dimensions.
__global__ __launch_bounds__(256) void fvae_kernel(const float* __restrict__ codes, const int n_rows, const int dims,
                                                   const int dp, const int* __restrict__ vote_idx,
                                                   const int* __restrict__ vote_factor, const int points,
                                                   const int batch, const int num_factors,
                                                   const double* __restrict__ gvar, const double thr,
                                                   int* __restrict__ votes, int* __restrict__ argmin_out,
                                                   double* __restrict__ ratio_out) {
  __shared__ double rs[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int G = 64 / dp, g = lane / dp, d = lane & (dp - 1);
  const long p = ((long)blockIdx.x * 4 + w) * G + g;
  const bool live = p < points && d < dims;
  const int* ip = vote_idx + (live ? p * batch : 0);
  float v[64];
#pragma unroll
  for (int r = 0; r < 64; ++r) {
    v[r] = 0.f;
    if (live && r < batch) v[r] = codes[row_of(ip, r, n_rows) * dims + d];
  }
  double s = 0.0;
#pragma unroll
  for (int r = 0; r < 64; ++r) s += (double)v[r];  // rows >= batch hold 0: exact
  const double mean = s / (double)batch;
  double ss = 0.0;
#pragma unroll
  for (int r = 0; r < 64; ++r)
    if (r < batch) {
      const double x = (double)v[r] - mean;
      ss += x * x;
    }
  const double var = ss / (double)(batch - 1);
  const double gv = live ? gvar[d] : 0.0;
  const bool active = live && sqrt(gv) >= thr;
  const double ratio = active ? var / gv : (double)INFINITY;
  if (live && ratio_out) ratio_out[p * dims + d] = ratio;
  rs[w][lane] = ratio;
  __syncthreads();
  if (d == 0 && p < points) {
    // np.argmin over the compacted active list: lowest index on a tie, the first NaN wins
    int best = -1, c = 0;
    double bv = 0.0;
    for (int j = 0; j < dims; ++j) {
      if (!(sqrt(gvar[j]) >= thr)) continue;
      const double r = rs[w][g * dp + j];
      if (best < 0 || r < bv || (r != r && bv == bv)) {
        best = c;
        bv = r;
      }
      ++c;
    }
    if (argmin_out) argmin_out[p] = best;
    const int f = vote_factor[p];
    if (best >= 0 && f >= 0 && f < num_factors) atomicAdd(&votes[f * dims + best], 1);
  }
}

// ------------------------------------------------------------------ MIG: edges, bins, joint counts
// Keeps the product opaque, so that -ffp-contract=fast cannot fuse it into the add that follows:
// numpy rounds the two separately.
ED_DEV float opaque(float x) {
  asm volatile("" : "+v"(x));
  return x;
}
ED_DEV double opaque(double x) {
  asm volatile("" : "+v"(x));
  return x;
}

// The first MT_BINS of np.histogram(x, 20)'s 21 edges for float32 x, i.e. np.linspace(first, last,
// 21, dtype=float32)[:-1] with (first, last) = (min, max), widened by 0.5 each way when equal.
//   edge_f64 == 0: NumPy >= 2 (NEP 50) evaluates linspace in float32 throughout;
//   edge_f64 != 0: NumPy 1.x evaluates it in float64 and rounds each edge to float32 at the end.
// Either way step = delta / 20, edge_i = i * step + first, product and sum rounded separately
// (i / 20 * delta when step underflows to 0, linspace's own special case).
ED_DEV float hist_edge(const float lo, const float hi, const int i, const int edge_f64) {
  if (edge_f64) {
    double first = lo, last = hi;
    if (first == last) {
      first -= 0.5;
      last += 0.5;
    }
    const double delta = last - first, step = delta / 20.0;
    const double y = step == 0.0 ? opaque(opaque((double)i / 20.0) * delta) : opaque((double)i * step);
    return (float)(y + first);
  }
  float first = lo, last = hi;
  if (first == last) {
    first = lo - 0.5f;
    last = hi + 0.5f;
  }
  const float delta = last - first;
  // fp32 quotient through fp64: 53 >= 2 * 24 + 2 bits, so the second rounding changes nothing
  const float step = (float)((double)delta / 20.0);
  const float y = step == 0.f ? opaque(opaque((float)((double)i / 20.0)) * delta) : opaque((float)i * step);
  return y + first;
}

// grid = dims blocks: min and max of one gathered column (exact, any order), then its edges
__global__ __launch_bounds__(256) void mig_edges_kernel(const float* __restrict__ codes, const int n_rows,
                                                        const int dims, const int* __restrict__ idx, const int m,
                                                        const int edge_f64, float* __restrict__ edges) {
  __shared__ float smin[256], smax[256];
  const int t = threadIdx.x, d = blockIdx.x;
  float lo = INFINITY, hi = -INFINITY;
  for (int i = t; i < m; i += 256) {
    const float x = codes[row_of(idx, i, n_rows) * dims + d];
    lo = fminf(lo, x);
    hi = fmaxf(hi, x);
  }
  smin[t] = lo;
  smax[t] = hi;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
      smin[t] = fminf(smin[t], smin[t + o]);
      smax[t] = fmaxf(smax[t], smax[t + o]);
    }
    __syncthreads();
  }
  if (t < MT_BINS) edges[d * MT_BINS + t] = hist_edge(smin[0], smax[0], t, edge_f64);
}

// grid = (row chunks, factors, dims): np.digitize of the block's rows of column d against the 20
// edges (bin = #{edges <= x}), joint counts against factor k in LDS, one flush per block.
__global__ __launch_bounds__(256) void mig_hist_kernel(const float* __restrict__ codes, const int n_rows,
                                                       const int dims, const int* __restrict__ idx, const int m,
                                                       const int* __restrict__ factors, const int num_factors,
                                                       const Sizes sz, const int vmax,
                                                       const float* __restrict__ edges, int* __restrict__ bins_out,
                                                       int* __restrict__ counts) {
  __shared__ int h[MT_BINS * MT_MAXV];
  __shared__ float e[MT_BINS];
  const int t = threadIdx.x, k = blockIdx.y, d = blockIdx.z, V = sz.v[k];
  for (int i = t; i < MT_BINS * V; i += 256) h[i] = 0;
  if (t < MT_BINS) e[t] = edges[d * MT_BINS + t];
  __syncthreads();
  const int i0 = blockIdx.x * MT_CHUNK, i1 = min(m, i0 + MT_CHUNK);
  for (int i = i0 + t; i < i1; i += 256) {
    const float x = codes[row_of(idx, i, n_rows) * dims + d];
    int b = 0;
#pragma unroll
    for (int j = 0; j < MT_BINS; ++j) b += e[j] <= x ? 1 : 0;
    if (k == 0 && bins_out) bins_out[(long)d * m + i] = b;
    const int f = factors[(long)k * m + i];
    if (b >= 1 && f >= 0 && f < V) atomicAdd(&h[(b - 1) * V + f], 1);
  }
  __syncthreads();
  int* c = counts + ((long)d * num_factors + k) * MT_BINS * vmax;
  for (int i = t; i < MT_BINS * V; i += 256)
    if (h[i]) atomicAdd(&c[(i / V) * vmax + i % V], h[i]);
}

// ------------------------------------------------------------------ MIG: mutual information, score
// fixed-order block sum of one fp64 partial per thread (256 threads)
ED_DEV double block_sum(double* red, const double v) {
  const int t = threadIdx.x;
  __syncthreads();
  red[t] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  return red[0];
}

// grid = (factors, dims): sklearn's mutual_info_score of (bin of column d, factor k) from the
// integer counts; the d == 0 blocks also give H[k] = MI(y_k, y_k) = the entropy of factor k.
__global__ __launch_bounds__(256) void mig_mi_kernel(const int* __restrict__ counts, const int num_factors,
                                                     const Sizes sz, const int vmax, const int m,
                                                     double* __restrict__ mi, double* __restrict__ hk) {
  __shared__ int a[MT_BINS], b[MT_MAXV];
  __shared__ double red[256];
  const int t = threadIdx.x, k = blockIdx.x, d = blockIdx.y, V = sz.v[k];
  const int* c = counts + ((long)d * num_factors + k) * MT_BINS * vmax;
  if (t < V) {
    int s = 0;
    for (int j = 0; j < MT_BINS; ++j) s += c[j * vmax + t];
    b[t] = s;
  }
  if (t < MT_BINS) {
    int s = 0;
    for (int v = 0; v < V; ++v) s += c[t * vmax + v];
    a[t] = s;
  }
  __syncthreads();
  const double M = (double)m;
  double acc = 0.0;
  for (int i = t; i < MT_BINS * V; i += 256) {
    const int j = i / V, v = i % V, n = c[j * vmax + v];
    if (n) acc += (double)n / M * log(M * (double)n / ((double)a[j] * (double)b[v]));
  }
  const double tot = block_sum(red, acc);
  if (t == 0) mi[d * num_factors + k] = fmax(tot, 0.0);
  if (d == 0) {
    double e = 0.0;
    if (t < V && b[t]) e = (double)b[t] / M * log(M / (double)b[t]);
    const double h = block_sum(red, e);
    if (t == 0) hk[k] = fmax(h, 0.0);
  }
}

// one block: per factor the gap between the two largest MI[:, k], over H[k]; the mean over factors
__global__ __launch_bounds__(64) void mig_score_kernel(const double* __restrict__ mi, const double* __restrict__ hk,
                                                       const int dims, const int num_factors,
                                                       double* __restrict__ score) {
  __shared__ double gap[MT_MAXK];
  const int k = threadIdx.x;
  if (k < num_factors) {
    double t1 = -INFINITY, t2 = -INFINITY;
    for (int d = 0; d < dims; ++d) {
      const double x = mi[d * num_factors + k];
      if (x > t1) {
        t2 = t1;
        t1 = x;
      } else if (x > t2) {
        t2 = x;
      }
    }
    gap[k] = (t1 - t2) / hk[k];
  }
  __syncthreads();
  if (k == 0) {
    double s = 0.0;
    for (int j = 0; j < num_factors; ++j) s += gap[j];
    *score = s / (double)num_factors;
  }
}

// factor_sizes (host) -> Sizes; the largest size in vmax.  False if a size is outside 1..256.
bool load_sizes(const int* factor_sizes, int num_factors, Sizes& sz, int& vmax) {
  vmax = 0;
  for (int k = 0; k < MT_MAXK; ++k) sz.v[k] = 0;
  for (int k = 0; k < num_factors; ++k) {
    if (factor_sizes[k] < 1 || factor_sizes[k] > MT_MAXV) return false;
    sz.v[k] = factor_sizes[k];
    vmax = factor_sizes[k] > vmax ? factor_sizes[k] : vmax;
  }
  return true;
}

}  // namespace

extern "C" int encdiff_gather_colvar(const float* codes, int n_rows, int dims, const int* idx, int n, double* var_out,
                                     void* stream) {
  if (!codes || !idx || !var_out) return ENCDIFF_ERR_ARG;
  if (n_rows <= 0 || dims < 1 || dims > MT_MAXD || n < 2) return ENCDIFF_ERR_SHAPE;
  hipLaunchKernelGGL(colvar_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, codes, n_rows, dims,
                     pow2_dims(dims), idx, n, var_out);
  ED_CHECK_LAUNCH();
  return ENCDIFF_OK;
}

extern "C" int encdiff_fvae_votes(const float* codes, int n_rows, int dims, const int* vote_idx,
                                  const int* vote_factor, int points, int batch, int num_factors,
                                  const double* global_var, double threshold, int* votes, int* argmin_out,
                                  double* ratio_out, void* stream) {
  if (!codes || !vote_idx || !vote_factor || !global_var || !votes) return ENCDIFF_ERR_ARG;
  if (n_rows <= 0 || dims < 1 || dims > MT_MAXD || points < 1 || batch < 2 || batch > 64 || num_factors < 1)
    return ENCDIFF_ERR_SHAPE;
  if ((long)points * batch >= (1L << 31) || (long)points * dims >= (1L << 31)) return ENCDIFF_ERR_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  zero_i32(votes, (long)num_factors * dims, s);
  ED_CHECK_LAUNCH();
  const int dp = pow2_dims(dims), per_block = 4 * (64 / dp);
  hipLaunchKernelGGL(fvae_kernel, dim3((points + per_block - 1) / per_block), dim3(256), 0, s, codes, n_rows, dims, dp,
                     vote_idx, vote_factor, points, batch, num_factors, global_var, threshold, votes, argmin_out,
                     ratio_out);
  ED_CHECK_LAUNCH();
  return ENCDIFF_OK;
}

extern "C" int encdiff_mig_hist(const float* codes, int n_rows, int dims, const int* mig_idx, int m,
                                const int* mig_factors, int num_factors, const int* factor_sizes, int edge_f64,
                                float* edges, int* bins_out, int* counts, void* stream) {
  if (!codes || !mig_idx || !mig_factors || !factor_sizes || !edges || !counts) return ENCDIFF_ERR_ARG;
  if (n_rows <= 0 || dims < 1 || dims > MT_MAXD || m < 1 || num_factors < 1 || num_factors > MT_MAXK)
    return ENCDIFF_ERR_SHAPE;
  if ((long)dims * m >= (1L << 31) || (long)num_factors * m >= (1L << 31)) return ENCDIFF_ERR_SHAPE;
  Sizes sz;
  int vmax;
  if (!load_sizes(factor_sizes, num_factors, sz, vmax)) return ENCDIFF_ERR_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  zero_i32(counts, (long)dims * num_factors * MT_BINS * vmax, s);
  ED_CHECK_LAUNCH();
  hipLaunchKernelGGL(mig_edges_kernel, dim3(dims), dim3(256), 0, s, codes, n_rows, dims, mig_idx, m, edge_f64, edges);
  ED_CHECK_LAUNCH();
  hipLaunchKernelGGL(mig_hist_kernel, dim3((m + MT_CHUNK - 1) / MT_CHUNK, num_factors, dims), dim3(256), 0, s, codes,
                     n_rows, dims, mig_idx, m, mig_factors, num_factors, sz, vmax, edges, bins_out, counts);
  ED_CHECK_LAUNCH();
  return ENCDIFF_OK;
}

extern "C" int encdiff_mig_finalize(const int* counts, int dims, int num_factors, const int* factor_sizes, int m,
                                    double* mi, double* h, double* score, void* stream) {
  if (!counts || !factor_sizes || !mi || !h || !score) return ENCDIFF_ERR_ARG;
  if (dims < 2 || dims > MT_MAXD || m < 1 || num_factors < 1 || num_factors > MT_MAXK) return ENCDIFF_ERR_SHAPE;
  Sizes sz;
  int vmax;
  if (!load_sizes(factor_sizes, num_factors, sz, vmax)) return ENCDIFF_ERR_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(mig_mi_kernel, dim3(num_factors, dims), dim3(256), 0, s, counts, num_factors, sz, vmax, m, mi, h);
  ED_CHECK_LAUNCH();
  hipLaunchKernelGGL(mig_score_kernel, dim3(1), dim3(64), 0, s, mi, h, dims, num_factors, score);
  ED_CHECK_LAUNCH();
  return ENCDIFF_OK;
}
