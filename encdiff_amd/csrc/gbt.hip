// Gradient-boosted depth-3 trees for DCI (evaluation/metrics/dci.py compute_importance_gbt): sklearn's
// GradientBoostingClassifier with its defaults (log loss, friedman_mse, best splitter, max_depth 3,
// subsample 1) fitted to one factor on the device, with the importances, the raw predictions of the
// training and test rows and the accuracy counts as results (encdiff_amd/metrics.py dci_score).
//
// A stage fits T trees at once (T = classes, 1 for two classes), and a tree level is four launches:
//   stats      grid (tree, node of the level): count, integer gradient sum, sums for impurity and leaf
//   scan       grid (tree, feature): best cut of every live node of the level in that feature
//   pick       thread (tree, node): leaf conditions, best feature (hash rule on a tie), threshold
//   partition  thread (tree, row): node <- 2 node + (x > threshold)
// Nodes carry heap ids (root 1, children 2 i and 2 i + 1, depth 3 ends at 8..15).
//
// Exactness.  Trees are grown on Gq = llrint(G * 2^32) as int64: |Gq| <= 2^32, a sum over at most
// 2^14 rows is below 2^46 and n * sum below 2^60, so the prefix sums of a scan are exact whatever
// their order and the proxy is one fp64 expression of (nL, sL, n, s): two features that cut a node
// into the same halves give the same bits, and the tie goes to the higher splitmix64 priority of
// (tie_seed, stage, tree, node, feature).  fp64 sums (squares for the impurity, leaf numerators and
// denominators) are taken in one fixed order -- thread t of 256 adds rows t, t + 256, ..., then a
// fixed LDS fold -- with no floating-point atomics, so a launch repeats bitwise.  This file is built
// with -ffp-contract=off: tests/gbt_restate.py rounds every product and sum on its own.
//
// Nothing is allocated or read back; the workspace size comes from encdiff_gbt_workspace.  Row
// indices (order, the gather's idx) are clamped; labels are only compared, never used as an index.
#include "common.h"

#include <float.h>

namespace {

constexpr int GB_MAXN = ENCDIFF_GBT_MAX_TRAIN;    // 16384 training rows: sums of Gq stay below 2^46
constexpr int GB_MAXD = ENCDIFF_METRICS_MAX_DIMS;  // 64
constexpr int GB_MAXC = ENCDIFF_GBT_MAX_CLASSES;   // 256
constexpr int GB_NODES = ENCDIFF_GBT_NODES;        // 15
constexpr int GB_IDS = 16;                         // tables indexed by heap id 0..15 (0 unused)
constexpr double GB_SCALE = 4294967296.0;          // 2^32

struct Best {
  double proxy;
  float xlo, xhi;
  int has, pad_;
};

struct Work {
  double* g;             // [T][N] onehot - P
  long long* gq;         // [T][N] llrint(g * 2^32)
  unsigned char* node;   // [T][N] heap id of the row in the tree
  int* st_cnt;           // [T][16] rows of the node
  long long* st_sq;      // [T][16] sum of gq
  double* st_ssq;        // [T][16] sum of (gq / 2^32)^2
  double* st_sg;         // [T][16] sum of g
  double* st_sp;         // [T][16] sum of p (1 - p)
  Best* best;            // [T][D][4]
  int* feat;             // [T][16] feature, -1 leaf, -2 no node
  float* thr;            // [T][16]
  double* val;           // [T][16] leaf value
  double* imp_tree;      // [T][D]
  double* imp_acc;       // [D]
  int* used;             // [1] trees with a split
};

inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// Carves the workspace; returns its size in bytes (base may be null: the size only).
size_t carve(char* base, int N, int D, int T, Work& w) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += up256(bytes);
    return p;
  };
  const size_t TN = (size_t)T * N, TI = (size_t)T * GB_IDS;
  w.g = (double*)take(TN * 8);
  w.gq = (long long*)take(TN * 8);
  w.node = (unsigned char*)take(TN);
  w.st_cnt = (int*)take(TI * 4);
  w.st_sq = (long long*)take(TI * 8);
  w.st_ssq = (double*)take(TI * 8);
  w.st_sg = (double*)take(TI * 8);
  w.st_sp = (double*)take(TI * 8);
  w.best = (Best*)take((size_t)T * D * 4 * sizeof(Best));
  w.feat = (int*)take(TI * 4);
  w.thr = (float*)take(TI * 4);
  w.val = (double*)take(TI * 8);
  w.imp_tree = (double*)take((size_t)T * D * 8);
  w.imp_acc = (double*)take((size_t)D * 8);
  w.used = (int*)take(4);
  return off;
}

ED_DEV uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

ED_DEV uint64_t tie_priority(uint64_t seed, int stage, int tree, int node, int feature) {
  uint64_t h = splitmix64(seed);
  h = splitmix64(h ^ (uint64_t)stage);
  h = splitmix64(h ^ (uint64_t)tree);
  h = splitmix64(h ^ (uint64_t)node);
  return splitmix64(h ^ (uint64_t)feature);
}

// mean(g^2) - mean(g)^2 of the quantised gradients of a node
ED_DEV double impurity(const int n, const long long s, const double ssq) {
  const double mean = ((double)s / GB_SCALE) / (double)n;
  return ssq / (double)n - mean * mean;
}

ED_DEV int clampi(const int v, const int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// ------------------------------------------------------------------ prepare
__global__ __launch_bounds__(256) void gather_kernel(const float* __restrict__ codes, const int n_rows, const int dims,
                                                     const int* __restrict__ idx, const long total,
                                                     float* __restrict__ out) {
  const long e = blockIdx.x * 256L + threadIdx.x;
  if (e >= total) return;
  const long i = e / dims;
  const int d = (int)(e - i * dims);
  out[e] = codes[(long)clampi(idx[i], n_rows) * dims + d];
}

__global__ __launch_bounds__(256) void init_kernel(const double* __restrict__ init_raw, const int kc, const long n_train,
                                                   const long n_test, double* __restrict__ raw_train,
                                                   double* __restrict__ raw_test, double* __restrict__ imp_acc,
                                                   const int dims, int* __restrict__ used, int* __restrict__ correct) {
  const long e = blockIdx.x * 256L + threadIdx.x;
  if (e < n_train * kc) raw_train[e] = init_raw[e % kc];
  if (e < n_test * kc) raw_test[e] = init_raw[e % kc];
  if (e < dims) imp_acc[e] = 0.0;
  if (e == 0) {
    *used = 0;
    correct[0] = correct[1] = 0;
  }
}

// ------------------------------------------------------------------ gradients: one row per wave
ED_DEV double wave_max_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
ED_DEV double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void grad_kernel(const double* __restrict__ raw, const int* __restrict__ y,
                                                   const int N, const int C, double* __restrict__ g,
                                                   long long* __restrict__ gq, unsigned char* __restrict__ node) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;  // whole waves leave: the shuffles below stay full
  const int yi = y[i];
  if (C == 2) {
    if (lane == 0) {
      const double p = 1.0 / (1.0 + exp(-raw[i]));
      const double gv = (yi == 1 ? 1.0 : 0.0) - p;
      g[i] = gv;
      gq[i] = llrint(gv * GB_SCALE);
      node[i] = 1;
    }
    return;
  }
  double v[4], m = -INFINITY;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int k = lane + 64 * q;
    v[q] = k < C ? raw[(long)i * C + k] : -INFINITY;
    m = fmax(m, v[q]);
  }
  m = wave_max_f64(m);
  double part = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    v[q] = lane + 64 * q < C ? exp(v[q] - m) : 0.0;
    part += v[q];
  }
  const double sum = wave_sum_f64(part);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int k = lane + 64 * q;
    if (k < C) {
      const double gv = (yi == k ? 1.0 : 0.0) - v[q] / sum;
      const long o = (long)k * N + i;
      g[o] = gv;
      gq[o] = llrint(gv * GB_SCALE);
      node[o] = 1;
    }
  }
}

// ------------------------------------------------------------------ node statistics of one level
// grid (T, nodes of the level): thread t adds the rows t, t + 256, ... that sit in the node, then the
// 256 partials are folded 128, 64, ..., 1 (the order block_sum of tests/gbt_restate.py repeats).
__global__ __launch_bounds__(256) void stats_kernel(const Work w, const int* __restrict__ y, const int N,
                                                    const int C, const int level) {
  __shared__ double r_ssq[256], r_sg[256], r_sp[256];
  __shared__ long long r_sq[256];
  __shared__ int r_cnt[256];
  const int t = blockIdx.x, nd = (1 << level) + blockIdx.y, tid = threadIdx.x;
  const int cls = C == 2 ? 1 : t;
  const long row0 = (long)t * N;
  double ssq = 0.0, sg = 0.0, sp = 0.0;
  long long sq = 0;
  int cnt = 0;
  for (int i = tid; i < N; i += 256) {
    if (w.node[row0 + i] != nd) continue;
    const double gv = w.g[row0 + i];
    const long long q = w.gq[row0 + i];
    const double gd = (double)q / GB_SCALE;
    const double p = (y[i] == cls ? 1.0 : 0.0) - gv;
    ssq += gd * gd;
    sg += gv;
    sp += p * (1.0 - p);
    sq += q;
    ++cnt;
  }
  r_ssq[tid] = ssq, r_sg[tid] = sg, r_sp[tid] = sp, r_sq[tid] = sq, r_cnt[tid] = cnt;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      r_ssq[tid] = r_ssq[tid] + r_ssq[tid + o];
      r_sg[tid] = r_sg[tid] + r_sg[tid + o];
      r_sp[tid] = r_sp[tid] + r_sp[tid + o];
      r_sq[tid] += r_sq[tid + o];
      r_cnt[tid] += r_cnt[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int o = t * GB_IDS + nd;
    w.st_cnt[o] = r_cnt[0], w.st_sq[o] = r_sq[0], w.st_ssq[o] = r_ssq[0], w.st_sg[o] = r_sg[0], w.st_sp[o] = r_sp[0];
  }
}

// ------------------------------------------------------------------ split scan
// grid (T, D), level 0..2 with 1, 2 or 4 live nodes ("slots").  Thread tid owns the positions
// [tid ch, (tid + 1) ch) of the feature's sorted order.  Pass 1: per slot the count, the integer
// gradient sum and the last value of the members in its chunk.  Then one thread per slot turns the
// 256 entries into exclusive prefixes (the last value carried over empty chunks).  Pass 2: the chunk
// again, every member whose value exceeds the previous member's by more than 1e-7 (float32 sum, as
// sklearn's FEATURE_THRESHOLD) is a cut with (nL, sL) = the running prefix; the largest proxy wins,
// the lowest position on a tie (strict >, ascending walk, then ascending threads).
__global__ __launch_bounds__(256) void scan_kernel(const Work w, const float* __restrict__ xs,
                                                   const int* __restrict__ order, const int N, const int D,
                                                   const int level) {
  __shared__ int cnt[4][256], bhas[4][256];
  __shared__ long long sum[4][256];
  __shared__ float last[4][256], blo[4][256], bhi[4][256];
  __shared__ double bp[4][256];
  const int t = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
  const int slots = 1 << level, base = 1 << level;
  const int ch = (N + 255) / 256, j0 = min(N, tid * ch), j1 = min(N, j0 + ch);
  const long row0 = (long)t * N, col0 = (long)f * N;
  for (int s = 0; s < slots; ++s) {
    cnt[s][tid] = 0, sum[s][tid] = 0, last[s][tid] = 0.f;
    bp[s][tid] = -INFINITY, bhas[s][tid] = 0, blo[s][tid] = 0.f, bhi[s][tid] = 0.f;
  }
  for (int j = j0; j < j1; ++j) {
    const int r = clampi(order[col0 + j], N);
    const unsigned s = (unsigned)w.node[row0 + r] - (unsigned)base;
    if (s < (unsigned)slots) {
      cnt[s][tid] += 1;
      sum[s][tid] += w.gq[row0 + r];
      last[s][tid] = xs[col0 + j];
    }
  }
  __syncthreads();
  if (tid < slots) {
    int c = 0;
    long long a = 0;
    float lv = 0.f;
    for (int i = 0; i < 256; ++i) {
      const int ci = cnt[tid][i];
      const long long si = sum[tid][i];
      const float li = last[tid][i];
      cnt[tid][i] = c, sum[tid][i] = a, last[tid][i] = lv;
      c += ci, a += si;
      if (ci) lv = li;
    }
  }
  __syncthreads();
  for (int j = j0; j < j1; ++j) {
    const int r = clampi(order[col0 + j], N);
    const unsigned s = (unsigned)w.node[row0 + r] - (unsigned)base;
    if (s >= (unsigned)slots) continue;
    const float x = xs[col0 + j];
    const int c = cnt[s][tid];
    const long long a = sum[s][tid];
    if (c > 0) {
      const float lo = last[s][tid];
      const float edge = lo + 1e-7f;
      if (x > edge) {
        const int n = w.st_cnt[t * GB_IDS + base + (int)s];
        const long long tot = w.st_sq[t * GB_IDS + base + (int)s];
        const double d = (double)((long long)n * a - (long long)c * tot);
        const double proxy = d * d / ((double)c * (double)(n - c));
        if (proxy > bp[s][tid]) bp[s][tid] = proxy, bhas[s][tid] = 1, blo[s][tid] = lo, bhi[s][tid] = x;
      }
    }
    cnt[s][tid] = c + 1;
    sum[s][tid] = a + w.gq[row0 + r];
    last[s][tid] = x;
  }
  __syncthreads();
  if (tid < slots) {
    Best b;
    b.proxy = -INFINITY, b.xlo = 0.f, b.xhi = 0.f, b.has = 0, b.pad_ = 0;
    for (int i = 0; i < 256; ++i)
      if (bhas[tid][i] && (!b.has || bp[tid][i] > b.proxy))
        b.proxy = bp[tid][i], b.xlo = blo[tid][i], b.xhi = bhi[tid][i], b.has = 1;
    w.best[((long)t * D + f) * 4 + tid] = b;
  }
}

// ------------------------------------------------------------------ pick: one thread per (tree, node)
__global__ __launch_bounds__(64) void pick_kernel(const Work w, const int T, const int D, const int level,
                                                  const int stage, const uint64_t tie_seed) {
  const int slots = 1 << level, e = blockIdx.x * 64 + threadIdx.x;
  if (e >= T * slots) return;
  const int t = e / slots, s = e - t * slots, nd = slots + s, o = t * GB_IDS + nd;
  const int n = w.st_cnt[o];
  w.thr[o] = 0.f;
  if (n == 0) {
    w.feat[o] = -2;
    return;
  }
  int bf = -1;
  if (n >= 2 && !(impurity(n, w.st_sq[o], w.st_ssq[o]) <= DBL_EPSILON)) {
    double bp = 0.0;
    uint64_t bprio = 0;
    for (int f = 0; f < D; ++f) {
      const Best& b = w.best[((long)t * D + f) * 4 + s];
      if (!b.has) continue;
      const uint64_t prio = tie_priority(tie_seed, stage, t, nd, f);
      if (bf < 0 || b.proxy > bp || (b.proxy == bp && prio > bprio)) bf = f, bp = b.proxy, bprio = prio;
    }
  }
  w.feat[o] = bf;
  if (bf >= 0) {
    const Best& b = w.best[((long)t * D + bf) * 4 + s];
    const float thr = (float)((double)b.xlo / 2.0 + (double)b.xhi / 2.0);
    w.thr[o] = thr == b.xhi ? b.xlo : thr;
  }
}

__global__ __launch_bounds__(256) void partition_kernel(const Work w, const float* __restrict__ x, const int N,
                                                        const int D, const int level) {
  const int t = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int nd = w.node[(long)t * N + i];
  if ((nd >> level) != 1) return;
  const int f = w.feat[t * GB_IDS + nd];
  if (f < 0) return;
  w.node[(long)t * N + i] = (unsigned char)(2 * nd + (x[(long)i * D + f] > w.thr[t * GB_IDS + nd] ? 1 : 0));
}

// ------------------------------------------------------------------ finish: one thread per tree
// Depth-3 nodes become leaves, leaf values, the tree's importances (internal nodes in id order) and
// the optional node tables.
__global__ __launch_bounds__(64) void finish_kernel(const Work w, const int T, const int D, const int N, const int C,
                                                    const int stage, int* __restrict__ dbg_feature,
                                                    float* __restrict__ dbg_threshold, int* __restrict__ dbg_count,
                                                    double* __restrict__ dbg_value) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= T) return;
  const int o = t * GB_IDS;
  for (int nd = 8; nd < 16; ++nd) w.feat[o + nd] = w.st_cnt[o + nd] > 0 ? -1 : -2, w.thr[o + nd] = 0.f;
  for (int nd = 1; nd < 16; ++nd) {
    double v = 0.0;
    if (w.feat[o + nd] == -1) {
      const double n = (double)w.st_cnt[o + nd];
      double num = w.st_sg[o + nd] / n;
      const double den = w.st_sp[o + nd] / n;
      if (C > 2) num = num * (((double)C - 1.0) / (double)C);
      v = fabs(den) < 1e-150 ? 0.0 : num / den;
    }
    w.val[o + nd] = v;
  }
  for (int f = 0; f < D; ++f) w.imp_tree[(long)t * D + f] = 0.0;
  for (int nd = 1; nd < 8; ++nd) {
    const int f = w.feat[o + nd];
    if (f < 0) continue;
    const int a = o + 2 * nd, b = a + 1, p = o + nd;
    const double term = ((double)w.st_cnt[p] * impurity(w.st_cnt[p], w.st_sq[p], w.st_ssq[p]) -
                         (double)w.st_cnt[a] * impurity(w.st_cnt[a], w.st_sq[a], w.st_ssq[a]) -
                         (double)w.st_cnt[b] * impurity(w.st_cnt[b], w.st_sq[b], w.st_ssq[b])) / (double)N;
    w.imp_tree[(long)t * D + f] = w.imp_tree[(long)t * D + f] + term;
  }
  if (dbg_feature) {
    const long d0 = ((long)stage * T + t) * GB_NODES;
    for (int nd = 1; nd < 16; ++nd) {
      dbg_feature[d0 + nd - 1] = w.feat[o + nd];
      dbg_threshold[d0 + nd - 1] = w.thr[o + nd];
      dbg_count[d0 + nd - 1] = w.feat[o + nd] == -2 ? 0 : w.st_cnt[o + nd];
      dbg_value[d0 + nd - 1] = w.val[o + nd];
    }
  }
}

// ------------------------------------------------------------------ leaf update: thread (tree, row)
__global__ __launch_bounds__(256) void update_kernel(const Work w, const float* __restrict__ x_test, const int N,
                                                     const int M, const int D, const int T, const double lr,
                                                     double* __restrict__ raw_train, double* __restrict__ raw_test) {
  const int t = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  const int o = t * GB_IDS;
  if (i < N) {
    raw_train[(long)i * T + t] += lr * w.val[o + w.node[(long)t * N + i]];
  } else if (i < N + M) {
    const int j = i - N;
    int nd = 1;
    for (int l = 0; l < 3; ++l) {
      const int f = w.feat[o + nd];
      if (f < 0) break;
      nd = 2 * nd + (x_test[(long)j * D + f] > w.thr[o + nd] ? 1 : 0);
    }
    raw_test[(long)j * T + t] += lr * w.val[o + nd];
  }
}

// the stage's trees with a split, added to the running importance sum in tree order
__global__ __launch_bounds__(64) void fold_kernel(const Work w, const int T, const int D) {
  const int f = threadIdx.x;
  int used = 0;
  double acc = f < D ? w.imp_acc[f] : 0.0;
  for (int t = 0; t < T; ++t) {
    if (w.feat[t * GB_IDS + 1] < 0) continue;
    ++used;
    if (f < D) acc = acc + w.imp_tree[(long)t * D + f];
  }
  if (f < D) w.imp_acc[f] = acc;
  if (f == 0) *w.used += used;
}

// ------------------------------------------------------------------ final
__global__ __launch_bounds__(64) void importance_kernel(const Work w, const int D, double* __restrict__ importance,
                                                        int* __restrict__ trees_used) {
  __shared__ double avg[GB_MAXD];
  __shared__ double total;
  const int f = threadIdx.x, used = *w.used;
  if (f < D) avg[f] = used ? w.imp_acc[f] / (double)used : 0.0;
  __syncthreads();
  if (f == 0) {
    double s = 0.0;
    for (int j = 0; j < D; ++j) s += avg[j];
    total = s;
    if (trees_used) *trees_used = used;
  }
  __syncthreads();
  if (f < D) importance[f] = used ? avg[f] / total : 0.0;
}

// argmax of the raw predictions (first maximum; raw >= 0 is class 1 for two classes) and the
// counts of correct rows: correct[0] training, correct[1] test
__global__ __launch_bounds__(256) void predict_kernel(const double* __restrict__ raw_train,
                                                      const double* __restrict__ raw_test,
                                                      const int* __restrict__ y_train, const int* __restrict__ y_test,
                                                      const int N, const int M, const int C,
                                                      int* __restrict__ pred_train, int* __restrict__ pred_test,
                                                      int* __restrict__ correct) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N + M) return;
  const bool test = i >= N;
  const long r = test ? i - N : i;
  const double* raw = test ? raw_test : raw_train;
  int best = 0;
  if (C == 2) {
    best = raw[r] >= 0.0 ? 1 : 0;
  } else {
    double bv = raw[r * C];
    for (int k = 1; k < C; ++k) {
      const double v = raw[r * C + k];
      if (v > bv) bv = v, best = k;
    }
  }
  (test ? pred_test : pred_train)[r] = best;
  if (best == (test ? y_test : y_train)[r]) atomicAdd(&correct[test ? 1 : 0], 1);
}

bool shape_ok(int n_train, int n_test, int dims, int classes) {
  return n_train >= 2 && n_train <= GB_MAXN && n_test >= 1 && n_test < (1 << 24) && dims >= 1 && dims <= GB_MAXD &&
         classes >= 2 && classes <= GB_MAXC;
}

}  // namespace

extern "C" int encdiff_gbt_gather(const float* codes, int n_rows, int dims, const int* idx, int n, float* out,
                                  void* stream) {
  if (!codes || !idx || !out) return ENCDIFF_ERR_ARG;
  if (n_rows <= 0 || dims < 1 || dims > GB_MAXD || n < 1 || n >= (1 << 24)) return ENCDIFF_ERR_SHAPE;
  const long total = (long)n * dims;
  hipLaunchKernelGGL(gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, codes,
                     n_rows, dims, idx, total, out);
  ED_CHECK_LAUNCH();
  return ENCDIFF_OK;
}

extern "C" int encdiff_gbt_workspace(int n_train, int n_test, int dims, int classes, long long* bytes) {
  if (!bytes) return ENCDIFF_ERR_ARG;
  if (!shape_ok(n_train, n_test, dims, classes)) return ENCDIFF_ERR_SHAPE;
  Work w;
  *bytes = (long long)carve(nullptr, n_train, dims, classes == 2 ? 1 : classes, w);
  return ENCDIFF_OK;
}

extern "C" int encdiff_gbt_fit(const EncdiffGbtArgs* a, void* stream) {
  if (!a || !a->x_train || !a->x_sorted || !a->order || !a->y_train || !a->x_test || !a->y_test || !a->init_raw ||
      !a->workspace || !a->raw_train || !a->raw_test || !a->pred_train || !a->pred_test || !a->correct ||
      !a->importance)
    return ENCDIFF_ERR_ARG;
  const bool dbg = a->dbg_feature || a->dbg_threshold || a->dbg_count || a->dbg_value;
  if (dbg && !(a->dbg_feature && a->dbg_threshold && a->dbg_count && a->dbg_value)) return ENCDIFF_ERR_ARG;
  if (!shape_ok(a->n_train, a->n_test, a->dims, a->classes) || a->n_estimators < 1 || a->n_estimators > 100000)
    return ENCDIFF_ERR_SHAPE;
  if (((uintptr_t)a->workspace & 7) != 0) return ENCDIFF_ERR_ARG;
  const int N = a->n_train, M = a->n_test, D = a->dims, C = a->classes, T = C == 2 ? 1 : C;
  Work w;
  carve((char*)a->workspace, N, D, T, w);
  hipStream_t s = (hipStream_t)stream;
  const long cells = (long)(N > M ? N : M) * T;
  hipLaunchKernelGGL(init_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, a->init_raw, T, (long)N,
                     (long)M, a->raw_train, a->raw_test, w.imp_acc, D, w.used, a->correct);
  ED_CHECK_LAUNCH();
  for (int stage = 0; stage < a->n_estimators; ++stage) {
    hipLaunchKernelGGL(grad_kernel, dim3((N + 3) / 4), dim3(256), 0, s, a->raw_train, a->y_train, N, C, w.g, w.gq,
                       w.node);
    ED_CHECK_LAUNCH();
    for (int level = 0; level < 4; ++level) {
      const int slots = 1 << level;
      hipLaunchKernelGGL(stats_kernel, dim3(T, slots), dim3(256), 0, s, w, a->y_train, N, C, level);
      ED_CHECK_LAUNCH();
      if (level == 3) break;
      hipLaunchKernelGGL(scan_kernel, dim3(T, D), dim3(256), 0, s, w, a->x_sorted, a->order, N, D, level);
      ED_CHECK_LAUNCH();
      hipLaunchKernelGGL(pick_kernel, dim3((T * slots + 63) / 64), dim3(64), 0, s, w, T, D, level, stage,
                         (uint64_t)a->tie_seed);
      ED_CHECK_LAUNCH();
      hipLaunchKernelGGL(partition_kernel, dim3((N + 255) / 256, T), dim3(256), 0, s, w, a->x_train, N, D, level);
      ED_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(finish_kernel, dim3((T + 63) / 64), dim3(64), 0, s, w, T, D, N, C, stage, a->dbg_feature,
                       a->dbg_threshold, a->dbg_count, a->dbg_value);
    ED_CHECK_LAUNCH();
    hipLaunchKernelGGL(update_kernel, dim3((N + M + 255) / 256, T), dim3(256), 0, s, w, a->x_test, N, M, D, T,
                       a->learning_rate, a->raw_train, a->raw_test);
    ED_CHECK_LAUNCH();
    hipLaunchKernelGGL(fold_kernel, dim3(1), dim3(64), 0, s, w, T, D);
    ED_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(importance_kernel, dim3(1), dim3(64), 0, s, w, D, a->importance, a->trees_used);
  ED_CHECK_LAUNCH();
  hipLaunchKernelGGL(predict_kernel, dim3((N + M + 255) / 256), dim3(256), 0, s, a->raw_train, a->raw_test, a->y_train,
                     a->y_test, N, M, C, a->pred_train, a->pred_test, a->correct);
  ED_CHECK_LAUNCH();
  return ENCDIFF_OK;
}
