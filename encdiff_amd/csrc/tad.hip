// TAD, the attribute metric of CelebA models (celeba_tad.py; ae_utils_exp.py aurocs_search, aurocs,
// calculate_auroc, LatentClass), over a device table z fp32 [n][L] of flattened concept tokens and
// one packed label word per row (bit a = attribute a, A <= 64).
//
// For every (attribute, column) pair the reference classifies the rows by z >= thr_k at 11
// thresholds between the column's minimum and maximum and integrates the ROC curve.  All it needs
// of the data are the counts
//     c[l][k][a] = #{n : z[n][l] >= thr[l][k] and label a of row n set},   a < A
//     c[l][k][A] = #{n : z[n][l] >= thr[l][k]}
// which are bit products: with M_lk the rows that pass threshold k of column l and T_a the rows
// that carry attribute a, both as bit vectors over the rows, c[l][k][a] = popcount(M_lk & T_a).
// The counting kernel builds both 64 rows at a time -- M from 11 comparisons per element, T by
// ballots over the label words -- and reads z once.
//
// Conventions of metrics.hip: integer atomics only (they commute: a second launch repeats bitwise),
// no floating-point atomics, no read-back and no allocation (graph-capturable), integer outputs
// zeroed by a kernel of this file.  Rows past n are never read and label bits >= A never counted.
#include "common.h"

namespace {

constexpr int TD_T = ENCDIFF_TAD_THRESHOLDS;   // 11
constexpr int TD_MAXA = ENCDIFF_TAD_MAX_ATTRS;  // 64
constexpr int TD_COLS = ENCDIFF_TAD_COL_TILE;   // 32 columns of a counting workgroup
constexpr int TD_STEP = ENCDIFF_TAD_ROW_STEP;   // 512 rows per pass: 4 waves x 2 half-waves x 64 rows
constexpr int TD_GROUPS = TD_STEP / 64;         // 8 groups of 64 rows
constexpr int TD_MAXROWS = 32768;               // rows of a counting workgroup: 16-bit LDS fields
constexpr int TD_MAXP = (TD_MAXA + 2) / 2;      // 33 pairs of (attribute | total) columns
constexpr int TD_LD = TD_COLS + 1;              // LDS row stride of the count table (odd: the flush
                                                // walks it across rows)

__global__ __launch_bounds__(256) void tad_zero_kernel(int* __restrict__ p, const long n) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) p[i] = 0;
}

void tad_zero(int* p, long n, hipStream_t s) {
  const long blocks = (n + 255) / 256;
  hipLaunchKernelGGL(tad_zero_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, s, p, n);
}

// Keeps a result opaque, so that -ffp-contract=fast cannot fuse it into the operation that follows:
// torch rounds the difference, the product and the sum separately.
ED_DEV float opaque(float x) {
  asm volatile("" : "+v"(x));
  return x;
}

// float <-> unsigned key with the same order (negative floats reversed below the positive ones), so
// that an exact minimum and maximum can be taken with integer atomics.
ED_DEV unsigned key_of(float x) {
  const unsigned u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
ED_DEV float float_of(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// ------------------------------------------------------------------ range and thresholds
__global__ __launch_bounds__(256) void tad_range_init_kernel(unsigned* __restrict__ kmax, unsigned* __restrict__ kmin,
                                                             const int L) {
  const int l = blockIdx.x * 256 + threadIdx.x;
  if (l < L) {
    kmax[l] = 0u;           // below every key
    kmin[l] = 0xffffffffu;  // above every key
  }
}

// grid = (column tiles of 64, row chunks); thread = (row phase t / 64, column t % 64): a wave reads
// 64 consecutive floats of a row.  A NaN makes both ends NaN, as torch's max and min do: its keys
// are the two extremes, which decode to NaNs.
__global__ __launch_bounds__(256) void tad_range_kernel(const float* __restrict__ z, const long n, const int L,
                                                        const long rows_per, unsigned* __restrict__ kmax,
                                                        unsigned* __restrict__ kmin) {
  __shared__ unsigned smax[256], smin[256];
  const int t = threadIdx.x, c = t & 63, ph = t >> 6;
  const long l = (long)blockIdx.x * 64 + c;
  const long r0 = (long)blockIdx.y * rows_per, r1 = r0 + rows_per < n ? r0 + rows_per : n;
  unsigned hi = 0u, lo = 0xffffffffu;
  if (l < L)
    for (long r = r0 + ph; r < r1; r += 4) {
      const float x = z[r * L + l];
      const bool nan = x != x;
      const unsigned k = key_of(x);
      const unsigned kh = nan ? 0xffffffffu : k, kl = nan ? 0u : k;
      hi = kh > hi ? kh : hi;
      lo = kl < lo ? kl : lo;
    }
  smax[t] = hi;
  smin[t] = lo;
  __syncthreads();
  if (t < 64 && l < L) {
    for (int p = 1; p < 4; ++p) {
      hi = smax[p * 64 + t] > hi ? smax[p * 64 + t] : hi;
      lo = smin[p * 64 + t] < lo ? smin[p * 64 + t] : lo;
    }
    if (r0 < r1) {
      atomicMax(&kmax[l], hi);
      atomicMin(&kmin[l], lo);
    }
  }
}

// keys -> floats in place, and thr[l][k] = t[k] * (ma - mi) + mi, each operation rounded on its own
__global__ __launch_bounds__(256) void tad_thr_kernel(unsigned* __restrict__ kmax, unsigned* __restrict__ kmin,
                                                      const float* __restrict__ t, const int L,
                                                      float* __restrict__ thr) {
  const int l = blockIdx.x * 256 + threadIdx.x;
  if (l >= L) return;
  const float ma = float_of(kmax[l]), mi = float_of(kmin[l]);
  kmax[l] = __float_as_uint(ma);
  kmin[l] = __float_as_uint(mi);
  const float d = opaque(ma - mi);
  for (int k = 0; k < TD_T; ++k) thr[(long)l * TD_T + k] = opaque(t[k] * d) + mi;
}

// ------------------------------------------------------------------ counts (the hot path)
// The 11 bit vectors of one column over 64 rows, bit r of M_k = (z[row r] >= thr_k): zp walks down
// the column by `stride` floats, and stops after `last` steps where the chunk ends inside the group
// (FULL: all 64 rows exist).  Loads go eight at a time, one batch ahead of the comparisons.
template <bool FULL>
ED_DEV void build_masks(const float* zp, const long stride, const int last, const float (&th)[TD_T],
                        unsigned (&mlo)[TD_T], unsigned (&mhi)[TD_T]) {
#pragma unroll
  for (int k = 0; k < TD_T; ++k) mlo[k] = mhi[k] = 0u;
  float x[2][8];
#pragma unroll
  for (int q = 0; q <= 8; ++q) {
    if (q < 8) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        x[q & 1][j] = *zp;
        zp += (FULL || q * 8 + j < last) ? stride : 0;
      }
    }
    // the loads of batch q stay ahead of the comparisons of batch q - 1 and no further: without the
    // fences the scheduler hoists all 64 loads and the kernel drops to one wave per SIMD
    __builtin_amdgcn_sched_barrier(0);
    if (q > 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int bit = ((q - 1) * 8 + j) & 31;
#pragma unroll
        for (int k = 0; k < TD_T; ++k) {
          const unsigned m = (x[(q - 1) & 1][j] >= th[k]) ? (1u << bit) : 0u;
          if (q - 1 < 4) mlo[k] |= m; else mhi[k] |= m;
        }
        __builtin_amdgcn_sched_barrier(0);  // row by row: 11 selects live, not 88
      }
    }
  }
}

// grid = column tiles x row chunks (tile fastest: neighbouring workgroups read neighbouring columns
// of the same rows).  A workgroup owns 32 columns and a chunk of at most 32768 rows, 512 rows a
// pass.  Lane = (half h, column c): half-wave h of wave w takes the 64 rows of group g = 2 w + h,
// so each row is read as 32 consecutive floats (128 bytes).  A lane keeps the 11 bit vectors M_k of
// its column over its 64 rows in registers.  The label words of a group are turned into the bit
// vectors T_a by one ballot per attribute (tb in LDS; T_A = the rows that exist).  Then, per pair of
// attributes, popcount(M_k & T_a) | popcount(M_k & T_a') << 16 goes into the LDS table with one
// ds_add: the two halves of a wave hit the same 32 words, which the LDS serves as two lane groups,
// and a 16-bit field holds a workgroup's rows.  One flush with global atomics at the end.
__global__ __launch_bounds__(256) void tad_counts_kernel(const float* __restrict__ z,
                                                         const unsigned long long* __restrict__ packed, const long n,
                                                         const int L, const int A, const int tiles,
                                                         const long rows_per, const float* __restrict__ thr,
                                                         int* __restrict__ counts) {
  __shared__ unsigned tab[TD_T * TD_MAXP * TD_LD];
  __shared__ unsigned long long tb[2 * TD_MAXP * TD_GROUPS];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, c = lane & 31, g = 2 * w + (lane >> 5);
  const int tile = blockIdx.x % tiles;
  const long chunk = blockIdx.x / tiles;
  const int A1 = A + 1, P = (A1 + 1) / 2;
  const long col = (long)tile * TD_COLS + c;
  const long colc = col < L ? col : (long)L - 1;  // a lane past the last column repeats it; never flushed
  const long r0 = chunk * rows_per, r1 = r0 + rows_per < n ? r0 + rows_per : n;

  for (int i = t; i < TD_T * P * TD_LD; i += 256) tab[i] = 0u;
  // the odd slot of the last pair when A + 1 is odd: no rows
  if ((A1 & 1) && t < TD_GROUPS) tb[A1 * TD_GROUPS + t] = 0ull;
  float th[TD_T];
#pragma unroll
  for (int k = 0; k < TD_T; ++k) th[k] = thr[colc * TD_T + k];

  for (long base = r0; base < r1; base += TD_STEP) {
    __syncthreads();  // tab zeroed / tb of the last pass consumed
    // labels: wave w ballots its two groups
    for (int h = 0; h < 2; ++h) {
      const long r = base + (2 * w + h) * 64 + lane;
      const bool ok = r < r1;
      const unsigned long long word = ok ? packed[r] : 0ull;
      for (int a = 0; a < A; ++a) {
        const unsigned long long b = __ballot((int)((word >> a) & 1ull));
        if (lane == 0) tb[a * TD_GROUPS + 2 * w + h] = b;
      }
      const unsigned long long v = __ballot(ok ? 1 : 0);
      if (lane == 0) tb[A * TD_GROUPS + 2 * w + h] = v;
    }
    // M_k of this lane's column over its group's 64 rows.  A row that does not exist repeats the
    // chunk's last row: its bits are dropped by the T_a, which are zero there.
    unsigned mlo[TD_T], mhi[TD_T];
    const long gr = base + g * 64, rem = r1 - gr;
    const float* zp = z + (rem > 0 ? gr : r1 - 1) * L + colc;
    if (base + TD_STEP <= r1)  // the same for the whole workgroup
      build_masks<true>(zp, L, 63, th, mlo, mhi);
    else
      build_masks<false>(zp, L, rem > 1 ? (int)(rem < 64 ? rem : 64) - 1 : 0, th, mlo, mhi);
    __syncthreads();  // tb written
    for (int p = 0; p < P; ++p) {
      const unsigned long long ta = tb[(2 * p) * TD_GROUPS + g], tc = tb[(2 * p + 1) * TD_GROUPS + g];
      const unsigned alo = (unsigned)ta, ahi = (unsigned)(ta >> 32), clo = (unsigned)tc, chi = (unsigned)(tc >> 32);
#pragma unroll
      for (int k = 0; k < TD_T; ++k) {
        const unsigned na = __popc(mlo[k] & alo) + __popc(mhi[k] & ahi);
        const unsigned nc = __popc(mlo[k] & clo) + __popc(mhi[k] & chi);
        atomicAdd(&tab[(k * P + p) * TD_LD + c], na | (nc << 16));
      }
    }
  }
  __syncthreads();
  // flush: i = (column, k, a) with a fastest, as the output lies
  const int per_col = TD_T * A1;
  for (int i = t; i < TD_COLS * per_col; i += 256) {
    const int cc = i / per_col, ka = i - cc * per_col, k = ka / A1, a = ka - k * A1;
    const long lc = (long)tile * TD_COLS + cc;
    const unsigned v = (tab[(k * P + (a >> 1)) * TD_LD + cc] >> (16 * (a & 1))) & 0xffffu;
    if (lc < L && v) atomicAdd(&counts[lc * per_col + ka], (int)v);
  }
}

// ------------------------------------------------------------------ label joint counts
// TT[i][j] = #{n : labels i and j of row n both set}.  A wave takes a group of 64 rows (lane = row),
// ballots the A attributes into T_a, then lane j adds popcount(T_i & T_j) for every i into
// registers; the four waves of a workgroup meet in LDS, one flush with global atomics.
__global__ __launch_bounds__(256) void tad_joint_kernel(const unsigned long long* __restrict__ packed, const long n,
                                                        const int A, int* __restrict__ joint) {
  __shared__ unsigned long long tb[4][TD_MAXA];
  __shared__ int acc_s[TD_MAXA * TD_MAXA];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  for (int i = t; i < A * A; i += 256) acc_s[i] = 0;
  int acc[TD_MAXA];
#pragma unroll
  for (int i = 0; i < TD_MAXA; ++i) acc[i] = 0;
  const long groups = (n + 63) / 64;
  for (long g0 = (long)blockIdx.x * 4; g0 < groups; g0 += (long)gridDim.x * 4) {
    const long r = (g0 + w) * 64 + lane;
    const unsigned long long word = r < n ? packed[r] : 0ull;
    unsigned long long mine = 0ull;
    for (int a = 0; a < A; ++a) {
      const unsigned long long b = __ballot((int)((word >> a) & 1ull));
      if (lane == 0) tb[w][a] = b;
      if (lane == a) mine = b;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < TD_MAXA; ++i)
      if (i < A) acc[i] += __popcll(tb[w][i] & mine);
    __syncthreads();  // tb is rewritten by the next group
  }
  __syncthreads();
  if (lane < A) {
#pragma unroll
    for (int i = 0; i < TD_MAXA; ++i)
      if (i < A && acc[i]) atomicAdd(&acc_s[i * A + lane], acc[i]);
  }
  __syncthreads();
  for (int i = t; i < A * A; i += 256)
    if (acc_s[i]) atomicAdd(&joint[i], acc_s[i]);
}

// ------------------------------------------------------------------ AUROC
// fp32 quotient of two counts as torch forms it: both converted to float32, then divided with one
// rounding (through fp64: 53 >= 2 * 24 + 2 bits, the second rounding changes nothing).  0 / 0 = NaN.
ED_DEV float ratio(const int a, const int b) { return (float)((double)(float)a / (double)(float)b); }

// thread = (attribute a, column l).  The reference sorts the 11 fpr and the 11 tpr values each on
// their own; both fall with k for the ">=" classifier (a reversal) and rise for the "<" one.
__global__ __launch_bounds__(256) void tad_auroc_kernel(const int* __restrict__ counts, const int* __restrict__ joint,
                                                        const float* __restrict__ ma, const float* __restrict__ mi,
                                                        const long n, const int L, const int A,
                                                        float* __restrict__ aurocs) {
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= (long)A * L) return;
  const int a = (int)(i / L);
  const long l = i - (long)a * L;
  if (!(opaque(ma[l] - mi[l]) > 0.2f)) {
    aurocs[i] = 0.5f;
    return;
  }
  const int pos = joint[a * A + a], neg = (int)(n - pos), A1 = A + 1;
  const int* c = counts + l * TD_T * A1;
  float pf[TD_T], pt[TD_T], nf[TD_T], nt[TD_T];
#pragma unroll
  for (int k = 0; k < TD_T; ++k) {
    const int tp = c[k * A1 + a], fp = c[k * A1 + A] - tp;
    pf[TD_T - 1 - k] = ratio(fp, neg);
    pt[TD_T - 1 - k] = ratio(tp, pos);
    nf[k] = ratio(neg - fp, neg);
    nt[k] = ratio(pos - tp, pos);
  }
  float pa = 0.f, na = 0.f;
#pragma unroll
  for (int k = 1; k < TD_T; ++k) {
    pa += opaque(pt[k] * opaque(pf[k] - pf[k - 1]));
    na += opaque(nt[k] * opaque(nf[k] - nf[k - 1]));
  }
  aurocs[i] = na > pa ? na : pa;  // Python's max(p, n)
}

}  // namespace

extern "C" int encdiff_tad_range(const float* z, long long n, int L, const float* t, float* col_max, float* col_min,
                                 float* thr, void* stream) {
  if (!z || !t || !col_max || !col_min || !thr) return ENCDIFF_ERR_ARG;
  if (n < 1 || n > 2147483647LL || L < 1) return ENCDIFF_ERR_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  const unsigned tiles = (unsigned)(((long)L + 63) / 64), lblocks = (unsigned)(((long)L + 255) / 256);
  // about 2048 workgroups; a chunk is a multiple of 4 rows and the grid's y is at most 65535
  long chunks = (2048 + (long)tiles - 1) / tiles;
  const long most = (n + 255) / 256;
  if (chunks > most) chunks = most;
  long rows_per = ((n + chunks - 1) / chunks + 3) / 4 * 4;
  chunks = (n + rows_per - 1) / rows_per;
  unsigned* kmax = (unsigned*)col_max;
  unsigned* kmin = (unsigned*)col_min;
  hipLaunchKernelGGL(tad_range_init_kernel, dim3(lblocks), dim3(256), 0, s, kmax, kmin, L);
  ED_CHECK_LAUNCH();
  hipLaunchKernelGGL(tad_range_kernel, dim3(tiles, (unsigned)chunks), dim3(256), 0, s, z, (long)n, L, rows_per, kmax,
                     kmin);
  ED_CHECK_LAUNCH();
  hipLaunchKernelGGL(tad_thr_kernel, dim3(lblocks), dim3(256), 0, s, kmax, kmin, t, L, thr);
  ED_CHECK_LAUNCH();
  return ENCDIFF_OK;
}

extern "C" int encdiff_tad_counts(const float* z, const long long* packed, long long n, int L, int A, const float* thr,
                                  int* counts, void* stream) {
  if (!z || !packed || !thr || !counts) return ENCDIFF_ERR_ARG;
  if (n < 1 || n > 2147483647LL || L < 1 || A < 1 || A > TD_MAXA) return ENCDIFF_ERR_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  const long tiles = ((long)L + TD_COLS - 1) / TD_COLS;
  // about 1024 workgroups, whole passes of 512 rows, at most 32768 rows each
  long chunks = (1024 + tiles - 1) / tiles;
  const long most = (n + TD_STEP - 1) / TD_STEP;
  if (chunks > most) chunks = most;
  long rows_per = ((n + chunks - 1) / chunks + TD_STEP - 1) / TD_STEP * TD_STEP;
  if (rows_per > TD_MAXROWS) rows_per = TD_MAXROWS;
  chunks = (n + rows_per - 1) / rows_per;
  if (tiles * chunks > 2147483647L) return ENCDIFF_ERR_SHAPE;
  tad_zero(counts, (long)L * TD_T * (A + 1), s);
  ED_CHECK_LAUNCH();
  hipLaunchKernelGGL(tad_counts_kernel, dim3((unsigned)(tiles * chunks)), dim3(256), 0, s, z,
                     (const unsigned long long*)packed, (long)n, L, A, (int)tiles, rows_per, thr, counts);
  ED_CHECK_LAUNCH();
  return ENCDIFF_OK;
}

extern "C" int encdiff_tad_label_joint(const long long* packed, long long n, int A, int* joint, void* stream) {
  if (!packed || !joint) return ENCDIFF_ERR_ARG;
  if (n < 1 || n > 2147483647LL || A < 1 || A > TD_MAXA) return ENCDIFF_ERR_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  tad_zero(joint, (long)A * A, s);
  ED_CHECK_LAUNCH();
  const long groups = ((long)n + 63) / 64, want = (groups + 3) / 4;
  hipLaunchKernelGGL(tad_joint_kernel, dim3((unsigned)(want < 256 ? want : 256)), dim3(256), 0, s,
                     (const unsigned long long*)packed, (long)n, A, joint);
  ED_CHECK_LAUNCH();
  return ENCDIFF_OK;
}

extern "C" int encdiff_tad_auroc(const int* counts, const int* joint, const float* col_max, const float* col_min,
                                 long long n, int L, int A, float* aurocs, void* stream) {
  if (!counts || !joint || !col_max || !col_min || !aurocs) return ENCDIFF_ERR_ARG;
  if (n < 1 || n > 2147483647LL || L < 1 || A < 1 || A > TD_MAXA) return ENCDIFF_ERR_SHAPE;
  const long cells = (long)A * L;
  hipLaunchKernelGGL(tad_auroc_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, (hipStream_t)stream, counts,
                     joint, col_max, col_min, (long)n, L, A, aurocs);
  ED_CHECK_LAUNCH();
  return ENCDIFF_OK;
}
