// The beta-VAE score (evaluation/metrics/beta_vae.py) on the device: the feature table
// mean_b |codes[idx1[p][b]] - codes[idx2[p][b]]|, sklearn's default multinomial LogisticRegression
// fitted on it, and the accuracy of its predictions.  tests/logreg_restate.py restates all three in
// numpy; this file is built with -ffp-contract=off, so every product and sum rounds on its own as
// it does there.
//
// The fit, logreg_fit_kernel, is the whole L-BFGS run in ONE launch of ONE workgroup of 1024
// threads: 10 000 rows of <= 64 features and <= 16 classes make one loss / gradient evaluation
// about 1 MFLOP, a run takes about 110 of them, and a grid-wide barrier between evaluations is not
// worth its risk.  The run is scipy's L-BFGS-B on an unconstrained problem as sklearn calls it:
// two-loop recursion over m = 10 pairs (initial scaling y.s / y.y of the newest pair), MINPACK-2's
// dcsrch / dcstep line search (ftol 1e-3, gtol 0.9, xtol 0.1, first trial step 1 / |d| in iteration
// 0 and 1 afterwards, at most 50 evaluations), and L-BFGS-B's stopping tests.  A line search that
// ends on anything but its convergence test ends the fit with status 3; L-BFGS-B's "drop the
// history and restart" path is not emulated.
//
// Reduction order (fixed, so a launch repeats bit for bit; no floating-point atomics):
//   * the loss: thread t adds the rows t, t + 1024, ... in ascending order, the 1024 partials are
//     folded by block_sum: a xor-shuffle tree inside every wave, then the 16 wave sums in wave order;
//   * the gradient entry (k, d): the rows are cut into S = max(1, 1024 / E) equal segments (E = K (D
//     + 1) entries), one thread adds the rows of one segment in ascending order, and the S partials
//     of an entry are added in segment order;
//   * every dot product of the recursion: thread t holds the entries t, t + 1024, then block_sum.
// All scalars of the solver (step, loss, directional derivative, the line search's state) are
// computed by every lane from the same reduced values, so the control flow is uniform and every
// barrier is reached by all lanes.  Every loop is bounded: max_iter <= 1000 iterations, <= 50
// evaluations per line search, 10 pairs.
//
// Memory: the parameters, gradient, direction and the previous point's copies live in LDS (5 x 1040
// doubles); the (n, K) residual (P - Y) / n and the ten (s, y) pairs (2 x 10 x 1040 doubles, more
// than the LDS holds) live in the caller's workspace.  A pair's entry is written and read by the
// thread that owns the entry; the residual is written by row owners and read by entry owners after
// a workgroup barrier.
#include "common.h"

namespace {

constexpr int BV_MAXD = ENCDIFF_METRICS_MAX_DIMS;      // 64
constexpr int BV_MAXK = ENCDIFF_METRICS_MAX_FACTORS;   // 16
constexpr int BV_MAXE = BV_MAXK * (BV_MAXD + 1);       // 1040 parameters
constexpr int BV_T = 1024;
constexpr int BV_PAIRS = 10;
constexpr int BV_MAXLS = 50;
constexpr double BV_EPS = 2.220446049250313e-16;
constexpr double BV_STPMAX = 1e10;

ED_DEV long clamp_row(int r, int n_rows) { return r < 0 ? 0 : (r >= n_rows ? n_rows - 1 : r); }

// ------------------------------------------------------------------ features
// One thread per output (p, d), adjacent threads adjacent d: a gathered code row is read
// contiguously.  The float32 sum runs in the order b = 0..B-1 and is divided (a true division) by
// (float)B, as np.mean of float32 rows does, then widened.
__global__ __launch_bounds__(256) void beta_features_kernel(const float* __restrict__ codes, const int n_rows,
                                                            const int dims, const int* __restrict__ idx1,
                                                            const int* __restrict__ idx2, const int points,
                                                            const int batch, double* __restrict__ out) {
  const long e = blockIdx.x * 256L + threadIdx.x;
  if (e >= (long)points * dims) return;
  const long p = e / dims;
  const int d = (int)(e - p * dims);
  float acc = 0.f;
  for (int b = 0; b < batch; ++b) {
    const long r1 = clamp_row(idx1[p * batch + b], n_rows), r2 = clamp_row(idx2[p * batch + b], n_rows);
    acc += fabsf(codes[r1 * dims + d] - codes[r2 * dims + d]);
  }
  out[e] = (double)(acc / (float)batch);
}

// ------------------------------------------------------------------ the fit
// The sum of v over the 1024 threads, the same bits in every thread.
ED_DEV double block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < BV_T / 64; ++i) s += red[i];
  return s;
}

ED_DEV double block_max(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < BV_T / 64; ++i) s = fmax(s, red[i]);
  return s;
}

ED_DEV double max3(double a, double b, double c) { return fmax(fmax(a, b), c); }

// MINPACK-2 dcstep
ED_DEV void dcstep(double& stx, double& fx, double& dx, double& sty, double& fy, double& dy, double& stp,
                   const double fp, const double dp, bool& brackt, const double stpmin, const double stpmax) {
  const double sgnd = dp * (dx / fabs(dx));
  double stpf;
  if (fp > fx) {
    const double theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp;
    const double s = max3(fabs(theta), fabs(dx), fabs(dp));
    double gamma = s * sqrt((theta / s) * (theta / s) - (dx / s) * (dp / s));
    if (stp < stx) gamma = -gamma;
    const double p = (gamma - dx) + theta, q = ((gamma - dx) + gamma) + dp, r = p / q;
    const double stpc = stx + r * (stp - stx);
    const double stpq = stx + ((dx / ((fx - fp) / (stp - stx) + dx)) / 2.0) * (stp - stx);
    stpf = fabs(stpc - stx) < fabs(stpq - stx) ? stpc : stpc + (stpq - stpc) / 2.0;
    brackt = true;
  } else if (sgnd < 0.0) {
    const double theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp;
    const double s = max3(fabs(theta), fabs(dx), fabs(dp));
    double gamma = s * sqrt((theta / s) * (theta / s) - (dx / s) * (dp / s));
    if (stp > stx) gamma = -gamma;
    const double p = (gamma - dp) + theta, q = ((gamma - dp) + gamma) + dx, r = p / q;
    const double stpc = stp + r * (stx - stp);
    const double stpq = stp + (dp / (dp - dx)) * (stx - stp);
    stpf = fabs(stpc - stp) > fabs(stpq - stp) ? stpc : stpq;
    brackt = true;
  } else if (fabs(dp) < fabs(dx)) {
    const double theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp;
    const double s = max3(fabs(theta), fabs(dx), fabs(dp));
    double gamma = s * sqrt(fmax(0.0, (theta / s) * (theta / s) - (dx / s) * (dp / s)));
    if (stp > stx) gamma = -gamma;
    const double p = (gamma - dp) + theta, q = (gamma + (dx - dp)) + gamma, r = p / q;
    double stpc;
    if (r < 0.0 && gamma != 0.0) stpc = stp + r * (stx - stp);
    else if (stp > stx) stpc = stpmax;
    else stpc = stpmin;
    const double stpq = stp + (dp / (dp - dx)) * (stx - stp);
    if (brackt) {
      stpf = fabs(stpc - stp) < fabs(stpq - stp) ? stpc : stpq;
      stpf = stp > stx ? fmin(stp + 0.66 * (sty - stp), stpf) : fmax(stp + 0.66 * (sty - stp), stpf);
    } else {
      stpf = fabs(stpc - stp) > fabs(stpq - stp) ? stpc : stpq;
      stpf = fmax(stpmin, fmin(stpmax, stpf));
    }
  } else {
    if (brackt) {
      const double theta = 3.0 * (fp - fy) / (sty - stp) + dy + dp;
      const double s = max3(fabs(theta), fabs(dy), fabs(dp));
      double gamma = s * sqrt((theta / s) * (theta / s) - (dy / s) * (dp / s));
      if (stp > sty) gamma = -gamma;
      const double p = (gamma - dp) + theta, q = ((gamma - dp) + gamma) + dy, r = p / q;
      stpf = stp + r * (sty - stp);
    } else if (stp > stx) {
      stpf = stpmax;
    } else {
      stpf = stpmin;
    }
  }
  if (fp > fx) {
    sty = stp, fy = fp, dy = dp;
  } else {
    if (sgnd < 0.0) sty = stx, fy = fx, dy = dx;
    stx = stp, fx = fp, dx = dp;
  }
  stp = stpf;
}

// MINPACK-2 dcsrch with stpmin = 0, stpmax = 1e10, as a state every lane carries.
struct LineSearch {
  bool brackt;
  int stage;
  double finit, ginit, gtest, width, width1, stx, fx, gx, sty, fy, gy, stmin, stmax, stp;

  ED_DEV void start(const double f, const double g, const double stp0) {
    brackt = false, stage = 1;
    finit = f, ginit = g, gtest = 1e-3 * g;
    width = BV_STPMAX, width1 = 2.0 * BV_STPMAX;
    stx = 0.0, fx = f, gx = g, sty = 0.0, fy = f, gy = g;
    stmin = 0.0, stmax = stp0 + 4.0 * stp0, stp = stp0;
  }

  // the values at stp: 0 evaluate the new stp, 1 converged, 2 ended on a warning
  ED_DEV int step(const double f, const double g) {
    const double ftest = finit + stp * gtest;
    if (stage == 1 && f <= ftest && g >= 0.0) stage = 2;
    const bool warn = (brackt && (stp <= stmin || stp >= stmax)) || (brackt && stmax - stmin <= 0.1 * stmax) ||
                      (stp == BV_STPMAX && f <= ftest && g <= gtest) || (stp == 0.0 && (f > ftest || g >= gtest));
    if (f <= ftest && fabs(g) <= 0.9 * (-ginit)) return 1;
    if (warn) return 2;
    if (stage == 1 && f <= fx && f > ftest) {
      const double fm = f - stp * gtest, gm = g - gtest;
      double fxm = fx - stx * gtest, fym = fy - sty * gtest, gxm = gx - gtest, gym = gy - gtest;
      dcstep(stx, fxm, gxm, sty, fym, gym, stp, fm, gm, brackt, stmin, stmax);
      fx = fxm + stx * gtest, fy = fym + sty * gtest, gx = gxm + gtest, gy = gym + gtest;
    } else {
      dcstep(stx, fx, gx, sty, fy, gy, stp, f, g, brackt, stmin, stmax);
    }
    if (brackt) {
      if (fabs(sty - stx) >= 0.66 * width1) stp = stx + 0.5 * (sty - stx);
      width1 = width;
      width = fabs(sty - stx);
      stmin = fmin(stx, sty), stmax = fmax(stx, sty);
    } else {
      stmin = stp + 1.1 * (stp - stx);
      stmax = stp + 4.0 * (stp - stx);
    }
    stp = fmin(fmax(stp, 0.0), BV_STPMAX);
    if ((brackt && (stp <= stmin || stp >= stmax)) || (brackt && stmax - stmin <= 0.1 * stmax)) stp = stx;
    return 0;
  }
};

struct FitShared {
  double w[BV_MAXE], g[BV_MAXE], d[BV_MAXE], w_old[BV_MAXE], g_old[BV_MAXE], part[BV_MAXE];
  double red[BV_T / 64], ys[BV_PAIRS];
};

// Loss and gradient at sh.w (sklearn's LinearModelLoss.loss_gradient of the half multinomial loss,
// unit weights): the loss is returned, the gradient left in sh.g.  Entry e = k (D + 1) + d, d == D
// the intercept of class k.
ED_DEV double loss_grad(FitShared& sh, const double* __restrict__ x, const int* __restrict__ y, const int n,
                        const int D, const int K, const double l2, double* __restrict__ resid) {
  const int t = threadIdx.x, D1 = D + 1, E = K * D1;
  __syncthreads();  // sh.w is complete
  double lsum = 0.0;
  for (int i = t; i < n; i += BV_T) {
    double z[BV_MAXK];
#pragma unroll
    for (int k = 0; k < BV_MAXK; ++k) z[k] = 0.0;
    const double* xi = x + (long)i * D;
    for (int d = 0; d < D; ++d) {
      const double xv = xi[d];
#pragma unroll
      for (int k = 0; k < BV_MAXK; ++k)
        if (k < K) z[k] += xv * sh.w[k * D1 + d];
    }
    int yi = y[i];
    yi = yi < 0 ? 0 : (yi >= K ? K - 1 : yi);
    double zmax = -INFINITY, zy = 0.0;
#pragma unroll
    for (int k = 0; k < BV_MAXK; ++k)
      if (k < K) {
        z[k] += sh.w[k * D1 + D];
        zmax = fmax(zmax, z[k]);
        zy = k == yi ? z[k] : zy;
      }
    double se = 0.0;
#pragma unroll
    for (int k = 0; k < BV_MAXK; ++k)
      if (k < K) {
        z[k] = exp(z[k] - zmax);
        se += z[k];
      }
    lsum += (zmax + log(se)) - zy;
#pragma unroll
    for (int k = 0; k < BV_MAXK; ++k)
      if (k < K) resid[(long)i * K + k] = (z[k] / se - (k == yi ? 1.0 : 0.0)) / (double)n;
  }
  double wsq = 0.0;
  for (int e = t; e < E; e += BV_T)
    if (e % D1 < D) wsq += sh.w[e] * sh.w[e];
  const double loss = block_sum(lsum, sh.red) / (double)n + 0.5 * l2 * block_sum(wsq, sh.red);
  __threadfence_block();
  __syncthreads();  // the residual is complete
  const int S = E >= BV_T ? 1 : BV_T / E;
  const int L = (n + S - 1) / S;
  for (int item = t; item < E * S; item += BV_T) {
    const int s = item / E, e = item - s * E, k = e / D1, d = e - k * D1;
    const int r0 = s * L, r1 = r0 + L < n ? r0 + L : n;
    double acc = 0.0;
    if (d < D) {
      for (int i = r0; i < r1; ++i) acc += resid[(long)i * K + k] * x[(long)i * D + d];
    } else {
      for (int i = r0; i < r1; ++i) acc += resid[(long)i * K + k];
    }
    sh.part[item] = acc;
  }
  __syncthreads();
  for (int e = t; e < E; e += BV_T) {
    double acc = 0.0;
    for (int s = 0; s < S; ++s) acc += sh.part[s * E + e];
    sh.g[e] = e % D1 < D ? acc + l2 * sh.w[e] : acc;
  }
  __syncthreads();  // sh.g is complete, sh.part may be written again
  return loss;
}

__global__ __launch_bounds__(BV_T) void logreg_fit_kernel(const double* __restrict__ x, const int* __restrict__ y,
                                                          const int n, const int D, const int K, const double l2,
                                                          const int max_iter, const double tol,
                                                          double* __restrict__ ws, double* __restrict__ coef,
                                                          double* __restrict__ intercept, int* __restrict__ info,
                                                          double* __restrict__ loss_out) {
  __shared__ FitShared sh;
  const int t = threadIdx.x, D1 = D + 1, E = K * D1;
  double* resid = ws;
  double* hs = ws + (long)n * K;          // s pairs [10][E]
  double* hy = hs + (long)BV_PAIRS * E;   // y pairs [10][E]
  for (int e = t; e < E; e += BV_T) sh.w[e] = 0.0;
  double f = loss_grad(sh, x, y, n, D, K, l2, resid);
  int nfev = 1, it = 0, status = -1, max_ls = 0, head = 0, count = 0;
  double theta = 1.0;
  {
    double gm = 0.0;
    for (int e = t; e < E; e += BV_T) gm = fmax(gm, fabs(sh.g[e]));
    if (block_max(gm, sh.red) <= tol) status = 0;
  }
  LineSearch ls;
  while (status < 0) {
    // two-loop recursion; q lives in sh.d, every thread touches its own entries only
    for (int e = t; e < E; e += BV_T) sh.d[e] = sh.g[e];
    double alpha[BV_PAIRS];
#pragma unroll
    for (int j = 0; j < BV_PAIRS; ++j) {
      alpha[j] = 0.0;
      if (j < count) {  // the newest pair first
        const int slot = (head + count - 1 - j) % BV_PAIRS;
        double acc = 0.0;
        for (int e = t; e < E; e += BV_T) acc += hs[slot * E + e] * sh.d[e];
        const double a = block_sum(acc, sh.red) / sh.ys[slot];
        alpha[j] = a;
        for (int e = t; e < E; e += BV_T) sh.d[e] -= a * hy[slot * E + e];
      }
    }
    for (int e = t; e < E; e += BV_T) sh.d[e] /= theta;
#pragma unroll
    for (int j = BV_PAIRS - 1; j >= 0; --j) {
      if (j < count) {  // the oldest pair first
        const int slot = (head + count - 1 - j) % BV_PAIRS;
        double acc = 0.0;
        for (int e = t; e < E; e += BV_T) acc += hy[slot * E + e] * sh.d[e];
        const double b = block_sum(acc, sh.red) / sh.ys[slot];
        for (int e = t; e < E; e += BV_T) sh.d[e] += hs[slot * E + e] * (alpha[j] - b);
      }
    }
    double dd = 0.0, gdp = 0.0;
    for (int e = t; e < E; e += BV_T) {
      const double de = -sh.d[e];
      sh.d[e] = de;
      dd += de * de;
      gdp += sh.g[e] * de;
      sh.w_old[e] = sh.w[e];
      sh.g_old[e] = sh.g[e];
    }
    const double dnorm = sqrt(block_sum(dd, sh.red));
    double gd = block_sum(gdp, sh.red);
    const double gd_old = gd, f_old = f;
    if (gd >= 0.0) {
      status = 3;
      break;
    }
    ls.start(f, gd, it == 0 ? fmin(1.0 / dnorm, BV_STPMAX) : 1.0);
    int evals = 0;
    double stp = 0.0;
    for (;;) {
      if (evals >= BV_MAXLS) {
        status = 3;
        break;
      }
      stp = ls.stp;
      for (int e = t; e < E; e += BV_T) sh.w[e] = sh.w_old[e] + stp * sh.d[e];
      f = loss_grad(sh, x, y, n, D, K, l2, resid);
      ++nfev, ++evals;
      double acc = 0.0;
      for (int e = t; e < E; e += BV_T) acc += sh.g[e] * sh.d[e];
      gd = block_sum(acc, sh.red);
      const int task = ls.step(f, gd);
      if (task == 1) break;
      if (task == 2) {
        status = 3;
        break;
      }
    }
    max_ls = evals > max_ls ? evals : max_ls;
    if (status >= 0) break;
    ++it;
    double gm = 0.0;
    for (int e = t; e < E; e += BV_T) gm = fmax(gm, fabs(sh.g[e]));
    if (block_max(gm, sh.red) <= tol) {
      status = 0;
      break;
    }
    if (f_old - f <= 64.0 * BV_EPS * max3(fabs(f_old), fabs(f), 1.0)) {
      status = 1;
      break;
    }
    double rrp = 0.0;
    for (int e = t; e < E; e += BV_T) {
      const double yv = sh.g[e] - sh.g_old[e];
      rrp += yv * yv;
    }
    const double rr = block_sum(rrp, sh.red);
    const double dr = (gd - gd_old) * stp;
    if (dr > BV_EPS * (-gd_old * stp)) {
      int slot;
      if (count == BV_PAIRS) {
        slot = head;
        head = (head + 1) % BV_PAIRS;
      } else {
        slot = (head + count) % BV_PAIRS;
        ++count;
      }
      for (int e = t; e < E; e += BV_T) {
        hs[slot * E + e] = stp * sh.d[e];
        hy[slot * E + e] = sh.g[e] - sh.g_old[e];
      }
      __syncthreads();  // every lane has read the pairs' scalars of this iteration
      if (t == 0) sh.ys[slot] = dr;
      __syncthreads();
      theta = rr / dr;
    }
    if (it >= max_iter) status = 2;
  }
  __syncthreads();
  for (int e = t; e < E; e += BV_T) {
    const int k = e / D1, d = e - k * D1;
    if (d < D) coef[k * D + d] = sh.w[e];
    else intercept[k] = sh.w[e];
  }
  if (t == 0) {
    info[0] = it, info[1] = nfev, info[2] = status, info[3] = max_ls;
    loss_out[0] = f;
  }
}

// ------------------------------------------------------------------ predictions
__global__ void zero_one_kernel(int* p) { p[0] = 0; }

// One thread per row: the K decisions x . coef[k] + intercept[k] (the sum over d in ascending order),
// the first maximum as np.argmax takes it, and the rows predicted as labelled counted with one
// integer atomic per wave.
__global__ __launch_bounds__(256) void logreg_predict_kernel(const double* __restrict__ x,
                                                             const int* __restrict__ labels, const int points,
                                                             const int D, const int K,
                                                             const double* __restrict__ coef,
                                                             const double* __restrict__ intercept,
                                                             int* __restrict__ correct, double* __restrict__ dec,
                                                             int* __restrict__ pred) {
  __shared__ double w[BV_MAXK * BV_MAXD], b[BV_MAXK];
  for (int e = threadIdx.x; e < K * D; e += 256) w[e] = coef[e];
  if (threadIdx.x < K) b[threadIdx.x] = intercept[threadIdx.x];
  __syncthreads();
  const int p = blockIdx.x * 256 + threadIdx.x;
  bool hit = false;
  if (p < points) {
    double z[BV_MAXK];
#pragma unroll
    for (int k = 0; k < BV_MAXK; ++k) z[k] = 0.0;
    const double* xp = x + (long)p * D;
    for (int d = 0; d < D; ++d) {
      const double xv = xp[d];
#pragma unroll
      for (int k = 0; k < BV_MAXK; ++k)
        if (k < K) z[k] += xv * w[k * D + d];
    }
    int best = 0;
    double zb = -INFINITY;
#pragma unroll
    for (int k = 0; k < BV_MAXK; ++k)
      if (k < K) {
        z[k] += b[k];
        if (dec) dec[(long)p * K + k] = z[k];
        if (k == 0 || z[k] > zb) zb = z[k], best = k;
      }
    if (pred) pred[p] = best;
    hit = best == labels[p];
  }
  const unsigned long long m = __ballot(hit);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(correct, __popcll(m));
}

}  // namespace

extern "C" int encdiff_beta_features(const float* codes, int n_rows, int dims, const int* idx1, const int* idx2,
                                     int points, int batch, double* out, void* stream) {
  if (!codes || !idx1 || !idx2 || !out) return ENCDIFF_ERR_ARG;
  if (n_rows <= 0 || dims < 1 || dims > BV_MAXD || points < 1 || batch < 2 || batch > 64) return ENCDIFF_ERR_SHAPE;
  if ((long)points * batch >= (1L << 31) || (long)points * dims >= (1L << 31)) return ENCDIFF_ERR_SHAPE;
  const long total = (long)points * dims;
  hipLaunchKernelGGL(beta_features_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     codes, n_rows, dims, idx1, idx2, points, batch, out);
  ED_CHECK_LAUNCH();
  return ENCDIFF_OK;
}

extern "C" int encdiff_logreg_workspace(int n, int dims, int classes, long long* bytes) {
  if (!bytes) return ENCDIFF_ERR_ARG;
  if (n < 1 || n > ENCDIFF_LOGREG_MAX_ROWS || dims < 1 || dims > BV_MAXD || classes < 3 || classes > BV_MAXK)
    return ENCDIFF_ERR_SHAPE;
  *bytes = 8LL * ((long long)n * classes + 2LL * BV_PAIRS * classes * (dims + 1));
  return ENCDIFF_OK;
}

extern "C" int encdiff_logreg_fit(const double* x, const int* y, int n, int dims, int classes, double C, int max_iter,
                                  double tol, void* workspace, double* coef, double* intercept, int* info,
                                  double* loss, void* stream) {
  if (!x || !y || !workspace || !coef || !intercept || !info || !loss) return ENCDIFF_ERR_ARG;
  if (((unsigned long long)workspace & 7) != 0) return ENCDIFF_ERR_ARG;
  if (n < 1 || n > ENCDIFF_LOGREG_MAX_ROWS || dims < 1 || dims > BV_MAXD || classes < 3 || classes > BV_MAXK ||
      max_iter < 1 || max_iter > 1000 || !(C > 0.0) || !(tol >= 0.0))
    return ENCDIFF_ERR_SHAPE;
  hipLaunchKernelGGL(logreg_fit_kernel, dim3(1), dim3(BV_T), 0, (hipStream_t)stream, x, y, n, dims, classes,
                     1.0 / (C * (double)n), max_iter, tol, (double*)workspace, coef, intercept, info, loss);
  ED_CHECK_LAUNCH();
  return ENCDIFF_OK;
}

extern "C" int encdiff_logreg_predict(const double* x, const int* labels, int points, int dims, int classes,
                                      const double* coef, const double* intercept, int* correct, double* decisions,
                                      int* pred, void* stream) {
  if (!x || !labels || !coef || !intercept || !correct) return ENCDIFF_ERR_ARG;
  if (points < 1 || points >= (1 << 24) || dims < 1 || dims > BV_MAXD || classes < 1 || classes > BV_MAXK)
    return ENCDIFF_ERR_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(zero_one_kernel, dim3(1), dim3(1), 0, s, correct);
  ED_CHECK_LAUNCH();
  hipLaunchKernelGGL(logreg_predict_kernel, dim3((points + 255) / 256), dim3(256), 0, s, x, labels, points, dims,
                     classes, coef, intercept, correct, decisions, pred);
  ED_CHECK_LAUNCH();
  return ENCDIFF_OK;
}
