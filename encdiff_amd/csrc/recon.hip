// Reconstruction scores of recon_metrics.py: per image the mean SSIM (calculate_ssim: 11 x 11
// Gaussian window, zero padding 5, C1 = 0.01^2, C2 = 0.03^2) and the mean squared difference
// (calculate_mse) of two float32 image batches, read in place through element strides.
//
// The reference forms the five windowed moments conv(a), conv(b), conv(a a), conv(b b), conv(a b)
// in float32 and subtracts mu^2 from the second moments there, which cancels on flat regions.
// Here the inputs and the 121 window weights stay the float32 values the reference has, and
// everything after them is fp64: the products w a, a a, a b are exact in fp64 (24 x 24 bits), the
// sums round once per tap.
//
// A workgroup of 256 lanes owns a TH x TW tile of one (image, channel) plane, one pixel a lane; the
// tile shape is picked per launch (recon_pick) so that a plane narrower than the window does not
// idle most lanes.  The tile and a 5-pixel halo of both images are staged once in LDS as mapped
// float32 pairs {a, b}: every global element is read once per tile, and a tap is one 8-byte LDS read.
//
// Conventions of metrics.hip: fp64 sums in a fixed order (LDS trees, then partials in index order),
// no atomics, no memset, no read-back and no allocation: graph-capturable, a second launch gives
// the same bits.
#include "common.h"

namespace {

constexpr int RC_W = ENCDIFF_SSIM_WINDOW;  // 11
constexpr int RC_R = RC_W / 2;             // 5: halo and zero padding
constexpr int RC_T = 256;                  // lanes = pixels of a tile

struct ReconK {
  const float *a, *b, *window;
  long long sa[4], sb[4];
  int ch, h, w, tiles_x, tiles;
  float pre_add, pre_mul;
  double* partial;
};

// Tile shapes (rows x columns, 256 pixels each).  The one that covers the plane with the fewest
// tiles is taken, the square one on a tie (the smallest halo).
constexpr int RC_SHAPES = 3;
constexpr int RC_TH[RC_SHAPES] = {16, 64, 4};
constexpr int RC_TW[RC_SHAPES] = {16, 4, 64};

int recon_pick(const int h, const int w, int* tiles_x, int* tiles) {
  int best = 0;
  long best_n = 0;
  for (int s = 0; s < RC_SHAPES; ++s) {
    const long tx = ((long)w + RC_TW[s] - 1) / RC_TW[s], ty = ((long)h + RC_TH[s] - 1) / RC_TH[s];
    if (s == 0 || tx * ty < best_n) {
      best = s;
      best_n = tx * ty;
      *tiles_x = (int)tx;
      *tiles = (int)(tx * ty);
    }
  }
  return best;
}

// Keeps a result opaque, so that -ffp-contract=fast cannot fuse the sum into the product that
// follows: torch rounds (x + 1.) and the division by 2. separately.
ED_DEV float opaque(float x) {
  asm volatile("" : "+v"(x));
  return x;
}

// Sum of one value per lane in a fixed order (the same tree whatever the data); the result in lane 0.
ED_DEV double block_sum(double v, double* red, const int t) {
  red[t] = v;
  __syncthreads();
#pragma unroll
  for (int o = RC_T / 2; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  return red[0];
}

// grid = planes x tiles, tile fastest.  LDS row stride LW: for the tiles narrower than 32 columns a
// 32-lane group of a ds_read_b64 spans several tile rows; with LW = TW + 32 pairs those rows start
// 2 TW dwords apart modulo 64 banks, so the group's 32 pairs fall on 64 different banks.
template <int TH, int TW>
__global__ __launch_bounds__(RC_T) void recon_tile_kernel(const ReconK k) {
  static_assert(TH * TW == RC_T, "one pixel a lane");
  constexpr int LH = TH + 2 * RC_R, LU = TW + 2 * RC_R, LW = TW < 32 ? TW + 32 : LU;
  static_assert(LW >= LU, "halo fits the row stride");
  __shared__ float2 img[LH * LW];
  __shared__ double win[RC_W * RC_W];
  __shared__ double red[RC_T];
  const int t = threadIdx.x;
  const int tile = (int)(blockIdx.x % (unsigned)k.tiles);
  const long plane = blockIdx.x / (unsigned)k.tiles;
  const int c = (int)(plane % k.ch);
  const long i = plane / k.ch;
  const int y0 = (tile / k.tiles_x) * TH, x0 = (tile % k.tiles_x) * TW;
  const float* pa = k.a + i * k.sa[0] + c * k.sa[1];
  const float* pb = k.b + i * k.sb[0] + c * k.sb[1];

  for (int e = t; e < RC_W * RC_W; e += RC_T) win[e] = (double)k.window[e];
  for (int e = t; e < LH * LU; e += RC_T) {
    const int r = e / LU, q = e - r * LU;
    const int gy = y0 - RC_R + r, gx = x0 - RC_R + q;
    float2 v = make_float2(0.f, 0.f);  // the zero padding: outside the plane nothing is read or mapped
    if (gy >= 0 && gy < k.h && gx >= 0 && gx < k.w) {
      v.x = opaque(opaque(pa[gy * k.sa[2] + gx * k.sa[3]] + k.pre_add) * k.pre_mul);
      v.y = opaque(opaque(pb[gy * k.sb[2] + gx * k.sb[3]] + k.pre_add) * k.pre_mul);
    }
    img[r * LW + q] = v;
  }
  __syncthreads();

  const int ty = t / TW, tx = t % TW;
  double ssim = 0.0, sq = 0.0;
  if (y0 + ty < k.h && x0 + tx < k.w) {
    double m1 = 0.0, m2 = 0.0, s11 = 0.0, s22 = 0.0, s12 = 0.0;
    for (int dy = 0; dy < RC_W; ++dy) {
      const float2* row = img + (ty + dy) * LW + tx;
#pragma unroll
      for (int dx = 0; dx < RC_W; ++dx) {
        const float2 v = row[dx];
        const double w = win[dy * RC_W + dx], a = (double)v.x, b = (double)v.y;
        const double wa = w * a, wb = w * b;  // exact
        m1 += wa;
        m2 += wb;
        s11 = __builtin_fma(wa, a, s11);
        s22 = __builtin_fma(wb, b, s22);
        s12 = __builtin_fma(wa, b, s12);
      }
    }
    const double C1 = 0.0001, C2 = 0.0009;  // 0.01 ** 2 and 0.03 ** 2 as Python evaluates them
    // sigma = E[xy] - mu_x mu_y with the product exact inside the FMA: one rounding where the
    // reference's float32 difference cancels; the three are bitwise equal when a == b
    const double v11 = __builtin_fma(-m1, m1, s11), v22 = __builtin_fma(-m2, m2, s22), v12 = __builtin_fma(-m1, m2, s12);
    const double num = (2.0 * (m1 * m2) + C1) * (2.0 * v12 + C2);
    const double den = (m1 * m1 + m2 * m2 + C1) * (v11 + v22 + C2);
    ssim = num / den;
    const float2 v = img[(ty + RC_R) * LW + tx + RC_R];
    const double d = (double)v.x - (double)v.y;
    sq = d * d;
  }
  const double ssim_sum = block_sum(ssim, red, t);
  __syncthreads();  // red[0] read by every lane before it is rewritten
  const double sq_sum = block_sum(sq, red, t);
  if (t == 0) {
    k.partial[2 * (long)blockIdx.x] = ssim_sum;
    k.partial[2 * (long)blockIdx.x + 1] = sq_sum;
  }
}

// grid = images.  A lane adds every 256th partial of the image in index order, the lanes meet in
// the fixed tree; both means divide by the ch * h * w pixels of the image.
__global__ __launch_bounds__(RC_T) void recon_mean_kernel(const double* __restrict__ partial, const long per_image,
                                                          const double pixels, double* __restrict__ ssim,
                                                          double* __restrict__ mse) {
  __shared__ double red[RC_T];
  const int t = threadIdx.x;
  const double* p = partial + 2 * per_image * blockIdx.x;
  double s = 0.0, q = 0.0;
  for (long j = t; j < per_image; j += RC_T) {
    s += p[2 * j];
    q += p[2 * j + 1];
  }
  const double ssim_sum = block_sum(s, red, t);
  __syncthreads();
  const double sq_sum = block_sum(q, red, t);
  if (t == 0) {
    ssim[blockIdx.x] = ssim_sum / pixels;
    mse[blockIdx.x] = sq_sum / pixels;
  }
}

// every axis >= 1 and fewer than 2^31 elements (checked factor by factor: no product overflows)
int recon_shape(const EncdiffReconArgs* p) {
  if (p->n < 1 || p->ch < 1 || p->h < 1 || p->w < 1) return ENCDIFF_ERR_SHAPE;
  long long e = p->n;
  for (const int f : {p->ch, p->h, p->w}) {
    e *= f;
    if (e >= 2147483648LL) return ENCDIFF_ERR_SHAPE;
  }
  return ENCDIFF_OK;
}

int recon_check(const EncdiffReconArgs* p) {
  if (!p || !p->a || !p->b || !p->window || !p->partial || !p->ssim || !p->mse) return ENCDIFF_ERR_ARG;
  return recon_shape(p);
}

}  // namespace

extern "C" int encdiff_ssim_mse_workspace(const EncdiffReconArgs* p, long long* bytes) {
  if (!p || !bytes) return ENCDIFF_ERR_ARG;
  if (recon_shape(p) != ENCDIFF_OK) return ENCDIFF_ERR_SHAPE;
  int tiles_x, tiles;
  recon_pick(p->h, p->w, &tiles_x, &tiles);
  *bytes = (long long)p->n * p->ch * tiles * 2 * (long long)sizeof(double);
  return ENCDIFF_OK;
}

extern "C" int encdiff_ssim_mse(const EncdiffReconArgs* p, void* stream) {
  const int rc = recon_check(p);
  if (rc != ENCDIFF_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  ReconK k;
  k.a = p->a, k.b = p->b, k.window = p->window;
  for (int d = 0; d < 4; ++d) k.sa[d] = p->sa[d], k.sb[d] = p->sb[d];
  k.ch = p->ch, k.h = p->h, k.w = p->w;
  k.pre_add = p->pre_add, k.pre_mul = p->pre_mul;
  k.partial = p->partial;
  const int shape = recon_pick(p->h, p->w, &k.tiles_x, &k.tiles);
  // at most one tile per pixel: below 2^31 workgroups
  const unsigned blocks = (unsigned)((long long)p->n * p->ch * k.tiles);
  if (shape == 0)
    hipLaunchKernelGGL((recon_tile_kernel<16, 16>), dim3(blocks), dim3(RC_T), 0, s, k);
  else if (shape == 1)
    hipLaunchKernelGGL((recon_tile_kernel<64, 4>), dim3(blocks), dim3(RC_T), 0, s, k);
  else
    hipLaunchKernelGGL((recon_tile_kernel<4, 64>), dim3(blocks), dim3(RC_T), 0, s, k);
  ED_CHECK_LAUNCH();
  hipLaunchKernelGGL(recon_mean_kernel, dim3((unsigned)p->n), dim3(RC_T), 0, s, (const double*)p->partial,
                     (long)p->ch * k.tiles, (double)p->ch * (double)p->h * (double)p->w, p->ssim, p->mse);
  ED_CHECK_LAUNCH();
  return ENCDIFF_OK;
}
