#pragma once
// gemm_plan.h -- host only: the WGL / WG3 eligibility checks, the launchers of every kernel, the
// TILES table, halo geometry, GemmPlan and prepare() (the validation of every launch), and the
// paired launchers.  Builds on gemm_tile.h, gemm_finalize.h, gemm_wg3.h and gemm_wgl.h.
#include <cstdlib>

#include "gemm_finalize.h"
#include "gemm_tile.h"
#include "gemm_wg3.h"
#include "gemm_wgl.h"

namespace {
int wgl_check(const EncdiffGemmArgs& p) {
  if (p.a_mode != ENCDIFF_OPA_ROWM || p.b_mode != ENCDIFF_OPB_ROWN) return ENCDIFF_ERR_UNSUPPORTED;
  if (p.c_mode != ENCDIFF_OUT_F32 && p.c_mode != ENCDIFF_OUT_F32_ACCUM) return ENCDIFF_ERR_UNSUPPORTED;
  if (p.M % 64 || p.N % 64 || p.split_k < 1 || p.K % (p.split_k * 128)) return ENCDIFF_ERR_SHAPE;
  if (p.lda % 8 || p.ldb % 8 || ((uintptr_t)p.a & 15) || ((uintptr_t)p.b & 15)) return ENCDIFF_ERR_SHAPE;
  if (p.split_k > 1 ? ((uintptr_t)p.workspace & 15) != 0 : (p.ldc % 4 || ((uintptr_t)p.c & 15))) return ENCDIFF_ERR_SHAPE;
  return ENCDIFF_OK;
}

hipError_t wgl_launch(const EncdiffGemmArgs& p, const EncdiffGemmArgs& pf, int nf, hipStream_t s) {
  constexpr size_t lds = wgl_lds<WGL_NS>();
  static const hipError_t attr_ok =
      hipFuncSetAttribute((const void*)wgradlin_kernel<WGL_NS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (attr_ok != hipSuccess) return attr_ok;
  const int nblk = (p.M / 64) * (p.N / 64) * p.split_k;
  hipLaunchKernelGGL((wgradlin_kernel<WGL_NS>), dim3((unsigned)(nblk + nf)), dim3(256), lds, s, p, nblk, pf, nf, p,
                     GemmAux{}, 0, 0);
  return hipGetLastError();
}

// eligibility of a prepared weight-gradient plan for the WG3 kernel
int wg3_check(const EncdiffGemmArgs& p) {
  const EncdiffConvGeom& g = p.conv;
  if (p.a_mode != ENCDIFF_OPA_ROWM || p.b_mode != ENCDIFF_OPB_IM2COL) return ENCDIFF_ERR_UNSUPPORTED;
  if (g.resample != ENCDIFF_RESAMPLE_NONE && g.resample != ENCDIFF_RESAMPLE_UP2) return ENCDIFF_ERR_UNSUPPORTED;
  if (g.h != g.w || (g.w != 4 && g.w != 8 && g.w != 16)) return ENCDIFF_ERR_UNSUPPORTED;
  if (p.M % 32 || g.cin % 16 || p.N != 9 * g.cin || (long)p.K != (long)g.batch * g.h * g.w) return ENCDIFF_ERR_SHAPE;
  if (p.c_mode != ENCDIFF_OUT_F32 && p.c_mode != ENCDIFF_OUT_F32_ACCUM) return ENCDIFF_ERR_UNSUPPORTED;
  const int ni = g.w == 16 ? 1 : 2, rows = g.w == 4 ? 4 : 2;
  if (p.split_k < 1 || g.batch % p.split_k || (g.batch / p.split_k) % ni) return ENCDIFF_ERR_SHAPE;
  const int nst = (g.batch / p.split_k / ni) * (g.h / rows);  // 32-pixel stages per chunk
  if (nst % wg3_waves(p.tile)) return ENCDIFF_ERR_SHAPE;
  if (p.lda % 8 || g.ld_src % 8 || ((uintptr_t)p.a & 15) || ((uintptr_t)p.b & 15)) return ENCDIFF_ERR_SHAPE;
  // float4 epilogue stores: slabs or C itself 16-byte aligned
  if (p.split_k > 1 ? ((uintptr_t)p.workspace & 15) != 0 : (p.ldc % 4 || ((uintptr_t)p.c & 15))) return ENCDIFF_ERR_SHAPE;
  return ENCDIFF_OK;
}

template <int W, bool UP, int NS, int WPG>
hipError_t wg3_launch_t(const EncdiffGemmArgs& p, const EncdiffGemmArgs& pf, int nf, hipStream_t s) {
  constexpr size_t lds = wg3_lds<W, NS, WPG>();
  static const hipError_t attr_ok = hipFuncSetAttribute((const void*)wgrad3x3_kernel<W, UP, NS, WPG>,
                                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (attr_ok != hipSuccess) return attr_ok;
  const int nblk = (p.M / 32) * (p.conv.cin / 16) * p.split_k;
  hipLaunchKernelGGL((wgrad3x3_kernel<W, UP, NS, WPG>), dim3((unsigned)(nblk + nf)), dim3(WPG * 64), lds, s, p, nblk, pf,
                     nf, p, GemmAux{}, 0, 0);
  return hipGetLastError();
}

template <int WPG>
hipError_t wg3_launch_w(const EncdiffGemmArgs& p, const EncdiffGemmArgs& pf, int nf, hipStream_t s) {
  const bool up = p.conv.resample == ENCDIFF_RESAMPLE_UP2;
  switch (p.conv.w) {
    case 4: return up ? wg3_launch_t<4, true, 3, WPG>(p, pf, nf, s) : wg3_launch_t<4, false, 3, WPG>(p, pf, nf, s);
    case 8: return up ? wg3_launch_t<8, true, 3, WPG>(p, pf, nf, s) : wg3_launch_t<8, false, 3, WPG>(p, pf, nf, s);
    default: return up ? wg3_launch_t<16, true, 3, WPG>(p, pf, nf, s) : wg3_launch_t<16, false, 3, WPG>(p, pf, nf, s);
  }
}

hipError_t wg3_launch(const EncdiffGemmArgs& p, int tile, const EncdiffGemmArgs& pf, int nf, hipStream_t s) {
  if (tile == 33) {
    // 8-wave workgroups: a riding finalize would reach gemm_finalize's barriers after waves 4-7
    // returned (a barrier after a divergent exit) -- run it as a launch of its own instead
    if (nf > 0) {
      hipLaunchKernelGGL(gemm_finalize_kernel, dim3((unsigned)nf), dim3(256), 0, s, pf);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
    }
    return wg3_launch_w<8>(p, pf, 0, s);
  }
  return wg3_launch_w<4>(p, pf, nf, s);
}

template <int BM, int BN, int AM, int BMD, int NS = 2, int KB = BK>
hipError_t launch_t(const EncdiffGemmArgs& p, const GemmAux& aux, hipStream_t s) {
  using G = Gemm<BM, BN, AM, BMD, NS, KB>;
  const size_t lds = G::LDS_BYTES;
  // dynamic LDS above 64 KiB must be opted in once per instantiation (thread-safe static init)
  static const hipError_t attr_ok = hipFuncSetAttribute(
      (const void*)gemm_kernel<BM, BN, AM, BMD, NS, KB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (attr_ok != hipSuccess) return attr_ok;
  dim3 grid((p.M + BM - 1) / BM, (p.N + BN - 1) / BN, p.split_k);
  hipLaunchKernelGGL((gemm_kernel<BM, BN, AM, BMD, NS, KB>), grid, dim3(256), lds, s, p, aux);
  return hipGetLastError();
}

// GroupNorm-in-staging forward conv (EncdiffGemmArgs.agn_*): 64x64 tiles, 2-deep ring, the
// per-(image, channel) coefficient table behind the ring in dynamic LDS
constexpr size_t AGN_LDS_MAX = 156 * 1024;

// dynamic LDS of the AGN kernel: prepare() refuses a problem whose table does not fit, launch_agn
// allocates the same figure
size_t agn_lds_bytes(const EncdiffGemmArgs& p) {
  using G = Gemm<64, 64, A_IM2COL_GN, B_ROWK, 2, BK>;
  const int hw = p.conv.h * p.conv.w;
  const int nimg = (63 / hw + 2) < p.conv.batch ? 63 / hw + 2 : p.conv.batch;  // images one 64-row tile reads
  return (size_t)G::LDS_BYTES + (size_t)nimg * p.conv.cin * 8;
}

hipError_t launch_agn(const EncdiffGemmArgs& p, const GemmAux& aux, hipStream_t s) {
  const size_t lds = agn_lds_bytes(p);
  static const hipError_t attr_ok = hipFuncSetAttribute((const void*)gemm_kernel<64, 64, A_IM2COL_GN, B_ROWK, 2, BK>,
                                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)AGN_LDS_MAX);
  if (attr_ok != hipSuccess) return attr_ok;
  if (lds > AGN_LDS_MAX) return hipErrorInvalidValue;  // prepare() refused it already
  dim3 grid((p.M + 63) / 64, (p.N + 63) / 64, p.split_k);
  hipLaunchKernelGGL((gemm_kernel<64, 64, A_IM2COL_GN, B_ROWK, 2, BK>), grid, dim3(256), lds, s, p, aux);
  return hipGetLastError();
}

// LayerNorm-in-staging linear (EncdiffGemmArgs.lna_*): 64x64 tiles, 2-deep ring, row statistics
// and gamma / beta behind the ring in dynamic LDS
hipError_t launch_lna(const EncdiffGemmArgs& p, const GemmAux& aux, hipStream_t s) {
  using G = Gemm<64, 64, A_ROWK_LN, B_ROWK, 2, BK>;
  const size_t lds = (size_t)G::LDS_BYTES + 64 * 8 + (size_t)p.K * 8;
  static const hipError_t attr_ok = hipFuncSetAttribute((const void*)gemm_kernel<64, 64, A_ROWK_LN, B_ROWK, 2, BK>,
                                                        hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024);
  if (attr_ok != hipSuccess) return attr_ok;
  if (lds > 156 * 1024) return hipErrorInvalidValue;
  dim3 grid((p.M + 63) / 64, (p.N + 63) / 64, p.split_k);
  hipLaunchKernelGGL((gemm_kernel<64, 64, A_ROWK_LN, B_ROWK, 2, BK>), grid, dim3(256), lds, s, p, aux);
  return hipGetLastError();
}

// halo tiles: ids 16..23, 3-deep B ring, window + ring in dynamic LDS
constexpr int HALO_NS = 3;
constexpr int HALO_LDS_MAX = 156 * 1024;  // 160 KiB less the paired kernel's static finalize scratch

// EncdiffGemmArgs.tile -> the shape of the single-GEMM tile kernel, stated ONCE: the dispatch
// (launch_tile), the halo geometry, the ln_y check and encdiff_gemm_tile_shape all read it.
// Ids without a row (bm == 0) are no tile shapes: 32-34 / 36 name the WG3 / WGL kernels.
struct TileDims { int bm, bn, kb, ns; };
constexpr int TILE_IDS = 24;
constexpr TileDims TILES[TILE_IDS] = {
    {},                                                                      // 0: auto (pick_tile)
    {128, 128, BK, 2}, {128, 64, BK, 2}, {64, 128, BK, 2}, {64, 64, BK, 2},  // 1-4: ring tiles
    {64, 64, BK, 4}, {64, 128, BK, 3}, {64, 64, 128, 2}, {64, 128, 128, 2},  // 5-8
    {64, 64, BK, 6}, {64, 64, BK, 8},                                        // 9, 10
    {}, {}, {}, {}, {},                                                      // 11-15
    {64, 64, BK, HALO_NS}, {128, 64, BK, HALO_NS}, {128, 128, BK, HALO_NS}, {256, 32, BK, HALO_NS},  // 16-19: halo tiles
    {128, 32, BK, HALO_NS}, {256, 64, BK, HALO_NS}, {64, 128, BK, HALO_NS}, {64, 32, BK, HALO_NS},   // 20-23
};
constexpr bool is_tile(int t) { return t > 0 && t < TILE_IDS && TILES[t].bm != 0; }

inline size_t halo_lds_bytes(const HaloGeom& h, int bm, int bn) {
  const size_t win = (size_t)h.chunks * 16 + (size_t)HALO_NS * bn * BK * 2;
  const size_t epi = (size_t)bm * (bn + 4) * 4;
  return win > epi ? win : epi;
}

template <int BM, int BN, int BMD>
hipError_t launch_halo_t(const EncdiffGemmArgs& p, const GemmAux& aux, hipStream_t s) {
  static const hipError_t attr_ok = hipFuncSetAttribute(
      (const void*)gemm_kernel<BM, BN, A_HALO, BMD, HALO_NS, BK>, hipFuncAttributeMaxDynamicSharedMemorySize, HALO_LDS_MAX);
  if (attr_ok != hipSuccess) return attr_ok;
  dim3 grid(p.M / BM, (p.N + BN - 1) / BN, p.split_k);
  hipLaunchKernelGGL((gemm_kernel<BM, BN, A_HALO, BMD, HALO_NS, BK>), grid, dim3(256), halo_lds_bytes(aux.halo, BM, BN), s,
                     p, aux);
  return hipGetLastError();
}

// the tile kernel of id T (a row of TILES) on operand modes AM x BMD (halo tiles: A_HALO x BMD)
template <int T, int AM, int BMD>
hipError_t launch_tile(const EncdiffGemmArgs& p, const GemmAux& aux, hipStream_t s) {
  constexpr TileDims t = TILES[T];
  static_assert(is_tile(T), "tile id without a shape");
  if constexpr (T >= 16) {
    static_assert(t.kb == BK && t.ns == HALO_NS, "halo tiles: one stage depth, one ring depth");
    return launch_halo_t<t.bm, t.bn, BMD>(p, aux, s);
  } else {
    return launch_t<t.bm, t.bn, AM, BMD, t.ns, t.kb>(p, aux, s);
  }
}

template <int BMD>
hipError_t launch_halo(const EncdiffGemmArgs& p, const GemmAux& aux, int tile, hipStream_t s) {
  switch (tile) {
    case 16: return launch_tile<16, A_HALO, BMD>(p, aux, s);
    case 17: return launch_tile<17, A_HALO, BMD>(p, aux, s);
    case 18: return launch_tile<18, A_HALO, BMD>(p, aux, s);
    case 19: return launch_tile<19, A_HALO, BMD>(p, aux, s);
    case 20: return launch_tile<20, A_HALO, BMD>(p, aux, s);
    case 21: return launch_tile<21, A_HALO, BMD>(p, aux, s);
    case 22: return launch_tile<22, A_HALO, BMD>(p, aux, s);
    default: return launch_tile<23, A_HALO, BMD>(p, aux, s);
  }
}

template <int AM, int BMD>
hipError_t launch_modes(const EncdiffGemmArgs& p, const GemmAux& aux, int tile, hipStream_t s) {
  if constexpr (AM == A_IM2COL && (BMD == B_ROWK || BMD == B_CONVD)) {
    if (tile >= 16) return launch_halo<BMD>(p, aux, tile, s);
  }
  switch (tile) {
    case 1: return launch_tile<1, AM, BMD>(p, aux, s);
    case 2: return launch_tile<2, AM, BMD>(p, aux, s);
    case 3: return launch_tile<3, AM, BMD>(p, aux, s);
    case 5: return launch_tile<5, AM, BMD>(p, aux, s);
    case 6: return launch_tile<6, AM, BMD>(p, aux, s);
    case 7: return launch_tile<7, AM, BMD>(p, aux, s);
    case 8: return launch_tile<8, AM, BMD>(p, aux, s);
    case 9: return launch_tile<9, AM, BMD>(p, aux, s);
    case 10: return launch_tile<10, AM, BMD>(p, aux, s);
    default: return launch_tile<4, AM, BMD>(p, aux, s);
  }
}

FDiv make_fdiv(int d) {
  FDiv f;
  f.d = d > 0 ? (uint32_t)d : 1u;
  f.mul = (1ull << 40) / f.d + 1;
  f.pad_ = 0;
  return f;
}

int pick_tile(const EncdiffGemmArgs& p) {
  int bm = (p.M <= 64) ? 64 : 128;
  int bn = (p.N <= 64) ? 64 : 128;
  auto blocks = [&](int a, int b) { return ((p.M + a - 1) / a) * ((p.N + b - 1) / b) * p.split_k; };
  if (blocks(bm, bn) < 512 && bm == 128) bm = 64;
  if (blocks(bm, bn) < 512 && bn == 128) bn = 64;
  if (bm == 128 && bn == 128) return 1;
  if (bm == 128) return 2;
  if (bn == 128) return 3;
  return 4;
}

int gcd_i(int a, int b) { return b ? gcd_i(b, a % b) : a; }

// Halo-tile eligibility and geometry (tiles 16..23): implicit-im2col A of a 3x3 (pad 1, optional
// nearest-up), VQ stride-2 or Encoder4 k4 s2 conv forward, or a plain 3x3 input gradient;
// BM pixels = whole rows of one image or whole images; window + B ring within 160 KiB of LDS.
int prepare_halo(const EncdiffGemmArgs& p, int tile, HaloGeom& h) {
  if (tile > 23 || p.a_mode != ENCDIFF_OPA_IM2COL) return ENCDIFF_ERR_UNSUPPORTED;
  const int rs = p.conv.resample;
  if (p.b_mode == ENCDIFF_OPB_ROWK) {
    if (rs != ENCDIFF_RESAMPLE_NONE && rs != ENCDIFF_RESAMPLE_UP2 && rs != ENCDIFF_RESAMPLE_STRIDE2 &&
        rs != ENCDIFF_RESAMPLE_K4S2)
      return ENCDIFF_ERR_UNSUPPORTED;
  } else if (p.b_mode != ENCDIFF_OPB_CONV_DGRAD || rs != ENCDIFF_RESAMPLE_NONE) {
    return ENCDIFF_ERR_UNSUPPORTED;
  }
  if (p.c_mode == ENCDIFF_OUT_F32_ATOMIC || p.c_mode == ENCDIFF_OUT_F32_ATOMIC_CONVW) return ENCDIFF_ERR_UNSUPPORTED;
  // split-K: each split stages and contracts its own slice of the source channels (gemm_tile)
  if (p.split_k > 1 && (p.conv.cin % (64 * p.split_k) || p.K % 64)) return ENCDIFF_ERR_SHAPE;
  const int bm = TILES[tile].bm, bn = TILES[tile].bn;
  const int H = p.conv.h, W = p.conv.w, HW = H * W, cin = p.conv.cin;
  if ((long)p.M != (long)p.conv.batch * HW || p.M % bm || bm % W || (HW % bm && bm % HW)) return ENCDIFF_ERR_SHAPE;
  const bool up = rs == ENCDIFF_RESAMPLE_UP2, s2 = rs == ENCDIFF_RESAMPLE_STRIDE2, k4 = rs == ENCDIFF_RESAMPLE_K4S2;
  if (up && ((H | W) & 1)) return ENCDIFF_ERR_SHAPE;
  h.s = (s2 || k4) ? 2 : 1;
  h.off = s2 ? 0 : -1;
  h.kt = k4 ? 4 : 3;
  if (p.K != h.kt * h.kt * cin || cin % 8) return ENCDIFF_ERR_SHAPE;
  h.lh = h.s * H;
  h.lw = h.s * W;
  h.ush = up ? 1 : 0;
  h.hs = up ? H / 2 : h.lh;
  h.ws = up ? W / 2 : h.lw;
  const int rows = bm / W < H ? bm / W : H;
  h.ni = bm > HW ? bm / HW : 1;
  h.hr = h.s * (rows - 1) + h.kt;
  h.hc = h.s * (W - 1) + h.kt;
  h.ch = cin / 8 / p.split_k;  // the split's channel slice
  h.npix = h.ni * h.hr * h.hc;
  h.chunks = (h.npix * h.ch + 255) & ~255;
  // bank swizzle: consecutive pixels advance q 16-B slots in the 16-slot bank row; g pixels share a
  // slot position, spread them over min(g, largest power of two dividing ch) slots
  const int q = h.ch % 16, g = q ? gcd_i(q, 16) : 16;
  int pw = 1;
  while (pw < 16 && h.ch % (2 * pw) == 0) pw *= 2;
  h.xmsk = (pw < g ? pw : g) - 1;
  int xsh = 0;
  while ((1 << xsh) < 16 / g) ++xsh;
  h.xsh = xsh;
  h.fch = make_fdiv(h.ch);
  h.fimg = make_fdiv(h.hr * h.hc);
  h.fhc = make_fdiv(h.hc);
  if (halo_lds_bytes(h, bm, bn) > (size_t)HALO_LDS_MAX) return ENCDIFF_ERR_SHAPE;
  return ENCDIFF_OK;
}

// Validated launch plan of one GEMM: the arguments the tile kernel sees (split-K slabs
// redirected into the workspace), the user's arguments for the finalize pass, aux constants.
struct GemmPlan {
  EncdiffGemmArgs p, user;
  GemmAux aux;
  int tile;
  bool ws_path;
  bool fold;  // split-K slabs combined in the kernel (no finalize pass)
};

// XCD-aware tile order (xcd_remap) per problem.  Measured per call over the step's GEMMs
// (tools/gemm_calls_time.py, round 4): it pays for the weight gradients whose A operand is
// k-outer (dY^T, deep split-K over pixels: the x / dY k-slices of 8 split-K parts and 8 M tiles
// stay in one L2; the 512x64x32768 linear pairs 22.4 -> 16.9 us) and LOSES for the forward /
// input-gradient convs (M = 2048 split-4 3x3 convs 14.6 -> 21.7 us: one XCD's 64 workgroups then
// start on the same two weight tiles at once).  ENCDIFF_GEMM_XCD: 0 off, 1 every GEMM, 2 (default)
// the k-outer-A GEMMs only.
int gemm_xcd_order(const EncdiffGemmArgs& p) {
  static const int v = [] {
    const char* e = getenv("ENCDIFF_GEMM_XCD");
    return e ? atoi(e) : 2;
  }();
  return v == 1 || (v == 2 && p.a_mode == ENCDIFF_OPA_ROWM);
}

int prepare(const EncdiffGemmArgs* pa, GemmPlan& g) {
  if (!pa || pa->dtype != ENCDIFF_DT_BF16) return ENCDIFF_ERR_ARG;  // fp32: encdiff_gemm only
  EncdiffGemmArgs p = *pa;
  if (p.M <= 0 || p.N <= 0 || p.K <= 0) return ENCDIFF_ERR_SHAPE;
  if (p.split_k < 1) p.split_k = 1;
  const bool ws_path = p.split_k > 1 && (p.c_mode == ENCDIFF_OUT_BF16 || p.c_mode == ENCDIFF_OUT_F32 ||
                                         p.c_mode == ENCDIFF_OUT_F32_ACCUM);
  if (ws_path && !p.workspace) return ENCDIFF_ERR_ARG;
  const bool k_inner = p.a_mode != ENCDIFF_OPA_ROWM || p.b_mode == ENCDIFF_OPB_ROWK;
  if (k_inner && p.K % 8) return ENCDIFF_ERR_SHAPE;
  if (p.a_mode == ENCDIFF_OPA_ROWM && p.M % 8) return ENCDIFF_ERR_SHAPE;
  if (p.b_mode != ENCDIFF_OPB_ROWK && p.N % 8) return ENCDIFF_ERR_SHAPE;
  const bool im2col = p.a_mode == ENCDIFF_OPA_IM2COL || p.b_mode == ENCDIFF_OPB_IM2COL;
  if (im2col && (p.conv.cin % 8)) return ENCDIFF_ERR_SHAPE;
  // exact fdiv range (pixel indices < 2^24, divisors < 2^16) and single-load im2col modes
  if (im2col && ((long)p.conv.batch * p.conv.h * p.conv.w >= (1L << 24) || p.conv.h * p.conv.w >= (1 << 16)))
    return ENCDIFF_ERR_SHAPE;
  if (im2col && p.conv.resample == ENCDIFF_RESAMPLE_DOWN2) return ENCDIFF_ERR_UNSUPPORTED;
  if (im2col && p.conv.resample == ENCDIFF_RESAMPLE_K4S2_TP) {  // parity-major rows, one parity per tile
    if (p.a_mode != ENCDIFF_OPA_IM2COL || p.b_mode != ENCDIFF_OPB_CONV_DGRAD) return ENCDIFF_ERR_UNSUPPORTED;
    if ((p.conv.h | p.conv.w) & 1 || (long)p.M != (long)p.conv.batch * p.conv.h * p.conv.w ||
        (p.M >> 2) % 128 || p.K != 4 * p.conv.cin)
      return ENCDIFF_ERR_SHAPE;
    if (p.c_mode == ENCDIFF_OUT_F32_ATOMIC || p.c_mode == ENCDIFF_OUT_F32_ATOMIC_CONVW) return ENCDIFF_ERR_UNSUPPORTED;
  }
  if (p.K >= (1 << 24)) return ENCDIFF_ERR_SHAPE;
  {  // the staging loads address every operand by 32-bit byte offsets from its base
    const long src = (long)p.conv.batch * p.conv.h * p.conv.w * 4 * p.conv.ld_src * 2;  // im2col source
    long ea = 0, eb = 0;
    if (p.a_mode == ENCDIFF_OPA_ROWK) ea = ((long)(p.M - 1) * p.lda + p.K) * 2;
    else if (p.a_mode == ENCDIFF_OPA_ROWM) ea = ((long)(p.K - 1) * p.lda + p.M) * 2;
    else ea = src;
    if (p.b_mode == ENCDIFF_OPB_ROWK) eb = ((long)(p.N - 1) * p.ldb + p.K) * 2;
    else if (p.b_mode == ENCDIFF_OPB_ROWN) eb = ((long)(p.K - 1) * p.ldb + p.N) * 2;
    else if (p.b_mode == ENCDIFF_OPB_CONV_DGRAD) eb = ((long)p.conv_cout * p.ldb + 16L * p.N) * 2;
    else eb = src;
    if (ea >= 0x7FFFFFF0L || eb >= 0x7FFFFFF0L) return ENCDIFF_ERR_SHAPE;
  }
  if (p.bias_grad && p.a_mode != ENCDIFF_OPA_ROWM) return ENCDIFF_ERR_ARG;
  if (p.gn_stats && (p.c_mode != ENCDIFF_OUT_BF16 || p.split_k != 1 || p.M % 64 || p.ld_gn_stats < p.N))
    return ENCDIFF_ERR_ARG;
  if (p.ln_y) {  // the tile must span every column: N <= BN, 8-column vectors
    const int bn = p.tile < 16 && is_tile(p.tile) ? TILES[p.tile].bn : 64;  // ring tiles; any other id counts as 64 wide
    if (p.c_mode != ENCDIFF_OUT_BF16 || p.split_k != 1 || !p.tile || p.N > bn || p.N % 8 || p.ld_ln_y % 8 ||
        !p.ln_gamma || !p.ln_beta || !p.ln_stats)
      return ENCDIFF_ERR_ARG;
    if ((uintptr_t)p.ln_y & 15) return ENCDIFF_ERR_ARG;  // written in 16-byte vectors on every path
  }
  if (p.c_mode == ENCDIFF_OUT_BF16_GEGLU || p.c_mode == ENCDIFF_OUT_BF16_GEGLU_BWD) {
    const bool fwd = p.c_mode == ENCDIFF_OUT_BF16_GEGLU;
    if (!p.aux || p.resid || p.split_k != 1 || p.N % 8 || p.ldc % 8 || p.ld_aux % 8) return ENCDIFF_ERR_ARG;
    // both epilogues read / write aux and C in 16-byte vectors only (no scalar form)
    if (((uintptr_t)p.aux & 15) || ((uintptr_t)p.c & 15)) return ENCDIFF_ERR_ARG;
    if (fwd && (p.a_mode != ENCDIFF_OPA_ROWK || p.b_mode != ENCDIFF_OPB_ROWK || p.N % 128)) return ENCDIFF_ERR_ARG;
  }
  if (p.agn_gamma) {  // GroupNorm in the A staging: forward 3x3 conv, 64x64 tiles
    if (p.a_mode != ENCDIFF_OPA_IM2COL || p.b_mode != ENCDIFF_OPB_ROWK || p.c_mode != ENCDIFF_OUT_BF16 ||
        !p.agn_beta || p.ln_y)
      return ENCDIFF_ERR_ARG;
    if (p.conv.resample != ENCDIFF_RESAMPLE_NONE && p.conv.resample != ENCDIFF_RESAMPLE_UP2)
      return ENCDIFF_ERR_UNSUPPORTED;
    if (p.conv.cin % 32 || p.conv.cin > 1024 || p.K != 9 * p.conv.cin ||
        (long)p.M != (long)p.conv.batch * p.conv.h * p.conv.w)
      return ENCDIFF_ERR_SHAPE;
    // the coefficient table of the images one tile reads sits behind the ring (M > 0: h w > 0)
    if (agn_lds_bytes(p) > AGN_LDS_MAX) return ENCDIFF_ERR_SHAPE;
    if (p.tile != 0 && p.tile != 4) return ENCDIFF_ERR_UNSUPPORTED;
    p.tile = 4;
  }
  if (p.lna_gamma) {  // LayerNorm in the A staging: linear forward, 64x64 tiles, no split
    if (p.a_mode != ENCDIFF_OPA_ROWK || p.b_mode != ENCDIFF_OPB_ROWK || p.c_mode != ENCDIFF_OUT_BF16 ||
        !p.lna_beta || p.ln_y || p.agn_gamma || p.split_k != 1)
      return ENCDIFF_ERR_ARG;
    if (p.K % 8 || p.K > 1024 || p.lda % 8 || ((uintptr_t)p.a & 15)) return ENCDIFF_ERR_SHAPE;
    if (p.tile != 0 && p.tile != 4) return ENCDIFF_ERR_UNSUPPORTED;
    p.tile = 4;
  }
  g.tile = p.tile ? p.tile : pick_tile(p);
  g.aux.halo = HaloGeom{};
  if (g.tile >= 32 && g.tile <= 34) {  // 3x3 conv weight gradient kernel (WG3)
    const int rc = wg3_check(p);
    if (rc != ENCDIFF_OK) return rc;
  } else if (g.tile == 36) {  // linear weight gradient kernel (WGL)
    const int rc = wgl_check(p);
    if (rc != ENCDIFF_OK) return rc;
  } else if (g.tile >= 16) {
    const int rc = prepare_halo(p, g.tile, g.aux.halo);
    if (rc != ENCDIFF_OK) return rc;
  }
  g.user = p;
  g.ws_path = ws_path;
  if (ws_path) {  // per-split fp32 slabs (plain stores); epilogue in the finalize pass
    p.c = p.workspace; p.ldc = p.N; p.c_mode = ENCDIFF_OUT_F32; p.alpha = 1.f;
    p.bias = nullptr; p.resid = nullptr;
  }
  // in-kernel split-K combine: vectorised slab / output rows, plain row mapping, no bias gradient
  g.aux.fold = SplitFold{};
  g.fold = false;
  if (ws_path && p.split_counters && p.a_mode != ENCDIFF_OPA_ROWM && !p.bias_grad && p.N % 8 == 0 &&
      !(im2col && p.conv.resample == ENCDIFF_RESAMPLE_K4S2_TP) && g.user.ldc % 8 == 0 &&
      ((uintptr_t)g.user.c & 15) == 0 && ((uintptr_t)p.workspace & 15) == 0 &&
      (!g.user.bias || ((uintptr_t)g.user.bias & 15) == 0) &&
      (!g.user.resid || (g.user.ld_resid % 8 == 0 && ((uintptr_t)g.user.resid & 15) == 0))) {
    g.fold = true;
    g.aux.fold = SplitFold{p.split_counters, g.user.c, g.user.ldc, g.user.c_mode, g.user.alpha, g.user.bias,
                           (const bf16_t*)g.user.resid, g.user.ld_resid};
  }
  g.p = p;
  g.aux.xcd = gemm_xcd_order(p);
  g.aux.cin = make_fdiv(p.conv.cin);
  g.aux.cout = make_fdiv(p.conv_cout);
  const bool tp = im2col && p.conv.resample == ENCDIFF_RESAMPLE_K4S2_TP;
  g.aux.hw = make_fdiv(tp ? (p.conv.h >> 1) * (p.conv.w >> 1) : p.conv.h * p.conv.w);  // output grid
  g.aux.w = make_fdiv(tp ? p.conv.w >> 1 : p.conv.w);
  return ENCDIFF_OK;
}

int fin_blocks(const EncdiffGemmArgs& u) {
  const long total = (long)u.M * u.N;
  const long per = fin_per_block(u);
  long g = (total + per - 1) / per;
  if (u.bias_grad && (u.M + 63) / 64 > g) g = (u.M + 63) / 64;
  return (int)(g > 2048 ? 2048 : g);
}

int launch_one(const GemmPlan& g, hipStream_t s) {
  const int am = g.p.a_mode, bm = g.p.b_mode;
  hipError_t e;
  if (g.tile >= 32 && g.tile <= 34) e = wg3_launch(g.p, g.tile, g.user, 0, s);
  else if (g.tile == 36) e = wgl_launch(g.p, g.user, 0, s);
  else if (am == ENCDIFF_OPA_ROWK && bm == ENCDIFF_OPB_ROWK)
    e = g.p.lna_gamma ? launch_lna(g.p, g.aux, s) : launch_modes<A_ROWK, B_ROWK>(g.p, g.aux, g.tile, s);
  else if (am == ENCDIFF_OPA_IM2COL && bm == ENCDIFF_OPB_ROWK)
    e = g.p.agn_gamma ? launch_agn(g.p, g.aux, s) : launch_modes<A_IM2COL, B_ROWK>(g.p, g.aux, g.tile, s);
  else if (am == ENCDIFF_OPA_ROWK && bm == ENCDIFF_OPB_ROWN) e = launch_modes<A_ROWK, B_ROWN>(g.p, g.aux, g.tile, s);
  else if (am == ENCDIFF_OPA_IM2COL && bm == ENCDIFF_OPB_CONV_DGRAD)
    e = launch_modes<A_IM2COL, B_CONVD>(g.p, g.aux, g.tile, s);
  else if (am == ENCDIFF_OPA_ROWM && bm == ENCDIFF_OPB_ROWN) e = launch_modes<A_ROWM, B_ROWN>(g.p, g.aux, g.tile, s);
  else if (am == ENCDIFF_OPA_ROWM && bm == ENCDIFF_OPB_IM2COL) e = launch_modes<A_ROWM, B_IM2COL>(g.p, g.aux, g.tile, s);
  else return ENCDIFF_ERR_UNSUPPORTED;
  if (e != hipSuccess) return ENCDIFF_ERR_LAUNCH - (int)e;
  if (g.ws_path && !g.fold) {
    hipLaunchKernelGGL(gemm_finalize_kernel, dim3((unsigned)fin_blocks(g.user)), dim3(256), 0, s, g.user);
    e = hipGetLastError();
    if (e != hipSuccess) return ENCDIFF_ERR_LAUNCH - (int)e;
  }
  return ENCDIFF_OK;
}

template <int AM1, int BMD1, int BM2, int BN2, int AM2, int BMD2, int NS2 = 2, int KB2 = BK, int KB1 = BK, int NS1 = 2>
hipError_t launch_pair_t(const GemmPlan& g1, const GemmPlan& g2, const EncdiffGemmArgs& pf, int nf, hipStream_t s) {
  using G1 = Gemm<64, 64, AM1, BMD1, NS1, KB1>;
  using G2 = Gemm<BM2, BN2, AM2, BMD2, NS2, KB2>;
  constexpr size_t lds = G1::LDS_BYTES > G2::LDS_BYTES ? G1::LDS_BYTES : G2::LDS_BYTES;
  static const hipError_t attr_ok = hipFuncSetAttribute(
      (const void*)gemm2_kernel<AM1, BMD1, BM2, BN2, AM2, BMD2, NS2, KB2, KB1, NS1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (attr_ok != hipSuccess) return attr_ok;
  const int gx1 = (g1.p.M + 63) / 64, gy1 = (g1.p.N + 63) / 64;
  const int gx2 = (g2.p.M + BM2 - 1) / BM2, gy2 = (g2.p.N + BN2 - 1) / BN2;
  const long nb = (long)gx1 * gy1 * g1.p.split_k + (long)gx2 * gy2 * g2.p.split_k + nf;
  hipLaunchKernelGGL((gemm2_kernel<AM1, BMD1, BM2, BN2, AM2, BMD2, NS2, KB2, KB1, NS1>), dim3((unsigned)nb), dim3(256), lds, s, g1.p,
                     g1.aux, g2.p, g2.aux, gx1, gy1, gx2, gy2, pf, nf);
  return hipGetLastError();
}

// paired launch whose input gradient runs on a halo tile: dynamic LDS = the larger of the two
template <int AM1, int BMD1, int BM2, int BN2, int KB1>
hipError_t launch_pair_halo_t(const GemmPlan& g1, const GemmPlan& g2, const EncdiffGemmArgs& pf, int nf, hipStream_t s) {
  using G1 = Gemm<64, 64, AM1, BMD1, 2, KB1>;
  auto kern = gemm2_kernel<AM1, BMD1, BM2, BN2, A_HALO, B_CONVD, HALO_NS, BK, KB1>;
  static const hipError_t attr_ok =
      hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, HALO_LDS_MAX);
  if (attr_ok != hipSuccess) return attr_ok;
  size_t lds = halo_lds_bytes(g2.aux.halo, BM2, BN2);
  if ((size_t)G1::LDS_BYTES > lds) lds = G1::LDS_BYTES;
  const int gx1 = (g1.p.M + 63) / 64, gy1 = (g1.p.N + 63) / 64;
  const int gx2 = g2.p.M / BM2, gy2 = (g2.p.N + BN2 - 1) / BN2;
  const long nb = (long)gx1 * gy1 * g1.p.split_k + (long)gx2 * gy2 * g2.p.split_k + nf;
  hipLaunchKernelGGL(kern, dim3((unsigned)nb), dim3(256), lds, s, g1.p, g1.aux, g2.p, g2.aux, gx1, gy1, gx2, gy2, pf, nf);
  return hipGetLastError();
}

template <int AM1, int BMD1, int KB1>
hipError_t launch_pair_halo(const GemmPlan& g1, const GemmPlan& g2, const EncdiffGemmArgs& pf, int nf, hipStream_t s) {
  switch (g2.tile) {
    case 16: return launch_pair_halo_t<AM1, BMD1, 64, 64, KB1>(g1, g2, pf, nf, s);
    case 17: return launch_pair_halo_t<AM1, BMD1, 128, 64, KB1>(g1, g2, pf, nf, s);
    case 18: return launch_pair_halo_t<AM1, BMD1, 128, 128, KB1>(g1, g2, pf, nf, s);
    case 22: return launch_pair_halo_t<AM1, BMD1, 64, 128, KB1>(g1, g2, pf, nf, s);
    default: return hipErrorInvalidValue;
  }
}

template <int AM1, int BMD1, int AM2, int BMD2>
hipError_t launch_pair_tiles(const GemmPlan& g1, const GemmPlan& g2, const EncdiffGemmArgs& pf, int nf,
                             hipStream_t s) {
  if constexpr (AM2 == A_IM2COL && BMD2 == B_CONVD) {
    if (g2.tile >= 16) {
      return g1.tile == 7 ? launch_pair_halo<AM1, BMD1, 128>(g1, g2, pf, nf, s)
                          : launch_pair_halo<AM1, BMD1, BK>(g1, g2, pf, nf, s);
    }
  }
  if (g1.tile == 5) {  // weight gradient with a 4-deep ring (64 KB of LDS): every k-tile of a short split in flight
    return launch_pair_t<AM1, BMD1, 64, 64, AM2, BMD2, 2, 64, 64, 4>(g1, g2, pf, nf, s);
  }
  if (g1.tile == 9 || g1.tile == 10) {  // 6- / 8-deep rings (96 / 128 KB): one workgroup per CU, all loads in flight
    const bool d6 = g1.tile == 9;
    switch (g2.tile) {
      case 9: return d6 ? launch_pair_t<AM1, BMD1, 64, 64, AM2, BMD2, 6, 64, 64, 6>(g1, g2, pf, nf, s)
                        : launch_pair_t<AM1, BMD1, 64, 64, AM2, BMD2, 6, 64, 64, 8>(g1, g2, pf, nf, s);
      case 10: return d6 ? launch_pair_t<AM1, BMD1, 64, 64, AM2, BMD2, 8, 64, 64, 6>(g1, g2, pf, nf, s)
                         : launch_pair_t<AM1, BMD1, 64, 64, AM2, BMD2, 8, 64, 64, 8>(g1, g2, pf, nf, s);
      default: return d6 ? launch_pair_t<AM1, BMD1, 64, 64, AM2, BMD2, 2, 64, 64, 6>(g1, g2, pf, nf, s)
                         : launch_pair_t<AM1, BMD1, 64, 64, AM2, BMD2, 2, 64, 64, 8>(g1, g2, pf, nf, s);
    }
  }
  if (g1.tile == 7) {  // weight gradient with 128-deep k stages (64 KB of LDS): dgrad tile 7 or 64x64
    if (g2.tile == 7) return launch_pair_t<AM1, BMD1, 64, 64, AM2, BMD2, 2, 128, 128>(g1, g2, pf, nf, s);
    return launch_pair_t<AM1, BMD1, 64, 64, AM2, BMD2, 2, 64, 128>(g1, g2, pf, nf, s);
  }
  switch (g2.tile) {
    case 1: return launch_pair_t<AM1, BMD1, 128, 128, AM2, BMD2>(g1, g2, pf, nf, s);
    case 2: return launch_pair_t<AM1, BMD1, 128, 64, AM2, BMD2>(g1, g2, pf, nf, s);
    case 3: return launch_pair_t<AM1, BMD1, 64, 128, AM2, BMD2>(g1, g2, pf, nf, s);
    case 5: return launch_pair_t<AM1, BMD1, 64, 64, AM2, BMD2, 4>(g1, g2, pf, nf, s);
    case 6: return launch_pair_t<AM1, BMD1, 64, 128, AM2, BMD2, 3>(g1, g2, pf, nf, s);
    case 7: return launch_pair_t<AM1, BMD1, 64, 64, AM2, BMD2, 2, 128>(g1, g2, pf, nf, s);
    case 8: return launch_pair_t<AM1, BMD1, 64, 128, AM2, BMD2, 2, 128>(g1, g2, pf, nf, s);
    default: return launch_pair_t<AM1, BMD1, 64, 64, AM2, BMD2>(g1, g2, pf, nf, s);
  }
}

template <int W, bool UP, int BM2, int BN2, int AM2, int BMD2, int NS2>
hipError_t wg3pair_launch_t(const GemmPlan& g1, const GemmPlan& g2, const EncdiffGemmArgs& pf, int nf, hipStream_t s) {
  static const hipError_t attr_ok =
      hipFuncSetAttribute((const void*)wgrad3x3_kernel<W, UP, WG3_PAIR_NS, 4, BM2, BN2, AM2, BMD2, NS2>,
                          hipFuncAttributeMaxDynamicSharedMemorySize, HALO_LDS_MAX);
  if (attr_ok != hipSuccess) return attr_ok;
  size_t lds = wg3_lds<W, WG3_PAIR_NS, 4>();
  if constexpr (AM2 == A_HALO) {
    const size_t h = halo_lds_bytes(g2.aux.halo, BM2, BN2);
    if (h > lds) lds = h;
  } else {
    constexpr size_t l2 = Gemm<BM2, BN2, AM2, BMD2, NS2, BK>::LDS_BYTES;
    if (l2 > lds) lds = l2;
  }
  const int n1 = (g1.p.M / 32) * (g1.p.conv.cin / 16) * g1.p.split_k;
  const int gx2 = AM2 == A_HALO ? g2.p.M / BM2 : (g2.p.M + BM2 - 1) / BM2, gy2 = (g2.p.N + BN2 - 1) / BN2;
  const long nb = (long)n1 + (long)gx2 * gy2 * g2.p.split_k + nf;
  hipLaunchKernelGGL((wgrad3x3_kernel<W, UP, WG3_PAIR_NS, 4, BM2, BN2, AM2, BMD2, NS2>), dim3((unsigned)nb), dim3(256), lds, s,
                     g1.p, n1, pf, nf, g2.p, g2.aux, gx2, gy2);
  return hipGetLastError();
}

template <int W, bool UP>
hipError_t wg3pair_launch_w(const GemmPlan& g1, const GemmPlan& g2, const EncdiffGemmArgs& pf, int nf, hipStream_t s) {
  switch (g2.tile) {
    case 4: return wg3pair_launch_t<W, UP, 64, 64, A_IM2COL, B_CONVD, 2>(g1, g2, pf, nf, s);
    case 2: return wg3pair_launch_t<W, UP, 128, 64, A_IM2COL, B_CONVD, 2>(g1, g2, pf, nf, s);
    case 16: return wg3pair_launch_t<W, UP, 64, 64, A_HALO, B_CONVD, HALO_NS>(g1, g2, pf, nf, s);
    case 17: return wg3pair_launch_t<W, UP, 128, 64, A_HALO, B_CONVD, HALO_NS>(g1, g2, pf, nf, s);
    case 22: return wg3pair_launch_t<W, UP, 64, 128, A_HALO, B_CONVD, HALO_NS>(g1, g2, pf, nf, s);
    default: return hipErrorInvalidValue;
  }
}

// the input-gradient tiles the paired WG3 launch covers
bool wg3pair_ok(const GemmPlan& g1, const GemmPlan& g2) {
  return g1.tile == 32 && g2.p.a_mode == ENCDIFF_OPA_IM2COL && g2.p.b_mode == ENCDIFF_OPB_CONV_DGRAD &&
         (g2.tile == 4 || g2.tile == 2 || g2.tile == 16 || g2.tile == 17 || g2.tile == 22);
}

hipError_t wg3pair_launch(const GemmPlan& g1, const GemmPlan& g2, const EncdiffGemmArgs& pf, int nf, hipStream_t s) {
  const bool up = g1.p.conv.resample == ENCDIFF_RESAMPLE_UP2;
  switch (g1.p.conv.w) {
    case 4: return up ? wg3pair_launch_w<4, true>(g1, g2, pf, nf, s) : wg3pair_launch_w<4, false>(g1, g2, pf, nf, s);
    case 8: return up ? wg3pair_launch_w<8, true>(g1, g2, pf, nf, s) : wg3pair_launch_w<8, false>(g1, g2, pf, nf, s);
    default: return up ? wg3pair_launch_w<16, true>(g1, g2, pf, nf, s) : wg3pair_launch_w<16, false>(g1, g2, pf, nf, s);
  }
}

template <int BM2, int BN2, int NS2, int KB2>
hipError_t wglpair_launch_t(const GemmPlan& g1, const GemmPlan& g2, const EncdiffGemmArgs& pf, int nf, hipStream_t s) {
  using G2 = Gemm<BM2, BN2, A_ROWK, B_ROWN, NS2, KB2>;
  constexpr size_t l1 = wgl_lds<WGL_PAIR_NS>(), lds = l1 > G2::LDS_BYTES ? l1 : G2::LDS_BYTES;
  static const hipError_t attr_ok =
      hipFuncSetAttribute((const void*)wgradlin_kernel<WGL_PAIR_NS, BM2, BN2, A_ROWK, B_ROWN, NS2, KB2>,
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (attr_ok != hipSuccess) return attr_ok;
  const int n1 = (g1.p.M / 64) * (g1.p.N / 64) * g1.p.split_k;
  const int gx2 = (g2.p.M + BM2 - 1) / BM2, gy2 = (g2.p.N + BN2 - 1) / BN2;
  const long nb = (long)n1 + (long)gx2 * gy2 * g2.p.split_k + nf;
  hipLaunchKernelGGL((wgradlin_kernel<WGL_PAIR_NS, BM2, BN2, A_ROWK, B_ROWN, NS2, KB2>), dim3((unsigned)nb), dim3(256), lds,
                     s, g1.p, n1, pf, nf, g2.p, g2.aux, gx2, gy2);
  return hipGetLastError();
}

bool wglpair_ok(const GemmPlan& g1, const GemmPlan& g2) {
  return g1.tile == 36 && g2.p.a_mode == ENCDIFF_OPA_ROWK && g2.p.b_mode == ENCDIFF_OPB_ROWN && !g2.fold &&
         (g2.tile >= 1 && g2.tile <= 5 || g2.tile == 7);
}

hipError_t wglpair_launch(const GemmPlan& g1, const GemmPlan& g2, const EncdiffGemmArgs& pf, int nf, hipStream_t s) {
  switch (g2.tile) {
    case 1: return wglpair_launch_t<128, 128, 2, BK>(g1, g2, pf, nf, s);
    case 2: return wglpair_launch_t<128, 64, 2, BK>(g1, g2, pf, nf, s);
    case 3: return wglpair_launch_t<64, 128, 2, BK>(g1, g2, pf, nf, s);
    case 5: return wglpair_launch_t<64, 64, 4, BK>(g1, g2, pf, nf, s);
    case 7: return wglpair_launch_t<64, 64, 2, 128>(g1, g2, pf, nf, s);
    default: return wglpair_launch_t<64, 64, 2, BK>(g1, g2, pf, nf, s);
  }
}

hipError_t launch_finalize(const EncdiffGemmArgs& u, hipStream_t s) {
  hipLaunchKernelGGL(gemm_finalize_kernel, dim3((unsigned)fin_blocks(u)), dim3(256), 0, s, u);
  return hipGetLastError();
}
}  // namespace
