// gemm.hip -- one MFMA GEMM engine for every conv / linear of the EncDiff UNet.
//
// C[M][N] = alpha * A[M][K] * B[K][N] (+bias)(+resid), bf16 operands, fp32 accumulate,
// v_mfma_f32_16x16x32_bf16 on gfx950.  256 threads = 4 waves in a 2x2 layout, each
// wave owns a (BM/2)x(BN/2) sub-tile.  K is staged 64 at a time through
// double-buffered LDS with register staging (global_load_dwordx4 -> ds_write_b128).
//
// Operands are loaded in their natural global layout ("k-inner": rows of K,
// read as MFMA fragments with ds_read_b128; "k-outer": rows of M/N, read with the
// gfx950 transpose read ds_read_b64_tr_b16), so the same engine runs
//   forward   conv3x3  : A = implicit im2col(x) [pixels][9*Cin], B = W [Cout][9*Cin]
//   dgrad     conv3x3  : A = im2col(dY),   B = W read through a flipped-tap map
//   wgrad     conv3x3  : A = dY^T (k-outer), B = im2col(x) (k-outer), split-K, atomics
//   linear fwd / dgrad / wgrad likewise with dense operands.
// Replaces: openaimodel_enc.py:204,230,237-241,508-512,521,687; attention.py:159-167,
// 43,58,233-259 (every Conv2d / Linear forward and their autograd backward).
// The engine lives in headers private to this translation unit (gemm_common.h maps them); this
// file holds the C entry points.
#include "gemm_common.h"
#include "gemm_finalize.h"
#include "gemm_tile.h"
#include "gemm_wg3.h"
#include "gemm_wgl.h"
#include "gemm_plan.h"
#include "gemm_group.h"

extern "C" int encdiff_gemm(const EncdiffGemmArgs* pa, void* stream) {
  if (pa && pa->dtype == ENCDIFF_DT_F32) return ed_gemm_f32(pa, (hipStream_t)stream);
  if (pa && pa->dtype != ENCDIFF_DT_BF16) return ENCDIFF_ERR_ARG;
  GemmPlan g;
  const int rc = prepare(pa, g);
  if (rc != ENCDIFF_OK) return rc;
  return launch_one(g, (hipStream_t)stream);
}

extern "C" int encdiff_gemm_ex(const EncdiffGemmArgs* pa, int defer_finalize, int* planned, void* stream) {
  if (planned) *planned = 0;
  if (!defer_finalize || (pa && pa->dtype == ENCDIFF_DT_F32)) return encdiff_gemm(pa, stream);
  GemmPlan g;
  const int rc = prepare(pa, g);
  if (rc != ENCDIFF_OK) return rc;
  if (!g.ws_path || g.fold) return launch_one(g, (hipStream_t)stream);
  GemmPlan t = g;
  t.ws_path = false;  // tile kernel only: the slabs wait for the consumer
  const int r = launch_one(t, (hipStream_t)stream);
  if (r == ENCDIFF_OK && planned) *planned = 1;
  return r;
}

// encdiff_gemm_pair_ex / encdiff_gemm_pair_dx: defer_d skips the input gradient's finalize
// (*dd = 1 when it had one to skip)
static int gemm_pair_impl(const EncdiffGemmArgs* wgrad, const EncdiffGemmArgs* dgrad,
                          const EncdiffGemmArgs* prev_wgrad, int defer, bool defer_d, int* dd, void* stream) {
  *dd = 0;
  GemmPlan g1, g2, gp;
  int rc = prepare(wgrad, g1);
  if (rc != ENCDIFF_OK) return rc;
  rc = prepare(dgrad, g2);
  if (rc != ENCDIFF_OK) return rc;
  bool have_prev = false;
  if (prev_wgrad) {
    rc = prepare(prev_wgrad, gp);
    if (rc != ENCDIFF_OK) return rc;
    have_prev = gp.ws_path;
  }
  hipStream_t s = (hipStream_t)stream;
  hipError_t e;
  const int a1 = g1.p.a_mode, b1 = g1.p.b_mode, a2 = g2.p.a_mode, b2 = g2.p.b_mode;
  const bool lin = a1 == ENCDIFF_OPA_ROWM && b1 == ENCDIFF_OPB_ROWN && a2 == ENCDIFF_OPA_ROWK && b2 == ENCDIFF_OPB_ROWN;
  const bool conv = a1 == ENCDIFF_OPA_ROWM && b1 == ENCDIFF_OPB_IM2COL && a2 == ENCDIFF_OPA_IM2COL &&
                    b2 == ENCDIFF_OPB_CONV_DGRAD;
  // both split-K problems need disjoint slabs
  if (g1.ws_path && g2.ws_path && g1.p.workspace == g2.p.workspace) return ENCDIFF_ERR_ARG;
  const bool defer1 = defer && g1.ws_path;
  const bool dslabs = g2.ws_path && !g2.fold;  // the input gradient has a finalize pass
  auto run_g2 = [&]() -> int {  // input gradient alone, its finalize unless deferred
    if (defer_d && dslabs) {
      GemmPlan t = g2;
      t.ws_path = false;
      const int r = launch_one(t, s);
      if (r == ENCDIFF_OK) *dd = 1;
      return r;
    }
    return launch_one(g2, s);
  };
  if (g1.tile == 36) {  // WGL weight gradient (+ input gradient, + previous finalize)
    const EncdiffGemmArgs& pf = have_prev ? gp.user : g1.user;
    const int nf = have_prev ? fin_blocks(gp.user) : 0;
    const bool paired = wglpair_ok(g1, g2);
    e = paired ? wglpair_launch(g1, g2, pf, nf, s) : wgl_launch(g1.p, pf, nf, s);
    if (e != hipSuccess) return ENCDIFF_ERR_LAUNCH - (int)e;
    if (g1.ws_path && !defer1 && (e = launch_finalize(g1.user, s)) != hipSuccess) return ENCDIFF_ERR_LAUNCH - (int)e;
    if (!paired) return run_g2();
    if (defer_d && dslabs) {
      *dd = 1;
      return ENCDIFF_OK;
    }
    if (g2.ws_path && (e = launch_finalize(g2.user, s)) != hipSuccess) return ENCDIFF_ERR_LAUNCH - (int)e;
    return ENCDIFF_OK;
  }
  if (g1.tile >= 32 && g1.tile <= 34) {
    const EncdiffGemmArgs& pf = have_prev ? gp.user : g1.user;
    const int nf = have_prev ? fin_blocks(gp.user) : 0;
    if (wg3pair_ok(g1, g2)) {  // WG3 + input gradient + previous finalize in one grid
      e = wg3pair_launch(g1, g2, pf, nf, s);
      if (e != hipSuccess) return ENCDIFF_ERR_LAUNCH - (int)e;
      const bool f1 = g1.ws_path && !defer1, f2 = dslabs && !defer_d;
      if (f1 && (e = launch_finalize(g1.user, s)) != hipSuccess) return ENCDIFF_ERR_LAUNCH - (int)e;
      if (f2 && (e = launch_finalize(g2.user, s)) != hipSuccess) return ENCDIFF_ERR_LAUNCH - (int)e;
      if (dslabs && defer_d) *dd = 1;
      return ENCDIFF_OK;
    }
    // WG3 weight gradient (+ the previous finalize riding along), then the input gradient
    e = wg3_launch(g1.p, g1.tile, pf, nf, s);
    if (e != hipSuccess) return ENCDIFF_ERR_LAUNCH - (int)e;
    if (g1.ws_path && !defer1 && (e = launch_finalize(g1.user, s)) != hipSuccess) return ENCDIFF_ERR_LAUNCH - (int)e;
    return run_g2();
  }
  if ((!lin && !conv) || (g1.tile != 4 && g1.tile != 5 && g1.tile != 7 && g1.tile != 9 && g1.tile != 10)) {
    // pairs the fused kernel does not cover
    if (have_prev && (e = launch_finalize(gp.user, s)) != hipSuccess) return ENCDIFF_ERR_LAUNCH - (int)e;
    GemmPlan w = g1;
    w.ws_path = g1.ws_path && !defer1;
    rc = launch_one(w, s);
    return rc != ENCDIFF_OK ? rc : run_g2();
  }
  const EncdiffGemmArgs pf = have_prev ? gp.user : g1.user;
  const int nf = have_prev ? fin_blocks(gp.user) : 0;
  e = lin ? launch_pair_tiles<A_ROWM, B_ROWN, A_ROWK, B_ROWN>(g1, g2, pf, nf, s)
          : launch_pair_tiles<A_ROWM, B_IM2COL, A_IM2COL, B_CONVD>(g1, g2, pf, nf, s);
  if (e != hipSuccess) return ENCDIFF_ERR_LAUNCH - (int)e;
  const bool f1 = g1.ws_path && !defer1;
  const bool f2 = dslabs && !defer_d;
  if (dslabs && defer_d) *dd = 1;
  if (f1 && f2) {
    const int n1 = fin_blocks(g1.user), n2 = fin_blocks(g2.user);
    hipLaunchKernelGGL(gemm_finalize2_kernel, dim3((unsigned)(n1 + n2)), dim3(256), 0, s, g1.user, g2.user, n1);
    e = hipGetLastError();
  } else if (f1) {
    e = launch_finalize(g1.user, s);
  } else if (f2) {
    e = launch_finalize(g2.user, s);
  } else {
    e = hipGetLastError();
  }
  return e != hipSuccess ? ENCDIFF_ERR_LAUNCH - (int)e : ENCDIFF_OK;
}

extern "C" int encdiff_gemm_pair_ex(const EncdiffGemmArgs* wgrad, const EncdiffGemmArgs* dgrad,
                                    const EncdiffGemmArgs* prev_wgrad, int defer, void* stream) {
  int dd;
  return gemm_pair_impl(wgrad, dgrad, prev_wgrad, defer, false, &dd, stream);
}

extern "C" int encdiff_gemm_pair_dx(const EncdiffGemmArgs* wgrad, const EncdiffGemmArgs* dgrad,
                                    const EncdiffGemmArgs* prev_wgrad, int defer, int defer_dgrad, int* dgrad_deferred,
                                    void* stream) {
  int dd = 0;
  const int rc = gemm_pair_impl(wgrad, dgrad, prev_wgrad, defer, defer_dgrad != 0, &dd, stream);
  if (dgrad_deferred) *dgrad_deferred = rc == ENCDIFF_OK ? dd : 0;
  return rc;
}

extern "C" int encdiff_gemm_pair(const EncdiffGemmArgs* wgrad, const EncdiffGemmArgs* dgrad, void* stream) {
  return encdiff_gemm_pair_ex(wgrad, dgrad, nullptr, 0, stream);
}

extern "C" int encdiff_gemm_finalize(const EncdiffGemmArgs* args, void* stream) {
  GemmPlan g;
  const int rc = prepare(args, g);
  if (rc != ENCDIFF_OK) return rc;
  if (!g.ws_path || g.fold) return ENCDIFF_OK;  // folded GEMMs combined their slabs in the kernel
  const hipError_t e = launch_finalize(g.user, (hipStream_t)stream);
  return e != hipSuccess ? ENCDIFF_ERR_LAUNCH - (int)e : ENCDIFF_OK;
}

extern "C" int encdiff_gemm_check(const EncdiffGemmArgs* pa, int* tile) {
  GemmPlan g;
  const int rc = prepare(pa, g);
  if (rc == ENCDIFF_OK && tile) *tile = g.tile;
  return rc;
}

extern "C" int encdiff_gemm_tile_shape(int tile, int* bm, int* bn, int* kb, int* stages) {
  if (!is_tile(tile)) return ENCDIFF_ERR_UNSUPPORTED;
  if (bm) *bm = TILES[tile].bm;
  if (bn) *bn = TILES[tile].bn;
  if (kb) *kb = TILES[tile].kb;
  if (stages) *stages = TILES[tile].ns;
  return ENCDIFF_OK;
}

extern "C" int encdiff_version(void) { return 1; }
