#pragma once
// gemm_group.h -- the grouped weight-gradient launch: wgrad_group_kernel, its planner (wg_prepare,
// wg_items) and its two exports, encdiff_wgrad_group_plan / _launch.  Builds on gemm_plan.h
// (prepare(), GemmPlan) and, for the workgroup bodies, gemm_wg3.h, gemm_wgl.h and gemm_tile.h.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gemm_plan.h"
#include "gemm_tile.h"
#include "gemm_wg3.h"
#include "gemm_wgl.h"

namespace {
// ---------------------------------------------------------------------------
// Grouped weight gradients (encdiff_wgrad_group_plan / _launch): the weight gradients of a whole
// backward region -- every nn.Linear / 3x3 conv / skip conv of the output blocks, or of the rest
// of the UNet (openaimodel_enc.py:255-275, attention.py:159-167, 211-261) -- in ONE grid, after
// the region's input-gradient chain has produced every dY.  Alone, each of these problems (output
// a few KB, K = 2 048 .. 32 768 pixels) fills the chip only through split-K, whose fp32 slabs and
// finalize passes were half the GEMM family's excess traffic; together there are thousands of
// output parts, so every problem runs WHOLE (split_k 1): each output element is produced by one
// workgroup in one ordered sum (reproducible), no slabs, no finalize.  The workgroup bodies are
// the WG3 (3x3 conv, h in {4, 8, 16}) and WGL (linear, 64 x 64 parts) kernels' and the generic
// 64 x 64 tile for the rest (2x2 convs, narrow / short-K linears).  Work items are ordered by
// cost, longest first, so the list scheduling of the dispatcher balances the CUs.
struct WgProb {
  EncdiffGemmArgs p;
  GemmAux aux;
  int kind, gx, nblk, pad_;
};
struct WgBlobHead {
  int magic, n_probs, n_items, lds;
  long probs_off, items_off, bytes, pad_;
};
constexpr int WGG_MAGIC = 0x57474731;  // "WGG1"
constexpr int WGG_WG3_NS = 3, WGG_WGL_NS = 2;
// kinds: 0..5 WG3 (w 16 / 8 / 4) x (resample none / up2), 6 WGL, 7 generic linear, 8 generic conv
enum { WGK_WGL = 6, WGK_GEN_LIN = 7, WGK_GEN_CONV = 8 };
constexpr size_t cmax(size_t a, size_t b) { return a > b ? a : b; }
constexpr size_t WGG_LDS =
    cmax(cmax(cmax(wg3_lds<16, WGG_WG3_NS, 4>(), wg3_lds<8, WGG_WG3_NS, 4>()), cmax(wg3_lds<4, WGG_WG3_NS, 4>(),
         wgl_lds<WGG_WGL_NS>())), cmax((size_t)Gemm<64, 64, A_ROWM, B_ROWN, 2, BK>::LDS_BYTES,
                                       (size_t)Gemm<64, 64, A_ROWM, B_IM2COL, 2, BK>::LDS_BYTES));

__global__ __launch_bounds__(256) void wgrad_group_kernel(const WgProb* __restrict__ probs,
                                                          const int* __restrict__ items) {
  extern __shared__ __attribute__((aligned(16))) char wsm[];
  const int it = items[blockIdx.x];
  if (it < 0) return;
  const int pi = it >> 20, loc = it & 0xFFFFF;
  const int kind = probs[pi].kind;
  const EncdiffGemmArgs p = probs[pi].p;  // read before any store: scalar loads
  const SplitFold fold = probs[pi].aux.fold;
  const SplitFold* fp = fold.cnt ? &fold : nullptr;  // chunks combined in the kernel
  switch (kind) {
    case 0: wgrad3x3_body<16, false, WGG_WG3_NS, 4, 9001>(p, loc, wsm, fp); return;
    case 1: wgrad3x3_body<16, true, WGG_WG3_NS, 4, 9002>(p, loc, wsm, fp); return;
    case 2: wgrad3x3_body<8, false, WGG_WG3_NS, 4, 9003>(p, loc, wsm, fp); return;
    case 3: wgrad3x3_body<8, true, WGG_WG3_NS, 4, 9004>(p, loc, wsm, fp); return;
    case 4: wgrad3x3_body<4, false, WGG_WG3_NS, 4, 9005>(p, loc, wsm, fp); return;
    case 5: wgrad3x3_body<4, true, WGG_WG3_NS, 4, 9006>(p, loc, wsm, fp); return;
    case WGK_WGL: wgradlin_body<WGG_WGL_NS, 9007>(p, loc, wsm, fp); return;
    default: {
      const GemmAux aux = probs[pi].aux;
      const int gx = probs[pi].gx;
      if (kind == WGK_GEN_LIN)
        gemm_tile<64, 64, A_ROWM, B_ROWN, 2, BK>(p, aux, loc % gx, loc / gx, 0, (bf16_t*)wsm);
      else
        gemm_tile<64, 64, A_ROWM, B_IM2COL, 2, BK>(p, aux, loc % gx, loc / gx, 0, (bf16_t*)wsm);
      return;
    }
  }
}

// Scratch the group's split-K chunks use: fp32 slabs (their own region of the caller's workspace)
// and one ticket per split output part (the caller's zeroed counter array; left zero).
struct WgScratch {
  float* ws;
  long ws_floats, ws_used;
  int* cnt;
  int n_cnt, cnt_used;
};

// 32-pixel / 32-token stages one wave of a group workgroup may run in sequence: deeper problems are
// cut into chunks of whole images / token ranges, combined in the kernel (wg_last_chunk).  At one
// or two waves per SIMD a wave's stage loop is latency-bound, so a long sequence would be the
// group's critical path (a whole 16x16 problem: 256 stages, ~120 us).  ENCDIFF_WGG_STAGES (32: a
// 16-stage plan of the WGL body at K = 8192 gave wrong sums in test_wgrad_group -- not pursued, the
// fused transformer backward uses its own kernel, encdiff_st_wgrad).
int wgg_stages() {
  static const int v = [] {
    const char* e = getenv("ENCDIFF_WGG_STAGES");
    return e ? atoi(e) : 32;
  }();
  return v;
}

// one problem of a group: the first body that accepts it (WG3, WGL, generic 64 x 64 tile), with
// the chunk count (split_k) that keeps each wave's stage sequence within wgg_stages()
int wg_prepare(const EncdiffGemmArgs& in, WgProb& w, double& block_flops, WgScratch& sc) {
  if (in.dtype != ENCDIFF_DT_BF16 || in.a_mode != ENCDIFF_OPA_ROWM) return ENCDIFF_ERR_ARG;
  if (in.c_mode != ENCDIFF_OUT_F32 && in.c_mode != ENCDIFF_OUT_F32_ACCUM) return ENCDIFF_ERR_UNSUPPORTED;
  if (in.b_mode != ENCDIFF_OPB_IM2COL && in.b_mode != ENCDIFF_OPB_ROWN) return ENCDIFF_ERR_UNSUPPORTED;
  EncdiffGemmArgs q = in;
  q.split_k = 1;
  q.workspace = nullptr;
  q.split_counters = nullptr;
  GemmPlan g;
  const bool conv = q.b_mode == ENCDIFF_OPB_IM2COL;
  q.tile = conv ? 32 : 36;
  if (prepare(&q, g) == ENCDIFF_OK) {
    int nparts, split = 1;
    if (conv) {
      const int wi = q.conv.w == 16 ? 0 : (q.conv.w == 8 ? 1 : 2);
      w.kind = 2 * wi + (q.conv.resample == ENCDIFF_RESAMPLE_UP2 ? 1 : 0);
      nparts = (q.M / 32) * (q.conv.cin / 16);
      const int ni = q.conv.w == 16 ? 1 : 2, rows = q.conv.w == 4 ? 4 : 2;
      auto spw = [&](int sp) {  // stages per wave, 0 when the chunking does not divide
        if (q.conv.batch % (sp * ni)) return 0;
        const int nst = (q.conv.batch / sp / ni) * (q.conv.h / rows);
        return nst % 4 ? 0 : nst / 4;
      };
      while (spw(split) > wgg_stages() && spw(2 * split) > 0) split *= 2;
      block_flops = 2.0 * 32 * 9 * 16 * (double)q.K / split;
    } else {
      w.kind = WGK_WGL;
      nparts = (q.M / 64) * (q.N / 64);
      while (q.K / (split * 128) > wgg_stages() && q.K % (2 * split * 128) == 0) split *= 2;
      block_flops = 2.0 * 64 * 64 * (double)q.K / split;
    }
    if (split > 1) {  // slabs + tickets, or whole when the scratch is exhausted
      // (regions 128-B aligned: a cache line never holds two problems' chunks -- see wg_last_chunk)
      const long need = ((long)split * q.M * q.N + (q.bias_grad ? (long)split * q.M : 0) + 31) & ~31L;
      if (sc.ws && sc.cnt && sc.ws_used + need <= sc.ws_floats && sc.cnt_used + nparts <= sc.n_cnt) {
        EncdiffGemmArgs qs = q;
        qs.split_k = split;
        qs.workspace = sc.ws + sc.ws_used;
        if (prepare(&qs, g) == ENCDIFF_OK) {
          g.aux.fold = SplitFold{sc.cnt + sc.cnt_used, g.user.c, g.user.ldc, g.user.c_mode, g.user.alpha,
                                 nullptr, nullptr, 0};
          sc.ws_used += need;
          sc.cnt_used += nparts;
        } else {
          split = 1;
        }
      } else {
        split = 1;
      }
      if (split == 1 && prepare(&q, g) != ENCDIFF_OK) return ENCDIFF_ERR_SHAPE;
    }
    if (split == 1) block_flops = (conv ? 2.0 * 32 * 9 * 16 : 2.0 * 64 * 64) * (double)q.K;
    w.nblk = nparts * split;
    w.gx = 0;
  } else {
    q.tile = 4;
    const int rc = prepare(&q, g);
    if (rc != ENCDIFF_OK) return rc;
    if (g.ws_path) return ENCDIFF_ERR_ARG;
    w.kind = conv ? WGK_GEN_CONV : WGK_GEN_LIN;
    w.gx = (q.M + 63) / 64;
    w.nblk = w.gx * ((q.N + 63) / 64);
    block_flops = 2.0 * 64 * 64 * (double)q.K;
  }
  w.p = g.p;
  w.aux = g.aux;
  w.aux.xcd = 0;
  w.pad_ = 0;
  return ENCDIFF_OK;
}

}  // namespace

// Work-item order of a group.  Blocks of one problem read the same dY / x rows (the whole K range:
// nothing is split), so they are kept on one XCD, whose L2 then serves the re-reads; problems go
// to the least-loaded XCD, largest first (those with more blocks than an XCD holds at once are
// cut into runs of consecutive blocks -- consecutive parts share their dY columns), and each XCD
// runs its blocks longest first.  Blocks are dealt round-robin over the XCDs by index (MI355X
// microarch guide: b and b + 8 share an XCD), so XCD x's list occupies indices x, x + 8, ...;
// shorter lists are padded with empty items.  ENCDIFF_WGG_ORDER=0: one global longest-first list.
static std::vector<int> wg_items(const std::vector<WgProb>& w, const std::vector<double>& cost) {
  const int n = (int)w.size();
  static const int order_mode = [] {
    const char* e = getenv("ENCDIFF_WGG_ORDER");
    return e ? atoi(e) : 1;
  }();
  std::vector<int> order((size_t)n);
  for (int i = 0; i < n; ++i) order[i] = i;
  std::vector<int> items;
  if (order_mode == 0) {
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cost[a] > cost[b]; });
    for (int i : order)
      for (int b = 0; b < w[i].nblk; ++b) items.push_back((i << 20) | b);
    return items;
  }
  constexpr int NX = 8, RUN = 64;  // XCDs; blocks of one problem per XCD run (32 CUs x 2 workgroups)
  std::stable_sort(order.begin(), order.end(),
                   [&](int a, int b) { return cost[a] * w[a].nblk > cost[b] * w[b].nblk; });
  std::vector<std::vector<int>> q(NX);
  double load[NX] = {0};
  for (int i : order) {
    for (int b0 = 0; b0 < w[i].nblk; b0 += RUN) {
      const int b1 = std::min(w[i].nblk, b0 + RUN);
      int x = 0;
      for (int k = 1; k < NX; ++k)
        if (load[k] < load[x]) x = k;
      load[x] += cost[i] * (b1 - b0);
      for (int b = b0; b < b1; ++b) q[x].push_back((i << 20) | b);
    }
  }
  size_t len = 0;
  for (auto& v : q) {
    std::stable_sort(v.begin(), v.end(), [&](int a, int b) { return cost[a >> 20] > cost[b >> 20]; });
    len = std::max(len, v.size());
  }
  items.assign(len * NX, -1);
  for (int x = 0; x < NX; ++x)
    for (size_t j = 0; j < q[x].size(); ++j) items[j * NX + x] = q[x][j];
  return items;
}

extern "C" int encdiff_wgrad_group_plan(const EncdiffGemmArgs* probs, int n, float* workspace, long ws_floats,
                                        int* counters, int n_counters, void* blob, long capacity, long* blob_bytes) {
  if (!probs || n <= 0 || n > 2047 || !blob_bytes || ws_floats < 0 || n_counters < 0) return ENCDIFF_ERR_ARG;
  if ((uintptr_t)workspace & 127) return ENCDIFF_ERR_ARG;
  std::vector<WgProb> w((size_t)n);
  std::vector<double> cost((size_t)n);
  WgScratch sc{workspace, workspace ? ws_floats : 0, 0, counters, counters ? n_counters : 0, 0};
  for (int i = 0; i < n; ++i) {
    std::memset(&w[i], 0, sizeof(WgProb));
    const int rc = wg_prepare(probs[i], w[i], cost[i], sc);
    if (rc != ENCDIFF_OK) return rc;
    if (w[i].nblk <= 0 || w[i].nblk >= (1 << 20)) return ENCDIFF_ERR_SHAPE;
  }
  const std::vector<int> items = wg_items(w, cost);
  if (items.size() >= (size_t)1 << 30) return ENCDIFF_ERR_SHAPE;
  const long probs_off = (long)((sizeof(WgBlobHead) + 63) & ~(size_t)63);
  const long items_off = probs_off + (long)(sizeof(WgProb) * (size_t)n);
  const long bytes = items_off + (long)items.size() * 4;
  *blob_bytes = bytes;
  if (!blob) return ENCDIFF_OK;
  if (capacity < bytes || ((uintptr_t)blob & 7)) return ENCDIFF_ERR_ARG;
  char* out = (char*)blob;
  WgBlobHead h{};
  h.magic = WGG_MAGIC;
  h.n_probs = n;
  h.n_items = (int)items.size();
  h.lds = (int)WGG_LDS;
  h.probs_off = probs_off;
  h.items_off = items_off;
  h.bytes = bytes;
  std::memset(out, 0, (size_t)probs_off);
  std::memcpy(out, &h, sizeof(h));
  std::memcpy(out + probs_off, w.data(), sizeof(WgProb) * (size_t)n);
  std::memcpy(out + items_off, items.data(), items.size() * 4);
  return ENCDIFF_OK;
}

extern "C" int encdiff_wgrad_group_launch(const void* host_blob, const void* dev_blob, void* stream) {
  if (!host_blob || !dev_blob) return ENCDIFF_ERR_ARG;
  WgBlobHead h;
  std::memcpy(&h, host_blob, sizeof(h));
  if (h.magic != WGG_MAGIC || h.n_items <= 0 || h.lds > HALO_LDS_MAX) return ENCDIFF_ERR_ARG;
  static const hipError_t attr_ok = hipFuncSetAttribute((const void*)wgrad_group_kernel,
                                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)WGG_LDS);
  if (attr_ok != hipSuccess) return ENCDIFF_ERR_LAUNCH - (int)attr_ok;
  const char* d = (const char*)dev_blob;
  hipLaunchKernelGGL(wgrad_group_kernel, dim3((unsigned)h.n_items), dim3(256), (size_t)h.lds, (hipStream_t)stream,
                     (const WgProb*)(d + h.probs_off), (const int*)(d + h.items_off));
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? ENCDIFF_ERR_LAUNCH - (int)e : ENCDIFF_OK;
}
