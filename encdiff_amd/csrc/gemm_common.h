#pragma once
// gemm_common.h -- what every part of the GEMM engine shares: operand modes, the LDS tile shape
// and its bank swizzle, exact division (FDiv), halo geometry, the in-kernel split-K combine's
// arguments (SplitFold), GemmAux, implicit im2col, the Gemm<> traits, the asm LDS reads and
// counted waits, and the chunk ticket and combined-part store of the weight-gradient kernels
// (gemm_wg3.h, gemm_wgl.h and, through their bodies, gemm_group.h).  Builds on common.h only.
//
// The gemm_*.h headers are private to ONE translation unit, gemm.hip: everything in them sits in
// its anonymous namespace, and nothing else includes them.  Includes go one way:
// common -> finalize -> tile -> wg3 / wgl -> plan -> group.
#include "common.h"

namespace {

constexpr int BK = 64;

enum { A_ROWK = ENCDIFF_OPA_ROWK, A_IM2COL = ENCDIFF_OPA_IM2COL, A_ROWM = ENCDIFF_OPA_ROWM };
enum { B_ROWK = ENCDIFF_OPB_ROWK, B_ROWN = ENCDIFF_OPB_ROWN, B_CONVD = ENCDIFF_OPB_CONV_DGRAD,
       B_IM2COL = ENCDIFF_OPB_IM2COL };

// internal A modes: implicit im2col read from a per-workgroup halo image in LDS (tiles >= 16);
// implicit im2col with GroupNorm(+FiLM)(+SiLU) applied to each staged A tile (EncdiffGemmArgs.agn_*)
enum { A_HALO = 16, A_IM2COL_GN = 17, A_ROWK_LN = 18 };

template <int AM> struct AKInner { static constexpr bool v = AM != A_ROWM; };
template <int BMd> struct BKInner { static constexpr bool v = BMd == B_ROWK; };

// LDS tiles are unpadded rows of 16-byte chunks, filled by LDS-DMA (global_load_lds_dwordx4:
// one wave instruction writes 1 KiB lane-linearly).  Bank conflicts of the fragment reads are
// removed by an XOR swizzle applied on the SOURCE side: the chunk stored at LDS slot s of
// row r is the global chunk s ^ (r & 7), and reads apply the same involution.
template <int ROWS, bool KINNER, int KB = BK>
struct TileShape {
  // k-inner: [ROWS][KB]; k-outer: [KB][ROWS]
  static constexpr int LD = KINNER ? KB : ROWS;            // elements per LDS row
  static constexpr int SLOTS = LD / 8;                      // 16-byte chunks per row
  static constexpr int ELEMS = ROWS * KB;
  static constexpr int CHUNKS = ROWS * KB / 8;  // 16-byte chunks per tile
  static constexpr int PER_THREAD = CHUNKS / 256;
  // swizzle mask: 16 rows of a 256-byte k-inner row (KB = 128) spread over all 64 banks;
  // a 4-slot k-outer row (32 columns) swizzles within its 4 slots
  static constexpr int SWM = (KINNER && KB >= 128) ? 15 : (SLOTS < 8 ? SLOTS - 1 : 7);
  // Bank swizzle (an involution on a row's slots): k-inner rows are read by ds_read_b128 along
  // rows (slot ^ row); k-outer rows by ds_read_b64_tr_b16, whose 32-lane groups read rows
  // {r..r+3, r+8..r+11} two slots each -- the XOR keeps each slot pair aligned and gives those
  // 8 rows distinct bank positions (slot ^ (row & 7) put rows r and r+8 on the same banks: ~half
  // the weight-gradient tiles' LDS cycles were conflicts)
  static ED_DEV int sw(int row, int slot) {
    if constexpr (KINNER || LD < 64) return slot ^ (row & SWM);
    else if constexpr (LD == 64) return slot ^ ((((row >> 1) & 1) << 1) | (((row >> 3) & 1) << 2));
    else return slot ^ (((row & 3) << 1) | (((row >> 3) & 1) << 3));
  }
};
ED_DEV int swz(int row, int slot, int mask = 7) { return slot ^ (row & mask); }

// 16 zero bytes in global memory: the source of masked (padding / out-of-range) chunks,
// so LDS-DMA lanes never need a branch.
__device__ __attribute__((aligned(16))) const uint4 g_zero16 = {0u, 0u, 0u, 0u};

// ---------------------------------------------------------------------------
// Exact division by a launch constant without a divider: n / d == (n * mul) >> 40 for
// n * d < 2^40 (pixels < 2^24, divisors < 2^16 here); mul = 2^40 / d + 1 from the host.
struct FDiv {
  unsigned long long mul;
  uint32_t d, pad_;
};
ED_DEV uint32_t fdiv(uint32_t n, const FDiv& f) { return (uint32_t)(((unsigned long long)n * f.mul) >> 40); }

// Halo tiles (A_HALO): a workgroup's BM output pixels are R whole rows of one image (or NI
// whole images); every conv-input pixel their taps reach -- an (hr x hc) window per image, all
// cin channels -- is staged into LDS ONCE by LDS-DMA, so the K loop streams only weights and the
// im2col operand is read from L2 once instead of once per tap.  Conv-input coordinate of halo
// pixel (hy, hx): (s*y0 + off + hy, off + hx), bounds (lh, lw); source pixel = coordinate >> ush
// (nearest-up) of an (hs x ws) image.  16-byte chunk c of halo pixel p sits at LDS slot
// c ^ ((p >> xsh) & xmsk): the 16 pixels an MFMA fragment read touches land on distinct banks.
struct HaloGeom {
  int hr, hc, ni;      // halo rows / cols per image, images per tile
  int s, off, kt;      // conv-input stride, window origin offset, taps per dimension
  int lh, lw, ush, hs, ws;
  int ch, xsh, xmsk;   // 16-B chunks per pixel (cin / 8), bank swizzle
  int npix, chunks;    // halo pixels, chunks rounded up to 256 (one per thread per DMA round)
  FDiv fch, fimg, fhc; // / ch, / (hr * hc), / hc
};

// In-kernel split-K combine (EncdiffGemmArgs.split_counters): the user's output of a slab GEMM
struct SplitFold {
  int* cnt;              // per-tile tickets (NULL: a finalize pass combines the slabs)
  void* c;
  long ldc;
  int mode;              // ENCDIFF_OUT_BF16 / F32 / F32_ACCUM
  float alpha;
  const float* bias;
  const bf16_t* resid;
  long ld_resid;
};

struct GemmAux {
  FDiv cin;   // A/B im2col: k (or n) -> (tap, channel)
  FDiv cout;  // B_CONVD: k -> (tap, co)
  FDiv hw;    // pixel -> (image, in-image index)
  FDiv w;     // in-image index -> (y, x)
  HaloGeom halo;
  SplitFold fold;
  int xcd;    // XCD-aware tile order (gemm_kernel / gemm2_kernel): see xcd_remap
};

// Implicit im2col, branch-free.  The launch's resample mode is folded into uniform
// constants once per thread; per chunk the source pixel of output pixel (b, y, x) and
// 3x3 tap (ty, tx) is  ys = sy*y + ty + oy  (limits lh x lw), then >> sh (nearest-up
// source), row = (b*hs + ys)*ws + xs.  Padding gives ok = false and row 0: the load is
// still issued (and masked when written to LDS), so no branch or early wait is needed.
//   K4S2   (Encoder4 Conv2d(k4, s2, p1), openaimodel_enc.py:1002-1009): 4x4 taps at
//          (2y + ty - 1, 2x + tx - 1) of the (2h, 2w) source;
//   K4S2_T (its input gradient): 4x4 taps t' = 15 - t at (y + ty' - 2, x + tx' - 2) of the
//          full-resolution grid, valid only at even coordinates, source pixel = coordinate / 2;
//   K4S2_TP (the same gradient by output parity): the M rows are ordered [parity q][b][y'][x']
//          over the half-resolution grid, and an output row (b, 2y'+py, 2x'+px), q = 2py+px,
//          receives only the 2x2 taps ty' = py + 2jy, tx' = px + 2jx: source (y'+py+jy-1,
//          x'+px+jx-1) of dY, weight tap 15 - (4ty' + tx').  K = 4*cout instead of 16*cout
//          (K4S2_T multiplies 3 zero taps of every 4).  A tile never straddles parities
//          (batch*h*w/4 % 128 == 0), so oy, ox and the weight-tap base are per workgroup.
struct Im2colMode {
  int sy, oy, ox, lh, lw, sh, hs, ws, par, k4, tb;
  ED_DEV Im2colMode(const EncdiffConvGeom& g) {
    const bool s2 = g.resample == ENCDIFF_RESAMPLE_STRIDE2;  // VQ Downsample: pad (0,1,0,1), k3 s2 p0
    const bool up = g.resample == ENCDIFF_RESAMPLE_UP2;      // nearest x2 (openaimodel_enc.py:116)
    const bool f4 = g.resample == ENCDIFF_RESAMPLE_K4S2;
    const bool t4 = g.resample == ENCDIFF_RESAMPLE_K4S2_T;
    const bool tp = g.resample == ENCDIFF_RESAMPLE_K4S2_TP;
    sy = (s2 || f4) ? 2 : 1;
    oy = s2 ? 0 : (t4 ? -2 : -1);
    ox = oy;
    lh = (s2 || f4) ? 2 * g.h : (tp ? g.h >> 1 : g.h);
    lw = (s2 || f4) ? 2 * g.w : (tp ? g.w >> 1 : g.w);
    sh = (up || t4) ? 1 : 0;
    hs = lh >> sh;
    ws = lw >> sh;
    par = t4 ? 1 : 0;
    k4 = tp ? 2 : ((f4 || t4) ? 1 : 0);
    tb = 15;
  }
  // K4S2_TP: the workgroup's parity class q = 2py + px
  ED_DEV void set_parity(int q) {
    oy = (q >> 1) - 1;
    ox = (q & 1) - 1;
    tb = 15 - 4 * (q >> 1) - (q & 1);
  }
  // weight tap of im2col tap `tap` for OPB_CONV_DGRAD (flipped kernel)
  ED_DEV uint32_t wtap(uint32_t tap) const {
    return k4 == 2 ? (uint32_t)tb - 8u * (tap >> 1) - 2u * (tap & 1u) : (k4 ? 15u : 8u) - tap;
  }
};

// tap index -> (ty, tx): 3x3 (tap / 3 via a multiply), 4x4 or 2x2 taps
ED_DEV void tap_yx(const Im2colMode& md, uint32_t tap, int& ty, int& tx) {
  ty = md.k4 ? (int)(tap >> (3 - md.k4)) : (int)((tap * 11u) >> 5);
  tx = (int)tap - (md.k4 ? (1 << (3 - md.k4)) : 3) * ty;
}

ED_DEV uint32_t im2col_row(const Im2colMode& md, uint32_t b, int y, int x, int ty, int tx, bool& ok) {
  const int ys = md.sy * y + ty + md.oy, xs = md.sy * x + tx + md.ox;
  ok = (unsigned)ys < (unsigned)md.lh && (unsigned)xs < (unsigned)md.lw && ((ys | xs) & md.par) == 0;
  const uint32_t row = (b * (uint32_t)md.hs + (uint32_t)(ys >> md.sh)) * (uint32_t)md.ws + (uint32_t)(xs >> md.sh);
  return ok ? row : 0u;
}

template <int BM, int BN, int AM, int BMD, int NS = 2, int KB = BK>
struct Gemm {
  static constexpr bool AKI = AKInner<AM>::v;
  static constexpr bool BKI = BKInner<BMD>::v;
  static constexpr int KT = KB;  // k per LDS stage
  using TA = TileShape<BM, AKI, KB>;
  using TB = TileShape<BN, BKI, KB>;
  static constexpr int TM = BM / 32;  // 16x16 MFMA tiles per wave along M
  static constexpr int TN = BN / 32;
  static constexpr bool HALO = AM == A_HALO;
  static constexpr bool AGN = AM == A_IM2COL_GN;  // GroupNorm applied to the staged A tiles
  static constexpr bool LNA = AM == A_ROWK_LN;    // LayerNorm applied to the staged A tiles (ROWK)
  static constexpr bool IM2 = AM == A_IM2COL || AGN;
  static constexpr int ASTAGE = HALO ? 0 : TA::ELEMS;  // halo mode: the ring holds B only
  static constexpr int STAGE = ASTAGE + TB::ELEMS;     // elements per LDS stage
  // LDS ring depth.  Measured on the step's GEMMs: 3-4 stages for every GEMM (one or two
  // workgroups per CU) lost 7% overall against 2 stages with up to five resident workgroups
  // per CU hiding the load latency instead; the deeper rings are tile choices of their own
  // (tiles 5, 6) that the measured table picks per problem.
  static constexpr int NSTAGE = NS;
  static constexpr int LPS = (HALO ? 0 : TA::PER_THREAD) + TB::PER_THREAD;  // LDS-DMA loads per thread per stage
  // the staging ring, reused by the fp32 epilogue tile [BM][BN + 4]
  static constexpr int LDS_BYTES =
      (NSTAGE * STAGE * 2 > BM * (BN + 4) * 4) ? NSTAGE * STAGE * 2 : BM * (BN + 4) * 4;
};

// ds_read_b64_tr_b16 as inline asm.  Through the builtin, hipcc cannot tell the transposed read
// from the LDS-DMA writes still in flight to ANOTHER ring slot and drains them (s_waitcnt
// vmcnt(0)) before every k-outer fragment read: the next stage's loads then never overlap the
// current tile's MFMAs in any backward GEMM.  The asm read is waited for explicitly (compute()).
ED_DEV v4s ds_read_tr16(const bf16_t* p) {
  typedef __attribute__((address_space(3))) const char lds_char;
  const uint32_t a = (uint32_t)(uintptr_t)(lds_char*)p;
  v4s r;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(r) : "v"(a));
  return r;
}

// ds_read_b128 as inline asm, for tiles whose fragment waits are counted by hand (compute()):
// a compiler-issued read would be waited for by the compiler, which does not count the asm reads.
ED_DEV v8bf ds_read_b128(const bf16_t* p) {
  typedef __attribute__((address_space(3))) const char lds_char;
  const uint32_t a = (uint32_t)(uintptr_t)(lds_char*)p;
  v4u32 r;
  asm volatile("ds_read_b128 %0, %1" : "=v"(r) : "v"(a));
  return __builtin_bit_cast(v8bf, r);
}

// Fragment reads software-pipelined across k-substeps (compute()): measured in the step with both
// builds on one box (round 4, tools/bench_ab.sh): 9.516-9.524 ms/step pipelined vs 9.503-9.522
// without -- no gain (five resident workgroups per CU already hide the LDS latency) for 4-12 more
// VGPRs, so it is off; -DED_FRAG_PIPE=1 builds it.
#ifndef ED_FRAG_PIPE
#define ED_FRAG_PIPE 0
#endif

// Wait until at most N of this thread's vector-memory loads are outstanding (LDS-DMA stages
// still in flight behind the one about to be read).
template <int N>
ED_DEV void vm_wait() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
template <int LPS, int MAXA = 2>
ED_DEV void vm_wait_stages(int ahead) {
  // ahead = stages still allowed in flight behind the one about to be read (<= ring depth - 2)
  if (MAXA >= 6 && ahead >= 6) vm_wait<6 * LPS>();
  else if (MAXA >= 5 && ahead == 5) vm_wait<5 * LPS>();
  else if (MAXA >= 4 && ahead == 4) vm_wait<4 * LPS>();
  else if (MAXA >= 3 && ahead == 3) vm_wait<3 * LPS>();
  else if (ahead >= 2) vm_wait<2 * LPS>();
  else if (ahead == 1) vm_wait<LPS>();
  else vm_wait<0>();
}

// ---- shared by the weight-gradient kernels (gemm_wg3.h, gemm_wgl.h; gemm_group.h runs their bodies)
// ds_read_b64_tr_b16 with an immediate byte offset (the tap / stage displacement)
template <int OFF>
ED_DEV v4s tr16_off(uint32_t a) {
  v4s r;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(r) : "v"(a), "i"(OFF));
  return r;
}
template <int N>
ED_DEV void lgkm_wait() {
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
  __builtin_amdgcn_sched_barrier(0);
}
ED_DEV v8bf cat8(v4s lo, v4s hi) {
  return __builtin_bit_cast(v8bf, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}
// LDS byte address of a shared-memory pointer
ED_DEV uint32_t lds_addr(const void* p) {
  typedef __attribute__((address_space(3))) const char lds_char;
  return (uint32_t)(uintptr_t)(lds_char*)p;
}

// Split-K combine of a grouped weight gradient (wgrad_group_kernel; the SplitFold that wg_prepare
// sets): the workgroup's slab stores were write-through (sc1); after draining them, one lane takes
// the output part's ticket (relaxed, agent scope), and the chunk that draws split - 1 acquires and
// returns true -- it then sums the part's slabs in chunk order (bitwise reproducible, independent
// of which chunk arrives last or where it runs) -- and leaves the ticket at zero for the next launch.
// The guide's write-through ticket recipe, as the GEMM tiles' in-kernel combine.
ED_DEV bool wg_last_chunk(int* cnt, int split, int* flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const int tk = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    flag[0] = tk == split - 1;
  }
  __syncthreads();
  if (!flag[0]) return false;
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  return true;
}
constexpr int WG3_PART = 32 * 9 * 16, WGL_PART = 64 * 64;  // floats of one output part
ED_DEV float4 f4add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
// the combined part written to the user's output: alpha, then += the output (F32_ACCUM)
ED_DEV void wg_fold_store(const SplitFold& f, float* o, float4 v) {
  v.x *= f.alpha; v.y *= f.alpha; v.z *= f.alpha; v.w *= f.alpha;
  if (f.mode == ENCDIFF_OUT_F32_ACCUM) v = f4add(v, *(const float4*)o);
  *(float4*)o = v;
}
}  // namespace
