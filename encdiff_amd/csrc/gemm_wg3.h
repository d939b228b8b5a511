#pragma once
// gemm_wg3.h -- device side of the 3x3 conv weight-gradient kernel (WG3, tiles 32-34): Wg3,
// Wg3Stage, wgrad3x3_body, wgrad3x3_kernel and its LDS size.  Builds on gemm_tile.h (the paired
// input-gradient tiles, xcd_remap) and gemm_finalize.h (the riding finalize).
#include "gemm_finalize.h"
#include "gemm_tile.h"

namespace {
// ---------------------------------------------------------------------------
// 3x3 conv weight gradient, tile id 32 (WG3): dW[co][tap*cin + ci] += sum_p dY[p][co] x[p+tap][ci]
// (openaimodel_enc.py ResBlock / Upsample convs, autograd's weight gradient).
//
// The GEMM form (M = cout, N = 9 cin, K = pixels) stages every k-tile of dY once per 64 output
// columns and the im2col of x once per tap, and fills the chip only through deep split-K whose
// fp32 slabs are most of its HBM traffic.  Here a workgroup owns an output part of 32 couts x
// 16 cins x all 9 taps and a chunk of whole images; its 4 waves run independently over a
// quarter of the chunk each (no barrier in the main loop) and their partials are summed in LDS
// at the end, so a chunk writes ONE slab for 4x the pixels.  Per 32-pixel stage a wave stages
// dY (32 pixels x 32 couts, 2 KiB) and a zero-bordered halo of x (the stage's rows +-1, 16
// channels, 32 B per pixel slot) by LDS-DMA into its own ring; the B operand of tap (ty, tx)
// is the halo read at a constant offset (the ds_read immediate), so 9 taps cost 9 reads of one
// staged image instead of 9 staged im2col tiles.  18 MFMAs (2 cout tiles x 9 taps) per stage.
// k order within a stage: k = 8 g4 + 4 t + tq is pixel (img, y, x0 + tq) of the lane quad
// (g4, t) below, chosen so that the two 16-lane groups of each 32-lane half read halo rows
// (or images) whose slot distance is 4 mod 8: the transposed reads are bank-conflict free.
template <int W>
struct Wg3 {
  static constexpr int NI = W == 16 ? 1 : 2;                   // images per 32-pixel stage
  static constexpr int R = W == 4 ? 4 : 2;                     // image rows per stage
  static constexpr int WP = W == 16 ? 20 : (W == 8 ? 12 : 6);  // halo row pitch in pixel slots
  static constexpr int HR = R + 2;                             // halo rows per image
  static constexpr int NSLOT = NI * HR * WP;                   // halo pixel slots (32 B each)
  static constexpr int HCH = (2 * NSLOT + 63) / 64;            // halo LDS-DMA instructions (1 KiB)
  static constexpr int DYB = 32 * 64;                          // 32 k-rows x 32 couts (bf16)
  static constexpr int STAGE = DYB + HCH * 1024;               // bytes per ring stage
  static constexpr int LPS = 2 + HCH;                          // LDS-DMA instructions per stage
  static constexpr int T1 = W == 4 ? WP * 32 : 128;            // halo byte step of the lane's 2nd quad
  // lane quad (g4, t) of a stage -> (image, row, first column), stage-relative
  static ED_DEV void quad(int g4, int t, int& img, int& y, int& x0) {
    if constexpr (W == 16) { img = 0; y = g4 & 1; x0 = 8 * (g4 >> 1) + 4 * t; }
    else if constexpr (W == 8) { img = g4 >> 1; y = g4 & 1; x0 = 4 * t; }
    else { img = g4 & 1; y = 2 * (g4 >> 1) + t; x0 = 0; }
  }
};

template <int W, int NS>
struct Wg3Stage {
  // one 32-pixel stage in ring slot J: 2 cout tiles x 9 taps of MFMAs, reads software-pipelined
  // PD taps ahead with counted lgkmcnt waits (asm reads: hipcc does not track them)
  template <int J>
  static ED_DEV void compute(uint32_t a0, uint32_t a1, uint32_t bb, v4f (&acc)[2][9], bool bg, float (&bs)[2]) {
    using G = Wg3<W>;
    constexpr int SB = J * G::STAGE;
    constexpr int PD = 4;
    v8bf af0 = cat8(tr16_off<SB>(a0), tr16_off<SB + 256>(a0));
    v8bf af1 = cat8(tr16_off<SB>(a1), tr16_off<SB + 256>(a1));
    v8bf bf[9];
#define WG3_B(T) bf[T] = cat8(tr16_off<SB + G::DYB + ((T) / 3 * G::WP + (T) % 3) * 32>(bb), \
                              tr16_off<SB + G::DYB + ((T) / 3 * G::WP + (T) % 3) * 32 + G::T1>(bb))
    WG3_B(0); WG3_B(1); WG3_B(2); WG3_B(3);
#define WG3_T(T, NEXT, WAITN)                                                          \
    if constexpr ((NEXT) < 9) { WG3_B(NEXT); }                                         \
    lgkm_wait<WAITN>();                                                                \
    acc[0][T] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af0, bf[T], acc[0][T], 0, 0, 0); \
    acc[1][T] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af1, bf[T], acc[1][T], 0, 0, 0);
    WG3_T(0, 4, 8) WG3_T(1, 5, 8) WG3_T(2, 6, 8) WG3_T(3, 7, 8) WG3_T(4, 8, 8)
    WG3_T(5, 9, 6) WG3_T(6, 9, 4) WG3_T(7, 9, 2) WG3_T(8, 9, 0)
#undef WG3_T
#undef WG3_B
    static_assert(PD == 4, "the wait counts above assume 4 taps in flight");
    if (bg) {  // bias gradient: this lane's 8 pixels of its cout in each tile
      const v8s s0 = __builtin_bit_cast(v8s, af0), s1 = __builtin_bit_cast(v8s, af1);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        bs[0] += bf2f((bf16_t)s0[e]);
        bs[1] += bf2f((bf16_t)s1[e]);
      }
    }
  }
};

// (the body is a __device__ function, as gemm_tile: a kernel template whose own body calls a lambda
// holding device builtins loses its host launch stub.  TAG: one body specialization per kernel --
// hipcc's host pass rejects a second kernel instantiation calling the same one)
template <int W, bool UP, int NS, int WPG, int TAG = 0>
__device__ __forceinline__ void wgrad3x3_body(const EncdiffGemmArgs& p, const int bid, char* wsm,
                                              const SplitFold* fold = nullptr) {
  using G = Wg3<W>;
  constexpr int H = W;
  constexpr uint32_t OOB = 0x80000000u;
  typedef __attribute__((address_space(3))) void lds_void;
  const int cin = p.conv.cin, cout = p.M;
  const int ncit = cin >> 4, nparts = (cout >> 5) * ncit;
  const int z = bid / nparts, part = bid - z * nparts;  // bid: the caller's logical block
  const int cot = part / ncit, cit = part - cot * ncit;
  const int co0 = cot * 32, ci0 = cit * 16;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int l16 = lane & 15, g4 = lane >> 4, tq = l16 >> 2, tp = l16 & 3;
  const int ipz = p.conv.batch / p.split_k;               // images of this chunk
  const int nst = (ipz / G::NI) * (H / G::R) / WPG;      // 32-pixel stages of this wave
  const int st0 = wave * nst;                             // its first stage (chunk order)
  const int zb = z * ipz;
  char* ring = wsm + wave * (NS * G::STAGE);
  const uint32_t ring_a = lds_addr(ring);
  const auto rsA = __builtin_amdgcn_make_buffer_rsrc((void*)p.a, 0, 0x7FFFFFF0, 0x00020000);
  const auto rsB = __builtin_amdgcn_make_buffer_rsrc((void*)p.b, 0, 0x7FFFFFF0, 0x00020000);
  const uint32_t lda2 = (uint32_t)p.lda * 2u, ldx2 = (uint32_t)p.conv.ld_src * 2u;

  // staging invariants: dY chunk i (row r = k order, 16-B slot with the odd-8-row half swap)
  uint32_t dy_off[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = lane + 64 * i, r = c >> 2, gs = (c & 3) ^ (((r >> 3) & 1) << 1);
    int img, y, x0;
    G::quad(r >> 3, (r >> 2) & 1, img, y, x0);
    dy_off[i] = (uint32_t)((img * H + y) * W + x0 + (r & 3)) * lda2 + (uint32_t)(co0 + gs * 8) * 2u;
  }
  // halo chunk i: pixel slot s = c / 2, channel half c % 2
  int h_img[G::HCH], h_hy[G::HCH], h_xs[G::HCH];
  uint32_t h_ch[G::HCH];
#pragma unroll
  for (int i = 0; i < G::HCH; ++i) {
    const int c = lane + 64 * i, s = c >> 1;
    h_img[i] = s / (G::HR * G::WP);
    const int rem = s - h_img[i] * (G::HR * G::WP);
    h_hy[i] = rem / G::WP;
    const int hx = rem - h_hy[i] * G::WP;
    h_xs[i] = (s < G::NSLOT && hx >= 1 && hx <= W) ? hx - 1 : -1;  // -1: zero border / pad slot
    h_ch[i] = (uint32_t)(ci0 + (c & 1) * 8) * 2u;
  }
  auto stage = [&](int slot, int sw) {
    const int st = st0 + sw;
    const int b0 = zb + (st / (H / G::R)) * G::NI, y0 = (st % (H / G::R)) * G::R;
    char* sd = ring + slot * G::STAGE;
    const uint32_t pix0 = (uint32_t)(b0 * H + y0) * W;
#pragma unroll
    for (int i = 0; i < 2; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_void*)(sd + i * 1024), 16, dy_off[i] + pix0 * lda2, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < G::HCH; ++i) {
      const int ys = y0 + h_hy[i] - 1, xs = h_xs[i];
      const bool ok = xs >= 0 && (unsigned)ys < (unsigned)H;
      const uint32_t b = (uint32_t)(b0 + h_img[i]);
      const uint32_t sp = UP ? (b * (H / 2) + (uint32_t)(ys >> 1)) * (W / 2) + (uint32_t)(xs >> 1)
                             : (b * H + (uint32_t)ys) * W + (uint32_t)xs;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_void*)(sd + G::DYB + i * 1024), 16, ok ? sp * ldx2 + h_ch[i] : OOB,
                                               0, 0, 0);
    }
  };
  // fragment read bases (ring slot 0; the slot offset is the reads' immediate)
  const uint32_t a0 = ring_a + (uint32_t)((g4 * 8 + tq) * 64 + ((0 ^ (g4 & 1)) * 32) + tp * 8);
  const uint32_t a1 = ring_a + (uint32_t)((g4 * 8 + tq) * 64 + ((1 ^ (g4 & 1)) * 32) + tp * 8);
  uint32_t bb;
  {
    int img, y, x0;
    G::quad(g4, 0, img, y, x0);
    bb = ring_a + (uint32_t)(((img * G::HR + y) * G::WP + x0 + tq) * 32 + tp * 8);
  }
  v4f acc[2][9];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[m][t] = (v4f){0.f, 0.f, 0.f, 0.f};
  const bool bg = p.bias_grad != nullptr && cit == 0;
  float bs[2] = {0.f, 0.f};

#pragma unroll
  for (int s = 0; s < NS - 1; ++s)
    if (s < nst) stage(s, s);
  for (int s0 = 0; s0 < nst; s0 += NS) {
#define WG3_IT(J)                                                                              \
    if (s0 + (J) < nst) {                                                                      \
      const int s = s0 + (J);                                                                  \
      if (s + NS - 1 < nst) { vm_wait<G::LPS * (NS - 2)>(); }                                  \
      else { vm_wait_stages<G::LPS, NS - 2>(nst - 1 - s); }                                    \
      if (s + NS - 1 < nst) stage(((J) + NS - 1) % NS, s + NS - 1);                           \
      Wg3Stage<W, NS>::template compute<J>(a0, a1, bb, acc, bg, bs);                           \
    }
    WG3_IT(0)
    WG3_IT(1)
    if constexpr (NS > 2) { WG3_IT(2) }
    if constexpr (NS > 3) { WG3_IT(3) }
    if constexpr (NS > 4) { WG3_IT(4) }
    if constexpr (NS > 5) { WG3_IT(5) }
    if constexpr (NS > 6) { WG3_IT(6) }
    static_assert(NS <= 7, "ring slots are unrolled up to 7");
#undef WG3_IT
  }

  // ---- epilogue, one cout tile (16 couts) at a time so the LDS image stays <= the ring: every
  // wave parks its partial [16 co][9 tap][16 ci] in LDS, then all threads sum the WPG partials in
  // wave order (fixed: reproducible) over float4 runs of 4 cins and store them 16 B per lane --
  // into this chunk's slab write-through (sc1: measured 1 us faster than write-back slabs, whose
  // dirty lines the end of the kernel flushes), or into C itself without split-K ----
  constexpr int HALF = 16 * 9 * 16;
  float* red = (float*)wsm;             // [WPG][HALF]
  float* bred = red + WPG * HALF;       // [WPG][32] bias partials
  const bool slab = p.split_k > 1;
  const long MN = (long)p.M * p.N;
  float* out = (float*)p.c + (slab ? (long)z * MN : 0);
  const long ldo = slab ? p.N : p.ldc;
  const auto rso = __builtin_amdgcn_make_buffer_rsrc((void*)out, 0, 0x7FFFFFF0, 0x00020000);
  const auto rsp = __builtin_amdgcn_make_buffer_rsrc((void*)p.c, 0, 0x7FFFFFF0, 0x00020000);
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    __syncthreads();  // ring (m = 0) / the previous half's image (m = 1) no longer read
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) red[wave * HALF + ((4 * g4 + q) * 9 + t) * 16 + l16] = acc[m][t][q];
    if (m == 0 && bg) {
#pragma unroll
      for (int mm = 0; mm < 2; ++mm) {
        float v = bs[mm];
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (lane < 16) bred[wave * 32 + mm * 16 + lane] = v;
      }
    }
    __syncthreads();
    for (int f = threadIdx.x; f < HALF / 4; f += WPG * 64) {
      float4 v = *(const float4*)(red + 4 * f);
#pragma unroll
      for (int w = 1; w < WPG; ++w) {
        const float4 u = *(const float4*)(red + w * HALF + 4 * f);
        v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
      }
      const int c4 = f & 3, ct = f >> 2, t = ct % 9, co = co0 + m * 16 + ct / 9;
      const long off = (long)co * ldo + t * cin + ci0 + 4 * c4;
      if (slab && fold) {  // part-major slab [z][part][32 co][9 tap][16 ci]: no cache line shared by two parts
        const long po = ((long)z * nparts + part) * WG3_PART + (m * 16 + ct / 9) * 144 + t * 16 + 4 * c4;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u32, v), rsp, (int)(po * 4), 0, 16);
      } else if (slab) {
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u32, v), rso, (int)(off * 4), 0, 16);
      } else {
        float4* o = (float4*)(out + off);
        v.x *= p.alpha; v.y *= p.alpha; v.z *= p.alpha; v.w *= p.alpha;
        if (p.c_mode == ENCDIFF_OUT_F32_ACCUM) {
          const float4 c = *o;
          v.x += c.x; v.y += c.y; v.z += c.z; v.w += c.w;
        }
        *o = v;
      }
    }
  }
  if (bg && threadIdx.x < 32) {
    float v = bred[threadIdx.x];
#pragma unroll
    for (int w = 1; w < WPG; ++w) v += bred[w * 32 + threadIdx.x];
    const int co = co0 + threadIdx.x;
    if (slab && fold) {  // write-through, as the slab, at [cout tile][z][32]: read by the combining chunk
      const auto rsw = __builtin_amdgcn_make_buffer_rsrc((void*)p.workspace, 0, 0x7FFFFFF0, 0x00020000);
      __builtin_amdgcn_raw_buffer_store_b32(
          __builtin_bit_cast(uint32_t, v), rsw,
          (int)(((long)p.split_k * MN + ((long)cot * p.split_k + z) * 32 + threadIdx.x) * 4), 0, 16);
    } else if (slab) {
      p.workspace[(long)p.split_k * MN + (long)z * p.M + co] = v;
    } else {
      p.bias_grad[co] += v;
    }
  }
  if (!(slab && fold) || !wg_last_chunk(fold->cnt + part, p.split_k, (int*)wsm)) return;
  // the combining chunk: the part's [32 co][9 tap][16 ci] summed over the chunks in order
  const float* s0 = (const float*)p.c + (long)part * WG3_PART;
  const long zs = (long)nparts * WG3_PART;
  for (int f = threadIdx.x; f < 32 * 9 * 4; f += WPG * 64) {
    const int cl = f / 36, r = f % 36, t = r >> 2, c4 = r & 3;
    const int lo = cl * 144 + t * 16 + 4 * c4;
    float4 v = *(const float4*)(s0 + lo);
    for (int zz = 1; zz < p.split_k; ++zz) v = f4add(v, *(const float4*)(s0 + zz * zs + lo));
    wg_fold_store(*fold, (float*)fold->c + (long)(co0 + cl) * fold->ldc + t * cin + ci0 + 4 * c4, v);
  }
  if (bg && threadIdx.x < 32) {
    const float* bz = p.workspace + (long)p.split_k * MN + (long)cot * p.split_k * 32 + threadIdx.x;
    float v = bz[0];
    for (int zz = 1; zz < p.split_k; ++zz) v += bz[zz * 32];
    p.bias_grad[co0 + threadIdx.x] += v;
  }
}

// The WG3 grid: blocks [0, nblk) the weight gradient, then (BM2 > 0) the layer's input-gradient
// GEMM tiles in the same grid (as gemm2_kernel pairs two GEMM tiles: each alone leaves most of the
// chip idle), then a deferred finalize of an earlier weight gradient riding along.
template <int W, bool UP, int NS, int WPG, int BM2 = 0, int BN2 = 0, int AM2 = 0, int BMD2 = 0, int NS2 = 0>
__global__ __launch_bounds__(WPG * 64) void wgrad3x3_kernel(const EncdiffGemmArgs p, int nblk, const EncdiffGemmArgs pf,
                                                            int nf, const EncdiffGemmArgs p2, const GemmAux aux2, int gx2,
                                                            int gy2) {
  extern __shared__ __attribute__((aligned(16))) char wsm[];
  int i = blockIdx.x;
  if (i < nblk) {
    // a chunk's parts (sharing dY / x rows) on one XCD
    wgrad3x3_body<W, UP, NS, WPG, BM2 * 1000 + BN2 * 10 + AM2>(p, xcd_remap(i, nblk), wsm);
    return;
  }
  i -= nblk;
  if constexpr (BM2 > 0) {
    const int n2 = gx2 * gy2 * p2.split_k;
    if (i < n2) {
      const int bx = i % gx2, t = i / gx2;
      gemm_tile<BM2, BN2, AM2, BMD2, NS2, BK>(p2, aux2, bx, t % gy2, t / gy2, (bf16_t*)wsm);
      return;
    }
    i -= n2;
  }
  // finalize blocks (4-wave grids only: wg3_launch launches a tile-33 grid's finalize on its own)
  if (WPG != 4) return;
  gemm_finalize(pf, i, nf);
}

// tile 32: 4 waves per workgroup, paired with the layer's input gradient in one grid where the pair
// path allows; 34: 4 waves, never paired; 33: 8 waves (two per SIMD on one workgroup per CU), never
// paired; 3-deep stage rings alone, 2-deep paired
template <int W, int NS, int WPG>
constexpr size_t wg3_lds() {
  constexpr size_t ring = WPG * NS * Wg3<W>::STAGE, red = (WPG * 16 * 9 * 16 + WPG * 32) * 4;
  return ring > red ? ring : red;
}
__host__ __device__ constexpr int wg3_waves(int tile) { return tile == 33 ? 8 : 4; }
constexpr int WG3_PAIR_NS = 2;  // paired launch: 2-deep rings keep the shared LDS size small
}  // namespace
