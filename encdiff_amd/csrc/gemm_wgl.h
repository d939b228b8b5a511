#pragma once
// gemm_wgl.h -- device side of the linear weight-gradient kernel (WGL, tile 36): Wgl, WglStage,
// wgradlin_body, wgradlin_kernel and its LDS size.  Builds on gemm_tile.h (the paired
// input-gradient tiles, xcd_remap) and gemm_finalize.h (the riding finalize).
#include "gemm_finalize.h"
#include "gemm_tile.h"

namespace {
// ---------------------------------------------------------------------------
// Linear weight gradient, tile id 36 (WGL): dW[m][n] += sum_t dY[t][m] x[t][n] over T tokens
// (every nn.Linear / 1x1 conv of the UNet: attention.py proj_in/out, to_q/k/v/out, ff; the
// ResBlock skip).  Small output, long K: as WG3, a workgroup owns a 64 x 64 output part and a
// chunk of tokens, its 4 waves run independently over a quarter of the chunk each (32-token
// stages: dY and x rows, 4 KiB each, staged by LDS-DMA into the wave's own ring; 4 x 4 MFMA tiles
// per stage) and their partials are summed in LDS: one slab per chunk.  Rows are 128 B (64
// bf16); the 32-B column groups a transposed read touches are XOR-swizzled by row bits 1 and 3
// so both 16-lane groups of a 32-lane half hit distinct banks.
struct Wgl {
  static constexpr int ROWB = 128;               // 64 columns x bf16
  static constexpr int OPB = 32 * ROWB;          // one operand of a 32-token stage (4 KiB)
  static constexpr int STAGE = 2 * OPB;          // dY rows then x rows
  static constexpr int LPS = 8;                  // LDS-DMA instructions per stage
  // 16-B slot of global chunk gc (0..7) in row r
  static ED_DEV int slot(int r, int gc) { return ((((gc >> 1) ^ ((r >> 1) & 1) ^ (((r >> 3) & 1) << 1))) << 1) | (gc & 1); }
};

template <int NS>
struct WglStage {
  template <int J>
  static ED_DEV void compute(const uint32_t (&ab)[4], const uint32_t (&bb)[4], v4f (&acc)[4][4], bool bg, float (&bs)[4]) {
    constexpr int SB = J * Wgl::STAGE;
    v8bf af[4], bf[4];
#define WGL_RD(F, BASE, I, OFF) F[I] = cat8(tr16_off<SB + (OFF)>(BASE[I]), tr16_off<SB + (OFF) + 4 * Wgl::ROWB>(BASE[I]))
    WGL_RD(af, ab, 0, 0); WGL_RD(af, ab, 1, 0); WGL_RD(af, ab, 2, 0); WGL_RD(af, ab, 3, 0);
    WGL_RD(bf, bb, 0, Wgl::OPB); WGL_RD(bf, bb, 1, Wgl::OPB);
    WGL_RD(bf, bb, 2, Wgl::OPB); WGL_RD(bf, bb, 3, Wgl::OPB);
    lgkm_wait<4>();  // A and B tiles 0, 1 landed (tiles 2, 3 = the 4 youngest reads)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bf[0], acc[i][0], 0, 0, 0);
      acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bf[1], acc[i][1], 0, 0, 0);
    }
    lgkm_wait<0>();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      acc[i][2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bf[2], acc[i][2], 0, 0, 0);
      acc[i][3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bf[3], acc[i][3], 0, 0, 0);
    }
#undef WGL_RD
    if (bg) {  // bias gradient: this lane's 8 tokens of its output column in each m tile
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const v8s sv = __builtin_bit_cast(v8s, af[i]);
#pragma unroll
        for (int e = 0; e < 8; ++e) bs[i] += bf2f((bf16_t)sv[e]);
      }
    }
  }
};

template <int NS, int TAG = 0>
__device__ __forceinline__ void wgradlin_body(const EncdiffGemmArgs& p, const int bid, char* wsm,
                                              const SplitFold* fold = nullptr) {
  typedef __attribute__((address_space(3))) void lds_void;
  const int ntn = p.N >> 6, nparts = (p.M >> 6) * ntn;
  const int z = bid / nparts, part = bid - z * nparts;  // bid: the caller's logical block
  const int mt = part / ntn, nt = part - mt * ntn;
  const int m0 = mt * 64, n0 = nt * 64;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int l16 = lane & 15, g4 = lane >> 4, tq = l16 >> 2, tp = l16 & 3;
  const int tpz = p.K / p.split_k;        // tokens of this chunk
  const int nst = tpz / (32 * 4);         // 32-token stages of this wave
  const int t0 = z * tpz + wave * nst * 32;
  char* ring = wsm + wave * (NS * Wgl::STAGE);
  const uint32_t ring_a = lds_addr(ring);
  const auto rsA = __builtin_amdgcn_make_buffer_rsrc((void*)p.a, 0, 0x7FFFFFF0, 0x00020000);
  const auto rsB = __builtin_amdgcn_make_buffer_rsrc((void*)p.b, 0, 0x7FFFFFF0, 0x00020000);
  const uint32_t lda2 = (uint32_t)p.lda * 2u, ldb2 = (uint32_t)p.ldb * 2u;
  // staging: LDS chunk c = lane + 64 i of an operand -> row r = c / 8, slot c % 8 holds global chunk gc
  uint32_t a_off[4], b_off[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = lane + 64 * i, r = c >> 3, sl = c & 7;
    int gc = 0;
#pragma unroll
    for (int g = 0; g < 8; ++g)
      if (Wgl::slot(r, g) == sl) gc = g;
    a_off[i] = (uint32_t)r * lda2 + (uint32_t)(m0 + gc * 8) * 2u;
    b_off[i] = (uint32_t)r * ldb2 + (uint32_t)(n0 + gc * 8) * 2u;
  }
  auto stage = [&](int slot, int sw) {
    char* sd = ring + slot * Wgl::STAGE;
    const uint32_t row0 = (uint32_t)(t0 + sw * 32);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_void*)(sd + i * 1024), 16, a_off[i] + row0 * lda2, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_void*)(sd + Wgl::OPB + i * 1024), 16, b_off[i] + row0 * ldb2, 0,
                                               0, 0);
  };
  // fragment bases (ring slot 0, first 4 rows of the lane's k group): column tile i at row r
  uint32_t ab[4], bb[4];
  {
    const int r = g4 * 8 + tq;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int gc = 2 * i + (tp >> 1);  // 16-B chunk of columns 16 i + 4 tp .. + 3
      const uint32_t o = (uint32_t)(r * Wgl::ROWB + Wgl::slot(r, gc) * 16 + (tp & 1) * 8);
      ab[i] = ring_a + o;
      bb[i] = ring_a + o;
    }
  }
  // (rows r and r + 4 differ in bit 2 only: same swizzle, the second read is 4 rows on)
  v4f acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (v4f){0.f, 0.f, 0.f, 0.f};
  const bool bg = p.bias_grad != nullptr && nt == 0;
  float bs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < NS - 1; ++s)
    if (s < nst) stage(s, s);
  for (int s0 = 0; s0 < nst; s0 += NS) {
#define WGL_IT(J)                                                                              \
    if (s0 + (J) < nst) {                                                                      \
      const int s = s0 + (J);                                                                  \
      if (s + NS - 1 < nst) { vm_wait<Wgl::LPS * (NS - 2)>(); }                                \
      else { vm_wait_stages<Wgl::LPS, NS - 2>(nst - 1 - s); }                                  \
      if (s + NS - 1 < nst) stage(((J) + NS - 1) % NS, s + NS - 1);                           \
      WglStage<NS>::template compute<J>(ab, bb, acc, bg, bs);                                  \
    }
    WGL_IT(0)
    WGL_IT(1)
    if constexpr (NS > 2) { WGL_IT(2) }
    if constexpr (NS > 3) { WGL_IT(3) }
    static_assert(NS <= 4, "ring slots are unrolled up to 4");
#undef WGL_IT
  }
  // ---- epilogue (as WG3's): 32 output rows at a time through LDS, partials summed in wave order
  constexpr int HALF = 32 * 64;
  float* red = (float*)wsm;        // [4][HALF]
  float* bred = red + 4 * HALF;    // [4][64]
  const bool slab = p.split_k > 1;
  const long MN = (long)p.M * p.N;
  float* out = (float*)p.c + (slab ? (long)z * MN : 0);
  const long ldo = slab ? p.N : p.ldc;
  const auto rso = __builtin_amdgcn_make_buffer_rsrc((void*)out, 0, 0x7FFFFFF0, 0x00020000);
  const auto rsp = __builtin_amdgcn_make_buffer_rsrc((void*)p.c, 0, 0x7FFFFFF0, 0x00020000);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) red[wave * HALF + (i * 16 + 4 * g4 + q) * 64 + j * 16 + l16] = acc[2 * h + i][j][q];
    if (h == 0 && bg) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float v = bs[i];
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (lane < 16) bred[wave * 64 + i * 16 + lane] = v;
      }
    }
    __syncthreads();
    for (int f = threadIdx.x; f < HALF / 4; f += 256) {
      float4 v = *(const float4*)(red + 4 * f);
#pragma unroll
      for (int w = 1; w < 4; ++w) {
        const float4 u = *(const float4*)(red + w * HALF + 4 * f);
        v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
      }
      const int row = m0 + h * 32 + (f >> 4), col = n0 + 4 * (f & 15);
      const long off = (long)row * ldo + col;
      if (slab && fold) {  // part-major slab [z][part][64][64]: no cache line shared by two parts
        const long po = ((long)z * nparts + part) * WGL_PART + (h * 32 + (f >> 4)) * 64 + 4 * (f & 15);
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
  if (bg && threadIdx.x < 64) {
    float v = bred[threadIdx.x];
#pragma unroll
    for (int w = 1; w < 4; ++w) v += bred[w * 64 + threadIdx.x];
    const int m = m0 + threadIdx.x;
    if (slab && fold) {  // write-through, as the slab, at [row tile][z][64]: read by the combining chunk
      const auto rsw = __builtin_amdgcn_make_buffer_rsrc((void*)p.workspace, 0, 0x7FFFFFF0, 0x00020000);
      __builtin_amdgcn_raw_buffer_store_b32(
          __builtin_bit_cast(uint32_t, v), rsw,
          (int)(((long)p.split_k * MN + ((long)mt * p.split_k + z) * 64 + threadIdx.x) * 4), 0, 16);
    } else if (slab) {
      p.workspace[(long)p.split_k * MN + (long)z * p.M + m] = v;
    } else {
      p.bias_grad[m] += v;
    }
  }
  if (!(slab && fold) || !wg_last_chunk(fold->cnt + part, p.split_k, (int*)wsm)) return;
  // the combining chunk: the 64 x 64 part summed over the chunks in order, 16 B per lane
  const float* s0 = (const float*)p.c + (long)part * WGL_PART;
  const long zs = (long)nparts * WGL_PART;
  for (int f = threadIdx.x; f < 64 * 16; f += 256) {
    const int lo = (f >> 4) * 64 + 4 * (f & 15);
    float4 v = *(const float4*)(s0 + lo);
    for (int zz = 1; zz < p.split_k; ++zz) v = f4add(v, *(const float4*)(s0 + zz * zs + lo));
    wg_fold_store(*fold, (float*)fold->c + (long)(m0 + (f >> 4)) * fold->ldc + n0 + 4 * (f & 15), v);
  }
  if (bg && threadIdx.x < 64) {
    const float* bz = p.workspace + (long)p.split_k * MN + (long)mt * p.split_k * 64 + threadIdx.x;
    float v = bz[0];
    for (int zz = 1; zz < p.split_k; ++zz) v += bz[zz * 64];
    p.bias_grad[m0 + threadIdx.x] += v;
  }
}

// The WGL grid: [0, nblk) the weight gradient, then (BM2 > 0) the layer's input-gradient GEMM tiles,
// then a deferred finalize riding along
template <int NS, int BM2 = 0, int BN2 = 0, int AM2 = 0, int BMD2 = 0, int NS2 = 0, int KB2 = BK>
__global__ __launch_bounds__(256) void wgradlin_kernel(const EncdiffGemmArgs p, int nblk, const EncdiffGemmArgs pf, int nf,
                                                       const EncdiffGemmArgs p2, const GemmAux aux2, int gx2, int gy2) {
  extern __shared__ __attribute__((aligned(16))) char wsm[];
  int i = blockIdx.x;
  if (i < nblk) {
    // a chunk's parts (sharing dY / x rows) on one XCD
    wgradlin_body<NS, BM2 * 100000 + BN2 * 100 + NS2 * 10 + (KB2 == BK ? 0 : 1)>(p, xcd_remap(i, nblk), wsm);
    return;
  }
  i -= nblk;
  if constexpr (BM2 > 0) {
    const int n2 = gx2 * gy2 * p2.split_k;
    if (i < n2) {
      const int bx = i % gx2, t = i / gx2;
      gemm_tile<BM2, BN2, AM2, BMD2, NS2, KB2>(p2, aux2, bx, t % gy2, t / gy2, (bf16_t*)wsm);
      return;
    }
    i -= n2;
  }
  gemm_finalize(pf, i, nf);
}

constexpr int WGL_NS = 3, WGL_PAIR_NS = 2;
template <int NS>
constexpr size_t wgl_lds() {
  constexpr size_t ring = 4 * NS * Wgl::STAGE, red = (4 * 32 * 64 + 4 * 64) * 4;
  return ring > red ? ring : red;
}
}  // namespace
