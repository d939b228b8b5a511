#pragma once
// gemm_tile.h -- the tile engine: gemm_tile() (one output tile of one split: staging, k-loop,
// epilogue), the XCD tile order, gemm_kernel and the paired gemm2_kernel.  Builds on
// gemm_common.h and gemm_finalize.h (the finalize blocks that ride in gemm2_kernel's grid).
#include "gemm_common.h"
#include "gemm_finalize.h"

namespace {
// One output tile (bx, by) of split bz.  Shared by the single-GEMM kernel and the paired
// kernel that runs two independent GEMMs (a layer's input- and weight-gradient) in one grid.
template <int BM, int BN, int AM, int BMD, int NS = 2, int KB = BK>
__device__ __forceinline__ void gemm_tile(const EncdiffGemmArgs& p, const GemmAux& aux, const int bx, const int by,
                                          const int bz, bf16_t* smem) {
  using G = Gemm<BM, BN, AM, BMD, NS, KB>;
  constexpr int BK = G::KT;  // shadows the default stage depth
  using TA = typename G::TA;
  using TB = typename G::TB;
  constexpr bool AKI = G::AKI, BKI = G::BKI;
  constexpr int TM = G::TM, TN = G::TN;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = (wave >> 1) * (BM / 2);
  const int wc = (wave & 1) * (BN / 2);
  const int m0 = bx * BM;
  const int n0 = by * BN;

  // split-K range
  const int ktiles_total = (p.K + BK - 1) / BK;
  const int kt_per = (ktiles_total + p.split_k - 1) / p.split_k;
  const int kt_begin = bz * kt_per;
  const int kt_end = min(ktiles_total, kt_begin + kt_per);
  int nkt = kt_end - kt_begin;
  // halo tiles with split-K: split bz owns the source channels [hcb, hcb + 8 h.ch) of every tap
  // (the window holds that slice only); its k-tiles run tap by tap over the slice's 64-channel
  // groups, k-tile (tap, g) = tap * cin / 64 + bz * ncc + g
  uint32_t hcb = 0;
  int kt_ncc = 0, kt_c64 = 0;
  if constexpr (G::HALO) {
    if (p.split_k > 1) {
      kt_ncc = aux.halo.ch >> 3;
      kt_c64 = p.conv.cin >> 6;
      hcb = (uint32_t)(bz * aux.halo.ch * 8);
      nkt = aux.halo.kt * aux.halo.kt * kt_ncc;
    }
  }
  auto ktile = [&](int it) -> int {
    if constexpr (G::HALO) {
      if (kt_ncc) {
        const int tap = it / kt_ncc;
        return tap * kt_c64 + bz * kt_ncc + (it - tap * kt_ncc);
      }
    }
    return kt_begin + it;
  };

  const bf16_t* __restrict__ A = (const bf16_t*)p.a;
  const bf16_t* __restrict__ B = (const bf16_t*)p.b;

  Im2colMode md(p.conv);
  // K4S2_TP: rows [parity][b][y'][x'], one parity per tile (host: batch*h*w/4 % 128 == 0)
  const int tp_q = md.k4 == 2 ? m0 / (p.M >> 2) : 0;
  const uint32_t mbase = md.k4 == 2 ? (uint32_t)(tp_q * (p.M >> 2)) : 0u;
  if (md.k4 == 2) md.set_parity(tp_q);

  // LDS-DMA staging: every chunk's global address is computed branch-free (masked chunks
  // read g_zero16) and copied straight into the lane-linear LDS image; tile t+1 is in
  // flight while tile t is multiplied (depth-1 prefetch, no staging VGPRs).
  typedef __attribute__((address_space(3))) void lds_void;
  typedef __attribute__((address_space(1))) const void gbl_void;
  // GEGLU proj (OUT_BF16_GEGLU): tile column c < BN/2 is value column by*BN/2 + c of f, the
  // rest gate column N/2 + by*BN/2 + c - BN/2, so one tile holds both halves of its outputs
  const bool gfwd = p.c_mode == ENCDIFF_OUT_BF16_GEGLU;
  auto gcol = [&](int c) -> int {
    return c < BN / 2 ? by * (BN / 2) + c : (p.N >> 1) + by * (BN / 2) + c - BN / 2;
  };
  // halo mode: the window sits at the LDS base, the B ring behind it
  bf16_t* ring = smem;
  if constexpr (G::HALO) ring = smem + aux.halo.chunks * 8;
  auto stage_halo = [&]() {
    const HaloGeom& h = aux.halo;
    const uint32_t b0 = fdiv((uint32_t)m0, aux.hw);
    const uint32_t y0 = fdiv((uint32_t)m0 - b0 * aux.hw.d, aux.w);  // 0 when the tile holds whole images
    const int cy0 = h.s * (int)y0 + h.off;
    for (int c = tid; c < h.chunks; c += 256) {
      const uint32_t px = fdiv((uint32_t)c, h.fch);
      const int gch = (c - (int)(px * (uint32_t)h.ch)) ^ ((int)(px >> h.xsh) & h.xmsk);
      const uint32_t j = fdiv(px, h.fimg);
      const uint32_t r = px - j * h.fimg.d;
      const uint32_t hy = fdiv(r, h.fhc);
      const int cy = cy0 + (int)hy, cx = h.off + (int)(r - hy * (uint32_t)h.hc);
      const bool ok = (int)px < h.npix && (unsigned)cy < (unsigned)h.lh && (unsigned)cx < (unsigned)h.lw;
      const uint32_t row = ((b0 + j) * (uint32_t)h.hs + (uint32_t)(cy >> h.ush)) * (uint32_t)h.ws + (uint32_t)(cx >> h.ush);
      const void* src = ok ? (const void*)(A + (size_t)row * p.conv.ld_src + hcb + gch * 8) : (const void*)&g_zero16;
      __builtin_amdgcn_global_load_lds((gbl_void*)src, (lds_void*)(smem + (c & ~63) * 8), 16, 0, 0);
    }
  };
  // Staging addresses.  Buffer-resource LDS-DMA with 32-bit byte offsets (host: every operand
  // spans < 2^31 bytes); a masked chunk (padding tap, tile tail) gets an out-of-range offset and
  // the DMA writes zeros.  What does not depend on the k-tile is computed once per thread here,
  // so a chunk costs a few adds and compares per k-tile: the earlier form (64-bit addresses, a
  // zero-page pointer per masked chunk, the pixel / tap decomposition redone per chunk) issued
  // 20-30 VALU per 16-byte chunk and left the MFMA pipe idle behind the address arithmetic.
  constexpr uint32_t OOB = 0x80000000u;
  const auto rsA = __builtin_amdgcn_make_buffer_rsrc((void*)A, 0, 0x7FFFFFF0, 0x00020000);
  const auto rsB = __builtin_amdgcn_make_buffer_rsrc((void*)B, 0, 0x7FFFFFF0, 0x00020000);
  constexpr int APT = G::HALO ? 0 : TA::PER_THREAD, BPT = TB::PER_THREAD;
  const uint32_t ldsrc2 = (uint32_t)p.conv.ld_src * 2u;
  // a k-tile of an im2col / flipped-weight operand lies inside one tap: tap and channel base are
  // uniform per k-tile
  const bool a_tapk = G::IM2 && (p.conv.cin % BK) == 0;
  const bool b_tapk = BMD == B_CONVD && (p.conv_cout % BK) == 0;
  // weight-gradient im2col operand (k = output pixel): with w | BK and hw | BK or BK | hw, pixel
  // k0 + r splits into a uniform part of k0 and a per-lane part of r (no per-k-tile division)
  bool b_pix = false;
  if constexpr (BMD == B_IM2COL) b_pix = (BK % aux.w.d) == 0 && ((aux.hw.d % BK) == 0 || (BK % aux.hw.d) == 0);
  uint32_t a_off[APT > 0 ? APT : 1];  // invariant byte offset (OOB: masked row)
  int a_k[APT > 0 ? APT : 1], a_y[APT > 0 ? APT : 1], a_x[APT > 0 ? APT : 1];
  int a_bl[APT > 0 ? APT : 1];  // AGN: the chunk row's image, relative to the tile's first image
  uint32_t agn_b0 = 0;          // AGN: the tile's first image
  uint32_t b_off[BPT], b_n2[BPT];
  int b_k[BPT], b_ys[BPT];
  uint32_t b_base[BPT], b_xsh[BPT];
#pragma unroll
  for (int i = 0; i < APT; ++i) {
    const int c = tid + 256 * i;
    const int row = c / TA::SLOTS, slot = c % TA::SLOTS;
    const int gs = TA::sw(row, slot);
    if constexpr (AM == A_ROWK || AM == A_ROWK_LN) {
      const int m = m0 + row;
      a_y[i] = row;  // LNA: the chunk's tile row (its LayerNorm statistics)
      a_k[i] = gs * 8;
      a_off[i] = m < p.M ? ((uint32_t)m * (uint32_t)p.lda + (uint32_t)(gs * 8)) * 2u : OOB;
    } else if constexpr (AM == A_ROWM) {
      const int m = m0 + gs * 8;
      a_k[i] = row;
      a_off[i] = m < p.M ? ((uint32_t)row * (uint32_t)p.lda + (uint32_t)m) * 2u : OOB;
    } else if constexpr (G::IM2) {  // this row = output pixel (fixed): source window origin
      const uint32_t mm0 = (uint32_t)(m0 + row);
      const bool min = mm0 < (uint32_t)p.M;
      const uint32_t mm = min ? mm0 - mbase : 0u;
      const uint32_t bb = fdiv(mm, aux.hw);
      if constexpr (G::AGN) a_bl[i] = (int)(bb - fdiv((uint32_t)m0, aux.hw));
      const uint32_t r = mm - bb * aux.hw.d;
      const int y = (int)fdiv(r, aux.w), x = (int)(r - (uint32_t)y * aux.w.d);
      a_k[i] = gs * 8;
      a_y[i] = min ? md.sy * y + md.oy : (1 << 28);  // out of range: masked row
      a_x[i] = md.sy * x + md.ox;
      a_off[i] = bb * (uint32_t)md.hs;
    }
  }
#pragma unroll
  for (int i = 0; i < BPT; ++i) {
    const int c = tid + 256 * i;
    const int row = c / TB::SLOTS, slot = c % TB::SLOTS;
    const int gs = TB::sw(row, slot);
    if constexpr (BKI) {  // B_ROWK: Bt[n][k], row = n
      const int n = gfwd ? gcol(row) : n0 + row;
      b_k[i] = gs * 8;
      b_off[i] = n < p.N ? ((uint32_t)n * (uint32_t)p.ldb + (uint32_t)(gs * 8)) * 2u : OOB;
    } else {  // k-outer: row = k, chunk = 8 columns of n
      const int n = n0 + gs * 8;
      b_k[i] = row;
      if constexpr (BMD == B_ROWN || BMD == B_CONVD) {
        b_off[i] = n < p.N ? ((uint32_t)row * (uint32_t)p.ldb + (uint32_t)n) * 2u : OOB;
        b_n2[i] = n < p.N ? (uint32_t)n * 2u : OOB;
      } else {  // B_IM2COL: column n = (tap, ci), invariant; row = pixel offset in the k-tile
        const uint32_t nn = n < p.N ? (uint32_t)n : 0u;
        const uint32_t tap = fdiv(nn, aux.cin);
        const uint32_t ci = nn - tap * (uint32_t)p.conv.cin;
        int ty, tx;
        tap_yx(md, tap, ty, tx);
        b_n2[i] = n < p.N ? ci * 2u : OOB;
        b_off[i] = (uint32_t)(ty * 16 + tx);  // general path: tap offsets
        if (b_pix) {
          const uint32_t bl = fdiv((uint32_t)row, aux.hw), rl = (uint32_t)row - bl * aux.hw.d;
          const uint32_t yl = fdiv(rl, aux.w), xl = rl - yl * aux.w.d;
          const int xs = md.sy * (int)xl + tx + md.ox;
          const bool xok = (unsigned)xs < (unsigned)md.lw && (xs & md.par) == 0 && n < p.N;
          b_ys[i] = xok ? md.sy * (int)yl + ty + md.oy : (1 << 28);
          b_base[i] = bl * (uint32_t)md.hs;
          b_xsh[i] = (uint32_t)(xs >> md.sh);
        }
      }
    }
  }
  auto stage = [&](bf16_t* s, int kt) {
    const int k0 = kt * BK;
    bf16_t* sa = s;
    bf16_t* sb = s + G::ASTAGE;
    // uniform per-k-tile values
    uint32_t a_ch = 0u, b_cv = 0u, b_pb = 0u;
    int a_ty = 0, a_tx = 0, b_yo = 0;
    if constexpr (G::IM2) {
      if (a_tapk) {
        const uint32_t tap = fdiv((uint32_t)k0, aux.cin);
        a_ch = (uint32_t)k0 - tap * (uint32_t)p.conv.cin;
        tap_yx(md, tap, a_ty, a_tx);
      }
    }
    if constexpr (BMD == B_CONVD) {
      if (b_tapk) {
        const uint32_t tap = fdiv((uint32_t)k0, aux.cout);
        const uint32_t co = (uint32_t)k0 - tap * (uint32_t)p.conv_cout;
        b_cv = (co * (uint32_t)p.ldb + md.wtap(tap) * (uint32_t)p.N) * 2u;
      }
    }
    if constexpr (BMD == B_IM2COL) {
      if (b_pix) {
        const uint32_t bs = fdiv((uint32_t)k0, aux.hw);
        const uint32_t ys = fdiv((uint32_t)k0 - bs * aux.hw.d, aux.w);
        b_yo = md.sy * (int)ys;
        b_pb = bs * (uint32_t)md.hs;
      }
    }
#pragma unroll
    for (int i = 0; i < APT; ++i) {
      const int c = tid + 256 * i;  // LDS chunk position (lane-linear)
      const int k = k0 + a_k[i];
      uint32_t vo;
      if constexpr (AM == A_ROWK || AM == A_ROWK_LN) {
        vo = k < p.K ? a_off[i] + 2u * (uint32_t)k0 : OOB;
      } else if constexpr (AM == A_ROWM) {
        vo = k < p.K ? a_off[i] + (uint32_t)k0 * (uint32_t)p.lda * 2u : OOB;
      } else {  // IM2COL
        uint32_t ch;
        int ty, tx;
        if (a_tapk) {
          ch = a_ch + (uint32_t)a_k[i];
          ty = a_ty;
          tx = a_tx;
        } else {
          const uint32_t kk = k < p.K ? (uint32_t)k : 0u;
          const uint32_t tap = fdiv(kk, aux.cin);
          ch = kk - tap * (uint32_t)p.conv.cin;
          tap_yx(md, tap, ty, tx);
        }
        const int ys = a_y[i] + ty, xs = a_x[i] + tx;
        const bool ok = k < p.K && (unsigned)ys < (unsigned)md.lh && (unsigned)xs < (unsigned)md.lw &&
                        ((ys | xs) & md.par) == 0;
        const uint32_t prow = (a_off[i] + (uint32_t)(ys >> md.sh)) * (uint32_t)md.ws + (uint32_t)(xs >> md.sh);
        vo = ok ? prow * ldsrc2 + ch * 2u : OOB;
      }
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_void*)(sa + (c & ~63) * 8), 16, vo, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < BPT; ++i) {
      const int c = tid + 256 * i;
      const int k = k0 + b_k[i];
      uint32_t vo;
      if constexpr (BKI) {
        vo = k < p.K ? b_off[i] + 2u * (uint32_t)k0 : OOB;
      } else if constexpr (BMD == B_ROWN) {
        vo = k < p.K ? b_off[i] + (uint32_t)k0 * (uint32_t)p.ldb * 2u : OOB;
      } else if constexpr (BMD == B_CONVD) {
        if (b_tapk) {
          vo = k < p.K ? b_off[i] + b_cv : OOB;
        } else {
          const uint32_t kk = k < p.K ? (uint32_t)k : 0u;
          const uint32_t tap = fdiv(kk, aux.cout);
          const uint32_t co = kk - tap * (uint32_t)p.conv_cout;
          vo = k < p.K ? b_n2[i] + (co * (uint32_t)p.ldb + md.wtap(tap) * (uint32_t)p.N) * 2u : OOB;
        }
      } else {  // B_IM2COL
        if (b_pix) {
          const int ys = b_ys[i] + b_yo;
          const bool ok = k < p.K && (unsigned)ys < (unsigned)md.lh && (ys & md.par) == 0;
          const uint32_t prow = (b_pb + b_base[i] + (uint32_t)(ys >> md.sh)) * (uint32_t)md.ws + b_xsh[i];
          vo = ok ? prow * ldsrc2 + b_n2[i] : OOB;
        } else {
          const uint32_t kk = k < p.K ? (uint32_t)k : 0u;
          const uint32_t bb = fdiv(kk, aux.hw);
          const uint32_t r = kk - bb * aux.hw.d;
          const int y = (int)fdiv(r, aux.w), x = (int)(r - (uint32_t)y * aux.w.d);
          const int ty = (int)(b_off[i] >> 4), tx = (int)(b_off[i] & 15u);
          bool inb;
          const uint32_t prow = im2col_row(md, bb, y, x, ty, tx, inb);
          vo = (k < p.K && inb) ? prow * ldsrc2 + b_n2[i] : OOB;
        }
      }
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_void*)(sb + (c & ~63) * 8), 16, vo, 0, 0, 0);
    }
  };

  v4f acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = (v4f){0.f, 0.f, 0.f, 0.f};

  // optional bias-gradient: column sums of the (k-outer) A operand over K
  const bool do_bgrad = (AM == A_ROWM) && p.bias_grad != nullptr && by == 0;
  float bsum = 0.f;

  const int l16 = lane & 15;
  const int g4 = lane >> 4;
  const int tq = l16 >> 2, tp = l16 & 3;  // transpose-read address roles

  auto frag_kinner = [&](const bf16_t* s, int row, int kk, int mask) -> v8bf {
    return *(const v8bf*)(s + row * BK + swz(row, kk * 4 + g4, mask) * 8);
  };
  auto frag_kinner_asm = [&](const bf16_t* s, int row, int kk, int mask) -> v8bf {
    return ds_read_b128(s + row * BK + swz(row, kk * 4 + g4, mask) * 8);
  };
  auto frag_kouter = [&](auto tile, const bf16_t* s, int colbase, int kk) -> v8bf {
    // rows k = kk*32 + g4*8 + tq (+4): 4 bf16 at column colbase + 4*tp, swizzled chunk
    using T = decltype(tile);
    typedef __attribute__((address_space(3))) v4s lds_v4s;
    const int r0 = kk * 32 + g4 * 8 + tq, r1 = r0 + 4;
    const int ch = (colbase >> 3) + (tp >> 1), sub = (tp & 1) * 4;
    v4s lo = ds_read_tr16(s + r0 * T::LD + T::sw(r0, ch) * 8 + sub);
    v4s hi = ds_read_tr16(s + r1 * T::LD + T::sw(r1, ch) * 8 + sub);
    v8s r = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(v8bf, r);
  };

  // halo mode: window pixel of each of this lane's fragment rows at tap (0, 0)
  uint32_t hpb[TM];
  if constexpr (G::HALO) {
    const HaloGeom& h = aux.halo;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const uint32_t m = (uint32_t)(wr + 16 * i + l16);
      const uint32_t j = fdiv(m, aux.hw), rr = m - j * aux.hw.d;
      const uint32_t ry = fdiv(rr, aux.w), rx = rr - ry * aux.w.d;
      hpb[i] = j * h.fimg.d + (uint32_t)h.s * (ry * (uint32_t)h.hc + rx);
    }
  }
  auto frag_halo = [&](int kt, int kk, int i) -> v8bf {
    const HaloGeom& h = aux.halo;
    uint32_t k = (uint32_t)(kt * BK + kk * 32 + g4 * 8);
    if (k >= (uint32_t)p.K) k = 0;  // tail of the last k-tile: B is zero there, keep A finite
    const uint32_t tap = fdiv(k, aux.cin), ci = k - tap * (uint32_t)p.conv.cin - hcb;
    const uint32_t ty = h.kt == 4 ? tap >> 2 : (tap * 11u) >> 5;
    const uint32_t hp = hpb[i] + ty * (uint32_t)h.hc + (tap - (uint32_t)h.kt * ty);
    const uint32_t slot = (ci >> 3) ^ ((hp >> h.xsh) & (uint32_t)h.xmsk);
    return *(const v8bf*)(smem + (hp * (uint32_t)h.ch + slot) * 8);
  };

  auto compute = [&](const bf16_t* s, int kt) {
    const bf16_t* sa = s;
    const bf16_t* sb = s + G::ASTAGE;
    if (do_bgrad) {
      // BM columns x BK rows; 256 threads -> 256/BM row-groups
      constexpr int RG = 256 / BM;
      const int col = tid % BM, rg = tid / BM;
#pragma unroll 4
      for (int r = rg * (BK / RG); r < (rg + 1) * (BK / RG); ++r)
        bsum += bf2f(sa[r * TA::LD + TA::sw(r, col >> 3) * 8 + (col & 7)]);
    }
    constexpr int KK = BK / 32;
    if constexpr (ED_FRAG_PIPE && (!AKI || !BKI) && !G::HALO && KK > 1) {
      // Tiles with a transposed (k-outer) operand read every fragment by inline asm, so the
      // waits are ours: the fragments of k-substep kk+1 are issued BEFORE the MFMAs of kk, which
      // wait only for kk's reads (counted lgkmcnt: LDS returns in order) -- the LDS latency of
      // the next substep hides behind this one's MFMAs instead of draining to zero each time.
      constexpr int RA = AKI ? 1 : 2, RB = BKI ? 1 : 2;
      constexpr int NR = TM * RA + TN * RB;          // LDS read instructions per substep
      constexpr int NW = NR > 15 ? 15 : NR;           // lgkmcnt is 4 bits: over-wait when larger
      v8bf af[2][TM], bfr[2][TN];
      auto load = [&](int kk, v8bf* a, v8bf* b) {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          if constexpr (AKI) a[i] = frag_kinner_asm(sa, wr + 16 * i + l16, kk, TA::SWM);
          else a[i] = frag_kouter(TA{}, sa, wr + 16 * i, kk);
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          if constexpr (BKI) b[j] = frag_kinner_asm(sb, wc + 16 * j + l16, kk, TB::SWM);
          else b[j] = frag_kouter(TB{}, sb, wc + 16 * j, kk);
        }
      };
      load(0, af[0], bfr[0]);
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        const int cur = kk & 1;
        if (kk + 1 < KK) {
          load(kk + 1, af[cur ^ 1], bfr[cur ^ 1]);
          asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(NW) : "memory");
        } else {
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[cur][i], bfr[cur][j], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      return;
    }
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      v8bf af[TM], bfr[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        if constexpr (G::HALO) af[i] = frag_halo(kt, kk, i);
        else if constexpr (AKI) af[i] = frag_kinner(sa, wr + 16 * i + l16, kk, TA::SWM);
        else af[i] = frag_kouter(TA{}, sa, wr + 16 * i, kk);
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        if constexpr (BKI) bfr[j] = frag_kinner(sb, wc + 16 * j + l16, kk, TB::SWM);
        else bfr[j] = frag_kouter(TB{}, sb, wc + 16 * j, kk);
      }
      if constexpr (!AKI || !BKI) {  // asm transposed reads: wait for them before the MFMAs use them
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
  };

  // AGN (EncdiffGemmArgs.agn_*): GroupNorm32(+FiLM)(+SiLU) of the im2col source, folded into the
  // staging.  Prologue: the statistics of every image the tile's rows read, from x itself (per
  // channel sum / sum of squares over the image's pixels -- thread = (8-channel vector, pixel
  // lane), lanes added in order -- then per group), turned into per-(image, channel) affine
  // coefficients z = x * mul + add (mul = rstd gamma (1 + scale), add = (beta - mean rstd gamma)
  // (1 + scale) + shift) in LDS behind the ring.  Per k-tile: every thread rewrites its own staged
  // A chunks in place (after its LDS-DMA landed, before the barrier that publishes the tile);
  // zero-padding chunks stay zero.
  float2* agn_coef = (float2*)((char*)smem + G::LDS_BYTES);
  if constexpr (G::AGN) {
    const int cin = p.conv.cin, nv = cin >> 3, cpg = cin >> 5;
    const int shw = md.hs * md.ws;  // source image pixels (UP2: the half-resolution image)
    const uint32_t last = min((uint32_t)(m0 + BM), (uint32_t)p.M) - 1u;
    agn_b0 = fdiv((uint32_t)m0, aux.hw);
    const int nimg = (int)fdiv(last, aux.hw) - (int)agn_b0 + 1;
    const int tv = tid % nv, tp = tid / nv, np = 256 / nv;  // host: cin <= 1024
    // pixel lanes per image: every image of the tile in ONE pass of loads (small levels hold many
    // images per 64-row tile; a loop over images serialised a global round trip per image)
    const int lpi = np / nimg > 0 ? np / nimg : 1, ipass = np / lpi;
    float* red = (float*)smem;        // [2][np][cin] per-lane partials (the ring is not staged yet)
    float* gst = red + 2 * np * cin;  // [nimg][32][2]
    float2* chs = agn_coef;           // [nimg][cin] (sum, sum of squares), then the coefficients
    const long lds = p.conv.ld_src;
    for (int j0 = 0; j0 < nimg; j0 += ipass) {
      const int j = j0 + tp / lpi, li = tp - (tp / lpi) * lpi;
      float sa[8], sq[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) sa[i] = sq[i] = 0.f;
      if (tp < ipass * lpi && j < nimg) {
        const bf16_t* xb = A + (size_t)(agn_b0 + j) * shw * lds + tv * 8;
        for (int px0 = li; px0 < shw; px0 += 8 * lpi) {
          uint4 u[8];
#pragma unroll
          for (int r = 0; r < 8; ++r) {
            const int px = px0 + r * lpi;
            u[r] = px < shw ? *(const uint4*)(xb + (size_t)px * lds) : make_uint4(0u, 0u, 0u, 0u);
          }
#pragma unroll
          for (int r = 0; r < 8; ++r) {
            float v[8];
            unpack8(u[r], v);
#pragma unroll
            for (int i = 0; i < 8; ++i) { sa[i] += v[i]; sq[i] += v[i] * v[i]; }
          }
        }
      }
      if (tp < np) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          red[tp * cin + tv * 8 + i] = sa[i];
          red[(np + tp) * cin + tv * 8 + i] = sq[i];
        }
      }
      __syncthreads();
      for (int e = tid; e < ipass * cin; e += 256) {  // (image, channel): its lanes added in order
        const int jj = e / cin, c = e - jj * cin;
        if (j0 + jj < nimg) {
          float a = 0.f, q = 0.f;
          for (int r = jj * lpi; r < (jj + 1) * lpi; ++r) { a += red[r * cin + c]; q += red[(np + r) * cin + c]; }
          chs[(j0 + jj) * cin + c] = make_float2(a, q);
        }
      }
      __syncthreads();
    }
    for (int e = tid; e < nimg * 32; e += 256) {  // (image, group) statistics
      const int j = e >> 5, g = e & 31;
      float a = 0.f, q = 0.f;
      for (int c = g * cpg; c < (g + 1) * cpg; ++c) { const float2 v = chs[j * cin + c]; a += v.x; q += v.y; }
      const float inv = 1.f / ((float)shw * (float)cpg);
      const float mean = a * inv, var = fmaxf(q * inv - mean * mean, 0.f);
      gst[2 * e] = mean;
      gst[2 * e + 1] = rsqrtf(var + p.agn_eps);
    }
    __syncthreads();
    for (int e = tid; e < nimg * cin; e += 256) {  // coefficients, in place of the channel sums
      const int j = e / cin, c = e - j * cin, g = c / cpg, b = (int)agn_b0 + j;
      float mul = gst[2 * (j * 32 + g) + 1] * p.agn_gamma[c];
      float add = p.agn_beta[c] - gst[2 * (j * 32 + g)] * mul;
      if (p.agn_film) {
        const float sc = 1.f + p.agn_film[(long)b * p.ld_agn_film + c];
        mul *= sc;
        add = add * sc + p.agn_film[(long)b * p.ld_agn_film + cin + c];
      }
      agn_coef[e] = make_float2(mul, add);
    }
    __syncthreads();  // the ring is staged next
  }
  auto agn_transform = [&](bf16_t* sa, int kt) {
    const int k0 = kt * BK;
    uint32_t ch0 = 0u;
    int ty0 = 0, tx0 = 0;
    if (a_tapk) {
      const uint32_t tap = fdiv((uint32_t)k0, aux.cin);
      ch0 = (uint32_t)k0 - tap * (uint32_t)p.conv.cin;
      tap_yx(md, tap, ty0, tx0);
    }
#pragma unroll
    for (int i = 0; i < APT; ++i) {
      const int k = k0 + a_k[i];
      if (k >= p.K) continue;
      uint32_t ch;
      int ty, tx;
      if (a_tapk) {
        ch = ch0 + (uint32_t)a_k[i];
        ty = ty0;
        tx = tx0;
      } else {
        const uint32_t tap = fdiv((uint32_t)k, aux.cin);
        ch = (uint32_t)k - tap * (uint32_t)p.conv.cin;
        tap_yx(md, tap, ty, tx);
      }
      const int ys = a_y[i] + ty, xs = a_x[i] + tx;
      if ((unsigned)ys >= (unsigned)md.lh || (unsigned)xs >= (unsigned)md.lw) continue;  // zero padding / masked row
      bf16_t* q = sa + (tid + 256 * i) * 8;  // this thread's LDS-DMA chunk (lane-linear)
      float v[8];
      unpack8(*(const uint4*)q, v);
      const float2* cf = agn_coef + a_bl[i] * p.conv.cin + ch;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float2 m = cf[e];
        const float z = v[e] * m.x + m.y;
        v[e] = p.agn_silu ? silu_f(z) : z;
      }
      *(uint4*)q = pack8(v);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the rewrites land before the barrier publishes them
  };

  // LNA (EncdiffGemmArgs.lna_*): LayerNorm of the A rows over K, folded into the staging.
  // Prologue: 4 lanes per tile row sum the row (fp32 sum / sum of squares, xor-shuffles over the
  // 4 lanes), mean / rstd per row and gamma / beta per channel into LDS behind the ring.  Per
  // k-tile every thread rewrites its own staged chunks in place (as AGN), masked rows / the K
  // tail left as staged (zeros).
  float2* lna_row = (float2*)((char*)smem + G::LDS_BYTES);  // [BM] (mean, rstd)
  float2* lna_gb = lna_row + BM;                             // [K] (gamma, beta)
  if constexpr (G::LNA) {
    static_assert(BM * 4 == 256, "LNA: 4 lanes per tile row");
    const int r = tid >> 2, q = tid & 3;
    const int m = m0 + r;
    float sa = 0.f, sq = 0.f;
    if (m < p.M) {
      const bf16_t* xr = A + (size_t)m * p.lda;
      for (int k = 8 * q; k < p.K; k += 32) {
        float v[8];
        unpack8(*(const uint4*)(xr + k), v);
#pragma unroll
        for (int e = 0; e < 8; ++e) { sa += v[e]; sq += v[e] * v[e]; }
      }
    }
    sa += __shfl_xor(sa, 1, 64); sq += __shfl_xor(sq, 1, 64);
    sa += __shfl_xor(sa, 2, 64); sq += __shfl_xor(sq, 2, 64);
    if (q == 0) {
      const float inv = 1.f / (float)p.K;
      const float mean = sa * inv, var = fmaxf(sq * inv - mean * mean, 0.f);
      lna_row[r] = make_float2(mean, rsqrtf(var + p.lna_eps));
    }
    for (int k = tid; k < p.K; k += 256) lna_gb[k] = make_float2(p.lna_gamma[k], p.lna_beta[k]);
    __syncthreads();  // the ring is staged next
  }
  auto lna_transform = [&](bf16_t* sa, int kt) {
    const int k0 = kt * BK;
#pragma unroll
    for (int i = 0; i < APT; ++i) {
      const int k = k0 + a_k[i];
      if (k >= p.K || m0 + a_y[i] >= p.M) continue;
      bf16_t* q = sa + (tid + 256 * i) * 8;  // this thread's LDS-DMA chunk (lane-linear)
      float v[8];
      unpack8(*(const uint4*)q, v);
      const float2 st = lna_row[a_y[i]];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float2 gb = lna_gb[k + e];
        v[e] = (v[e] - st.x) * st.y * gb.x + gb.y;
      }
      *(uint4*)q = pack8(v);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  };

  // NSTAGE-deep LDS ring: tiles it+1 .. it+NSTAGE-2 stay in flight while tile it is
  // multiplied, so the K loop is bound by MFMA / bandwidth rather than by one load latency
  // per k-tile.  Per iteration: wait for tile it (vmcnt = loads issued after it), one
  // barrier (tile it visible to all waves; every wave is done with tile it-1, whose slot is
  // refilled next), issue tile it+NSTAGE-1, multiply tile it.
  constexpr int D = G::NSTAGE;
  static_assert(D - 2 <= 6 && (D - 2) * G::LPS <= 63, "vm_wait_stages covers up to six stages ahead");
  if (nkt > 0) {
    // halo mode: the window's DMAs are issued first, so the wait for ring tile 0 covers them
    if constexpr (G::HALO) stage_halo();
#pragma unroll
    for (int st = 0; st < D - 1; ++st)
      if (st < nkt) stage(ring + st * G::STAGE, ktile(st));
    int rd = 0, wr = D - 1;  // ring slots of the tile read now / the tile issued next
    for (int it = 0; it < nkt; ++it) {
      vm_wait_stages<G::LPS, D - 2>(min(D - 2, nkt - 1 - it));
      if constexpr (G::AGN) agn_transform(ring + rd * G::STAGE, kt_begin + it);
      if constexpr (G::LNA) lna_transform(ring + rd * G::STAGE, kt_begin + it);
      asm volatile("s_barrier" ::: "memory");  // (asm: the compiler may not move LDS-DMA issue across it)
      if (it + D - 1 < nkt) stage(ring + wr * G::STAGE, ktile(it + D - 1));
      compute(ring + rd * G::STAGE, ktile(it));
      // this wave's fragment reads of slot rd retire before it reaches the next barrier
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      rd = rd + 1 == D ? 0 : rd + 1;
      wr = wr + 1 == D ? 0 : wr + 1;
    }
    __syncthreads();  // every wave is done with the ring before the epilogue reuses it
  }

  if (do_bgrad) {
    // column sums of the k-outer A: rows 0..RG-1 of each column partial -> combine in LDS
    // order, then ONE writer per column: a split-K slab (summed in order by the finalize),
    // a plain += (single K range), or an atomic for the atomic output modes.
    constexpr int RG = 256 / BM;
    float* red = (float*)smem;  // staging buffers are free after the last barrier
    const int col = tid % BM, rg = tid / BM;
    red[rg * BM + col] = bsum;
    __syncthreads();
    if (rg == 0 && m0 + col < p.M) {
      float t = 0.f;
#pragma unroll
      for (int r = 0; r < RG; ++r) t += red[r * BM + col];
      const bool slab = p.split_k > 1 && p.c == (void*)p.workspace;
      if (slab)
        p.workspace[(long)p.split_k * p.M * p.N + (long)bz * p.M + m0 + col] = t;
      else if (p.c_mode == ENCDIFF_OUT_F32_ATOMIC || p.c_mode == ENCDIFF_OUT_F32_ATOMIC_CONVW || p.split_k > 1)
        atomicAdd(p.bias_grad + m0 + col, t);
      else
        p.bias_grad[m0 + col] += t;
    }
    __syncthreads();
  }

  // ---- epilogue -------------------------------------------------------------
  // Stage the fp32 tile through LDS (the staging buffers are free after the last barrier),
  // then write whole 16-byte row segments (bf16/fp32 outputs) or lane-contiguous fp32 atomics.
  const bool add_bias = p.bias != nullptr && bz == 0;
  const bf16_t* R = (const bf16_t*)p.resid;
  if (p.c_mode == ENCDIFF_OUT_F32_ATOMIC_CONVW) {  // reference-layout scatter (rare path)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int col = n0 + wc + 16 * j + l16;
        if (col >= p.N) continue;
        const float bv = add_bias ? p.bias[col] : 0.f;
        const int tap = col / p.convw_cin;
        const int ci = col - tap * p.convw_cin;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int row = m0 + wr + 16 * i + 4 * g4 + q;
          if (row < p.M) atomicAdd((float*)p.c + (long)row * p.ldc + ci * 9 + tap, p.alpha * acc[i][j][q] + bv);
        }
      }
    return;
  }
  float* p_c_slab = (float*)p.c;
  constexpr int SLD = BN + 4;
  static_assert(BM * SLD * 4 <= G::LDS_BYTES, "epilogue staging must fit the LDS allocation");
  float* sc = (float*)smem;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) sc[(wr + 16 * i + 4 * g4 + q) * SLD + wc + 16 * j + l16] = acc[i][j][q];
  __syncthreads();
  if (p.c_mode == ENCDIFF_OUT_F32_ATOMIC) {
    // lanes along columns: one wave instruction = 64 consecutive floats of one row
    for (int e = tid; e < BM * BN; e += 256) {
      const int r = e / BN, cc = e - r * BN;
      const int row = m0 + r, col = n0 + cc;
      if (row < p.M && col < p.N)
        atomicAdd((float*)p.c + (long)row * p.ldc + col, p.alpha * sc[r * SLD + cc] + (add_bias ? p.bias[col] : 0.f));
    }
    return;
  }
  if (p.split_k > 1 && p.c_mode == ENCDIFF_OUT_F32) {  // split-K slab of this z (workspace path)
    p_c_slab = (float*)p.c + (long)bz * p.M * p.N;
  }
  if (p.c_mode == ENCDIFF_OUT_BF16_GEGLU) {  // f (both halves) and y = value * gelu(gate)
    constexpr int H2 = BN / 2, CPH = H2 / 8;
    for (int e = tid; e < BM * CPH; e += 256) {
      const int r = e / CPH, c8 = (e - r * CPH) * 8, row = m0 + r;
      if (row >= p.M) continue;
      const int jv = gcol(c8), jg = gcol(c8 + H2);
      float a[8], g[8], y[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        a[k] = p.alpha * sc[r * SLD + c8 + k] + (p.bias ? p.bias[jv + k] : 0.f);
        g[k] = p.alpha * sc[r * SLD + H2 + c8 + k] + (p.bias ? p.bias[jg + k] : 0.f);
      }
      bf16_t* F = (bf16_t*)p.c + (long)row * p.ldc;
      *(uint4*)(F + jv) = pack8(a);
      *(uint4*)(F + jg) = pack8(g);
#pragma unroll
      for (int k = 0; k < 8; ++k) y[k] = bf16_round(a[k]) * gelu_erf(bf16_round(g[k]));  // from the stored f
      *(uint4*)((bf16_t*)p.aux + (long)row * p.ld_aux + jv) = pack8(y);
    }
    return;
  }
  if (p.c_mode == ENCDIFF_OUT_BF16_GEGLU_BWD) {  // dy tile -> d(value), d(gate) from f
    constexpr int CPR = BN / 8;
    for (int e = tid; e < BM * CPR; e += 256) {
      const int r = e / CPR, c8 = (e - r * CPR) * 8;
      const int row = m0 + r, col = n0 + c8;
      if (row >= p.M || col >= p.N) continue;
      const bf16_t* F = (const bf16_t*)p.aux + (long)row * p.ld_aux;
      float a[8], g[8], da[8], dg[8];
      unpack8(*(const uint4*)(F + col), a);
      unpack8(*(const uint4*)(F + p.N + col), g);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float d = bf16_round(p.alpha * sc[r * SLD + c8 + k]);  // dy as the unfused path stores it
        da[k] = d * gelu_erf(g[k]);
        dg[k] = d * a[k] * gelu_erf_grad(g[k]);
      }
      bf16_t* D = (bf16_t*)p.c + (long)row * p.ldc;
      *(uint4*)(D + col) = pack8(da);
      *(uint4*)(D + p.N + col) = pack8(dg);
    }
    return;
  }
  // output row of GEMM row `row`: K4S2_TP rows are parity-major, each written to its pixel
  // (split-K slabs stay in GEMM row order; the finalize maps them)
  const bool slab_out = p.split_k > 1 && p.c == (void*)p.workspace;
  auto orow = [&](int row) -> long {
    if (md.k4 != 2 || slab_out) return row;
    const uint32_t mm = (uint32_t)row - mbase;
    const uint32_t b = fdiv(mm, aux.hw), r = mm - b * aux.hw.d;
    const uint32_t y = fdiv(r, aux.w), x = r - y * aux.w.d;
    return ((long)b * p.conv.h + 2 * y + (tp_q >> 1)) * p.conv.w + 2 * x + (tp_q & 1);
  };
  // in-kernel split-K combine: this split's slab goes out write-through (sc1)
  const bool fold = aux.fold.cnt != nullptr && slab_out;
  // (write-through stores for every slab measured slower in the step: 9.53 -> 9.64 ms, same box)
  const auto slab_rs = __builtin_amdgcn_make_buffer_rsrc(p.c, 0, fold ? p.split_k * p.M * p.N * 4 : 0, 0x00020000);
  const bool vec = (p.N % 8 == 0) && (p.ldc % 8 == 0) && (((uintptr_t)p.c & 15) == 0) &&
                   (!add_bias || (((uintptr_t)p.bias & 15) == 0)) &&
                   (!R || ((p.ld_resid % 8 == 0) && (((uintptr_t)R & 15) == 0)));
  if (vec) {
    constexpr int CPR = BN / 8;  // 8-column chunks per row
    for (int e = tid; e < BM * CPR; e += 256) {
      const int r = e / CPR, c8 = (e - r * CPR) * 8;
      const int row = m0 + r, col = n0 + c8;
      if (row >= p.M || col >= p.N) continue;
      const long ro = orow(row);
      float v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = p.alpha * sc[r * SLD + c8 + k];
      if (add_bias) {
        const float4 b0 = *(const float4*)(p.bias + col), b1 = *(const float4*)(p.bias + col + 4);
        v[0] += b0.x; v[1] += b0.y; v[2] += b0.z; v[3] += b0.w;
        v[4] += b1.x; v[5] += b1.y; v[6] += b1.z; v[7] += b1.w;
      }
      if (R) {
        float rr[8];
        unpack8(*(const uint4*)(R + ro * p.ld_resid + col), rr);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] += rr[k];
      }
      if (p.c_mode == ENCDIFF_OUT_BF16) {
        const uint4 pk = pack8(v);
        *(uint4*)((bf16_t*)p.c + ro * p.ldc + col) = pk;
        if (p.gn_stats || p.ln_y) {  // the stored (bf16) values feed the statistics below
          float rv[8];
          unpack8(pk, rv);
#pragma unroll
          for (int k = 0; k < 8; ++k) sc[r * SLD + c8 + k] = rv[k];
        }
      } else {
        float* cp = p_c_slab + ro * p.ldc + col;
        if (p.c_mode == ENCDIFF_OUT_F32_ACCUM) {
          const float4 c0 = *(const float4*)cp, c1 = *(const float4*)(cp + 4);
          v[0] += c0.x; v[1] += c0.y; v[2] += c0.z; v[3] += c0.w;
          v[4] += c1.x; v[5] += c1.y; v[6] += c1.z; v[7] += c1.w;
        }
        if (fold) {  // write-through (sc1) slab stores: visible to the combining split without a release fence
          const int bo = (int)((cp - (const float*)p.c) * 4);
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u32, make_float4(v[0], v[1], v[2], v[3])), slab_rs,
                                                 bo, 0, 16);
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u32, make_float4(v[4], v[5], v[6], v[7])), slab_rs,
                                                 bo + 16, 0, 16);
        } else {
          *(float4*)cp = make_float4(v[0], v[1], v[2], v[3]);
          *(float4*)(cp + 4) = make_float4(v[4], v[5], v[6], v[7]);
        }
      }
    }
  } else {
    for (int e = tid; e < BM * BN; e += 256) {
      const int r = e / BN, cc = e - r * BN;
      const int row = m0 + r, col = n0 + cc;
      if (row >= p.M || col >= p.N) continue;
      const long ro = orow(row);
      float v = p.alpha * sc[r * SLD + cc] + (add_bias ? p.bias[col] : 0.f);
      if (R) v += bf2f(R[ro * p.ld_resid + col]);
      if (p.c_mode == ENCDIFF_OUT_BF16) ((bf16_t*)p.c)[ro * p.ldc + col] = f2bf(v);
      else if (p.c_mode == ENCDIFF_OUT_F32_ACCUM) p_c_slab[ro * p.ldc + col] += v;
      else p_c_slab[ro * p.ldc + col] = v;
      if (p.gn_stats || p.ln_y) sc[r * SLD + cc] = bf16_round(v);
    }
  }
  if (fold) {
    // In-kernel split-K combine (the guide's write-through ticket recipe): every wave drains its
    // sc1 slab stores, then one lane takes the tile's ticket (relaxed, agent scope); the split that
    // draws split_k - 1 acquires and sums the tile's slabs in split order (bitwise reproducible,
    // placement independent), writes the user's output and leaves the ticket at zero.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int* flag = (int*)smem;  // the staging LDS is free: every thread is past its last read of it
    const int tile_id = by * ((p.M + BM - 1) / BM) + bx;
    if (tid == 0) {
      const int tk = __hip_atomic_fetch_add(aux.fold.cnt + tile_id, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      flag[0] = tk == p.split_k - 1;
    }
    __syncthreads();
    if (!flag[0]) return;
    if (tid == 0) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(aux.fold.cnt + tile_id, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    const SplitFold& f = aux.fold;
    const long total = (long)p.M * p.N;
    constexpr int CPR = BN / 8;
    for (int e = tid; e < BM * CPR; e += 256) {
      const int r = e / CPR, c8 = (e - r * CPR) * 8;
      const int row = m0 + r, col = n0 + c8;
      if (row >= p.M || col >= p.N) continue;
      const float* s = (const float*)p.c + (long)row * p.N + col;
      float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
      for (int z = 0; z < p.split_k; ++z) {
        const float4 a0 = *(const float4*)(s + z * total), a1 = *(const float4*)(s + z * total + 4);
        v[0] += a0.x; v[1] += a0.y; v[2] += a0.z; v[3] += a0.w;
        v[4] += a1.x; v[5] += a1.y; v[6] += a1.z; v[7] += a1.w;
      }
      {
        float bb[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (f.bias) {
          const float4 b0 = *(const float4*)(f.bias + col), b1 = *(const float4*)(f.bias + col + 4);
          bb[0] = b0.x; bb[1] = b0.y; bb[2] = b0.z; bb[3] = b0.w;
          bb[4] = b1.x; bb[5] = b1.y; bb[6] = b1.z; bb[7] = b1.w;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = splitk_scale(v[k], f.alpha, bb[k]);
      }
      if (f.resid) {
        float rr[8];
        unpack8(*(const uint4*)(f.resid + (long)row * f.ld_resid + col), rr);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] += rr[k];
      }
      if (f.mode == ENCDIFF_OUT_BF16) {
        *(uint4*)((bf16_t*)f.c + (long)row * f.ldc + col) = pack8(v);
      } else {
        float* cp = (float*)f.c + (long)row * f.ldc + col;
        if (f.mode == ENCDIFF_OUT_F32_ACCUM) {
          const float4 c0 = *(const float4*)cp, c1 = *(const float4*)(cp + 4);
          v[0] += c0.x; v[1] += c0.y; v[2] += c0.z; v[3] += c0.w;
          v[4] += c1.x; v[5] += c1.y; v[6] += c1.z; v[7] += c1.w;
        }
        *(float4*)cp = make_float4(v[0], v[1], v[2], v[3]);
        *(float4*)(cp + 4) = make_float4(v[4], v[5], v[6], v[7]);
      }
    }
    return;
  }
  if (p.ln_y) {
    // LayerNorm of each produced row (host: n0 == 0 and N <= BN, OUT_BF16, split_k 1): TPR
    // adjacent lanes per row, mean then centred variance (two-pass, as the LayerNorm kernel),
    // from the stored bf16 values; normalised row written to ln_y.
    constexpr int TPR = 256 / BM;
    __syncthreads();
    const int r = tid / TPR, part = tid % TPR, row = m0 + r;
    const float* sr = sc + r * SLD;
    float sm = 0.f;
    for (int c8 = part * 8; c8 < p.N; c8 += TPR * 8)
#pragma unroll
      for (int k = 0; k < 8; ++k) sm += sr[c8 + k];
#pragma unroll
    for (int o = 1; o < TPR; o <<= 1) sm += __shfl_xor(sm, o, 64);
    const float mean = sm / (float)p.N;
    float sq = 0.f;
    for (int c8 = part * 8; c8 < p.N; c8 += TPR * 8)
#pragma unroll
      for (int k = 0; k < 8; ++k) { const float d = sr[c8 + k] - mean; sq += d * d; }
#pragma unroll
    for (int o = 1; o < TPR; o <<= 1) sq += __shfl_xor(sq, o, 64);
    const float rstd = rsqrtf(sq / (float)p.N + p.ln_eps);
    if (row < p.M) {
      if (part == 0) { p.ln_stats[2L * row] = mean; p.ln_stats[2L * row + 1] = rstd; }
      for (int c8 = part * 8; c8 < p.N; c8 += TPR * 8) {
        float o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = (sr[c8 + k] - mean) * rstd * p.ln_gamma[c8 + k] + p.ln_beta[c8 + k];
        *(uint4*)((bf16_t*)p.ln_y + (long)row * p.ld_ln_y + c8) = pack8(o);
      }
    }
  }
  if (p.gn_stats) {
    // GroupNorm statistics of the produced tensor (host: OUT_BF16, split_k 1, M % 64 == 0):
    // per 64-row segment and column, sum and sum of squares of the stored bf16 values.  Q row
    // phases per column, their partials added in phase order through LDS: deterministic.
    constexpr int Q = 256 / BN, NSEG = BM / 64;
    const int c = tid % BN, q = tid / BN;
    float ps[NSEG], pq[NSEG];
    __syncthreads();
#pragma unroll
    for (int sg = 0; sg < NSEG; ++sg) {
      float a = 0.f, b = 0.f;
#pragma unroll 4
      for (int r = sg * 64 + q; r < sg * 64 + 64; r += Q) {
        const float v = sc[r * SLD + c];
        a += v;
        b += v * v;
      }
      ps[sg] = a;
      pq[sg] = b;
    }
    __syncthreads();
    float* red = sc;  // [NSEG][2][Q][BN]
#pragma unroll
    for (int sg = 0; sg < NSEG; ++sg) {
      red[((sg * 2) * Q + q) * BN + c] = ps[sg];
      red[((sg * 2 + 1) * Q + q) * BN + c] = pq[sg];
    }
    __syncthreads();
    if (q == 0 && n0 + c < p.N) {
#pragma unroll
      for (int sg = 0; sg < NSEG; ++sg) {
        if (m0 + sg * 64 >= p.M) break;
        float a = 0.f, b = 0.f;
        for (int qq = 0; qq < Q; ++qq) {
          a += red[((sg * 2) * Q + qq) * BN + c];
          b += red[((sg * 2 + 1) * Q + qq) * BN + c];
        }
        const long slot = (m0 >> 6) + sg;
        p.gn_stats[(2 * slot) * p.ld_gn_stats + n0 + c] = a;
        p.gn_stats[(2 * slot + 1) * p.ld_gn_stats + n0 + c] = b;
      }
    }
  }
}

// Bijective XCD remap of a 1-D block id: the dispatcher deals workgroups round-robin over the 8
// XCDs (block b runs on XCD b % 8), so blocks b and b + 8 share an L2; the remap gives the blocks
// of one XCD CONSECUTIVE logical ids, i.e. neighbouring tiles: the same weight columns / k-slice
// (and, for implicit im2col, the neighbouring image rows the 3x3 taps reach) stay in one L2
// instead of being fetched by all eight.
ED_DEV int xcd_remap(int b, int n) {
  const int q = n >> 3, r = n & 7, x = b & 7;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (b >> 3);
}

template <int BM, int BN, int AM, int BMD, int NS, int KB>
__global__ __launch_bounds__(256) void gemm_kernel(const EncdiffGemmArgs p, const GemmAux aux) {
  extern __shared__ __attribute__((aligned(16))) bf16_t smem[];
  int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  if (aux.xcd) {  // logical tile order x (M tiles) fastest, then y (N tiles), then z (k-slices)
    const int gx = gridDim.x, gy = gridDim.y;
    const int l = xcd_remap(bx + gx * (by + gy * bz), gx * gy * (int)gridDim.z);
    bx = l % gx;
    const int t = l / gx;
    by = t % gy;
    bz = t / gy;
  }
  gemm_tile<BM, BN, AM, BMD, NS, KB>(p, aux, bx, by, bz, smem);
}

// Two independent GEMMs in one 1-D grid: blocks [0, n1) run problem 1 (64 x 64 tiles),
// the next n2 problem 2 (tile BM2 x BN2), the last nf the split-K finalize of an EARLIER
// launch's weight gradient (pf), deferred into this launch.  A layer's weight gradient
// (problem 1: deep split-K, the longer-running blocks, dispatched first) and its input
// gradient (problem 2) share the machine instead of running back to back, each too small
// to fill 256 CUs; the previous layer's weight-gradient finalize rides along, so neither
// needs a launch of its own.
template <int AM1, int BMD1, int BM2, int BN2, int AM2, int BMD2, int NS2, int KB2, int KB1, int NS1 = 2>
__global__ __launch_bounds__(256) void gemm2_kernel(const EncdiffGemmArgs p1, const GemmAux aux1,
                                                    const EncdiffGemmArgs p2, const GemmAux aux2, int gx1,
                                                    int gy1, int gx2, int gy2, const EncdiffGemmArgs pf, int nf) {
  extern __shared__ __attribute__((aligned(16))) bf16_t smem[];
  const int n1 = gx1 * gy1 * p1.split_k;
  const int n2 = gx2 * gy2 * p2.split_k;
  int i = blockIdx.x;
  if (i < n1) {
    // XCD of block i is i % 8 in both ranges (a rotation of the labels in the second): the remap
    // over each range keeps it bijective and XCD-grouped
    if (aux1.xcd) i = xcd_remap(i, n1);
    const int bx = i % gx1, t = i / gx1;
    gemm_tile<64, 64, AM1, BMD1, NS1, KB1>(p1, aux1, bx, t % gy1, t / gy1, smem);
  } else if (i < n1 + n2) {
    i -= n1;
    if (aux2.xcd) i = xcd_remap(i, n2);
    const int bx = i % gx2, t = i / gx2;
    gemm_tile<BM2, BN2, AM2, BMD2, NS2, KB2>(p2, aux2, bx, t % gy2, t / gy2, smem);
  } else {
    gemm_finalize(pf, i - n1 - n2, nf);
  }
}
}  // namespace
