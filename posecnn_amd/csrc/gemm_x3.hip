// The precision-1 path of pcnn_gemm (gemm.hip).
//
// Split-bf16 ("bf16x3") GEMM: x = x_hi + x_lo with x_hi = bf16(x),
// x_lo = bf16(x - x_hi) (16 significant bits), a*b ~ a_hi b_hi + a_hi b_lo +
// a_lo b_hi accumulated in fp32 by v_mfma_f32_32x32x16_bf16 — relative error
// ~1e-5 per product (fp32-class for the 1e-4 quaternion tolerance) at 3/16 of
// the fp32-MFMA cost.  fp32 operands are split while staging into LDS, so the
// weights stay fp32 in HBM (no conversion pass).
//
// Tile 256 x 256 x 32, 512 threads (8 waves as 2 (M) x 4 (N), 128 x 64 per
// wave = 4 x 2 accumulators of 32 x 32), one workgroup per CU with two 64 KiB
// LDS stages: the global loads of step s+2 are in flight (registers) while
// step s computes and step s+1 sits in LDS.  At 512 flop per staged fp32 byte
// pair the tile needs ~21 B/clk/CU at the MFMA rate, inside the L2 share.
// Shapes with an edge <= 128 (the fc8 GEMMs: N = 4C, or K = 4C in dX) use a
// 128 x 128 instance (256 threads, 2 x 2 waves of 64 x 64, two workgroups per
// CU): 4x the workgroups of an output- or latency-bound shape.  Measured
// (scripts/gemm_bench.py): fc8 23-26 us vs 33-40 us at 256; 128 everywhere
// loses 20-25% on fc6 and is even on fc7.
#include "gemm_common.h"

using namespace pcnn_gk;

namespace {

constexpr int XBK = 32;
// Tile geometry: T = 256 (the large shapes) or 128 (shapes with an edge of
// <= 128 or too few 256-tiles to fill the chip: 256 threads as 2 x 2 waves of
// 64 x 64, 64 KiB LDS, two workgroups per CU).
template <int T>
struct XTile {
  static constexpr int threads = 2 * T;
  static constexpr int part = T * 64;       // one operand half (hi or lo): T rows x 32 bf16
  static constexpr int stage = 4 * part;    // a_hi, a_lo, b_hi, b_lo
  static constexpr int lds = 2 * stage;     // 128 / 64 KiB
  static constexpr int wn = T / 64;         // waves along N (64 columns each); 2 along M
  static constexpr int am = T / 64;         // 32-row accumulators per wave along M
};

// LDS image of an operand half: rows of 64 B = 4 chunks of 8 bf16 (k), chunk
// XOR-swizzled by g(row) = r2 | (r1 ^ r3) << 1 — conflict-free for the
// ds_read_b128 fragment reads (4 x 16-lane groups), the KC-staging
// ds_write_b64 and the NC-staging ds_write_b128 (searched exhaustively over
// linear GF(2) swizzles against the gfx950 lane-group table).
__device__ __forceinline__ int x_off(int row, int c) {
  const int g = ((row >> 2) & 1) | ((((row >> 1) ^ (row >> 3)) & 1) << 1);
  return row * 64 + 16 * (c ^ g);
}

// Staging of one 256-row x 32-k operand tile into 16 fp32 registers.
// KC (operand stored k-contiguous): lane -> k quad t & 7 of rows (t >> 3) + 64 i
// (8 full 128-B lines per load instruction).  NC (stored row-contiguous, k
// rows of ld): wave w takes rows 64 (w >> 1) .. +63 and k 16 (w & 1) .. +15;
// lane l -> row quad l >> 2 (float4 along the row direction) and k quad l & 3,
// so each load instruction reads four 256-B runs and the transposed LDS
// writes of a 16-lane group spread over both halves of each chunk.
// Rows past rlim and k past ke load as 0.  RAGGED: some float4 may straddle
// the K edge (KC) or the row edge (NC) -> element-wise fallback; the common
// instantiation has no divergent branch, so a K step is one basic block.
template <int T, bool KC, bool RAGGED, bool A2>
__device__ __forceinline__ void x_load_part(const XOp& P, const XOp& P2, int r0, int rlim, int k0, int ke,
                                            float (&v)[16], int q) {
  // Every mask is applied to the load ADDRESS (out-of-range voffset -> the
  // hardware returns 0), never to the loaded data: nothing consumes a loaded
  // register before the staging store of the next step, so all loads of a
  // step stay in flight together.  (A2: the summed operand of the generic
  // A + A2 form adds right after its loads.)  Part q = one float4 load.
  const int t = threadIdx.x;
  xf4 x;
  if (KC) {
    const int kq = t & 7;
    const int row = r0 + (t >> 3) + (T / 4) * q;
    const int kl = k0 + 4 * kq;
    const bool ok = row < rlim && kl < ke;
    const unsigned vo = ok ? (unsigned)(row * P.ld + kl) * 4u : kXOob;
    if (!RAGGED || kl + 4 <= ke || !ok) {
      x = x_ld4(P, vo, 0);
      if (A2) x += x_ld4(P2, vo, 0);
    } else {
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const unsigned ve = kl + e < ke ? vo + 4u * e : kXOob;
        x[e] = x_ld1(P, ve, 0);
        if (A2) x[e] += x_ld1(P2, ve, 0);
      }
    }
  } else {
    const int w = t >> 6, l = t & 63;
    const int rq = r0 + 64 * (w >> 1) + 4 * (l >> 2);
    const int k = k0 + 16 * (w & 1) + 4 * (l & 3) + q;
    const bool ok = rq < rlim && k < ke;
    const unsigned vo = ok ? (unsigned)(k * P.ld + rq) * 4u : kXOob;
    if (!RAGGED || rq + 4 <= rlim || !ok) {
      x = x_ld4(P, vo, 0);
      if (A2) x += x_ld4(P2, vo, 0);
    } else {
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const unsigned ve = rq + e < rlim ? vo + 4u * e : kXOob;
        x[e] = x_ld1(P, ve, 0);
        if (A2) x[e] += x_ld1(P2, ve, 0);
      }
    }
  }
  v[4 * q + 0] = x[0]; v[4 * q + 1] = x[1]; v[4 * q + 2] = x[2]; v[4 * q + 3] = x[3];
}

template <int T, bool KC, bool RAGGED, bool A2>
__device__ __forceinline__ void x_load(const XOp& P, const XOp& P2, int r0, int rlim, int k0, int ke,
                                       float (&v)[16]) {
#pragma unroll
  for (int q = 0; q < 4; q++) x_load_part<T, KC, RAGGED, A2>(P, P2, r0, rlim, k0, ke, v, q);
}

// Split of two fp32 values into packed bf16 (hi, lo) pairs: hi = bf16(x)
// (RNE), lo = bf16(x - hi) (the subtraction is exact).  One pack-convert for
// both hi halves, the fp32 value of each hi half by a shift / mask of that
// pack, one pack-convert for both lo halves.
__device__ __forceinline__ void x_split2(float a, float b, unsigned& hi, unsigned& lo) {
  const bf16x2 h = __builtin_convertvector((f32x2){a, b}, bf16x2);
  hi = __builtin_bit_cast(unsigned, h);
  const float ah = __uint_as_float(hi << 16), bh = __uint_as_float(hi & 0xffff0000u);
  lo = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){a - ah, b - bh}, bf16x2));
}

// Part q of the split-and-store of a staged operand: KC rows (t >> 3) + T/4 q
// (register quad q); NC row rb + q, i.e. element q of every register quad —
// so an NC part needs all four loads of the operand, a KC part only its own.
template <int T, bool KC>
__device__ __forceinline__ void x_store_part(const float (&v)[16], char* hi, char* lo, int q) {
  const int t = threadIdx.x;
  unsigned h0, h1, l0, l1;
  int o;
  if (KC) {
    const int kq = t & 7;
    const int row = (t >> 3) + (T / 4) * q;
    x_split2(v[4 * q + 0], v[4 * q + 1], h0, l0);
    x_split2(v[4 * q + 2], v[4 * q + 3], h1, l1);
    o = x_off(row, kq >> 1) + (kq & 1) * 8;
  } else {  // v[4 j + e] = (k = k-quad base + j, row = row-quad base + e): transpose into k-contiguous rows
    const int w = t >> 6, l = t & 63;
    const int row = 64 * (w >> 1) + 4 * (l >> 2) + q;
    const int kq = 4 * (w & 1) + (l & 3);  // k quad index 0..7 within the 32-k step
    x_split2(v[q], v[4 + q], h0, l0);
    x_split2(v[8 + q], v[12 + q], h1, l1);
    o = x_off(row, kq >> 1) + (kq & 1) * 8;
  }
  *(uint2*)(hi + o) = make_uint2(h0, h1);
  *(uint2*)(lo + o) = make_uint2(l0, l1);
}

template <int T, bool KC>
__device__ __forceinline__ void x_store(const float (&v)[16], char* hi, char* lo) {
#pragma unroll
  for (int q = 0; q < 4; q++) x_store_part<T, KC>(v, hi, lo, q);
}

// GEN: the general form (split-K and stream-K plans, for device-side M);
// without it the kernel runs whole tiles only (a static-M shape whose plan
// is tile mode, e.g. the weight gradients) and carries none of the partial-
// sum code, which keeps its registers free of spills.
template <int T, bool A_T, bool B_T, bool RAGGED, bool A2, bool GEN>
__global__ void __launch_bounds__(XTile<T>::threads, T == 256 ? 1 : 2) k_gemm_x3(GemmArgs g) {
  using X = XTile<T>;
  constexpr int kXPart = X::part, kXStage = X::stage, AM = X::am;
  extern __shared__ __attribute__((aligned(16))) char xl[];
  constexpr bool A_KC = !A_T, B_KC = B_T;
  const int Meff = eff_dim(g.M, g.M_dev);
  const int Keff = eff_dim(g.K, g.K_dev);
  XPlan pl = x_plan(Meff, g.N, Keff, T, g.xgrid, XBK);
  if constexpr (!GEN) {
    pl.mode = 0;
    pl.S = 1;
  }
  const int active = min(g.xgrid, pl.tiles * pl.S);
  // XCD-aware order: the first `active` blocks are dealt round-robin over the
  // 8 XCDs; renumbered so the workgroups of one XCD take consecutive items —
  // the M tiles of a column (one B panel) and neighbouring columns — and
  // shared operand rows meet in one L2
  int wg = blockIdx.x;
  if (wg >= active) return;
  wg = xcd_remap(wg, active);
  const int lane = pcnn::lane_id(), wave = threadIdx.x >> 6;
  const int wm = wave / X::wn, wn = wave % X::wn;
  const int r = lane & 31, hsel = lane >> 5;
  // operand extents (elements): A (M,K) or (K,M); B (K,N) or (N,K)
  const long a_el = A_T ? (long)(g.K - 1) * g.lda + g.M : (long)(g.M - 1) * g.lda + g.K;
  const long b_el = B_T ? (long)(g.N - 1) * g.ldb + g.K : (long)(g.K - 1) * g.ldb + g.N;
  const XOp oa = x_op(g.A, g.lda, a_el), oa2 = x_op(g.A2, g.lda, a_el), ob = x_op(g.B, g.ldb, b_el),
            onull = x_op(nullptr, 0, 0);
  // fragment offsets (bytes) inside an operand half, per k16 sub-step
  int a_off[2][AM], b_off[2][2];
#pragma unroll
  for (int ks = 0; ks < 2; ks++) {
#pragma unroll
    for (int i = 0; i < AM; i++) a_off[ks][i] = x_off(wm * (T / 2) + i * 32 + r, 2 * ks + hsel);
#pragma unroll
    for (int j = 0; j < 2; j++) b_off[ks][j] = x_off(wn * 64 + j * 32 + r, 2 * ks + hsel);
  }

  // One segment: K steps [kl, kh) of tile t, then its epilogue (whole tile)
  // or its slab (+ the fix-up if it is the tile's last segment to finish).
  auto segment = [&](int t, int kl, int kh, int z) {
    const int mi = pl.mi_of(t);
    const int m0 = mi * pl.Tm, n0 = pl.ni_of(t) * T;
    const int rl = min(Meff, m0 + pl.Tm);  // the tile's rows: [m0, rl)
    const int kb = kl * XBK, ke = min(Keff, kh * XBK);
    const int nsteps = kh > kl ? kh - kl : 0;
    // live 32-row accumulator blocks of this wave (rows past the tile are padding)
    const int live = rl - (m0 + wm * (T / 2));
    int amw = live <= 0 ? 0 : (live + 31) / 32;
    amw = __builtin_amdgcn_readfirstlane(amw < AM ? amw : AM);
    f32x16 acc[AM][2];
#pragma unroll
    for (int i = 0; i < AM; i++)
#pragma unroll
      for (int j = 0; j < 2; j++) acc[i][j] = (f32x16){};
    if (nsteps > 0) {
      float va[16], vb[16];
      // prologue: stage 0 -> LDS buffer 0, stage 1 -> registers
      x_load<T, A_KC, RAGGED, A2>(oa, oa2, m0, rl, kb, ke, va);
      x_load<T, B_KC, RAGGED, false>(ob, onull, n0, g.N, kb, ke, vb);
      x_store<T, A_KC>(va, xl, xl + kXPart);
      x_store<T, B_KC>(vb, xl + 2 * kXPart, xl + 3 * kXPart);
      const int k1 = kb + (nsteps > 1 ? XBK : 0);
      x_load<T, A_KC, RAGGED, A2>(oa, oa2, m0, rl, k1, ke, va);
      x_load<T, B_KC, RAGGED, false>(ob, onull, n0, g.N, k1, ke, vb);
      __syncthreads();
      // Staging part c of step s+1 (registers -> the other LDS buffer) and the
      // matching loads of step s+2 (clamped to the last step: the surplus
      // stores land in a buffer nobody reads).  Parts 0-3 are A, 4-7 B.  The
      // `nxt` buffer was last read in step s-1, before the barrier, so it may
      // be written at any point of step s.
      auto stage_part = [&](int c, char* nxt, int kn) {
        if (c < 4) {
          x_store_part<T, A_KC>(va, nxt, nxt + kXPart, c);
          if (A_KC) {
            x_load_part<T, true, RAGGED, A2>(oa, oa2, m0, rl, kn, ke, va, c);
          } else if (c == 3) {
#pragma unroll
            for (int q = 0; q < 4; q++) x_load_part<T, false, RAGGED, A2>(oa, oa2, m0, rl, kn, ke, va, q);
          }
        } else {
          x_store_part<T, B_KC>(vb, nxt + 2 * kXPart, nxt + 3 * kXPart, c - 4);
          if (B_KC) {
            x_load_part<T, true, RAGGED, false>(ob, onull, n0, g.N, kn, ke, vb, c - 4);
          } else if (c == 7) {
#pragma unroll
            for (int q = 0; q < 4; q++) x_load_part<T, false, RAGGED, false>(ob, onull, n0, g.N, kn, ke, vb, q);
          }
        }
      };
      // The K loop, specialised on AMW = the wave's live accumulator blocks:
      // at M = 405 in 256-row tiles the second tile's lower waves (rows
      // 384-511) have one live block of four, so they issue a quarter of the
      // MFMAs and their SIMD partners run the matrix pipe alone (the schedule
      // weights that tile lighter).  Each specialisation keeps one basic block
      // per K step: after each accumulator row (six MFMAs) its share of the
      // eight staging parts, so the conversion VALU and LDS writes fill MFMA
      // gaps.
      auto kloop = [&](auto amw_c) {
        constexpr int AMW = decltype(amw_c)::value;
        constexpr int SLOTS = 2 * AMW;
        for (int s = 0; s < nsteps; s++) {
          const char* cur = xl + (s & 1) * kXStage;
          char* nxt = xl + ((s + 1) & 1) * kXStage;
          const int kn = kb + (s + 2 < nsteps ? s + 2 : nsteps - 1) * XBK;
          if constexpr (AMW == 0) {
#pragma unroll
            for (int c = 0; c < 8; c++) stage_part(c, nxt, kn);
          } else {
#pragma unroll
            for (int ks = 0; ks < 2; ks++) {
              bf16x8 bh[2], bl[2];
#pragma unroll
              for (int j = 0; j < 2; j++) {
                bh[j] = *(const bf16x8*)(cur + 2 * kXPart + b_off[ks][j]);
                bl[j] = *(const bf16x8*)(cur + 3 * kXPart + b_off[ks][j]);
              }
              // A fragments one accumulator row ahead: the reads of row i + 1
              // are in flight while row i's six MFMAs issue
              bf16x8 ah[2], al[2];
              ah[0] = *(const bf16x8*)(cur + a_off[ks][0]);
              al[0] = *(const bf16x8*)(cur + kXPart + a_off[ks][0]);
#pragma unroll
              for (int i = 0; i < AMW; i++) {
                if (i + 1 < AMW) {
                  ah[(i + 1) & 1] = *(const bf16x8*)(cur + a_off[ks][i + 1]);
                  al[(i + 1) & 1] = *(const bf16x8*)(cur + kXPart + a_off[ks][i + 1]);
                }
#pragma unroll
                for (int j = 0; j < 2; j++) {
                  acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i & 1], bh[j], acc[i][j], 0, 0, 0);
                  acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i & 1], bl[j], acc[i][j], 0, 0, 0);
                  acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i & 1], bh[j], acc[i][j], 0, 0, 0);
                }
                const int slot = ks * AMW + i;
#pragma unroll
                for (int c = slot * 8 / SLOTS; c < (slot + 1) * 8 / SLOTS; c++) stage_part(c, nxt, kn);
              }
            }
          }
          __syncthreads();
        }
      };
      if (amw == AM) kloop(IC<AM>{});
      else if (amw == 0) kloop(IC<0>{});
      else if (amw == 1) kloop(IC<1>{});
      else if constexpr (AM >= 4) {
        if (amw == 2) kloop(IC<2>{});
        else kloop(IC<3>{});
      }
    }

    x_epilogue<T, AM>(g, pl, acc, m0, n0, rl, z, wm, wn, r, hsel);
  };

  // this workgroup's items: every active-th (tile, K slice); one call site,
  // so the segment body is instantiated once
  const int kstep = (pl.ns + pl.S - 1) / pl.S;  // split-K: K steps per slice
  for (int item = wg; item < pl.tiles * pl.S; item += active) {
    const int z = item / pl.tiles, t = item % pl.tiles;
    const int kl = z * kstep;
    segment(t, kl, min(pl.ns, kl + kstep), z);
  }
}

struct X3Family {
  template <int T>
  using Tile = XTile<T>;
  // plain launch: after a precision-1 GEMM without a reduce the completion event stays pending
  static constexpr bool takes_done_event = false;
  template <int T, bool AT, bool BT, bool RG, bool S2, bool GN>
  static constexpr auto kernel() {
    return &k_gemm_x3<T, AT, BT, RG, S2, GN>;
  }
};

}  // namespace

namespace pcnn_gk {

void launch_gemm_x3(const GemmArgs& g, const SplitVariant& v, hipStream_t st) { SplitLaunch<X3Family>::launch(g, v, st); }

}  // namespace pcnn_gk
