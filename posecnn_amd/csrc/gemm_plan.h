// Shape -> launch arithmetic of the pose-head GEMMs: the tile plan the split
// kernels and k_gemm_reduce evaluate on the device, the fp32 kernel's split,
// and the host's launch plan (tile edge, grid, kernel form, whether a reduce
// follows, workspace).  Plain C++ with no HIP call, so a host program can
// include it on its own (tests/gemm_plan_check.cpp).
#pragma once
#include <stddef.h>

#ifdef __HIPCC__
#define PCNN_HD __host__ __device__
#define PCNN_HDI __host__ __device__ inline __attribute__((always_inline))
#else
#define PCNN_HD
#define PCNN_HDI inline
#endif

namespace pcnn_gk {

// K step of a split kernel: 32 (x3: hi / lo planes, 64-B LDS rows) or 16
// (x6: hi / mid / lo planes, 48-B LDS rows; three planes of a 32-deep step
// would not fit two LDS stages)
PCNN_HD constexpr int split_bk(int prec) { return prec == 2 ? 16 : 32; }

// tile edge of the split kernels for a (capacity) shape
PCNN_HDI int tile_x3(int M, int N, int K) { return (M <= 128 || N <= 128 || K <= 128) ? 128 : 256; }

// largest grid of a split kernel at tile edge T: the workgroups resident on
// 256 CUs (one per CU at 256, two at 128)
PCNN_HD constexpr int x_max_grid(int T) { return T == 256 ? 256 : 512; }

// Plan of the split kernels for an effective shape (M and K may live on the
// device; the host evaluates the same plan for workspace sizing).
//  - M tiles are balanced: mt = ceil(M / T) tiles of Tm rows each, Tm the
//    smallest multiple of 32 >= M / mt (M = 405: 224 + 181 rows, not
//    256 + 149), so the tiles of one N column carry about the same number of
//    live 32-row accumulator blocks; rows past a tile's end are padding whose
//    MFMAs the K loop skips.  The tiles of a column run side by side on one
//    XCD, share their B panel through L2 and finish together (fc6 dX, 196
//    tiles in one round: 318 -> 295 us).
//  - Tile mode: whole tiles dealt round-robin.
//  - Split-K (fewer than G/2 tiles, long K): S K slices per tile, partial
//    slabs reduced in slice order by k_gemm_reduce (the forward shapes); a
//    slice keeps at least 128 of K.
//  Measured and dropped: stream-K over the tiles of a column (K ranges cut
//  evenly over workgroup pairs, partial tiles fixed up in fixed order by the
//  last segment to finish): fc6 dX 295 -> 343 us — the slab round trip and
//  the per-segment fix-up cost more than the balance gains.
#ifndef PCNN_MAX_SPLIT_X
#define PCNN_MAX_SPLIT_X 32
#endif
constexpr int kMaxSplitX = PCNN_MAX_SPLIT_X;  // split-K slices
struct XPlan {
  int mt, nt, ns, Tm, tiles, mode, S;
  bool m_fast;  // tile order: the dimension with fewer tiles runs fastest (its
                // neighbours share the other operand's tile in L2)
  PCNN_HD int mi_of(int t) const { return m_fast ? t % mt : t / nt; }
  PCNN_HD int ni_of(int t) const { return m_fast ? t / mt : t % nt; }
};

PCNN_HDI XPlan x_plan(int Meff, int N, int Keff, int T, int G, int BK) {
  XPlan p;
  p.mt = (Meff + T - 1) / T;
  p.nt = (N + T - 1) / T;
  p.ns = (Keff + BK - 1) / BK;
  p.tiles = p.mt * p.nt;
  p.m_fast = p.mt <= p.nt;
  const int rows = p.mt ? (Meff + p.mt - 1) / p.mt : 0;
  p.Tm = (rows + 31) / 32 * 32;
  p.mode = 0;
  p.S = 1;
  if (p.tiles > 0 && p.tiles < G / 2) {
    int s = G / p.tiles;
    if (s > p.ns / (128 / BK)) s = p.ns / (128 / BK);
    if (s > kMaxSplitX) s = kMaxSplitX;
    if (s > 1) {
      p.mode = 1;
      p.S = s;
    }
  }
  return p;
}

// fp32 kernel: 128 x 128 tiles; split-K factor for the effective shape
// (shared by the GEMM and the reducer)
constexpr int kF32Tile = 128;
constexpr int kF32MaxSplit = 8;
PCNN_HDI int split_for(int M, int N, int K) {
  const int tiles = ((M + kF32Tile - 1) / kF32Tile) * ((N + kF32Tile - 1) / kF32Tile);
  if (tiles >= 256 || M == 0) return 1;
  int s = (512 + tiles - 1) / tiles;
  int smax = K / 512;
  if (s > smax) s = smax;
  if (s > kF32MaxSplit) s = kF32MaxSplit;
  return s < 1 ? 1 : s;
}

// Whether the GEMM epilogue of a whole-tile plan already applied 1 / keep
// (x_epilogue, 128-row tiles, no forward drop mask): then k_gemm_reduce has
// nothing left to do for S == 1.
PCNN_HDI bool keep_in_epilogue(int prec, int tile, const void* drop) {
  return prec != 0 && tile == 128 && drop == nullptr;
}

// How the host launches one GEMM of a (capacity) shape.
struct LaunchPlan {
  int tile;        // tile edge: 128 or 256 (fp32 kernel: 128)
  int grid;        // workgroups of the persistent tile loop
  bool gen;        // the general kernel form; false: the lean whole-tile form (tile 256 only)
  bool may_split;  // some effective shape splits K, so k_gemm_reduce must follow
  bool c_stream;   // store C non-temporally
};

// precision 0: fp32 MFMA, 1: split-bf16 x3, 2: split-bf16 x6.  m_dynamic: the
// row count lives on the device (M is its capacity).  tile: a kernel with one
// tile edge only (k_gemm_tp) passes it; 0 = by shape.
inline LaunchPlan plan_launch(int M, int N, int K, bool m_dynamic, int precision, int tile = 0) {
  LaunchPlan p;
  p.gen = true;
  p.c_stream = false;
  if (precision == 0) {
    // persistent grid sized for the capacity shape at its split.  No device-
    // side M can make the shape split when a static M's tile count already
    // fills the grid (split 1 for every K).
    const long tiles = (long)((M + kF32Tile - 1) / kF32Tile) * ((N + kF32Tile - 1) / kF32Tile);
    const long items = tiles * split_for(M, N, K);
    p.tile = kF32Tile;
    p.grid = (int)(items < 512 ? 512 : items < 2048 ? items : 2048);
    p.may_split = m_dynamic || tiles < 256;
    return p;
  }
  const int T = tile ? tile : tile_x3(M, N, K);
  const int max_grid = x_max_grid(T);
  long grid = max_grid;
  if (m_dynamic) {
    // device-side M: the fewest tiles (M = 1) give the largest split; if even
    // that plan runs whole tiles, no effective M splits (fc8 dX, K = 88)
    p.may_split = x_plan(1, N, K, T, max_grid, split_bk(precision)).mode == 1;
  } else {
    // static M: if the plan runs whole tiles (a device-side K can only lower
    // the split), use the fewest workgroups that keep the same number of
    // rounds (fc6 dW: 1568 tiles -> 224 workgroups x 7): the makespan is
    // unchanged and the spare CUs run the other stream's kernels
    const XPlan pl = x_plan(M, N, K, T, max_grid, split_bk(precision));
    p.may_split = pl.mode == 1;
    if (pl.mode == 0) {
      p.gen = T != 256;  // the lean whole-tile kernel (instantiated for T = 256)
      const long items = pl.tiles;
      const long rounds = (items + max_grid - 1) / max_grid;
      grid = (items + rounds - 1) / rounds;
      grid = (grid + 7) / 8 * 8;
      if (grid > max_grid) grid = max_grid;
    }
  }
  p.tile = T;
  p.grid = (int)grid;
  // an output larger than the 256 MB MALL is written through without cache
  // allocation (fc6 dW, 411 MB: 316 -> 300 us; the 64 MB fc7 dW and the
  // small activations, re-read by the next GEMM, lose a little with it)
  p.c_stream = (long)M * N * 4 > (256l << 20);
  return p;
}

// Ragged edges of a split kernel's operands: a KC (k-contiguous) operand whose
// K (or device-side K) is not a multiple of 4, or an NC (row-contiguous)
// operand whose row count is not -> a float4 of a staging load may straddle
// the operand's edge, and the kernel takes element-wise edge loads.
inline bool split_ragged(bool a_trans, bool b_trans, int M, int N, int K, bool k_dynamic) {
  const bool a_kc = !a_trans, b_kc = b_trans;
  return ((a_kc || b_kc) && (K % 4 != 0 || k_dynamic)) || (!a_kc && M % 4 != 0) || (!b_kc && N % 4 != 0);
}

// Whether k_gemm_reduce follows the GEMM kernel: to sum split-K slabs when
// the plan can split, or to apply dropout / the backward's 1 / keep.  (A
// no-op launch is not free: queued behind a persistent GEMM on another stream
// it holds back everything after it on its own stream.)
inline bool reduce_follows(const LaunchPlan& p, int precision, const void* drop, float keep_prob) {
  return p.may_split || drop || (keep_prob != 1.f && !keep_in_epilogue(precision, p.tile, drop));
}

// Workspace of one GEMM: split-K slabs [S][M][N] at the largest split any
// effective M <= M can take (the fewest tiles: the split only grows when a
// device-side M shrinks)
inline size_t gemm_workspace_bytes(int M, int N, int K, bool m_dynamic, int precision) {
  if (M <= 0 || N <= 0) return 256;
  int s;
  if (precision == 1 || precision == 2) {
    const int T = tile_x3(M, N, K);
    s = x_plan(m_dynamic ? 1 : M, N, K, T, x_max_grid(T), split_bk(precision)).S;
  } else {
    s = split_for(m_dynamic ? 1 : M, N, K);
  }
  if (s <= 1) return 256;
  return ((size_t)s * M * N * sizeof(float) + 255) / 256 * 256 + 256;
}

}  // namespace pcnn_gk
