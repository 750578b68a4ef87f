// Exact-fp32 MFMA GEMM of the pose-head FC layers (precision 0 of pcnn_gemm,
// gemm.hip).
//
// C = epilogue(op(A) (+ op(A2)) * op(B)) on 128x128 tiles, BK = 16, 4 waves
// per workgroup in a 2x2 arrangement of 64x64 sub-tiles, each a 2x2 grid of
// v_mfma_f32_32x32x2_f32 accumulators (exact fp32: the MFMA is an fp32 fmaf
// chain).  The row count M and the contraction length K may live on the
// device: the grid is a persistent tile loop that reads them.  Small-tile-
// count shapes split K (split_for, gemm_plan.h); partial slabs are reduced in
// fixed order by k_gemm_reduce, which also applies the epilogue (bit-stable
// across runs).  The pool5 + pool4 addition is fused into the A-tile load.
#include "gemm_common.h"

using namespace pcnn_gk;

namespace {

constexpr int BM = kF32Tile, BN = kF32Tile, BK = 16;
constexpr int kGemmThreads = 256;

// Load a 4-float chunk along the contiguous dimension, zero-filled past `lim`.
__device__ __forceinline__ float4 load4(const float* p, int start, int lim, bool row_ok) {
  if (!row_ok) return make_float4(0.f, 0.f, 0.f, 0.f);
  if (start + 3 < lim && ((((uintptr_t)(p + start)) & 15) == 0)) return *(const float4*)(p + start);
  float4 r;
  r.x = start + 0 < lim ? p[start + 0] : 0.f;
  r.y = start + 1 < lim ? p[start + 1] : 0.f;
  r.z = start + 2 < lim ? p[start + 2] : 0.f;
  r.w = start + 3 < lim ? p[start + 3] : 0.f;
  return r;
}

__device__ __forceinline__ float4 add4(float4 a, float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

// Tile staging.  A tile is stored in LDS k-major: As[k][m] (m contiguous), the
// layout whose fragment reads (lane: m = l & 31, k = l >> 5) are conflict-free.
template <bool A_T>
struct ATile {
  float4 r[2];
  __device__ __forceinline__ void load(const GemmArgs& g, int m0, int k0, int Meff, int Keff) {
    const int t = threadIdx.x;
    if (!A_T) {  // A (M,K): thread -> row m, two 4-wide k chunks
      const int m = m0 + (t & 127), kq = (t >> 7) * 4;
      const bool ok = m < Meff;
      const float* ar = g.A + (size_t)(ok ? m : 0) * g.lda;
      r[0] = load4(ar, k0 + kq, Keff, ok);
      r[1] = load4(ar, k0 + 8 + kq, Keff, ok);
      if (g.A2) {
        const float* a2 = g.A2 + (size_t)(ok ? m : 0) * g.lda;
        r[0] = add4(r[0], load4(a2, k0 + kq, Keff, ok));
        r[1] = add4(r[1], load4(a2, k0 + 8 + kq, Keff, ok));
      }
    } else {  // A stored (K,M): thread -> k row, 4-wide m chunk
      const int mq = (t & 31) * 4, kr = t >> 5;
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int k = k0 + kr + 8 * h;
        const bool ok = k < Keff;
        const float* ar = g.A + (size_t)(ok ? k : 0) * g.lda;
        r[h] = load4(ar, m0 + mq, Meff, ok);
        if (g.A2) r[h] = add4(r[h], load4(g.A2 + (size_t)(ok ? k : 0) * g.lda, m0 + mq, Meff, ok));
      }
    }
  }
  __device__ __forceinline__ void store(float (*As)[BM]) {
    const int t = threadIdx.x;
    if (!A_T) {
      const int m = t & 127, kq = (t >> 7) * 4;
#pragma unroll
      for (int h = 0; h < 2; h++) {
        As[8 * h + kq + 0][m] = r[h].x;
        As[8 * h + kq + 1][m] = r[h].y;
        As[8 * h + kq + 2][m] = r[h].z;
        As[8 * h + kq + 3][m] = r[h].w;
      }
    } else {
      const int mq = (t & 31) * 4, kr = t >> 5;
#pragma unroll
      for (int h = 0; h < 2; h++) *(float4*)&As[kr + 8 * h][mq] = r[h];
    }
  }
};

template <bool B_T>
struct BTile {
  float4 r[2];
  __device__ __forceinline__ void load(const GemmArgs& g, int n0, int k0, int Keff) {
    const int t = threadIdx.x;
    if (!B_T) {  // B (K,N): thread -> k row, 4-wide n chunk
      const int nq = (t & 31) * 4, kr = t >> 5;
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int k = k0 + kr + 8 * h;
        const bool ok = k < Keff;
        r[h] = load4(g.B + (size_t)(ok ? k : 0) * g.ldb, n0 + nq, g.N, ok);
      }
    } else {  // B stored (N,K): thread -> n row, two 4-wide k chunks
      const int n = n0 + (t & 127), kq = (t >> 7) * 4;
      const bool ok = n < g.N;
      const float* br = g.B + (size_t)(ok ? n : 0) * g.ldb;
      r[0] = load4(br, k0 + kq, Keff, ok);
      r[1] = load4(br, k0 + 8 + kq, Keff, ok);
    }
  }
  __device__ __forceinline__ void store(float (*Bs)[BN]) {
    const int t = threadIdx.x;
    if (!B_T) {
      const int nq = (t & 31) * 4, kr = t >> 5;
#pragma unroll
      for (int h = 0; h < 2; h++) *(float4*)&Bs[kr + 8 * h][nq] = r[h];
    } else {
      const int n = t & 127, kq = (t >> 7) * 4;
#pragma unroll
      for (int h = 0; h < 2; h++) {
        Bs[8 * h + kq + 0][n] = r[h].x;
        Bs[8 * h + kq + 1][n] = r[h].y;
        Bs[8 * h + kq + 2][n] = r[h].z;
        Bs[8 * h + kq + 3][n] = r[h].w;
      }
    }
  }
};

template <bool A_T, bool B_T>
__global__ void __launch_bounds__(kGemmThreads) k_gemm_f32(GemmArgs g) {
  __shared__ __attribute__((aligned(16))) float As[BK][BM];
  __shared__ __attribute__((aligned(16))) float Bs[BK][BN];
  const int Meff = eff_dim(g.M, g.M_dev);
  const int Keff = eff_dim(g.K, g.K_dev);
  const int mt = (Meff + BM - 1) / BM, nt = (g.N + BN - 1) / BN;
  const int S = split_for(Meff, g.N, Keff);
  const int kchunk = ((Keff + S - 1) / S + BK - 1) / BK * BK;
  const int items = mt * nt * S;
  const int lane = pcnn::lane_id(), wave = threadIdx.x >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    // consecutive items share the B (weight) tile: n-tile outermost, m-tile inner
    const int z = item % S;
    const int rest = item / S;
    const int mi = rest % mt, ni = rest / mt;
    const int m0 = mi * BM, n0 = ni * BN;
    const int kb = z * kchunk, ke = min(Keff, kb + kchunk);
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 2; j++) acc[i][j] = (f32x16){};
    ATile<A_T> at;
    BTile<B_T> bt;
    if (kb < ke) {
      at.load(g, m0, kb, Meff, ke);
      bt.load(g, n0, kb, ke);
    }
    for (int k0 = kb; k0 < ke; k0 += BK) {
      __syncthreads();
      at.store(As);
      bt.store(Bs);
      __syncthreads();
      if (k0 + BK < ke) {  // prefetch the next tile into registers under the MFMAs
        at.load(g, m0, k0 + BK, Meff, ke);
        bt.load(g, n0, k0 + BK, ke);
      }
#pragma unroll
      for (int kk = 0; kk < BK / 2; kk++) {
        const int kr = 2 * kk + (lane >> 5);
        float a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; i++) a[i] = As[kr][wm * 64 + i * 32 + (lane & 31)];
#pragma unroll
        for (int j = 0; j < 2; j++) b[j] = Bs[kr][wn * 64 + j * 32 + (lane & 31)];
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
          for (int j = 0; j < 2; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
      }
    }
    // C/D map: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const int m = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
          const int n = n0 + wn * 64 + j * 32 + (lane & 31);
          if (m < Meff && n < g.N) {
            if (S == 1) g.C[(size_t)m * g.ldc + n] = epilogue(acc[i][j][r], g, m, n);
            else g.slab[((size_t)z * g.M + m) * g.N + n] = acc[i][j][r];
          }
        }
    __syncthreads();
  }
}

}  // namespace

namespace pcnn_gk {

void launch_gemm_f32(const GemmArgs& g, bool a_trans, bool b_trans, hipStream_t st) {
  const dim3 grid(g.xgrid), block(kGemmThreads);
  if (!a_trans && !b_trans) hipLaunchKernelGGL((k_gemm_f32<false, false>), grid, block, 0, st, g);
  else if (!a_trans && b_trans) hipLaunchKernelGGL((k_gemm_f32<false, true>), grid, block, 0, st, g);
  else if (a_trans && !b_trans) hipLaunchKernelGGL((k_gemm_f32<true, false>), grid, block, 0, st, g);
  else hipLaunchKernelGGL((k_gemm_f32<true, true>), grid, block, 0, st, g);
}

}  // namespace pcnn_gk
