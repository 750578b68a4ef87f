// The short launches between the fc7 forward GEMM and fc7 dX of the pose step
// (posecnn_amd/pipeline.py), fused: at 4C <= 128 columns fc8 is a skinny GEMM
// whose split-K reduce passes and generic tile machinery cost more than its
// arithmetic, and the chain they sit on runs alone on the chip.
//
//  k_fc8_fwd_fused        fc7's split-K reduce (slab sum, bias, relu, dropout
//                         draw: k_gemm_reduce's vector branch, gemm.hip) done
//                         while staging the A operand of the fc8 forward, whose
//                         K slices write today's fc8 slabs
//  k_fc8_reduce_head_fwd  fc8's split-K reduce (+ b8) inside the pose head's
//                         row pass (k_head_fwd, pose_head.hip)
//  k_fc8_dx_skinny        dY7 = mask(Y7 > 0) (dY8 W8^T) / keep with every
//                         operand loaded once, no LDS
//
// All three compute bit for bit what pcnn_gemm_drop_gen (fc7) -> pcnn_gemm
// (fc8) -> pcnn_pose_head_fwd and pcnn_gemm_drop (fc8 dX) compute at
// precision 2: the same plans (x_plan, gemm_plan.h) decide the slab counts
// and the K slices, the operands are split by x_split3, and every output
// element sees k_gemm_x6's MFMA sequence -- K steps of 16 in order, the six
// plane products lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi, fragments
// lane -> row (column) lane & 31, k 8 (lane >> 5) .. +7, zeros past K.  An
// output element of v_mfma_f32_32x32x16_bf16 depends only on its own A row and
// B column, so regrouping rows into 32-row blocks changes nothing.
#include "gemm_common.h"
#include "head_common.h"
#include "pcnn_philox.h"

using namespace pcnn_gk;

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int F8BK = 16;                      // the x6 K step
constexpr int F8CH = 8;                       // K steps staged at a time (128 of K; fc8 forward: one slice)
// bytes per LDS plane row: 128 bf16 + 16 B (the fragment reads spread over the banks)
constexpr int F8ROW = F8CH * F8BK * 2 + 16;
constexpr int F8PLANE = 32 * F8ROW;
constexpr int F8MAXD = 128;                   // columns: one wave per 32-column block, four waves

// value q of a 32 x 32 accumulator block: row qrow(q) + 4 (lane >> 5), column lane & 31
__device__ __forceinline__ int f8_qrow(int q) { return (q & 3) + 8 * (q >> 2); }

// eight consecutive k of one row / column -> the three packed bf16 fragments
__device__ __forceinline__ void f8_split8(const float (&v)[8], bf16x8& hi, bf16x8& mid, bf16x8& lo) {
  u32x4 h, m, l;
#pragma unroll
  for (int p = 0; p < 4; p++) {
    unsigned a, b, c;
    x_split3(v[2 * p], v[2 * p + 1], a, b, c);
    h[p] = a;
    m[p] = b;
    l[p] = c;
  }
  hi = __builtin_bit_cast(bf16x8, h);
  mid = __builtin_bit_cast(bf16x8, m);
  lo = __builtin_bit_cast(bf16x8, l);
}

// one K step of k_gemm_x6: the six plane products, smallest first
__device__ __forceinline__ f32x16 f8_mfma6(bf16x8 ah, bf16x8 am, bf16x8 al, bf16x8 bh, bf16x8 bm, bf16x8 bl,
                                           f32x16 acc) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
  return acc;
}

struct Fc8Fwd {
  const float* W8;  // [K8 = g.N][D]
  int ldb, D;
  int tile8, grid8;  // the launch plan of today's fc8 forward (its x_plan inputs)
  float* slab8;      // [S8][g.M][D]
};

// g: the argument block k_gemm_reduce would get for the fc7 forward.  Items
// are (32-row block, fc8 K slice); every y7 element belongs to exactly one.
__global__ void __launch_bounds__(256, 2) k_fc8_fwd_fused(GemmArgs g, Fc8Fwd a) {
  __shared__ __attribute__((aligned(16))) char xl[3 * F8PLANE];
  const int Meff = eff_dim(g.M, g.M_dev);
  const int K8 = g.N;
  const int S7 = x_plan(Meff, g.N, eff_dim(g.K, g.K_dev), g.tile, g.xgrid, split_bk(g.prec)).S;
  const XPlan p8 = x_plan(Meff, a.D, K8, a.tile8, a.grid8, F8BK);
  const int kstep = (p8.ns + p8.S - 1) / p8.S;
  const int mb = (Meff + 31) / 32;
  const int items = mb * p8.S;
  const int t = threadIdx.x, lane = pcnn::lane_id(), wave = t >> 6;
  const int r = lane & 31, hsel = lane >> 5;
  const bool mm = wave * 32 < a.D;  // this wave owns a live 32-column block
  const bool dr = g.drop || g.keep != 1.f;
  const uint32_t step = g.drop_gen && g.drop_step ? (uint32_t)*g.drop_step : 0u;
  const int n4 = g.N >> 2;
  const size_t slab_stride = (size_t)g.M * g.N;
  const XOp oc = x_op(g.C, g.ldc, (long)(g.M - 1) * g.ldc + g.N);
  const XOp ow = x_op(a.W8, a.ldb, (long)(K8 - 1) * a.ldb + a.D);
  const int ncol = wave * 32 + r;  // this lane's fc8 column

  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int z = item / mb, m0 = (item - z * mb) * 32;
    const int kl = z * kstep, kh = min(p8.ns, kl + kstep);
    const int nsteps = kh > kl ? kh - kl : 0;
    f32x16 acc = (f32x16){};
    for (int c0 = 0; c0 < nsteps; c0 += F8CH) {
      const int nch = min(F8CH, nsteps - c0);
      const int kb = (kl + c0) * F8BK, ke = min(K8, kb + nch * F8BK);
      // A: the slice's y7 quads (32 rows x 32 quads, four per thread; a wave
      // reads two 512-B row segments per load) formed as k_gemm_reduce forms them
      unsigned vo[4];
      bool ok[4];
      xf4 v[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int qi = t + 256 * u;
        const int m = m0 + (qi >> 5), n = kb + 4 * (qi & 31);
        ok[u] = m < Meff && n < ke;
        vo[u] = ok[u] ? (unsigned)(m * g.N + n) * 4u : kXOob;
      }
      if (S7 == 1) {  // whole tiles: the GEMM's epilogue wrote bias / act into C
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const int qi = t + 256 * u;
          const int m = m0 + (qi >> 5), n = kb + 4 * (qi & 31);
          v[u] = x_ld4(oc, ok[u] ? (unsigned)(m * g.ldc + n) * 4u : kXOob, 0);
        }
      } else {  // slab sums in slice order z = 0, 1, ...
        const XOp o0 = x_op(g.slab, g.N, (long)slab_stride);
#pragma unroll
        for (int u = 0; u < 4; u++) v[u] = x_ld4(o0, vo[u], 0);
        // eight slabs' loads in flight at a time (the flagship's S7 is 8 or
        // 16): one memory round trip per group, added in slice order
        int zz = 1;
        for (; zz + 7 <= S7; zz += 7) {
          xf4 tt[7][4];
#pragma unroll
          for (int d = 0; d < 7; d++) {
            const XOp oz = x_op(g.slab + (zz + d) * slab_stride, g.N, (long)slab_stride);
#pragma unroll
            for (int u = 0; u < 4; u++) tt[d][u] = x_ld4(oz, vo[u], 0);
          }
#pragma unroll
          for (int d = 0; d < 7; d++)
#pragma unroll
            for (int u = 0; u < 4; u++) {
              v[u][0] += tt[d][u][0]; v[u][1] += tt[d][u][1]; v[u][2] += tt[d][u][2]; v[u][3] += tt[d][u][3];
            }
        }
        for (; zz < S7; zz++) {
          const XOp oz = x_op(g.slab + zz * slab_stride, g.N, (long)slab_stride);
#pragma unroll
          for (int u = 0; u < 4; u++) {
            const xf4 tt = x_ld4(oz, vo[u], 0);
            v[u][0] += tt[0]; v[u][1] += tt[1]; v[u][2] += tt[2]; v[u][3] += tt[3];
          }
        }
      }
      // B: this lane's W8 column, k 8 hsel .. +7 of every step, straight to
      // registers (issued once the slab loads have landed: both sets at once
      // would cost the second workgroup per CU; W8 comes from L2 under the
      // epilogue and the staging below)
      float bv[F8CH][8];
#pragma unroll
      for (int s = 0; s < F8CH; s++)
#pragma unroll
        for (int e = 0; e < 8; e++) {
          const int k = kb + F8BK * s + 8 * hsel + e;
          const bool okb = mm && ncol < a.D && k < ke;
          bv[s][e] = x_ld1(ow, okb ? (unsigned)(k * a.ldb + ncol) * 4u : kXOob, 0);
        }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int qi = t + 256 * u;
        const int row = qi >> 5, kq = qi & 31;
        const int m = m0 + row, n = kb + 4 * kq;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok[u]) {
          o = make_float4(v[u][0], v[u][1], v[u][2], v[u][3]);
          if (S7 != 1)
            o = make_float4(epilogue(o.x, g, m, n), epilogue(o.y, g, m, n + 1), epilogue(o.z, g, m, n + 2),
                            epilogue(o.w, g, m, n + 3));
          if (g.drop_gen) {  // one Philox block per float4: the element quad
            const uint32_t q = pcnn_philox::keep_quad((uint64_t)(m * n4 + (n >> 2)), g.drop_k0, g.drop_k1, g.drop_sid,
                                                      step, g.keep);
            *(uint32_t*)((uint8_t*)g.drop + (size_t)m * g.ldd + n) = q;
            o = make_float4((g.keep != 1.f ? o.x / g.keep : o.x) * (float)(q & 1u),
                            (g.keep != 1.f ? o.y / g.keep : o.y) * (float)((q >> 8) & 1u),
                            (g.keep != 1.f ? o.z / g.keep : o.z) * (float)((q >> 16) & 1u),
                            (g.keep != 1.f ? o.w / g.keep : o.w) * (float)((q >> 24) & 1u));
          } else if (dr) {
            o = make_float4(drop_epi(o.x, g, m, n), drop_epi(o.y, g, m, n + 1), drop_epi(o.z, g, m, n + 2),
                            drop_epi(o.w, g, m, n + 3));
          }
          if (S7 != 1 || dr) *(float4*)(g.C + (size_t)m * g.ldc + n) = o;
        }
        unsigned h0, m0_, l0, h1, m1, l1;
        x_split3(o.x, o.y, h0, m0_, l0);
        x_split3(o.z, o.w, h1, m1, l1);
        char* p = xl + row * F8ROW + 8 * kq;
        *(uint2*)p = make_uint2(h0, h1);
        *(uint2*)(p + F8PLANE) = make_uint2(m0_, m1);
        *(uint2*)(p + 2 * F8PLANE) = make_uint2(l0, l1);
      }
      __syncthreads();
      if (mm) {
        // (B is split step by step: the 96 registers of all its planes at
        // once would cost the second workgroup per CU)
#pragma unroll
        for (int s = 0; s < F8CH; s++)
          if (s < nch) {
            const char* p = xl + r * F8ROW + 2 * (F8BK * s + 8 * hsel);
            const bf16x8 ah = *(const bf16x8*)p;
            const bf16x8 am = *(const bf16x8*)(p + F8PLANE);
            const bf16x8 al = *(const bf16x8*)(p + 2 * F8PLANE);
            bf16x8 bh, bm, bl;
            f8_split8(bv[s], bh, bm, bl);
            acc = f8_mfma6(ah, am, al, bh, bm, bl, acc);
          }
      }
      __syncthreads();  // the next chunk / item restages the planes
    }
    // the raw partial block to fc8's slab z (k_gemm_x6's split-K epilogue)
    if (mm && ncol < a.D) {
#pragma unroll
      for (int q = 0; q < 16; q++) {
        const int m = m0 + 4 * hsel + f8_qrow(q);
        const float vq = acc[q];
        if (m < Meff) a.slab8[((size_t)z * g.M + m) * a.D + ncol] = vq;
      }
    }
  }
}

// k_head_fwd's row pass (one wave per row) with y8 formed in place: the fc8
// slabs in slice order, then + b8 (k_gemm_reduce; vec: its float4 branch
// starts from slab 0, its scalar branch from 0.f).
__global__ void __launch_bounds__(256) k_fc8_reduce_head_fwd(const float* __restrict__ slab,
                                                              const float* __restrict__ b8, int M, int K, int D,
                                                              int tile8, int grid8, int vec,
                                                              const int32_t* __restrict__ M_dev,
                                                              const float* __restrict__ pw, float* __restrict__ y8,
                                                              float* __restrict__ t_out, float* __restrict__ pred) {
  const int R = eff_dim(M, M_dev);
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = pcnn::lane_id();
  if (row >= R) return;
  const int S = x_plan(R, D, K, tile8, grid8, F8BK).S;
  const size_t slab_stride = (size_t)M * D;
  float y[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int c = lane + 64 * k;
    y[k] = 0.f;
    if (c < D) {
      const float* sp = slab + (size_t)row * D + c;
      // every slab's load in flight at once (S <= kMaxSplitX; slices past
      // S re-read the last one and are not added): one round trip per row
      float sv[kMaxSplitX];
#pragma unroll
      for (int z = 0; z < kMaxSplitX; z++) sv[z] = sp[(z < S ? z : S - 1) * slab_stride];
      float v = (vec || S == 1) ? sv[0] : 0.f + sv[0];
#pragma unroll
      for (int z = 1; z < kMaxSplitX; z++) v = z < S ? v + sv[z] : v;
      v += b8[c];
      y8[(size_t)row * D + c] = v;
      y[k] = v;
    }
  }
  pcnn_head::head_fwd_row(y, pw, row, D, lane, t_out, pred);
}

struct Fc8Dx {
  int M, D, N;  // capacity rows, fc8 columns (the contraction), fc7 units
  const float* dy8;
  int lda;
  const float* W8;  // [N][D]
  int ldb;
  const float* mask;  // y7 (relu + dropout backward), or null
  int ldm;
  float keep;
  float* C;
  int ldc;
  const int32_t* M_dev;
};

// Items are (32-row block, 128-column group), one 32 x 32 block per wave.
// Both fragments come straight from memory (a lane's 8 k of a step are two
// float4 of its dY8 row / W8 row), the loads of step s + 1 in flight under
// the MFMAs of step s.  No LDS and at most 128 registers: on the step's
// chain this kernel starts beside the next minibatch's vote kernels, which
// fill every SIMD with small waves -- a workgroup that needs half a SIMD's
// registers or LDS waits for several of them to retire.
__global__ void __launch_bounds__(256, 4) k_fc8_dx_skinny(Fc8Dx a) {
  const int Meff = eff_dim(a.M, a.M_dev);
  const int mb = (Meff + 31) / 32, ng = (a.N + 127) / 128;
  const int lane = pcnn::lane_id(), wave = threadIdx.x >> 6;
  const int r = lane & 31, hsel = lane >> 5;
  const int ns = (a.D + F8BK - 1) / F8BK;
  const XOp oa = x_op(a.dy8, a.lda, (long)(a.M - 1) * a.lda + a.D);
  const XOp ob = x_op(a.W8, a.ldb, (long)(a.N - 1) * a.ldb + a.D);
  const XOp om = x_op(a.mask, a.ldm, a.mask ? (long)(a.M - 1) * a.ldm + a.N : 0);
  const XOp oc = x_op(a.C, a.ldc, (long)(a.M - 1) * a.ldc + a.N);
  const bool msk = a.mask != nullptr;
  for (int item = blockIdx.x; item < mb * ng; item += gridDim.x) {
    const int cg = item / mb, m0 = (item - cg * mb) * 32;
    const int n0 = cg * 128 + wave * 32;
    if (n0 >= a.N) continue;
    const int am = m0 + r, bn = n0 + r;
    const bool aok = am < Meff, bok = bn < a.N;
    const unsigned abase = (unsigned)(am * a.lda + 8 * hsel) * 4u, bbase = (unsigned)(bn * a.ldb + 8 * hsel) * 4u;
    // quad h of step s: k = 16 s + 8 hsel + 4 h (D % 4 == 0: inside K or past it -> zeros)
    auto load = [&](int s, xf4 (&x)[2], xf4 (&w)[2]) {
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const bool in = s < ns && F8BK * s + 8 * hsel + 4 * h < a.D;
        const unsigned ko = (unsigned)(F8BK * s + 4 * h) * 4u;
        x[h] = x_ld4(oa, in && aok ? abase + ko : kXOob, 0);
        w[h] = x_ld4(ob, in && bok ? bbase + ko : kXOob, 0);
      }
    };
    xf4 xa[2][2], xb[2][2];
    load(0, xa[0], xb[0]);
    // the 16 mask values of the block, in flight under the K steps
    const int rlane = m0 + 4 * hsel;
    float mv[16];
    if (msk) {
#pragma unroll
      for (int q = 0; q < 16; q++) {
        const bool ok = bok && rlane + f8_qrow(q) < Meff;
        mv[q] = x_ld1(om, ok ? (unsigned)((rlane + f8_qrow(q)) * a.ldm + bn) * 4u : kXOob, 0);
      }
    }
    f32x16 acc = (f32x16){};
#pragma unroll
    for (int s = 0; s < F8MAXD / F8BK; s++)
      if (s < ns) {
        if (s + 1 < F8MAXD / F8BK) load(s + 1, xa[(s + 1) & 1], xb[(s + 1) & 1]);
        float va[8], vb[8];
#pragma unroll
        for (int h = 0; h < 2; h++)
#pragma unroll
          for (int e = 0; e < 4; e++) {
            va[4 * h + e] = xa[s & 1][h][e];
            vb[4 * h + e] = xb[s & 1][h][e];
          }
        bf16x8 ah, am_, al, bh, bm, bl;
        f8_split8(va, ah, am_, al);
        f8_split8(vb, bh, bm, bl);
        acc = f8_mfma6(ah, am_, al, bh, bm, bl, acc);
      }
    // x_epilogue's expressions (gemm_common.h) with no bias: acc + 0.f, the
    // mask test, the 128-tile form's v / keep
#pragma unroll
    for (int q = 0; q < 16; q++) {
      const bool ok = bok && rlane + f8_qrow(q) < Meff;
      float v = acc[q] + 0.f;
      if (msk && !(mv[q] > 0.f)) v = 0.f;
      if (a.keep != 1.f) v = v / a.keep;
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), oc.rs,
                                            ok ? (unsigned)((rlane + f8_qrow(q)) * a.ldc + bn) * 4u : kXOob, 0, 0);
    }
  }
}

// the inputs of today's fc8 forward plan (pcnn_gemm at precision 2)
inline LaunchPlan fc8_plan(int M, int D, int K, bool m_dynamic) { return plan_launch(M, D, K, m_dynamic, 2); }

}  // namespace

extern "C" int pcnn_fc8_fwd_fused(int M, int N7, int K7, const void* fc7_workspace, size_t fc7_workspace_bytes,
                                  const float* b7, int act7, float* y7, int ld7, uint8_t* drop, int ldd,
                                  float keep_prob, int drop_gen, uint64_t seed, const int64_t* step_dev,
                                  int stream_id, const float* W8, int ldb, int D, const int32_t* M_dev,
                                  void* fc8_workspace, size_t fc8_workspace_bytes, void* stream) {
  PCNN_REQUIRE(M >= 0 && N7 > 0 && K7 >= 0 && fc7_workspace && y7 && W8 && fc8_workspace);
  PCNN_REQUIRE(D > 0 && D <= F8MAXD && ldb >= D && ld7 >= N7);
  PCNN_REQUIRE(act7 == 0 || act7 == 1);
  PCNN_REQUIRE(keep_prob > 0.f && keep_prob <= 1.f && (keep_prob == 1.f || drop));
  PCNN_REQUIRE(!drop_gen || (drop && stream_id >= 0));
  // the shapes k_gemm_reduce's float4 branch takes, and 32-bit buffer offsets
  PCNN_REQUIRE(N7 % 4 == 0 && ld7 % 4 == 0 &&
               ((((uintptr_t)fc7_workspace) | ((uintptr_t)y7) | ((uintptr_t)b7)) & 15) == 0);
  PCNN_REQUIRE(!drop || (ldd >= N7 && ldd % 4 == 0 && ((uintptr_t)drop & 3) == 0 && (long)M * ldd < (1l << 31)));
  PCNN_REQUIRE((long)M * ld7 < (1l << 29) && (long)N7 * ldb < (1l << 29) && (long)M * N7 < (1l << 29));
  if (M == 0) return PCNN_OK;
  const bool dyn = M_dev != nullptr;
  if (fc7_workspace_bytes < gemm_workspace_bytes(M, N7, K7, dyn, 2) ||
      fc8_workspace_bytes < gemm_workspace_bytes(M, D, N7, dyn, 2) ||
      fc8_workspace_bytes < (size_t)M * D * sizeof(float))
    return PCNN_ECAPACITY;
  const LaunchPlan p7 = plan_launch(M, N7, K7, dyn, 2), p8 = fc8_plan(M, D, N7, dyn);
  GemmArgs g{M, N7, K7, nullptr, nullptr, 0, nullptr, 0, y7, ld7, b7, act7, nullptr, 0, M_dev, nullptr,
             (float*)fc7_workspace, 2, p7.tile, p7.grid, 0, drop, ldd, keep_prob};
  if (drop_gen) {
    g.drop_gen = 1;
    g.drop_k0 = (uint32_t)seed;
    g.drop_k1 = (uint32_t)(seed >> 32);
    g.drop_sid = (uint32_t)stream_id;
    g.drop_step = step_dev;
  }
  const Fc8Fwd a{W8, ldb, D, p8.tile, p8.grid, (float*)fc8_workspace};
  const long items = (long)((M + 31) / 32) * kMaxSplitX;
  const int grid = (int)(items < 512 ? items : 512);
  hipLaunchKernelGGL(k_fc8_fwd_fused, dim3(grid), dim3(256), 0, (hipStream_t)stream, g, a);
  PCNN_CHECK_LAUNCH();
  return PCNN_OK;
}

extern "C" int pcnn_fc8_reduce_head_fwd(const void* fc8_workspace, size_t fc8_workspace_bytes, const float* b8,
                                        int R_cap, int K, int D, const int32_t* num_rois_dev,
                                        const float* poses_weight, float* y8, float* tanh_out, float* pred,
                                        void* stream) {
  PCNN_REQUIRE(fc8_workspace && b8 && poses_weight && y8 && tanh_out && pred && R_cap >= 0 && K >= 0);
  PCNN_REQUIRE(D > 0 && D <= F8MAXD);
  if (R_cap == 0) return PCNN_OK;
  const bool dyn = num_rois_dev != nullptr;
  if (fc8_workspace_bytes < gemm_workspace_bytes(R_cap, D, K, dyn, 2) ||
      fc8_workspace_bytes < (size_t)R_cap * D * sizeof(float))
    return PCNN_ECAPACITY;
  const LaunchPlan p8 = fc8_plan(R_cap, D, K, dyn);
  // k_gemm_reduce's float4 condition for this shape (C = y8, ldc = D)
  const int vec = (D & 3) == 0 && ((((uintptr_t)fc8_workspace) | ((uintptr_t)y8) | ((uintptr_t)b8)) & 15) == 0;
  hipLaunchKernelGGL(k_fc8_reduce_head_fwd, dim3((R_cap + 3) / 4), dim3(256), 0, (hipStream_t)stream,
                     (const float*)fc8_workspace, b8, R_cap, K, D, p8.tile, p8.grid, vec, num_rois_dev, poses_weight,
                     y8, tanh_out, pred);
  PCNN_CHECK_LAUNCH();
  return PCNN_OK;
}

extern "C" int pcnn_fc8_dx_skinny(const float* dy8, int lda, const float* W8, int ldb, const float* mask, int ldm,
                                  float keep_prob, float* dy7, int ldc, int M, int D, int N7,
                                  const int32_t* M_dev, void* stream) {
  PCNN_REQUIRE(dy8 && W8 && dy7 && M >= 0 && N7 > 0);
  PCNN_REQUIRE(D > 0 && D <= F8MAXD && D % 4 == 0);
  PCNN_REQUIRE(lda >= D && ldb >= D && ldc >= N7 && (!mask || ldm >= N7));
  PCNN_REQUIRE(keep_prob > 0.f && keep_prob <= 1.f);
  PCNN_REQUIRE(lda % 4 == 0 && ldb % 4 == 0 && ((((uintptr_t)dy8) | ((uintptr_t)W8)) & 15) == 0);
  PCNN_REQUIRE((long)M * lda < (1l << 29) && (long)N7 * ldb < (1l << 29) && (long)M * ldc < (1l << 29) &&
               (!mask || (long)M * ldm < (1l << 29)));
  if (M == 0) return PCNN_OK;
  const Fc8Dx a{M, D, N7, dy8, lda, W8, ldb, mask, ldm, keep_prob, dy7, ldc, M_dev};
  const long items = (long)((M + 31) / 32) * ((N7 + 127) / 128);
  const int grid = (int)(items < 2048 ? items : 2048);
  pcnn::launch_last(k_fc8_dx_skinny, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
  PCNN_CHECK_LAUNCH();
  return PCNN_OK;
}
