// Entry points of the pose-head FC GEMMs (pcnn_gemm, pcnn_gemm_drop,
// pcnn_gemm_drop_gen, pcnn_gemm_workspace_size) and the split-K reducer.
//
// Replaces the TF matmuls of Network.fc (lib/networks/network.py:393-423) as
// wired by vgg16_convs.py:186-197: pool5 + pool4 -> fc6 (25088 -> 4096, relu)
// -> fc7 (4096 -> 4096, relu) -> fc8 (4096 -> 4C), and their backward
// products.  C = epilogue(op(A) (+ op(A2)) * op(B)); the kernels are
// k_gemm_f32 (gemm_f32.hip, precision 0), k_gemm_x3 (gemm_x3.hip, 1) and
// k_gemm_x6 (gemm_x6.hip, 2).  The row count M and, for the weight gradients,
// the contraction length K may live on the device, so the whole pose step
// runs without a host sync.  The host plans the launch from the capacity
// shape (plan_launch, gemm_plan.h); shapes with few tiles split K, and
// k_gemm_reduce sums the partial slabs in fixed order and applies the
// epilogue and the dropout.
#include "gemm_common.h"
#include "pcnn_philox.h"

using namespace pcnn_gk;

namespace {

// drop_gen: keep byte of element (m, n), drawn (element quad m N/4 + n/4) and
// stored for the backward; the lane whose n is the quad's first stores all four
__device__ __forceinline__ float drop_gen_epi(float v, const GemmArgs& g, uint32_t step, int m, int n) {
  const uint32_t q = pcnn_philox::keep_quad((uint64_t)m * (uint64_t)(g.N >> 2) + (uint64_t)(n >> 2), g.drop_k0,
                                            g.drop_k1, g.drop_sid, step, g.keep);
  if ((n & 3) == 0) *(uint32_t*)((uint8_t*)g.drop + (size_t)m * g.ldd + n) = q;
  if (g.keep != 1.f) v = v / g.keep;
  return v * (float)((q >> (8 * (n & 3))) & 1u);
}

__global__ void __launch_bounds__(256) k_gemm_reduce(GemmArgs g) {
  const int Meff = eff_dim(g.M, g.M_dev);
  const int Keff = eff_dim(g.K, g.K_dev);
  const int S = g.prec ? x_plan(Meff, g.N, Keff, g.tile, g.xgrid, split_bk(g.prec)).S : split_for(Meff, g.N, Keff);
  const bool dr = g.drop || g.keep != 1.f;
  const uint32_t step = g.drop_gen && g.drop_step ? (uint32_t)*g.drop_step : 0u;
  auto dropv = [&](float v, int m, int n) { return g.drop_gen ? drop_gen_epi(v, g, step, m, n) : drop_epi(v, g, m, n); };
  if (S == 1) {
    // whole tiles: the GEMM's own epilogue wrote bias / act / mask; dropout
    // (or the backward's 1 / keep) is applied here, in place -- unless the
    // 128-tile epilogue already scaled by 1 / keep
    if (!dr || keep_in_epilogue(g)) return;
    const long total = (long)Meff * g.N;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
      const int m = (int)(i / g.N), n = (int)(i % g.N);
      float* c = g.C + (size_t)m * g.ldc + n;
      *c = dropv(*c, m, n);
    }
    return;
  }
  // slab sums in slice order z = 0, 1, ... (0 + s0 == s0, so starting from
  // s0 is the same fp32 sum); float4 along N when rows stay 16-B aligned
  const size_t slab_stride = (size_t)g.M * g.N;
  const bool vec = (long)g.M * g.N < (1l << 31) && (g.N & 3) == 0 && (g.ldc & 3) == 0 && (!g.mask || (g.ldm & 3) == 0) &&
                   (!g.drop || (g.ldd & 3) == 0) &&
                   ((((uintptr_t)g.slab) | ((uintptr_t)g.C) | ((uintptr_t)g.mask) | ((uintptr_t)g.bias)) & 15) == 0;
  if (vec) {
    const int n4 = g.N >> 2;
    const int total4 = Meff * n4;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += gridDim.x * blockDim.x) {
      const int m = i / n4, n = (i - m * n4) << 2;
      const float4* sp = (const float4*)(g.slab + (size_t)m * g.N + n);
      float4 v = sp[0];
      for (int z = 1; z < S; z++) {
        const float4 t = sp[z * (slab_stride >> 2)];
        v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
      }
      float4 o = make_float4(epilogue(v.x, g, m, n), epilogue(v.y, g, m, n + 1), epilogue(v.z, g, m, n + 2),
                             epilogue(v.w, g, m, n + 3));
      if (g.drop_gen) {  // one Philox block per float4: the element quad
        const uint32_t q = pcnn_philox::keep_quad((uint64_t)i, g.drop_k0, g.drop_k1, g.drop_sid, step, g.keep);
        *(uint32_t*)((uint8_t*)g.drop + (size_t)m * g.ldd + n) = q;
        o = make_float4((g.keep != 1.f ? o.x / g.keep : o.x) * (float)(q & 1u),
                        (g.keep != 1.f ? o.y / g.keep : o.y) * (float)((q >> 8) & 1u),
                        (g.keep != 1.f ? o.z / g.keep : o.z) * (float)((q >> 16) & 1u),
                        (g.keep != 1.f ? o.w / g.keep : o.w) * (float)((q >> 24) & 1u));
      } else if (dr) {
        o = make_float4(drop_epi(o.x, g, m, n), drop_epi(o.y, g, m, n + 1), drop_epi(o.z, g, m, n + 2),
                        drop_epi(o.w, g, m, n + 3));
      }
      *(float4*)(g.C + (size_t)m * g.ldc + n) = o;
    }
    return;
  }
  const long total = (long)Meff * g.N;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int m = (int)(i / g.N), n = (int)(i % g.N);
    float v = 0.f;
    for (int z = 0; z < S; z++) v += g.slab[((size_t)z * g.M + m) * g.N + n];
    v = epilogue(v, g, m, n);
    g.C[(size_t)m * g.ldc + n] = dr ? dropv(v, m, n) : v;
  }
}

}  // namespace

namespace pcnn_gk {
void launch_gemm_reduce(const GemmArgs& g, hipStream_t st) {
  hipLaunchKernelGGL(k_gemm_reduce, dim3(1024), dim3(256), 0, st, g);
}
}  // namespace pcnn_gk

extern "C" size_t pcnn_gemm_workspace_size(int M, int N, int K, int m_dynamic, int precision) {
  return gemm_workspace_bytes(M, N, K, m_dynamic != 0, precision);
}

extern "C" int pcnn_gemm(int M, int N, int K, const float* A, const float* A2, int lda, int a_trans, const float* B,
                         int ldb, int b_trans, float* Cm, int ldc, const float* bias, int act, const float* mask,
                         int ldm, const int32_t* M_dev, const int32_t* K_dev, int precision, void* workspace,
                         size_t workspace_bytes, void* stream) {
  return pcnn_gemm_drop(M, N, K, A, A2, lda, a_trans, B, ldb, b_trans, Cm, ldc, bias, act, mask, ldm, nullptr, 0, 1.f,
                        M_dev, K_dev, precision, workspace, workspace_bytes, stream);
}

static int gemm_impl(int M, int N, int K, const float* A, const float* A2, int lda, int a_trans, const float* B,
                     int ldb, int b_trans, float* Cm, int ldc, const float* bias, int act, const float* mask, int ldm,
                     const uint8_t* drop, int ldd, float keep_prob, const int32_t* M_dev, const int32_t* K_dev,
                     int precision, void* workspace, size_t workspace_bytes, void* stream, int drop_gen,
                     uint64_t seed, const int64_t* step_dev, int stream_id, bool skip_reduce = false) {
  PCNN_REQUIRE(M >= 0 && N > 0 && K >= 0 && A && B && Cm);
  PCNN_REQUIRE(!drop_gen || (drop && N % 4 == 0 && ldd % 4 == 0 && ((uintptr_t)drop & 3) == 0 && stream_id >= 0 &&
                             (long)M * (N / 4) < (1l << 31)));
  PCNN_REQUIRE(keep_prob > 0.f && keep_prob <= 1.f);
  PCNN_REQUIRE(!drop || (ldd >= N && (long)M * ldd < (1l << 31)));
  PCNN_REQUIRE(precision >= 0 && precision <= 2);
  PCNN_REQUIRE(lda >= (a_trans ? M : K) && ldb >= (b_trans ? K : N) && ldc >= N);
  PCNN_REQUIRE(!mask || ldm >= N);
  PCNN_REQUIRE(act == 0 || act == 1);
  // split-bf16 path: 16-B vector staging loads, 32-bit buffer offsets
  PCNN_REQUIRE(precision == 0 || (lda % 4 == 0 && ldb % 4 == 0 && ((uintptr_t)A & 15) == 0 &&
                                  ((uintptr_t)B & 15) == 0 && (!A2 || ((uintptr_t)A2 & 15) == 0)));
  PCNN_REQUIRE(precision == 0 || ((long)(a_trans ? K : M) * lda < (1l << 29) && (long)(b_trans ? N : K) * ldb < (1l << 29) &&
                                  (long)M * ldc < (1l << 29) && (!mask || (long)M * ldm < (1l << 29))));
  if (M == 0) return PCNN_OK;
  if (workspace_bytes < pcnn_gemm_workspace_size(M, N, K, M_dev != nullptr, precision) || !workspace)
    return PCNN_ECAPACITY;
  const LaunchPlan plan = plan_launch(M, N, K, M_dev != nullptr, precision);
  GemmArgs g{M, N, K, A, A2, lda, B, ldb, Cm, ldc, bias, act, mask, ldm, M_dev, K_dev, (float*)workspace, precision,
             plan.tile, plan.grid, plan.c_stream, drop, ldd, keep_prob};
  if (drop_gen) {
    g.drop_gen = 1;
    g.drop_k0 = (uint32_t)seed;
    g.drop_k1 = (uint32_t)(seed >> 32);
    g.drop_sid = (uint32_t)stream_id;
    g.drop_step = step_dev;
  }
  hipStream_t st = (hipStream_t)stream;
  // the op's completion event goes to whichever launch is last: held back
  // from the GEMM kernel when a reduce follows
  const bool reduce_after = !skip_reduce && reduce_follows(plan, precision, drop, keep_prob);
  if (precision == 0) {
    launch_gemm_f32(g, a_trans, b_trans, st);
    if (reduce_after) launch_gemm_reduce(g, st);
    PCNN_CHECK_LAUNCH();
    return PCNN_OK;
  }
  const bool ragged = split_ragged(a_trans != 0, b_trans != 0, M, N, K, K_dev != nullptr);
  const SplitVariant v{a_trans != 0, b_trans != 0, ragged, A2 != nullptr, plan.gen};
  const hipEvent_t done_ev = reduce_after ? pcnn::take_done_event() : nullptr;
  if (precision == 2) launch_gemm_x6(g, v, st);
  else launch_gemm_x3(g, v, st);
  if (reduce_after) {
    pcnn::t_done_event = done_ev;
    pcnn::launch_last(k_gemm_reduce, dim3(1024), dim3(256), 0, st, g);
  }
  PCNN_CHECK_LAUNCH();
  return PCNN_OK;
}

extern "C" int pcnn_gemm_drop(int M, int N, int K, const float* A, const float* A2, int lda, int a_trans,
                              const float* B, int ldb, int b_trans, float* Cm, int ldc, const float* bias, int act,
                              const float* mask, int ldm, const uint8_t* drop, int ldd, float keep_prob,
                              const int32_t* M_dev, const int32_t* K_dev, int precision, void* workspace,
                              size_t workspace_bytes, void* stream) {
  return gemm_impl(M, N, K, A, A2, lda, a_trans, B, ldb, b_trans, Cm, ldc, bias, act, mask, ldm, drop, ldd, keep_prob,
                   M_dev, K_dev, precision, workspace, workspace_bytes, stream, 0, 0, nullptr, 0);
}

extern "C" int pcnn_gemm_drop_gen(int M, int N, int K, const float* A, const float* A2, int lda, int a_trans,
                                  const float* B, int ldb, int b_trans, float* Cm, int ldc, const float* bias, int act,
                                  uint8_t* drop_out, int ldd, float keep_prob, uint64_t seed,
                                  const int64_t* step_dev, int stream_id, const int32_t* M_dev, const int32_t* K_dev,
                                  int precision, void* workspace, size_t workspace_bytes, void* stream) {
  return gemm_impl(M, N, K, A, A2, lda, a_trans, B, ldb, b_trans, Cm, ldc, bias, act, nullptr, 0, drop_out, ldd,
                   keep_prob, M_dev, K_dev, precision, workspace, workspace_bytes, stream, 1, seed, step_dev,
                   stream_id);
}

extern "C" int pcnn_gemm_partial(int M, int N, int K, const float* A, const float* A2, int lda, int a_trans,
                                 const float* B, int ldb, int b_trans, float* Cm, int ldc, const float* bias, int act,
                                 const int32_t* M_dev, const int32_t* K_dev, int precision, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  return gemm_impl(M, N, K, A, A2, lda, a_trans, B, ldb, b_trans, Cm, ldc, bias, act, nullptr, 0, nullptr, 0, 1.f,
                   M_dev, K_dev, precision, workspace, workspace_bytes, stream, 0, 0, nullptr, 0, true);
}
