// Fused momentum-SGD update of a set of parameter tensors (include/posecnn_train.h):
// TF's ApplyMomentum on the gradient of loss + sum weight_reg l2_loss(var), the
// reference's train_op (lib/fcn/train.py:481,530-534), with the staircase
// learning rate and the step counter on the device.
//
// One launch walks every tensor: the unit of work is a chunk of kChunk elements
// of one tensor, a block finds its chunk's tensor by binary search over the
// chunk prefix, the grid strides over the chunks.  The update is memory bound:
// 20 B per element (read w, g, m; write w, m), 16 B per lane on each of the five
// streams.  A one-block finishing kernel behind it adds the chunks' partial
// sums of w^2 (the L2 loss value), stores the learning rate used and bumps the
// counter -- in stream order after every block that read it.
#include "pcnn_common.h"
#include "../../include/posecnn_train.h"

// Cache policy of the streams, a build-time switch for the A/B measurement
// (DESIGN.md "Momentum SGD"): bit 0: non-temporal loads of g, bit 1:
// non-temporal stores of w and m.
#ifndef PCNN_MOMENTUM_NT
#define PCNN_MOMENTUM_NT 0
#endif

namespace {

constexpr int kThreads = 256;
constexpr int kPerThread = 4;                         // float4 per thread and chunk
constexpr int kChunk = kThreads * kPerThread * 4;     // 4096 elements
constexpr int kFinishThreads = 1024;
constexpr int kBlocksPerCU = 4;  // 4 waves per SIMD, resident at up to 128 VGPRs

struct Hyper {
  float lr0, gamma;
  int stepsize;
  float momentum, weight_reg;
};

// lr0 gamma^(n / stepsize) in float64 by repeated multiplication, rounded once.
// A product that no longer changes (0, inf, gamma = 1) ends the loop: every
// later product is the same number.
__device__ __forceinline__ float lr_at(int64_t n, const Hyper& h) {
  double x = (double)h.lr0;
  const double gm = (double)h.gamma;
  const int64_t p = h.stepsize > 0 && n > 0 ? n / h.stepsize : 0;
  for (int64_t i = 0; i < p; ++i) {
    const double nx = x * gm;
    if (nx == x) break;
    x = nx;
  }
  return (float)x;
}

// The table holds addresses as integers: pointers made from them are typed as
// global memory here, so that the accesses are global_* and not flat_*.
typedef float v4f __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) float gf32;
typedef __attribute__((address_space(1))) v4f gv4f;

template <typename V>
__device__ __forceinline__ V load_g(const __attribute__((address_space(1))) V* p) {
#if PCNN_MOMENTUM_NT & 1
  return __builtin_nontemporal_load(p);
#else
  return *p;
#endif
}
template <typename V>
__device__ __forceinline__ void store_out(__attribute__((address_space(1))) V* p, V v) {
#if PCNN_MOMENTUM_NT & 2
  __builtin_nontemporal_store(v, p);
#else
  *p = v;
#endif
}

// One element: the six separately rounded operations of the header; `sq`
// collects w^2 of the weight before the update.
__device__ __forceinline__ void update(float& w, float g, float& m, float lr, float momentum, float weight_reg,
                                       bool reg, float& sq) {
  sq = sq + w * w;
  const float g2 = reg ? g + weight_reg * w : g;
  const float mn = momentum * m + g2;
  const float u = lr * mn;
  m = mn;
  w = w - u;
}

__device__ __forceinline__ void update_one(gf32* w, const gf32* g, gf32* m, float lr, const Hyper& h, bool reg,
                                           float& sq) {
  float wv = *w, mv = *m;
  update(wv, load_g(g), mv, lr, h.momentum, h.weight_reg, reg, sq);
  store_out(m, mv);
  store_out(w, wv);
}

__global__ void __launch_bounds__(kThreads) k_momentum(const int64_t* __restrict__ table,
                                                       const int32_t* __restrict__ chunk_start, int T,
                                                       int total_chunks, Hyper h,
                                                       const int64_t* __restrict__ step_dev,
                                                       float* __restrict__ partials) {
  __shared__ float s_wave[kThreads / PCNN_WAVE];
  const int tid = (int)threadIdx.x;
  const float lr = lr_at(*step_dev, h);
  for (int c = (int)blockIdx.x; c < total_chunks; c += (int)gridDim.x) {
    // the last tensor whose first chunk is <= c (tensors without elements have no chunk and are skipped)
    int lo = 0, hi = T - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (chunk_start[mid] <= c) lo = mid; else hi = mid - 1;
    }
    const int64_t* row = table + (size_t)lo * 5;
    const int64_t off = (int64_t)(c - chunk_start[lo]) * kChunk;
    gf32* w = (gf32*)row[0] + off;
    const gf32* g = (const gf32*)row[1] + off;
    gf32* m = (gf32*)row[2] + off;
    const int64_t left = row[3] - off;
    const int cnt = left < kChunk ? (int)left : kChunk;
    const bool reg = (row[4] & PCNN_MOMENTUM_REGULARIZE) != 0;
    const bool vec = (((uint64_t)row[0] | (uint64_t)row[1] | (uint64_t)row[2]) & 15) == 0;
    float sq = 0.f;
    if (vec) {
      const int nq = cnt >> 2;  // whole quads; the tail's owner is the thread of quad nq
      v4f W[kPerThread], G[kPerThread], M[kPerThread];
#pragma unroll
      for (int j = 0; j < kPerThread; ++j) {
        const int q = tid + kThreads * j;
        if (q < nq) {
          W[j] = ((const gv4f*)w)[q];
          G[j] = load_g((const gv4f*)g + q);
          M[j] = ((const gv4f*)m)[q];
        }
      }
#pragma unroll
      for (int j = 0; j < kPerThread; ++j) {
        const int q = tid + kThreads * j;
        if (q < nq) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            float wv = W[j][k], mv = M[j][k];
            update(wv, G[j][k], mv, lr, h.momentum, h.weight_reg, reg, sq);
            W[j][k] = wv;
            M[j][k] = mv;
          }
          store_out((gv4f*)m + q, M[j]);
          store_out((gv4f*)w + q, W[j]);
        }
      }
      if ((cnt & 3) && (nq & (kThreads - 1)) == tid)  // fewer than 4 elements, after this thread's quads
        for (int e = nq * 4; e < cnt; ++e) update_one(w + e, g + e, m + e, lr, h, reg, sq);
    } else {  // a base at an odd element offset: the same elements per thread, one at a time
      for (int j = 0; j < kPerThread; ++j) {
        const int e0 = (tid + kThreads * j) * 4;
        for (int e = e0; e < e0 + 4 && e < cnt; ++e) update_one(w + e, g + e, m + e, lr, h, reg, sq);
      }
    }
    if (partials) {  // (uniform) the chunk's sum of w^2: wave butterfly, then (s0 + s1) + (s2 + s3)
      const float s = pcnn::wave_sum(sq);
      if ((tid & 63) == 0) s_wave[tid >> 6] = s;
      __syncthreads();
      if (tid == 0) partials[c] = reg ? (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]) : 0.f;
      __syncthreads();  // s_wave is rewritten by the block's next chunk
    }
  }
}

__global__ void __launch_bounds__(kFinishThreads) k_momentum_finish(const float* __restrict__ partials,
                                                                    int total_chunks, Hyper h,
                                                                    int64_t* __restrict__ step_dev,
                                                                    float* __restrict__ reg_loss,
                                                                    float* __restrict__ lr_out) {
  __shared__ double s_wave[kFinishThreads / PCNN_WAVE];
  const int tid = (int)threadIdx.x;
  if (reg_loss) {
    double s = 0.0;
    for (int i = tid; i < total_chunks; i += kFinishThreads) s = s + (double)partials[i];
    s = pcnn::wave_sum(s);
    if ((tid & 63) == 0) s_wave[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
      double sum = s_wave[0];
      for (int k = 1; k < kFinishThreads / PCNN_WAVE; ++k) sum = sum + s_wave[k];
      reg_loss[0] = (float)(((double)h.weight_reg * 0.5) * sum);
    }
  }
  if (tid == 0) {
    const int64_t n = *step_dev;
    if (lr_out) lr_out[0] = lr_at(n, h);
    *step_dev = n + 1;
  }
}

int cu_count() {
  static int cus[pcnn::kMaxDevices] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= pcnn::kMaxDevices) return 256;
  if (cus[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cus[dev] = n;
  }
  return cus[dev];
}

}  // namespace

extern "C" int pcnn_train_abi_version(void) { return 1; }

extern "C" int pcnn_momentum_chunk(void) { return kChunk; }

extern "C" size_t pcnn_momentum_workspace_size(long total_chunks) {
  return pcnn::align_up((size_t)(total_chunks > 0 ? total_chunks : 1) * sizeof(float), 256);
}

extern "C" int pcnn_momentum_sgd(const int64_t* table, const int32_t* chunk_start, int T, long total_chunks,
                                 float lr0, float gamma, int stepsize, float momentum, float weight_reg,
                                 int64_t* step_dev, float* reg_loss, float* lr_out, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  PCNN_REQUIRE(T >= 0 && total_chunks >= 0 && total_chunks < (1l << 31) && step_dev);
  PCNN_REQUIRE(T == 0 ? total_chunks == 0 : (table && chunk_start));
  // (written so that a NaN fails)
  PCNN_REQUIRE(momentum >= 0.f && momentum < 1.f && lr0 >= 0.f && weight_reg >= 0.f && gamma > 0.f && stepsize >= 0);
  PCNN_REQUIRE(!reg_loss || (workspace && workspace_bytes >= pcnn_momentum_workspace_size(total_chunks)));
  PCNN_REQUIRE(((uintptr_t)workspace & 3) == 0);
  const Hyper h{lr0, gamma, stepsize, momentum, weight_reg};
  float* partials = reg_loss ? (float*)workspace : nullptr;
  const hipStream_t st = (hipStream_t)stream;
  if (total_chunks > 0) {
    const long cap = (long)cu_count() * kBlocksPerCU;
    const unsigned grid = (unsigned)(total_chunks < cap ? total_chunks : cap);
    hipLaunchKernelGGL(k_momentum, dim3(grid), dim3(kThreads), 0, st, table, chunk_start, T, (int)total_chunks, h,
                       (const int64_t*)step_dev, partials);
    PCNN_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_momentum_finish, dim3(1), dim3(kFinishThreads), 0, st, (const float*)partials,
                     (int)total_chunks, h, step_dev, reg_loss, lr_out);
  PCNN_CHECK_LAUNCH();
  return PCNN_OK;
}
