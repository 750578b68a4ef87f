// Evaluation on the device (include/posecnn_eval.h): the pose errors of
// lib/utils/pose_error.py (add, adi, re, te, reproj) per (estimate, ground
// truth) pair, their per-class tally (lib/datasets/lov.py:582-607) and the
// confusion matrix of two label maps (imdb.fast_hist, lib/datasets/imdb.py:
// 123-125).
//
// Pose errors.  ADD-S is the cost: P^2 point pairs per row.  A 256-thread
// workgroup owns (row, chunk of kChunk = 256 query points).  The class's
// estimate-transformed candidates are staged once per workgroup in LDS as
// float4 (whole up to kTile = 8192 points = 128 KB, tiled with a running
// minimum above); each of the four waves scans its quarter of the candidates
// for the same 256 ground-truth-transformed queries, kPPL = 4 per lane, as
// wave-uniform broadcast reads: one ds_read_b128 (4 LDS cycles per wave)
// feeds 4 x 9 VALU operations per lane, so the four SIMDs' VALU and not the
// LDS array bounds the scan.  Queries per lane, with as many waves per
// workgroup (POSE_EVAL_PPL), the whole op at N = 64, P = 2620: 1: 377 us,
// 2: 245 us, 4: 145 us (kept), 8: 160 us -- the order average_distance.hip's
// exact scan found for the loss.  The quarters meet
// in LDS; a minimum does not depend on the order.  The same workgroup
// computes ADD and reproj of its 256 points, one per thread, and reduces the
// three per-point values in float64 in the header's fixed order.  A second
// kernel, one thread per row, folds the chunk sums and computes re and te.
//
// Confusion.  Memory bound (8 B per pixel), and almost every lane of a wave
// holds the same key (background): a lane whose four pixels share a key
// counts them as one item of weight 4, the lanes of a wave that share a key
// add once, by their count, and only the waves on a region's edge go through
// the four components one by one.  A workgroup counts in an int32 LDS table
// (C <= 128) and flushes the non-zero entries to the int64 table once.
// Geometry sweep (DESIGN.md "Evaluation", B = 8, 480 x 640, C = 22, rendered
// labels / all background, us per call in a replayed graph, the copy of the
// same bytes 5.8): 1024 threads, one int4 pair per thread, one workgroup per
// CU 11.8 / 6.2 (kept); two per CU 11.7 / 6.7; two pairs per thread 15.6 /
// 6.4; 512 threads, four per CU 13.5 / 10.1.  A grid capped at 128 or 64
// workgroups was slower, not faster, so the flush is not what the rendered
// case waits for: it is the key loop of the edge waves.
#include "pcnn_common.h"
#include "../../include/posecnn_eval.h"
#include <atomic>
#include <cmath>

namespace {

using pcnn::lane_id;

// Build-time switches of the geometry sweeps (DESIGN.md "Evaluation"); the header's summation order
// and the tests hold at the defaults.
#ifndef POSE_EVAL_PPL
#define POSE_EVAL_PPL 4
#endif
#ifndef CONF_THREADS
#define CONF_THREADS 1024
#endif
#ifndef CONF_VEC
#define CONF_VEC 1
#endif
#ifndef CONF_BLOCKS_PER_CU
#define CONF_BLOCKS_PER_CU 1
#endif
#ifndef CONF_GRID
#define CONF_GRID 0  // > 0: the grid's cap as a number, not per CU
#endif

constexpr int kPPL = POSE_EVAL_PPL;         // query points per lane (independent min chains)
constexpr int kChunk = PCNN_WAVE * kPPL;    // query points per (row, chunk) workgroup
constexpr int kThreads = kChunk;            // one point per thread for ADD and reproj
constexpr int kWaves = kThreads / PCNN_WAVE;
constexpr int kTile = 8192;                 // float4 candidates in LDS (128 KB)
constexpr int kRowThreads = 256;            // the per-row kernels

constexpr int kConfThreads = CONF_THREADS;  // 1024: 16 waves per CU in one workgroup, one workgroup per CU
constexpr int kConfVec = CONF_VEC;          // int4 pairs per thread and iteration
constexpr int kConfLdsClasses = 128;        // 4 C^2 <= 64 KB

__device__ __forceinline__ int rows_of(const int32_t* dev, int cap) {
  if (!dev) return cap;
  const int r = *dev;
  return r < 0 ? 0 : (r < cap ? r : cap);
}

// ((r0 x + r1 y) + r2 z) + t per coordinate; rt is a row-major [R | t]
__device__ __forceinline__ void xform(const float* rt, float x, float y, float z, float& X, float& Y, float& Z) {
  X = ((rt[0] * x + rt[1] * y) + rt[2] * z) + rt[3];
  Y = ((rt[4] * x + rt[5] * y) + rt[6] * z) + rt[7];
  Z = ((rt[8] * x + rt[9] * y) + rt[10] * z) + rt[11];
}

__device__ __forceinline__ float dist2(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ void project(const float* k, float X, float Y, float Z, float& u, float& v) {
  const float w = (k[6] * X + k[7] * Y) + k[8] * Z;
  u = ((k[0] * X + k[1] * Y) + k[2] * Z) / w;
  v = ((k[3] * X + k[4] * Y) + k[5] * Z) / w;
}

// the class of a scored row and its point count, or 0
__device__ __forceinline__ int scored_points(const int32_t* cls, const int32_t* num_points, int row, int rows, int C,
                                             int P, int& c) {
  if (row >= rows) return 0;
  c = cls[row];
  if (c <= 0 || c >= C) return 0;
  const int n = num_points[c];
  return n < P ? (n > 0 ? n : 0) : P;
}

__global__ void __launch_bounds__(kThreads) k_pose_scan(const int32_t* __restrict__ cls,
                                                        const float* __restrict__ rt_est,
                                                        const float* __restrict__ rt_gt,
                                                        const int32_t* __restrict__ num_rows_dev, int N_cap,
                                                        const float* __restrict__ points,
                                                        const int32_t* __restrict__ num_points, int C, int P,
                                                        const float* __restrict__ K, int nchunks, int tile,
                                                        double* __restrict__ partials) {
  extern __shared__ __attribute__((aligned(16))) float4 s_cand[];  // [tile]
  __shared__ float s_min[kWaves][kChunk];
  __shared__ double s_wave[3][kWaves];
  const int row = (int)(blockIdx.x / (unsigned)nchunks), chunk = (int)(blockIdx.x % (unsigned)nchunks);
  int c = 0;
  const int n = scored_points(cls, num_points, row, rows_of(num_rows_dev, N_cap), C, P, c);
  if (chunk * kChunk >= n) return;  // (block-uniform) not scored, or the class has no such chunk
  const float* __restrict__ pts = points + (size_t)c * P * 3;
  float E[12], G[12], Kc[9];
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    E[i] = rt_est[(size_t)row * 12 + i];
    G[i] = rt_gt[(size_t)row * 12 + i];
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) Kc[i] = K[i];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // ADD and reproj of this thread's point
  const int q = chunk * kChunk + tid;
  float v_add = 0.f, v_rep = 0.f;
  if (q < n) {
    const float x = pts[3 * q], y = pts[3 * q + 1], z = pts[3 * q + 2];
    float ex, ey, ez, gx, gy, gz, ue, ve, ug, vg;
    xform(E, x, y, z, ex, ey, ez);
    xform(G, x, y, z, gx, gy, gz);
    v_add = sqrtf(dist2(ex, ey, ez, gx, gy, gz));
    project(Kc, ex, ey, ez, ue, ve);
    project(Kc, gx, gy, gz, ug, vg);
    const float du = ue - ug, dv = ve - vg;
    v_rep = sqrtf(du * du + dv * dv);
  }

  // ADD-S: the lane's kPPL ground-truth-transformed queries (one past n repeats the last point; its minimum is dropped)
  float qx[kPPL], qy[kPPL], qz[kPPL], m[kPPL];
#pragma unroll
  for (int k = 0; k < kPPL; ++k) {
    int i = chunk * kChunk + lane + PCNN_WAVE * k;
    i = i < n ? i : n - 1;
    xform(G, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], qx[k], qy[k], qz[k]);
    m[k] = INFINITY;
  }
  for (int t0 = 0; t0 < n; t0 += tile) {
    const int tn = n - t0 < tile ? n - t0 : tile;
    if (t0 > 0) __syncthreads();  // the previous tile has been scanned
    for (int j = tid; j < tn; j += kThreads) {
      const int i = t0 + j;
      float4 e;
      xform(E, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], e.x, e.y, e.z);
      e.w = 0.f;
      s_cand[j] = e;
    }
    __syncthreads();
    const int quarter = (tn + kWaves - 1) / kWaves;
    const int j0 = wave * quarter;
    const int j1 = j0 + quarter < tn ? j0 + quarter : tn;
#pragma unroll 4
    for (int j = j0; j < j1; ++j) {  // j is wave-uniform: a broadcast read
      const float4 e = s_cand[j];
#pragma unroll
      for (int k = 0; k < kPPL; ++k) {
        const float d = dist2(qx[k], qy[k], qz[k], e.x, e.y, e.z);
        m[k] = d < m[k] ? d : m[k];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kPPL; ++k) s_min[wave][lane + PCNN_WAVE * k] = m[k];
  __syncthreads();
  float v_adds = 0.f;
  if (q < n) {
    float mm = s_min[0][tid];
#pragma unroll
    for (int g = 1; g < kWaves; ++g) mm = s_min[g][tid] < mm ? s_min[g][tid] : mm;
    v_adds = sqrtf(mm);
  }

  // float64 sums: wave butterfly, then the four waves in order
  const double a = pcnn::wave_sum((double)v_add);
  const double s = pcnn::wave_sum((double)v_adds);
  const double r = pcnn::wave_sum((double)v_rep);
  if (lane == 0) {
    s_wave[0][wave] = a;
    s_wave[1][wave] = s;
    s_wave[2][wave] = r;
  }
  __syncthreads();
  if (tid < 3) {
    double t = s_wave[tid][0];
#pragma unroll
    for (int g = 1; g < kWaves; ++g) t = t + s_wave[tid][g];
    partials[((size_t)row * nchunks + chunk) * 3 + tid] = t;
  }
}

__global__ void __launch_bounds__(kRowThreads) k_pose_finish(const int32_t* __restrict__ cls,
                                                          const float* __restrict__ rt_est,
                                                          const float* __restrict__ rt_gt,
                                                          const int32_t* __restrict__ num_rows_dev, int N_cap,
                                                          const int32_t* __restrict__ num_points, int C, int P,
                                                          int nchunks, const double* __restrict__ partials,
                                                          float* __restrict__ errors) {
  const int row = (int)(blockIdx.x * kRowThreads + threadIdx.x);
  if (row >= N_cap) return;
  float* out = errors + (size_t)row * 5;
  int c = 0;
  const int n = scored_points(cls, num_points, row, rows_of(num_rows_dev, N_cap), C, P, c);
  if (n <= 0) {
#pragma unroll
    for (int k = 0; k < 5; ++k) out[k] = -1.f;
    return;
  }
  double sum[3] = {0.0, 0.0, 0.0};
  const int used = (n + kChunk - 1) / kChunk;
  for (int ch = 0; ch < used; ++ch)
#pragma unroll
    for (int k = 0; k < 3; ++k) sum[k] = sum[k] + partials[((size_t)row * nchunks + ch) * 3 + k];
  const float* e = rt_est + (size_t)row * 12;
  const float* g = rt_gt + (size_t)row * 12;
  double tr = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) tr = tr + (double)e[4 * i + j] * (double)g[4 * i + j];
  double cs = 0.5 * (tr - 1.0);
  cs = cs < -1.0 ? -1.0 : (cs > 1.0 ? 1.0 : cs);
  const double dx = (double)e[3] - (double)g[3], dy = (double)e[7] - (double)g[7], dz = (double)e[11] - (double)g[11];
  out[0] = (float)(sum[0] / (double)n);
  out[1] = (float)(sum[1] / (double)n);
  out[2] = (float)((acos(cs) * 180.0) / 3.14159265358979323846);
  out[3] = (float)sqrt((dx * dx + dy * dy) + dz * dz);
  out[4] = (float)(sum[2] / (double)n);
}

__device__ __forceinline__ void count64(int64_t* p) { atomicAdd((unsigned long long*)p, 1ull); }

// the first t with err < thr[t] (thr ascending), T if none
__device__ __forceinline__ int first_below(const float* __restrict__ thr, int T, float err) {
  int lo = 0, hi = T;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (err < thr[mid]) hi = mid; else lo = mid + 1;
  }
  return lo;
}

__global__ void __launch_bounds__(kRowThreads) k_pose_tally(const float* __restrict__ errors,
                                                         const int32_t* __restrict__ cls,
                                                         const int32_t* __restrict__ num_rows_dev, int N_cap,
                                                         const float* __restrict__ symmetry,
                                                         const float* __restrict__ thresholds, int C,
                                                         const float* __restrict__ curve_thr, int T,
                                                         int64_t* __restrict__ scored, int64_t* __restrict__ correct,
                                                         int64_t* __restrict__ first_add,
                                                         int64_t* __restrict__ first_adds) {
  const int row = (int)(blockIdx.x * kRowThreads + threadIdx.x);
  if (row >= rows_of(num_rows_dev, N_cap)) return;
  const int c = cls[row];
  if (c <= 0 || c >= C) return;
  const float add = errors[(size_t)row * 5], adds = errors[(size_t)row * 5 + 1];
  if (!(add >= 0.f)) return;
  count64(scored + c);
  const float metric = symmetry[c] > 0.f ? adds : add;
  if (metric < thresholds[c]) count64(correct + c);
  count64(first_add + (size_t)c * (T + 1) + first_below(curve_thr, T, add));
  count64(first_adds + (size_t)c * (T + 1) + first_below(curve_thr, T, adds));
}

// ---- confusion ----
// key: gt C + pred of a binned pixel, C C of a counted pixel with pred out of range, -1 of a pixel that does not count
__device__ __forceinline__ int conf_key(int g, int p, int C) {
  if (g < 0 || g >= C) return -1;
  return p >= 0 && p < C ? g * C + p : C * C;
}

// The lanes of the wave that hold the same key add once: the first pending lane's key is read, the lanes that
// match it are balloted, that lane adds their count times `weight`, until no lane is pending.  All 64 lanes
// must be here.
template <bool kLds>
__device__ __forceinline__ void wave_count(int key, unsigned weight, int CC, int* table, int64_t* hist,
                                           int64_t* skipped) {
  unsigned long long todo = __ballot(key >= 0);
  const int lane = lane_id();
  while (todo) {
    const int src = __builtin_ctzll(todo);
    const int k = __builtin_amdgcn_readlane(key, src);
    const unsigned long long same = __ballot(key == k);
    if (lane == src) {
      const unsigned cnt = (unsigned)__popcll(same) * weight;
      if (kLds && k != CC)
        atomicAdd(table + k, (int)cnt);
      else  // (an out-of-range pred is rare: its count goes straight to the global counter)
        atomicAdd((unsigned long long*)(k == CC ? skipped : hist + k), (unsigned long long)cnt);
    }
    todo &= ~same;
  }
}

// Four consecutive pixels of a lane.  Inside a region all four have one key: those lanes count once, by 4;
// only the waves that hold a lane with mixed keys (a region's edge) go through the four components.
template <bool kLds>
__device__ __forceinline__ void wave_count4(bool live, int4 g, int4 p, int C, int CC, int* table, int64_t* hist,
                                            int64_t* skipped) {
  const int k0 = live ? conf_key(g.x, p.x, C) : -1, k1 = live ? conf_key(g.y, p.y, C) : -1;
  const int k2 = live ? conf_key(g.z, p.z, C) : -1, k3 = live ? conf_key(g.w, p.w, C) : -1;
  const bool one = k0 == k1 && k1 == k2 && k2 == k3;
  wave_count<kLds>(one ? k0 : -1, 4u, CC, table, hist, skipped);
  if (__ballot(!one)) {  // (wave-uniform)
    wave_count<kLds>(one ? -1 : k0, 1u, CC, table, hist, skipped);
    wave_count<kLds>(one ? -1 : k1, 1u, CC, table, hist, skipped);
    wave_count<kLds>(one ? -1 : k2, 1u, CC, table, hist, skipped);
    wave_count<kLds>(one ? -1 : k3, 1u, CC, table, hist, skipped);
  }
}

// Elements [head, head + 4 n4) are read as int4 (both bases 16-byte aligned there); the others one by one.
template <bool kLds>
__global__ void __launch_bounds__(kConfThreads) k_confusion(const int32_t* __restrict__ gt,
                                                            const int32_t* __restrict__ pred, int n, int head,
                                                            int n4, int C, int64_t* __restrict__ hist,
                                                            int64_t* __restrict__ skipped) {
  extern __shared__ __attribute__((aligned(16))) int s_table[];  // [C C] (kLds)
  const int tid = (int)threadIdx.x, CC = C * C;
  if (kLds) {
    for (int i = tid; i < CC; i += kConfThreads) s_table[i] = 0;
    __syncthreads();
  }
  const int4* __restrict__ g4 = (const int4*)(gt + head);
  const int4* __restrict__ p4 = (const int4*)(pred + head);
  const int step = kConfThreads * kConfVec;
  // (the loop bounds are block-uniform: every lane of a wave reaches wave_count)
  for (long base = (long)blockIdx.x * step; base < n4; base += (long)gridDim.x * step) {
    int4 g[kConfVec], p[kConfVec];
    bool live[kConfVec];
#pragma unroll
    for (int v = 0; v < kConfVec; ++v) {
      const long i = base + tid + (long)kConfThreads * v;
      live[v] = i < n4;
      g[v] = p[v] = make_int4(0, 0, 0, 0);
      if (live[v]) {
        g[v] = g4[i];
        p[v] = p4[i];
      }
    }
#pragma unroll
    for (int v = 0; v < kConfVec; ++v) wave_count4<kLds>(live[v], g[v], p[v], C, CC, s_table, hist, skipped);
  }
  // the scalar elements: [0, head) and [head + 4 n4, n)
  const int tail0 = head + 4 * n4;
  const int ns = head + (n - tail0);
  for (long base = (long)blockIdx.x * kConfThreads; base < ns; base += (long)gridDim.x * kConfThreads) {
    const long s = base + tid;
    int key = -1;
    if (s < ns) {
      const long i = s < head ? s : s - head + tail0;
      key = conf_key(gt[i], pred[i], C);
    }
    wave_count<kLds>(key, 1u, CC, s_table, hist, skipped);
  }
  if (kLds) {
    __syncthreads();
    for (int i = tid; i < CC; i += kConfThreads) {
      const int v = s_table[i];
      if (v) atomicAdd((unsigned long long*)(hist + i), (unsigned long long)(unsigned)v);
    }
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

// k_pose_scan may take kTile float4 of dynamic LDS (above the 64 KB a kernel gets unasked): once per device
bool scan_lds_ready() {
  static std::atomic<int> done[pcnn::kMaxDevices];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= pcnn::kMaxDevices) return false;
  int have = done[dev].load(std::memory_order_acquire);
  if (have == 0) {
    have = hipFuncSetAttribute((const void*)k_pose_scan, hipFuncAttributeMaxDynamicSharedMemorySize,
                               kTile * (int)sizeof(float4)) == hipSuccess ? 1 : -1;
    if (have < 0) (void)hipGetLastError();
    done[dev].store(have, std::memory_order_release);
  }
  return have > 0;
}

inline int chunks_of(int P) { return (P + kChunk - 1) / kChunk; }

}  // namespace

extern "C" int pcnn_eval_abi_version(void) { return 1; }

extern "C" int pcnn_pose_errors_chunk(void) { return kChunk; }

extern "C" size_t pcnn_pose_errors_workspace_size(int N_cap, int P) {
  const size_t rows = N_cap > 0 ? (size_t)N_cap : 1, ch = P > 0 ? (size_t)chunks_of(P) : 1;
  return pcnn::align_up(rows * ch * 3 * sizeof(double), 256);
}

extern "C" int pcnn_pose_errors(const int32_t* cls, const float* rt_est, const float* rt_gt,
                                const int32_t* num_rows_dev, int N_cap, const float* points,
                                const int32_t* num_points, int C, int P, const float* K, float* errors,
                                void* workspace, size_t workspace_bytes, void* stream) {
  PCNN_REQUIRE(N_cap >= 0 && C >= 1 && P >= 1);
  if (N_cap == 0) return PCNN_OK;
  const int nchunks = chunks_of(P);
  PCNN_REQUIRE((long)N_cap * nchunks < (1l << 31));
  PCNN_REQUIRE(cls && rt_est && rt_gt && points && num_points && K && errors && workspace);
  PCNN_REQUIRE(workspace_bytes >= pcnn_pose_errors_workspace_size(N_cap, P) && ((uintptr_t)workspace & 7) == 0);
  const int tile = P < kTile ? P : kTile;
  const size_t lds = (size_t)tile * sizeof(float4);
  if (lds > 48 * 1024 && !scan_lds_ready()) return PCNN_EHIP;
  const hipStream_t st = (hipStream_t)stream;
  double* partials = (double*)workspace;
  hipLaunchKernelGGL(k_pose_scan, dim3((unsigned)((long)N_cap * nchunks)), dim3(kThreads), lds, st, cls, rt_est, rt_gt,
                     num_rows_dev, N_cap, points, num_points, C, P, K, nchunks, tile, partials);
  PCNN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_pose_finish, dim3((unsigned)((N_cap + kRowThreads - 1) / kRowThreads)), dim3(kRowThreads), 0, st, cls,
                     rt_est, rt_gt, num_rows_dev, N_cap, num_points, C, P, nchunks, (const double*)partials, errors);
  PCNN_CHECK_LAUNCH();
  return PCNN_OK;
}

extern "C" int pcnn_pose_tally(const float* errors, const int32_t* cls, const int32_t* num_rows_dev, int N_cap,
                               const float* symmetry, const float* thresholds, int C, const float* curve_thr, int T,
                               int64_t* scored, int64_t* correct, int64_t* first_add, int64_t* first_adds,
                               void* stream) {
  PCNN_REQUIRE(N_cap >= 0 && C >= 1 && T >= 0);
  if (N_cap == 0) return PCNN_OK;
  PCNN_REQUIRE(errors && cls && symmetry && thresholds && scored && correct && first_add && first_adds);
  PCNN_REQUIRE(T == 0 || curve_thr);
  hipLaunchKernelGGL(k_pose_tally, dim3((unsigned)((N_cap + kRowThreads - 1) / kRowThreads)), dim3(kRowThreads), 0,
                     (hipStream_t)stream, errors, cls, num_rows_dev, N_cap, symmetry, thresholds, C, curve_thr, T,
                     scored, correct, first_add, first_adds);
  PCNN_CHECK_LAUNCH();
  return PCNN_OK;
}

extern "C" int pcnn_confusion(const int32_t* gt, const int32_t* pred, long n, int C, int64_t* hist, int64_t* skipped,
                              void* stream) {
  PCNN_REQUIRE(n >= 0 && n < (1l << 31) && C >= 1 && C <= 32768);
  if (n == 0) return PCNN_OK;
  PCNN_REQUIRE(gt && pred && hist && skipped);
  PCNN_REQUIRE((((uintptr_t)gt | (uintptr_t)pred) & 3) == 0);
  // elements before gt reaches 16-byte alignment; int4 loads only if pred reaches it at the same element
  int head = (int)(((16 - ((uintptr_t)gt & 15)) & 15) >> 2);
  if (head > n) head = (int)n;
  int n4 = (int)((n - head) >> 2);
  if ((((uintptr_t)(pred + head)) & 15) != 0) {
    head = (int)n;
    n4 = 0;
  }
  const long ns = n - 4l * n4;
  // the int4 items in equal shares: as many sweeps as the capped grid needs, then as few blocks as do them
  const long cap = CONF_GRID > 0 ? (long)CONF_GRID : (long)cu_count() * CONF_BLOCKS_PER_CU;
  const long per_vec = (long)kConfThreads * kConfVec;
  const long sweeps = (n4 + cap * per_vec - 1) / (cap * per_vec);
  long blocks = sweeps > 0 ? (n4 + per_vec * sweeps - 1) / (per_vec * sweeps) : 0;
  const long blocks_s = (ns + kConfThreads - 1) / kConfThreads;
  if (blocks_s > blocks) blocks = blocks_s;
  if (blocks > cap) blocks = cap;
  const hipStream_t st = (hipStream_t)stream;
  if (C <= kConfLdsClasses) {
    hipLaunchKernelGGL(k_confusion<true>, dim3((unsigned)blocks), dim3(kConfThreads), (size_t)C * C * sizeof(int), st,
                       gt, pred, (int)n, head, n4, C, hist, skipped);
  } else {
    hipLaunchKernelGGL(k_confusion<false>, dim3((unsigned)blocks), dim3(kConfThreads), 0, st, gt, pred, (int)n, head,
                       n4, C, hist, skipped);
  }
  PCNN_CHECK_LAUNCH();
  return PCNN_OK;
}
