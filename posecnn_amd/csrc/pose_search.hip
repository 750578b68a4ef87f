// Nelder-Mead on optEnergy, on the device (round 5).  solveICP's refinePose
// (synthesize.cpp:2221-2250 -> poseWithOpt :2529-2573, NLopt LN_NELDERMEAD,
// 7 parameters, bounds +-0.1 / +-0.01 / +-0.1, at most `iterations`
// evaluations of optEnergy :2476-2526) used to run as Python generators with
// one energy launch and one host read per simplex step.  Here:
//   k_rec_count / k_rec_scatter  the object's pixels whose live vertex lies in
//       the depth range (the pose-independent half of optEnergy's test), in
//       raster order, as (rendered vertex, live vertex) records per problem;
//   energy_rec  optEnergy of one pose over a problem's records by one
//       1024-thread workgroup, a fixed summation order (thread-strided float
//       sums, then a fixed wave / workgroup tree): k_energy_rec evaluates K
//       poses, and k_nm runs whole searches, one workgroup per problem, with
//       no host read until the end.  The search is the bounded Nelder-Mead of
//       posecnn_amd/synthesize/icp.py nelder_mead_steps, operation for
//       operation in double (NLopt is absent: its trajectory is unpinned), so
//       the device search and the host search over k_energy_rec give the
//       same bits.  Its body is pcnn_nm::search (nelder_mead.h); the kernels
//       here differ only in the evaluator they hand it.
#include "nelder_mead.h"
#include "refine_common.h"

namespace pcnn_refine {

constexpr int kNmThreads = 1024;
constexpr int kNmDim = 7;

__global__ void __launch_bounds__(kBlk) k_rec_count(const float* __restrict__ live_all, int n_live,
                                                    const int32_t* __restrict__ label, int HW, float znear, float zfar,
                                                    const int32_t* __restrict__ prob_obj,
                                                    const int32_t* __restrict__ prob_live, int nseg,
                                                    int32_t* __restrict__ segcnt) {
  __shared__ int sh[kBlk / 64];
  const int p = blockIdx.y, seg = blockIdx.x;
  const int obj = prob_obj[p], li = prob_live[p];
  const bool ok_live = li >= 0 && li < n_live;
  const float* __restrict__ live = live_all + (ok_live ? (size_t)li * HW * 3 : 0);
  int c = 0;
  for (int i = threadIdx.x; i < kSeg; i += kBlk) {
    const int j = seg * kSeg + i;
    if (ok_live && j < HW && label[j] == obj) {
      const float lz = live[(size_t)j * 3 + 2];
      c += (lz > znear && lz < zfar) ? 1 : 0;  // :2514
    }
  }
  c = block_sum_int<kBlk>(c, sh);
  if (threadIdx.x == 0) segcnt[(size_t)p * nseg + seg] = c;
}

__global__ void __launch_bounds__(kBlk) k_rec_scatter(const float* __restrict__ live_all, int n_live,
                                                      const int32_t* __restrict__ label,
                                                      const float* __restrict__ pv_all, int HW, float znear,
                                                      float zfar, const int32_t* __restrict__ prob_obj,
                                                      const int32_t* __restrict__ prob_live, int nseg,
                                                      const int32_t* __restrict__ segcnt, float* __restrict__ rec,
                                                      int32_t* __restrict__ count) {
  __shared__ int sh[kBlk / 64];
  __shared__ int wc[kBlk / 64];
  const int p = blockIdx.y, seg = blockIdx.x;
  const int obj = prob_obj[p], li = prob_live[p];
  const bool ok_live = li >= 0 && li < n_live;
  const float* __restrict__ live = live_all + (ok_live ? (size_t)li * HW * 3 : 0);
  const float* __restrict__ pv = pv_all + (size_t)p * HW * 4;
  const int32_t* sc = segcnt + (size_t)p * nseg;
  int o = 0, tot = 0;
  for (int s = threadIdx.x; s < nseg; s += kBlk) {
    o += s < seg ? sc[s] : 0;
    tot += sc[s];
  }
  int off = block_sum_int<kBlk>(o, sh);
  const int total = block_sum_int<kBlk>(tot, sh);
  if (seg == 0 && threadIdx.x == 0) count[p] = total;
  float* out = rec + (size_t)p * HW * 6;
  const int wave = threadIdx.x >> 6;
  for (int i0 = 0; i0 < kSeg; i0 += kBlk) {
    const int j = seg * kSeg + i0 + threadIdx.x;
    bool ok = false;
    if (ok_live && j < HW && label[j] == obj) {
      const float lz = live[(size_t)j * 3 + 2];
      ok = lz > znear && lz < zfar;
    }
    const uint64_t m = __ballot(ok);
    if (pcnn::lane_id() == 0) wc[wave] = __popcll(m);
    __syncthreads();
    int base = off;
    for (int w = 0; w < wave; w++) base += wc[w];
    if (ok) {
      float* r = out + (size_t)(base + __popcll(m & pcnn::lanemask_lt())) * 6;
      r[0] = pv[(size_t)j * 4 + 0];
      r[1] = pv[(size_t)j * 4 + 1];
      r[2] = pv[(size_t)j * 4 + 2];
      r[3] = live[(size_t)j * 3 + 0];
      r[4] = live[(size_t)j * 3 + 1];
      r[5] = live[(size_t)j * 3 + 2];
    }
    for (int w = 0; w < kBlk / 64; w++) off += wc[w];
    __syncthreads();
  }
}

// the record sums of virtual thread vt (of kNmThreads): records vt, vt +
// kNmThreads, ... in order, four records' loads issued per pass (the loop
// was bound by one record's load latency at a time; the order is unchanged)
__device__ __forceinline__ void rec_sums(const float* __restrict__ r, int n, const Quat& q, const float (&P)[7],
                                         float znear, float zfar, int vt, float& s, float& c) {
  s = 0.f;
  c = 0.f;
  auto term = [&](const float* x) {
    float p0, p1, p2;
    rotate(q, x[0], x[1], x[2], p0, p1, p2);
    p0 = p0 + P[4];
    p1 = p1 + P[5];
    p2 = p2 + P[6];
    if (!isnan(p0) && !isnan(p1) && !isnan(p2) && p2 > znear && p2 < zfar) {  // :2514 (the live half: records)
      const float dx = p0 - x[3], dy = p1 - x[4], dz = p2 - x[5];
      s += sqrtf(dx * dx + dy * dy + dz * dz);
      c += 1.f;
    }
  };
  int i = vt;
  for (; i + 3 * kNmThreads < n; i += 4 * kNmThreads) {
    float v[4][6];
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
      for (int e = 0; e < 6; e++) v[u][e] = r[(size_t)(i + u * kNmThreads) * 6 + e];
#pragma unroll
    for (int u = 0; u < 4; u++) term(v[u]);
  }
  for (; i < n; i += kNmThreads) term(r + (size_t)i * 6);
}

__device__ __forceinline__ Quat rec_quat(const float (&P)[7]) {
  const float qn = sqrtf(P[0] * P[0] + P[1] * P[1] + P[2] * P[2] + P[3] * P[3]);
  return {P[0] / qn, P[1] / qn, P[2] / qn, P[3] / qn};
}

// optEnergy (:2476-2526) of pose P (float, quaternion normalised as
// k_pose_energy does) over n records; every thread of a 1024-thread
// workgroup calls it and gets the value
__device__ float energy_rec(const float* __restrict__ r, int n, const float (&P)[7], float znear, float zfar,
                            float* sh) {
  const Quat q = rec_quat(P);
  float s, c;
  rec_sums(r, n, q, P, znear, zfar, threadIdx.x, s, c);
  s = pcnn::wave_sum(s);
  c = pcnn::wave_sum(c);
  const int wave = threadIdx.x >> 6;
  if (pcnn::lane_id() == 0) {
    sh[2 * wave] = s;
    sh[2 * wave + 1] = c;
  }
  __syncthreads();
  float S = 0.f, Cn = 0.f;
  for (int w = 0; w < kNmThreads / 64; w++) {
    S += sh[2 * w];
    Cn += sh[2 * w + 1];
  }
  __syncthreads();
  return Cn > 0.f ? S / Cn : 0.f;  // distance /= c (:2520-2521)
}

__global__ void __launch_bounds__(kNmThreads) k_energy_rec(const float* __restrict__ rec,
                                                           const int32_t* __restrict__ count, int stride,
                                                           const float* __restrict__ poses,
                                                           const int32_t* __restrict__ pose_prob, float znear,
                                                           float zfar, float* __restrict__ energy) {
  __shared__ float sh[2 * kNmThreads / 64];
  const int k = blockIdx.x;
  const int p = pose_prob[k];
  float P[7];
  for (int e = 0; e < 7; e++) P[e] = poses[(size_t)k * 7 + e];
  const float v = energy_rec(rec + (size_t)p * stride * 6, count[p], P, znear, zfar, sh);
  if (threadIdx.x == 0) energy[k] = v;
}

// The evaluators handed to pcnn_nm::search.  One workgroup per problem:
// energy_rec of one point at a time.
struct RecEval {
  static constexpr int kBatch = 1;
  static constexpr bool kBarrierAfterReflection = true;
  const float* r;
  int nr;
  float znear, zfar;
  float* sh;  // LDS, 2 * kNmThreads / 64 floats
  __device__ __forceinline__ double value(const double (*xs)[kNmDim], int k) {
    __syncthreads();  // xs[k] (thread 0) is visible
    float P[7];
    for (int e = 0; e < kNmDim; e++) P[e] = (float)xs[k][e];  // the host path evaluates float32 points
    return (double)energy_rec(r, nr, P, znear, zfar, sh);
  }
  __device__ __forceinline__ bool failed() const { return false; }
};

// Arrive-and-wait of the workgroups of one problem on its counter (thread 0
// of each): release the workgroup's partial sums, wait until every workgroup
// of the problem has arrived for this round.  Bounded: a wait that never
// completes (not expected: the launch is cooperative) gives up and raises the
// problem's failure flag; a workgroup waiting while the flag is up gives up at
// once.  A workgroup whose wait fails leaves the search (failed(), read after
// the round's barrier), so every workgroup of the problem stops at its next
// barrier instead of running on with sums that were never written, and the
// problem reports nev = -1.
__device__ __forceinline__ bool coop_arrive_wait(uint32_t* bar, uint32_t target, uint32_t* fail) {
  __hip_atomic_fetch_add(bar, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  uint32_t cur = __hip_atomic_load(bar, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
  for (int it = 0; cur < target && it < (1 << 24); it++) {
    if (__hip_atomic_load(fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return false;
    __builtin_amdgcn_s_sleep(2);
    cur = __hip_atomic_load(bar, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (cur >= target) return true;
  __hip_atomic_fetch_or(fail, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return false;
}

template <int S>
struct CoopLds {
  double fs[S];  // the values of a speculative round's points
  int failed;    // a cross-workgroup wait of this workgroup gave up
};

// S groups of G workgroups per problem: the 1024 "virtual threads" of
// optEnergy's reduction split over the G workgroups (of kNmThreads / G) of a
// group, each group evaluating one point of a round, every workgroup running
// the same search.  A point's record sums are those of energy_rec -- virtual
// thread v sums records v, v + 1024, ... in order, each 64 of them fold by the
// same butterfly, the 16 wave sums add in order -- so the value is identical
// for every G and S; the wave sums cross workgroups through `part`
// (double-buffered by round parity) and one arrive-and-wait per round on the
// problem's counter, whose target is (round + 1) G S.
//   S = 1: a round per evaluation, on demand.
//   S > 1: speculative rounds.  A round evaluates every point the next step
//       may need: reflection, expansion and both contractions of an iteration
//       (the search then takes them in its own order and counts only those it
//       uses), up to S points of the initial simplex or of a shrink.
//       optEnergy is a pure function of the point, so the simplex, the
//       evaluation count and the result are the sequential search's bit for
//       bit; an iteration costs one round (plus the shrink's) instead of one
//       to three.
template <int G, int S>
struct CoopEval {
  static constexpr int kBatch = S;
  static constexpr bool kBarrierAfterReflection = true;
  static constexpr int kT = kNmThreads / G;
  static constexpr int kW = 2 * kNmThreads / 64;  // (sum, count) per virtual wave
  const float* r;
  int nr;
  float znear, zfar;
  float* part;     // the problem's 2 x S x kW partial sums
  uint32_t* bar;   // the problem's arrival counter
  uint32_t* fail;  // the problem's failure flag
  int sp, g;       // this workgroup's group and its place in it
  CoopLds<S>* lds;
  int rnd;  // rounds so far (the same in every thread of every workgroup of the problem)

  // one round, every thread: the wave sums of xs[0 .. cnt) cross the
  // problem's workgroups; returns the round's buffer, readable by every thread
  __device__ __forceinline__ const float* round(const double (*xs)[kNmDim], int cnt) {
    const int t = threadIdx.x;
    __syncthreads();
    float* slot = part + (size_t)(rnd & 1) * S * kW;
    if (sp < cnt) {
      float P[7];
      for (int e = 0; e < kNmDim; e++) P[e] = (float)xs[sp][e];  // the host path evaluates float32 points
      const int vt = g * kT + t;
      const Quat q = rec_quat(P);
      float a, c;
      rec_sums(r, nr, q, P, znear, zfar, vt, a, c);
      a = pcnn::wave_sum(a);
      c = pcnn::wave_sum(c);
      if (pcnn::lane_id() == 0) {
        slot[sp * kW + 2 * (vt >> 6)] = a;
        slot[sp * kW + 2 * (vt >> 6) + 1] = c;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
    if (t == 0 && !coop_arrive_wait(bar, (uint32_t)(rnd + 1) * G * S, fail)) lds->failed = 1;
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    rnd++;
    return slot;
  }
  // the value of the round's point k: the 16 wave sums in order, as energy_rec
  static __device__ __forceinline__ double point_value(const float* slot, int k) {
    float S_ = 0.f, C_ = 0.f;
    for (int w = 0; w < kNmThreads / 64; w++) {
      S_ += slot[k * kW + 2 * w];
      C_ += slot[k * kW + 2 * w + 1];
    }
    return (double)(C_ > 0.f ? S_ / C_ : 0.f);  // distance /= c (:2520-2521)
  }
  __device__ __forceinline__ void prefetch(const double (*xs)[kNmDim], int cnt) {
    const float* slot = round(xs, cnt);
    if (threadIdx.x < cnt) lds->fs[threadIdx.x] = point_value(slot, threadIdx.x);
    __syncthreads();
  }
  __device__ __forceinline__ double value(const double (*xs)[kNmDim], int k) {
    if constexpr (S == 1)
      return point_value(round(xs + k, 1), 0);  // every thread sums for itself
    else
      return lds->fs[k];
  }
  __device__ __forceinline__ bool failed() const { return lds->failed != 0; }
};

// nev reported by workgroup 0 of problem p: -1 when a cross-workgroup wait of
// the problem gave up (its own or another workgroup's: results invalid)
__device__ __forceinline__ int nm_report(int nev, bool failed, const uint32_t* fail, int p) {
  if (failed) return -1;
  if (fail && __hip_atomic_load(fail + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return -1;
  return nev;
}

struct NmIo {  // the search kernels' per-problem inputs and outputs
  const double* x0;
  const double* lb;
  const double* ub;
  int max_eval;
  double* x;
  double* f;
  int32_t* nev;
  const uint32_t* fail;
};

// problem p's search with evaluator ev: bounds and start in, the best point,
// its value and the evaluation count out (written by the one workgroup with
// `writer`)
template <class Ev>
__device__ __forceinline__ void nm_problem(pcnn_nm::Simplex<kNmDim>& sx, Ev& ev, int p, bool writer,
                                           const NmIo& io) {
  constexpr int n = kNmDim;
  if (threadIdx.x == 0)
    for (int e = 0; e < n; e++) {
      sx.lb[e] = io.lb[(size_t)p * n + e];
      sx.ub[e] = io.ub[(size_t)p * n + e];
      sx.pts[0][e] = io.x0[(size_t)p * n + e];
    }
  const int nev = pcnn_nm::search(sx, ev, io.max_eval);
  if (threadIdx.x == 0 && writer) {
    const int b = pcnn_nm::best(sx);
    for (int e = 0; e < n; e++) io.x[(size_t)p * n + e] = sx.pts[b][e];
    io.f[p] = sx.vals[b];
    io.nev[p] = nm_report(nev, ev.failed(), io.fail, p);
  }
}

// G workgroups per problem, one evaluation at a time (G = 1: one 1024-thread
// workgroup and energy_rec; G > 1: CoopEval<G, 1>)
template <int G>
__global__ void __launch_bounds__(kNmThreads / G) k_nm(const float* __restrict__ rec,
                                                       const int32_t* __restrict__ count, int stride,
                                                       const double* __restrict__ x0_all,
                                                       const double* __restrict__ lb_all,
                                                       const double* __restrict__ ub_all, int max_eval, float znear,
                                                       float zfar, double* __restrict__ x_out,
                                                       double* __restrict__ f_out, int32_t* __restrict__ nev_out,
                                                       float* __restrict__ part, uint32_t* __restrict__ bar,
                                                       uint32_t* __restrict__ fail) {
  __shared__ pcnn_nm::Simplex<kNmDim> sx;
  const int p = blockIdx.x / G, g = blockIdx.x % G;
  const NmIo io{x0_all, lb_all, ub_all, max_eval, x_out, f_out, nev_out, fail};
  if constexpr (G == 1) {
    __shared__ float sh[2 * kNmThreads / 64];
    RecEval ev{rec + (size_t)p * stride * 6, count[p], znear, zfar, sh};
    nm_problem(sx, ev, p, true, io);
  } else {
    __shared__ CoopLds<1> lds;
    if (threadIdx.x == 0) lds.failed = 0;
    using Ev = CoopEval<G, 1>;
    Ev ev{rec + (size_t)p * stride * 6, count[p], znear, zfar, part + (size_t)p * 2 * Ev::kW, bar + p, fail + p,
          0, g, &lds, 0};
    nm_problem(sx, ev, p, g == 0, io);
  }
}

// The same search in speculative rounds: kNmSpecW groups of G workgroups per
// problem (CoopEval<G, S>)
constexpr int kNmSpecW = 4;
template <int G, int S>
__global__ void __launch_bounds__(kNmThreads / G) k_nm_spec(const float* __restrict__ rec,
                                                            const int32_t* __restrict__ count, int stride,
                                                            const double* __restrict__ x0_all,
                                                            const double* __restrict__ lb_all,
                                                            const double* __restrict__ ub_all, int max_eval,
                                                            float znear, float zfar, double* __restrict__ x_out,
                                                            double* __restrict__ f_out, int32_t* __restrict__ nev_out,
                                                            float* __restrict__ part, uint32_t* __restrict__ bar,
                                                            uint32_t* __restrict__ fail) {
  __shared__ pcnn_nm::Simplex<kNmDim> sx;
  __shared__ CoopLds<S> lds;
  const int p = blockIdx.x / (G * S), sp = (blockIdx.x / G) % S, g = blockIdx.x % G;
  if (threadIdx.x == 0) lds.failed = 0;
  using Ev = CoopEval<G, S>;
  Ev ev{rec + (size_t)p * stride * 6, count[p], znear, zfar, part + (size_t)p * 2 * S * Ev::kW, bar + p, fail + p,
        sp, g, &lds, 0};
  nm_problem(sx, ev, p, g == 0 && sp == 0, NmIo{x0_all, lb_all, ub_all, max_eval, x_out, f_out, nev_out, fail});
}

}  // namespace pcnn_refine

using namespace pcnn_refine;

extern "C" size_t pcnn_energy_records_workspace_size(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return 256;
  const int nseg = (H * W + kSeg - 1) / kSeg;
  return (size_t)N * nseg * sizeof(int32_t) + 256;
}

extern "C" int pcnn_energy_records(const float* live, int n_live, const int32_t* label, const float* pred_vertices,
                                   int H, int W, float znear, float zfar, int N, const int32_t* prob_obj,
                                   const int32_t* prob_live, float* records, int32_t* counts, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  PCNN_REQUIRE(live && label && pred_vertices && prob_obj && prob_live && records && counts && workspace);
  PCNN_REQUIRE(N > 0 && H > 0 && W > 0 && n_live > 0 && (long)H * W < (1l << 30));
  const int HW = H * W, nseg = (HW + kSeg - 1) / kSeg;
  if (workspace_bytes < (size_t)N * nseg * sizeof(int32_t)) return PCNN_ECAPACITY;
  int32_t* segcnt = (int32_t*)workspace;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_rec_count, dim3(nseg, N), dim3(kBlk), 0, st, live, n_live, label, HW, znear, zfar, prob_obj,
                     prob_live, nseg, segcnt);
  hipLaunchKernelGGL(k_rec_scatter, dim3(nseg, N), dim3(kBlk), 0, st, live, n_live, label, pred_vertices, HW, znear,
                     zfar, prob_obj, prob_live, nseg, segcnt, records, counts);
  PCNN_CHECK_LAUNCH();
  return PCNN_OK;
}

extern "C" int pcnn_energy_rec(const float* records, const int32_t* counts, int stride, const float* poses,
                               const int32_t* pose_prob, int K, float znear, float zfar, float* energy, void* stream) {
  PCNN_REQUIRE(records && counts && poses && pose_prob && energy && K > 0 && stride > 0);
  hipLaunchKernelGGL(k_energy_rec, dim3(K), dim3(kNmThreads), 0, (hipStream_t)stream, records, counts, stride, poses,
                     pose_prob, znear, zfar, energy);
  PCNN_CHECK_LAUNCH();
  return PCNN_OK;
}

extern "C" int pcnn_nelder_mead_energy(const float* records, const int32_t* counts, int stride, int N,
                                       const double* x0, const double* lb, const double* ub, int max_eval,
                                       float znear, float zfar, double* x_out, double* f_out, int32_t* nev_out,
                                       void* stream) {
  PCNN_REQUIRE(records && counts && x0 && lb && ub && x_out && f_out && nev_out && N > 0 && stride > 0);
  // at least the initial simplex: NLopt's maxeval also counts it, and a
  // budget below n + 1 is refused rather than overrun
  PCNN_REQUIRE(max_eval >= pcnn_refine::kNmDim + 1 && max_eval <= (1 << 20));
  hipLaunchKernelGGL(k_nm<1>, dim3(N), dim3(kNmThreads), 0, (hipStream_t)stream, records, counts, stride, x0, lb,
                     ub, max_eval, znear, zfar, x_out, f_out, nev_out, nullptr, nullptr, nullptr);
  PCNN_CHECK_LAUNCH();
  return PCNN_OK;
}

// The same searches with kNmCoop workgroups per problem (the evaluation's
// records spread over kNmCoop CUs), launched cooperatively so that the
// workgroups of a problem are resident together; bit-identical results.
constexpr int kNmCoop = 8;
constexpr int kNmSpecMaxN = 32;  // N x 8 x 4 workgroups of 128 threads: 1024 at N = 32

static inline size_t nm_part_bytes(int N) {  // per problem: 2 parities x kNmSpecW points x the wave sums
  return pcnn::align_up((size_t)N * 2 * kNmSpecW * (2 * kNmThreads / 64) * sizeof(float), 256);
}
extern "C" size_t pcnn_nelder_mead_energy_workspace_size(int N) {
  if (N <= 0) return 256;
  return nm_part_bytes(N) + 2 * (size_t)N * sizeof(uint32_t) + 256;  // + the arrival counters and failure flags
}

extern "C" int pcnn_nelder_mead_energy_coop_path(const float* records, const int32_t* counts, int stride, int N,
                                                 const double* x0, const double* lb, const double* ub, int max_eval,
                                                 float znear, float zfar, double* x_out, double* f_out,
                                                 int32_t* nev_out, void* workspace, size_t workspace_bytes,
                                                 int force_path, int32_t* path_out, void* stream) {
  PCNN_REQUIRE(records && counts && x0 && lb && ub && x_out && f_out && nev_out && N > 0 && stride > 0);
  PCNN_REQUIRE(max_eval >= pcnn_refine::kNmDim + 1 && max_eval <= (1 << 20) && N <= 128);
  PCNN_REQUIRE(force_path >= 0 && force_path <= 3);
  if (!workspace || workspace_bytes < pcnn_nelder_mead_energy_workspace_size(N)) return PCNN_ECAPACITY;
  float* part = (float*)workspace;
  uint32_t* bar = (uint32_t*)((char*)workspace + nm_part_bytes(N));
  uint32_t* fail = bar + N;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(bar, 0, 2 * (size_t)N * sizeof(uint32_t), st) != hipSuccess) return PCNN_EHIP;
  void* args[] = {(void*)&records, (void*)&counts, (void*)&stride, (void*)&x0, (void*)&lb, (void*)&ub,
                  (void*)&max_eval, (void*)&znear, (void*)&zfar, (void*)&x_out, (void*)&f_out, (void*)&nev_out,
                  (void*)&part, (void*)&bar, (void*)&fail};
  // speculative rounds while the N x kNmCoop x kNmSpecW workgroups fit the
  // chip at once (path 1); then one evaluation per round (2); then one
  // workgroup per problem (3).  force_path pins one (0: the first that
  // launches); path_out (host int, may be null) reports the one that ran.
  int path = 0;
  if ((force_path == 0 || force_path == 1) && N <= kNmSpecMaxN &&
      hipLaunchCooperativeKernel((const void*)k_nm_spec<kNmCoop, kNmSpecW>, dim3(N * kNmCoop * kNmSpecW),
                                 dim3(kNmThreads / kNmCoop), args, 0, st) == hipSuccess)
    path = 1;
  if (!path) (void)hipGetLastError();
  if (!path && (force_path == 0 || force_path == 2) &&
      hipLaunchCooperativeKernel((const void*)k_nm<kNmCoop>, dim3(N * kNmCoop), dim3(kNmThreads / kNmCoop), args, 0,
                                 st) == hipSuccess)
    path = 2;
  if (!path) (void)hipGetLastError();
  if (!path && (force_path == 0 || force_path == 3)) {  // the one-workgroup search (same bits)
    hipLaunchKernelGGL(k_nm<1>, dim3(N), dim3(kNmThreads), 0, st, records, counts, stride, x0, lb, ub, max_eval,
                       znear, zfar, x_out, f_out, nev_out, nullptr, nullptr, nullptr);
    path = 3;
  }
  if (path_out) *path_out = path;
  if (!path) return PCNN_EHIP;  // the forced path could not launch
  PCNN_CHECK_LAUNCH();
  return PCNN_OK;
}

extern "C" int pcnn_nelder_mead_energy_coop(const float* records, const int32_t* counts, int stride, int N,
                                            const double* x0, const double* lb, const double* ub, int max_eval,
                                            float znear, float zfar, double* x_out, double* f_out, int32_t* nev_out,
                                            void* workspace, size_t workspace_bytes, void* stream) {
  return pcnn_nelder_mead_energy_coop_path(records, counts, stride, N, x0, lb, ub, max_eval, znear, zfar, x_out, f_out,
                                           nev_out, workspace, workspace_bytes, 0, nullptr, stream);
}
