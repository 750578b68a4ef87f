// RGB-only pose estimation: Synthesizer::estimatePose2D
// (lib/synthesize/synthesize.cpp:1571-1766, synthesizer.pyx:74-82, called from
// lib/fcn/test.py:1364 under cfg.TEST.VERTEX_REG_3D) -- preemptive RANSAC
// over 2-D / 3-D correspondences from an object-coordinate vertex map.
//
// The reference runs it on the host: 256 hypotheses sampled by OpenMP threads
// (4 random pixels of one object, P3P, a reprojection and box-area check),
// then 8 preemptive rounds of inlier counting over a growing random subset of
// the object's pixels (std::mt19937 + negative_binomial skips), each round
// keeping the better half.  Here (what estimatePose3D, pose3d.hip, also uses
// is in pose_ransac.h):
//   k_p2d_colcount / k_p2d_scan / k_p2d_scatter  the per-class pixel lists in
//       the reference's column-major order (getLabels, :1010-1031): per-column
//       class counts, a per-class scan over columns, an ordered scatter;
//   k_p2d_objs: object_ids (classes with > 400 pixels, :1027) and the list
//       offsets, on the device: no host round trip anywhere in the call;
//   k_p2d_subset: the 8 rounds' pixel subsets of each object (countInliers2D,
//       :1183-1213 -- identical for every hypothesis of a round).  The
//       reference skips max(1, G) pixels, G ~ negative_binomial(1, p) =
//       geometric with p = maxPixels / N, drawn from a default-seeded
//       std::mt19937.  Here G is drawn from a Philox stream per (class, round)
//       by inverse CDF on exact double products (G = the largest k with
//       U < q^k, q = 1 - p): the same distribution, computed identically by
//       the oracle; one workgroup per (object, round) draws 1024 gaps at a
//       time and places them by a block scan (round 5; the earlier host
//       replay of mt19937 draws cost 5.6 of the 6.2 ms per frame and pinned
//       nothing, since the hypotheses already use Philox streams);
//   k_attempts<false> / k_pick<false>: the rejection-sampling loop (samplePoint2D
//       x 4, degeneracy tests, Grunert P3P in double, the reprojection and
//       getBB2D area checks) as independent attempts, each on its own Philox
//       stream: the first 32 attempts of every hypothesis run at once (one
//       lane each), then one lane per hypothesis keeps its first accepted
//       attempt (one wave per hypothesis: 64 further attempts at a time, the
//       first accepted in attempt order, if none of the 32 was);
//   k_p2d_collect / k_p2d_count / k_select_sum / k_p2d_finish: the 8 rounds
//       as launches: per round one workgroup per (surviving hypothesis,
//       object) counts inliers over the round's subset (double projections),
//       then one workgroup per object keeps the better half by a stable rank
//       sort; the survivor's pose is written in the reference's (3, 4, C)
//       layout.
// The reference's refinement steps are inert in this path (updateHyp3D on an
// empty 3-D inlier list, optEnergy2D divided by that list's size: NLopt keeps
// the start point) and are not run; the oracle (oracle/orc_pose2d.cpp)
// documents the same reading.
#include "pose_ransac.h"

namespace {

__global__ void __launch_bounds__(1024) k_p2d_subset(uint64_t seed, P2dWs ws) {
  __shared__ int wsum[16];
  const int c = blockIdx.x, r = blockIdx.y, t = threadIdx.x;
  const int N = ws.count[c];
  if (c == 0 || !((float)N > 400.0f)) return;  // not an object (block-uniform)
  int* S = ws.sub + (size_t)kRounds * ws.listoff[c] + (size_t)r * N;
  const int maxPixels = 1000 * (r + 1);
  const float rate = maxPixels / (float)N;  // :1191
  if (!(rate < 1)) {  // every pixel (:1212-1213)
    for (int i = t; i < N; i += blockDim.x) S[i] = i;
    if (t == 0) ws.subcnt[c * kRounds + r] = N;
    return;
  }
  subset_nohole(seed, c, r, N, 1.0 - (double)rate, S, ws.subcnt + c * kRounds + r, wsum);
}

// grid (hypothesis slot, object, kCntZ): workgroup z counts the subset chunks
// z, z + kCntZ, ... of kCntChunk entries (round 5: one workgroup per
// hypothesis walked the whole subset, 26 us per round) and writes its partial
// count; k_select_sum adds the partials (integers)
__global__ void __launch_bounds__(256) k_p2d_count(const float* __restrict__ vm, const float* __restrict__ ext, int W,
                                                   int C, Cam k, P2dWs ws, int r) {
  __shared__ int part[4];
  const int j = blockIdx.x, oi = blockIdx.y, z = blockIdx.z;
  if (oi >= *ws.nobj || j >= ws.rm[oi]) return;  // block-uniform
  const int obj = ws.objs[oi];
  const int* L = ws.lists + ws.listoff[obj];
  const int h = ws.rl[oi * kMaxHypBlock + j];
  const int* S = ws.sub + (size_t)kRounds * ws.listoff[obj] + (size_t)r * ws.count[obj];
  const int ns = ws.subcnt[obj * kRounds + r];
  const double* hr = ws.hyp + (size_t)h * 16;
  Pose P;
  for (int i = 0; i < 9; i++) P.R[i] = hr[1 + i];
  for (int i = 0; i < 3; i++) P.t[i] = hr[10 + i];
  int cnt = 0;
  for (int c0 = z * kCntChunk; c0 < ns; c0 += (int)gridDim.z * kCntChunk) {  // countInliers2D (:1171-1214)
    for (int i = c0 + threadIdx.x; i < c0 + kCntChunk && i < ns; i += 256) {
      const int idx = L[S[i]];
      const double u0 = idx % W, v0 = idx / W;
      const F3 o = mode3d(vm, ext, C, obj, idx);
      double u, v;
      project(P, D3{o.x, o.y, o.z}, k, u, v);
      if (sqrt((u0 - u) * (u0 - u) + (v0 - v) * (v0 - v)) < 10.0f) cnt++;
    }
  }
  cnt = pcnn::wave_sum(cnt);
  if (pcnn::lane_id() == 0) part[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) ws.pcnt[((size_t)oi * kMaxHypBlock + j) * kCntZ + z] = part[0] + part[1] + part[2] + part[3];
}

__global__ void __launch_bounds__(64) k_p2d_finish(int C, int n_hyp, P2dWs ws, int32_t* __restrict__ final_out,
                                                   float* __restrict__ poses_out) {
  const int oi = blockIdx.x, lane = pcnn::lane_id();  // one wave per object
  if (oi >= *ws.nobj || ws.rm[oi] == 0) return;
  const int obj = ws.objs[oi];
  const int h = ws.rl[oi * kMaxHypBlock];
  int nh = 0;
  for (int q = lane; q < n_hyp; q += 64) nh += ws.hyp[(size_t)q * 16] == (double)obj;
  nh = pcnn::wave_sum(nh);
  if (lane != 0) return;
  final_out[obj * 3] = h;
  final_out[obj * 3 + 1] = ws.rc[oi * kMaxHypBlock];
  final_out[obj * 3 + 2] = nh;
  const double* hr = ws.hyp + (size_t)h * 16;
  for (int y = 0; y < 3; y++)
    for (int x = 0; x < 4; x++) poses_out[obj + C * (y * 4 + x)] = x < 3 ? (float)hr[1 + y * 3 + x] : (float)hr[10 + y];
}

}  // namespace

extern "C" size_t pcnn_pose2d_workspace_size(int H, int W, int C, int n_hyp) {
  if (H <= 0 || W <= 0 || C <= 0 || n_hyp <= 0) return 256;
  pcnn::Carve cv(nullptr);
  carve_base(cv, H, W, C, n_hyp);
  return cv.off;
}

extern "C" int pcnn_pose2d(const int32_t* label, const float* vertmap, const float* extents, int H, int W, int C,
                           float fx, float fy, float px, float py, uint64_t seed, int n_hyp, int max_iter,
                           float* poses_out, float* hyps_out, int32_t* hyp_px, int32_t* inl_out, int32_t* final_out,
                           void* workspace, size_t workspace_bytes, void* stream) {
  PCNN_REQUIRE(label && vertmap && extents && poses_out && hyps_out && hyp_px && inl_out && final_out);
  // n_hyp <= 256: the reference's ransacIterations (:1601), so that 8 halving
  // rounds leave one hypothesis per object, as getWorkingQueue (:1150-1160)
  // stops at
  PCNN_REQUIRE(H > 0 && W > 0 && C > 1 && C <= 64 && n_hyp > 0 && n_hyp <= kMaxHyp && max_iter > 0);
  PCNN_REQUIRE((long)H * W < (1l << 28));
  pcnn::Carve cv(workspace);
  const P2dWs ws = carve_base(cv, H, W, C, n_hyp);
  if (!workspace || workspace_bytes < cv.off) return PCNN_ECAPACITY;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(poses_out, 0, (size_t)12 * C * sizeof(float), st) != hipSuccess) return PCNN_EHIP;
  if (hipMemsetAsync(inl_out, 0xFF, (size_t)n_hyp * kRounds * sizeof(int32_t), st) != hipSuccess) return PCNN_EHIP;
  if (hipMemsetAsync(final_out, 0xFF, (size_t)C * 3 * sizeof(int32_t), st) != hipSuccess) return PCNN_EHIP;
  if (hipMemsetAsync(ws.rm, 0, (size_t)C * sizeof(int32_t), st) != hipSuccess) return PCNN_EHIP;
  const Cam k{fx, fy, px, py};
  // every count, object list and subset stays on the device: the call is
  // asynchronous on `stream` (round 5; it used to read the class counts
  // back and draw the subsets on host threads)
  hipLaunchKernelGGL(k_p2d_colcount, dim3((W + 3) / 4), dim3(256), 0, st, label, H, W, C, ws.colcnt);
  hipLaunchKernelGGL(k_p2d_scan, dim3(C), dim3(1024), 0, st, ws.colcnt, W, ws.coloff, ws.count);
  hipLaunchKernelGGL(k_p2d_objs, dim3(1), dim3(64), 0, st, C, ws);
  hipLaunchKernelGGL(k_p2d_scatter, dim3((W + 3) / 4), dim3(256), 0, st, label, H, W, C, ws);
  hipLaunchKernelGGL(k_p2d_subset, dim3(C, kRounds), dim3(1024), 0, st, seed, ws);
  const int T = max_iter < kAttempts ? max_iter : kAttempts;
  const AttArgs A{vertmap, extents, nullptr, H, W, C, k, seed};
  hipLaunchKernelGGL(k_attempts<false>, dim3((n_hyp * T + 63) / 64), dim3(64), 0, st, A, n_hyp, T, ws);
  hipLaunchKernelGGL(k_pick<false>, dim3(n_hyp), dim3(64), 0, st, A, n_hyp, max_iter, T, ws, hyps_out, hyp_px);
  hipLaunchKernelGGL(k_p2d_collect, dim3(C), dim3(64), 0, st, n_hyp, ws);
  for (int r = 0; r < kRounds; r++) {
    const int gx = std::max(1, n_hyp >> r);  // survivors halve each round (one stays one)
    hipLaunchKernelGGL(k_p2d_count, dim3(gx, C, count_z(r)), dim3(256), 0, st, vertmap, extents, W, C, k, ws, r);
    hipLaunchKernelGGL(k_select_sum, dim3(C), dim3(1024), 0, st, ws, r, count_z(r), inl_out);
  }
  hipLaunchKernelGGL(k_p2d_finish, dim3(C), dim3(64), 0, st, C, n_hyp, ws, final_out, poses_out);
  PCNN_CHECK_LAUNCH();
  return PCNN_OK;
}
