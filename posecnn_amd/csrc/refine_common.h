// What the pose-refinement sources share (icp.hip: live vertices, df::icp,
// the full-frame optEnergy and the SegICP score; pose_search.hip: the record
// energy and the Nelder-Mead searches over it).
#pragma once
#include "pcnn_common.h"

namespace pcnn_refine {

constexpr int kSeg = 2048;       // pixels per compaction / reduction block
constexpr int kBlk = 256;        // threads of the per-pixel kernels

struct Quat { float w, x, y, z; };

// Eigen Quaternion::_transformVector (the point action of Sophus SO3)
__device__ __forceinline__ void rotate(const Quat& q, float v0, float v1, float v2, float& o0, float& o1,
                                       float& o2) {
  float uv0 = q.y * v2 - q.z * v1;
  float uv1 = q.z * v0 - q.x * v2;
  float uv2 = q.x * v1 - q.y * v0;
  uv0 = uv0 + uv0;
  uv1 = uv1 + uv1;
  uv2 = uv2 + uv2;
  const float c0 = q.y * uv2 - q.z * uv1;
  const float c1 = q.z * uv0 - q.x * uv2;
  const float c2 = q.x * uv1 - q.y * uv0;
  o0 = v0 + q.w * uv0 + c0;
  o1 = v1 + q.w * uv1 + c1;
  o2 = v2 + q.w * uv2 + c2;
}

__device__ __forceinline__ bool in_range(float z, float znear, float zfar) { return !(z < znear || z > zfar); }

// Block-wide sum of an int (all threads call; result in every thread).
template <int T>
__device__ __forceinline__ int block_sum_int(int v, int* sh) {
  v = pcnn::wave_sum(v);
  if (pcnn::lane_id() == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  int s = 0;
#pragma unroll
  for (int w = 0; w < T / 64; w++) s += sh[w];
  __syncthreads();
  return s;
}

}  // namespace pcnn_refine
