// Pose head of PoseCNN on MI355X (gfx950): fc8 -> tanh -> * poses_weight ->
// l2_normalize (vgg16_convs.py:193-197, network.py:440-445) and its backward,
// and the column sums of the FC bias gradients.  The FC contraction that feeds
// it is in gemm.hip.
#include "gemm_common.h"
#include "head_common.h"
#include <math.h>

using namespace pcnn_gk;

namespace {

// Column sums (bias gradients): block = 64 columns x 16 row groups; each thread
// sums rows m = g, g+16, ... (coalesced 256 B rows), the 16 partials are then
// added in fixed order (deterministic).
__global__ void __launch_bounds__(1024) k_colsum(const float* __restrict__ X, int M, int N, int ldx,
                                                 const int32_t* __restrict__ M_dev, float* __restrict__ out) {
  __shared__ float part[16][65];
  const int Meff = eff_dim(M, M_dev);
  const int col = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int n = blockIdx.x * 64 + col;
  float s = 0.f;
  if (n < N)
    for (int m = grp; m < Meff; m += 16) s += X[(size_t)m * ldx + n];
  part[grp][col] = s;
  __syncthreads();
  if (grp == 0 && n < N) {
    float t = 0.f;
    for (int g = 0; g < 16; g++) t += part[g][col];
    out[n] = t;
  }
}

// one wave per row; D <= 256
__global__ void __launch_bounds__(256) k_head_fwd(const float* __restrict__ y8, const float* __restrict__ pw,
                                                   int R_cap, const int32_t* __restrict__ num_rois_dev, int D,
                                                   float* __restrict__ t_out, float* __restrict__ pred) {
  const int R = eff_dim(R_cap, num_rois_dev);
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = pcnn::lane_id();
  if (row >= R) return;
  float y[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int c = lane + 64 * k;
    y[k] = c < D ? y8[(size_t)row * D + c] : 0.f;
  }
  pcnn_head::head_fwd_row(y, pw, row, D, lane, t_out, pred);
}

__global__ void __launch_bounds__(256) k_head_bwd(const float* __restrict__ dpred, const float* __restrict__ t_in,
                                                   const float* __restrict__ pw, const float* __restrict__ pred,
                                                   int R_cap, const int32_t* __restrict__ num_rois_dev, int D,
                                                   const float* __restrict__ dscale, float* __restrict__ dy8) {
  const int R = eff_dim(R_cap, num_rois_dev);
  // d_pred = top_diff[0] * bottom_diff when the ADD-loss gradient op is folded
  // in (AveragedistanceBackward, cu.cc:346-354: the same product); 1 * x == x
  const float g = dscale ? dscale[0] : 1.f;
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = pcnn::lane_id();
  if (row >= R) return;
  float dp[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int c = lane + 64 * k;
    dp[k] = c < D ? g * dpred[(size_t)row * D + c] : 0.f;
  }
  pcnn_head::head_bwd_row(dp, t_in, pw, pred, row, D, lane, dy8);
}

}  // namespace

extern "C" int pcnn_colsum(const float* X, int M, int N, int ldx, const int32_t* M_dev, float* out, void* stream) {
  PCNN_REQUIRE(X && out && M >= 0 && N > 0 && ldx >= N);
  hipLaunchKernelGGL(k_colsum, dim3((N + 63) / 64), dim3(1024), 0, (hipStream_t)stream, X, M, N, ldx, M_dev, out);
  PCNN_CHECK_LAUNCH();
  return PCNN_OK;
}

extern "C" int pcnn_pose_head_fwd(const float* y8, const float* poses_weight, int R_cap, const int32_t* num_rois_dev,
                                  int D, float* tanh_out, float* pred, void* stream) {
  PCNN_REQUIRE(y8 && poses_weight && tanh_out && pred && R_cap >= 0 && D > 0 && D <= 256);
  if (R_cap == 0) return PCNN_OK;
  hipLaunchKernelGGL(k_head_fwd, dim3((R_cap + 3) / 4), dim3(256), 0, (hipStream_t)stream, y8, poses_weight, R_cap,
                     num_rois_dev, D, tanh_out, pred);
  PCNN_CHECK_LAUNCH();
  return PCNN_OK;
}

extern "C" int pcnn_pose_head_bwd(const float* d_pred, const float* d_pred_scale, const float* tanh_out,
                                  const float* poses_weight, const float* pred, int R_cap,
                                  const int32_t* num_rois_dev, int D, float* d_y8, void* stream) {
  PCNN_REQUIRE(d_pred && tanh_out && poses_weight && pred && d_y8 && R_cap >= 0 && D > 0 && D <= 256);
  if (R_cap == 0) return PCNN_OK;
  hipLaunchKernelGGL(k_head_bwd, dim3((R_cap + 3) / 4), dim3(256), 0, (hipStream_t)stream, d_pred, tanh_out,
                     poses_weight, pred, R_cap, num_rois_dev, D, d_pred_scale, d_y8);
  PCNN_CHECK_LAUNCH();
  return PCNN_OK;
}
