// Scene renderer for the synthetic training frames (pcnn_render_scenes,
// pcnn_vertex_targets_expand, include/posecnn_hip.h): the role of the
// reference's Synthesizer::render (lib/synthesize/synthesize.cpp:345-609), of
// the label / visibility steps of its render worker (tools/train_net.py:
// 209-230) and of _generate_vertex_targets (lib/gt_synthesize_layer/
// minibatch.py:517-575).  S scenes hold K object instances in all; the
// instances of a scene share one depth test and the scene's label, depth,
// vertmap and vote-target maps are written from the winners.
//
// The geometry (sampling, coverage, culling, values) is that of render.hip,
// taken from render_common.h; only the visibility key and the resolve differ.
// The scene passes themselves are in render_scene_common.h, which
// pcnn_render_scenes_lit (render_lit.hip) runs with a shading resolve.
//
//  Scenes     scene s holds the instance rows [scene_offset[s],
//             scene_offset[s+1]) (a CSR: the ranges of valid scenes are meant
//             to be disjoint).  A range that is decreasing, leaves [0, K] or
//             holds more than 256 rows makes the scene all background; so does
//             an empty one.  A row that two valid scenes name is drawn in the
//             lower-numbered scene only.
//  Visibility per scene pixel one 64-bit atomicMin of
//             (float_bits(Z) << 32) | (rank << 24) | face, rank = the
//             instance's position inside its scene: the nearest Z wins, an
//             equal Z goes to the lower rank, then to the lower face.  Hence
//             at most 2^24 faces per mesh and 256 instances per scene.  A
//             scene of one instance has rank 0 throughout and gives the bits
//             of pcnn_render_meshes.
//  Targets    of the pixel's winning instance, pose translation (tx, ty, tz):
//             c = (fx (tx / tz) + px, fy (ty / tz) + py) in float32
//             (synthesize.cpp:558-562); channels 0, 1 = (c - (x, y)) /
//             (|c - (x, y)| + 1e-10) with the difference, norm and quotient
//             in double, rounded to float32 on store (numpy's types in
//             minibatch.py:556-567); channel 2 = (float)log((double)tz)
//             (:568).  The reference keeps one centre per CLASS (it samples
//             distinct classes); here every pixel uses its own instance's
//             centre, which is the same thing when a class occurs once per
//             scene and the sensible one when it does not.
//
// Passes (one stream, nothing allocated, nothing read back, capturable):
//  clear      z-buffer keys to all-ones, queue count and `visible` to 0,
//             the instance -> scene map to "none"
//  setup      one thread per instance: centre and log depth; one per scene:
//             validates its range and claims its rows (atomicMin of the scene)
//  vertex     render_common.h, one problem per instance
//  triangle,  render_common.h's two triangle passes, the ones render.hip runs,
//  large      given SceneTarget: the owning scene's z-buffer and the
//             instance's rank in the key
//  resolve    one thread per scene pixel: the winning instance and face from
//             the key, weights recomputed, every map written (background
//             included), `visible` counted with one atomic per wave and
//             distinct instance
#include "render_scene_common.h"

namespace pcnn {
namespace {

__global__ void __launch_bounds__(256)
    k_targets_expand(const int32_t* __restrict__ label, const float* __restrict__ vertex3, int C, float w_inside,
                     size_t n, float* __restrict__ targets, float* __restrict__ weights) {
  const size_t e0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (e0 >= n) return;
  const int row = 3 * C;
  float t[4], w[4];
  size_t p = e0 / row;
  int ch = (int)(e0 - p * row);
  int l = label[p];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    t[j] = 0.f;
    w[j] = 0.f;
    if (e0 + j < n) {
      const int c = ch / 3;
      if (l >= 1 && l < C && c == l) {
        t[j] = vertex3[p * 3 + (ch - 3 * c)];
        w[j] = w_inside;
      }
      if (++ch == row) {
        ch = 0;
        ++p;
        if (e0 + j + 1 < n) l = label[p];
      }
    }
  }
  if (e0 + 3 < n) {
    *(float4*)(targets + e0) = make_float4(t[0], t[1], t[2], t[3]);
    *(float4*)(weights + e0) = make_float4(w[0], w[1], w[2], w[3]);
  } else {
    for (int j = 0; e0 + j < n; ++j) {
      targets[e0 + j] = t[j];
      weights[e0 + j] = w[j];
    }
  }
}

}  // namespace
}  // namespace pcnn

extern "C" size_t pcnn_render_scenes_workspace_size(int S, int K, int H, int W, int V_total, int F_max) {
  if (!pcnn::scene_dims_ok(S, K, H, W, V_total, F_max)) return 0;
  return pcnn::carve_scene(nullptr, S, K, H, W, V_total, F_max).bytes;
}

extern "C" int pcnn_render_scenes(const float* vertices, const float* normals, const int32_t* faces,
                                  const int32_t* vert_offset, const int32_t* face_offset, int M, int V_total,
                                  int F_total, int F_max, const int32_t* mesh_index, const int32_t* class_id,
                                  const float* poses, int K, const int32_t* scene_offset, int S, int H, int W,
                                  float fx, float fy, float px, float py, float znear, float zfar, int32_t* label,
                                  float* depth, float* vertmap, float* vertex3, int32_t* inst_id, int32_t* visible,
                                  float* centers, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace pcnn;
  PCNN_REQUIRE(vertices && normals && faces && vert_offset && face_offset && mesh_index && class_id && poses);
  PCNN_REQUIRE(scene_offset && label && depth && vertmap && vertex3 && visible && centers && workspace);
  PCNN_REQUIRE(M > 0 && F_total > 0 && F_max <= F_total && scene_dims_ok(S, K, H, W, V_total, F_max));
  PCNN_REQUIRE(znear > 0.f && zfar >= znear);  // Z > 0: the depth's bits order like its value
  PCNN_REQUIRE(((uintptr_t)label & 3) == 0 && ((uintptr_t)depth & 3) == 0 && ((uintptr_t)vertmap & 3) == 0 &&
               ((uintptr_t)vertex3 & 3) == 0 && ((uintptr_t)inst_id & 3) == 0 && ((uintptr_t)visible & 3) == 0 &&
               ((uintptr_t)centers & 7) == 0 && ((uintptr_t)workspace & 15) == 0);
  const SceneWs ws = carve_scene(workspace, S, K, H, W, V_total, F_max);
  if (workspace_bytes < ws.bytes) return PCNN_ECAPACITY;
  return run_scene_passes(vertices, normals, faces, vert_offset, face_offset, M, V_total, F_total, F_max, mesh_index,
                          class_id, poses, K, scene_offset, S, H, W, fx, fy, px, py, znear, zfar, label, depth, vertmap,
                          vertex3, inst_id, visible, centers, ws, NoShade{}, (hipStream_t)stream);
}

extern "C" int pcnn_vertex_targets_expand(const int32_t* label, const float* vertex3, int B, int H, int W, int C,
                                          float w_inside, float* vertex_targets, float* vertex_weights,
                                          void* stream) {
  using namespace pcnn;
  PCNN_REQUIRE(label && vertex3 && vertex_targets && vertex_weights);
  PCNN_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && C <= (1 << 20));
  PCNN_REQUIRE(((uintptr_t)vertex_targets & 15) == 0 && ((uintptr_t)vertex_weights & 15) == 0 &&
               ((uintptr_t)label & 3) == 0 && ((uintptr_t)vertex3 & 3) == 0);
  const size_t n = (size_t)B * H * W * 3 * C;
  PCNN_REQUIRE((size_t)B * H * W <= (1ull << 38) && (n + 3) / 4 <= 0x7fffffffull * 256);
  k_targets_expand<<<dim3((unsigned)(((n + 3) / 4 + 255) / 256)), 256, 0, (hipStream_t)stream>>>(
      label, vertex3, C, w_inside, n, vertex_targets, vertex_weights);
  PCNN_CHECK_LAUNCH();
  return PCNN_OK;
}
