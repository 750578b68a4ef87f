// The scene renderer's own passes (clear, setup, the triangle passes' target,
// resolve) and its workspace, shared by pcnn_render_scenes (render_scene.hip)
// and pcnn_render_scenes_lit (render_lit.hip).  The rules are written at the
// top of render_scene.hip; this is their only statement in code.  The two ops
// differ in one thing: the resolve's `Shade` parameter, which turns the
// winner's weights into the colour attachment (NoShade: no attachment, and
// nothing of it left in the kernel).
#pragma once
#include "render_common.h"

namespace pcnn {
namespace {

constexpr int kMaxRank = 256;          // instances per scene: 8 bits of the key
constexpr int kMaxFaces = 1 << 24;     // faces per mesh: 24 bits of the key
constexpr uint32_t kNoScene = ~0u;

// The rows of scene s; false when the range is empty or invalid.
__device__ __forceinline__ bool scene_rows(const int32_t* __restrict__ scene_offset, int s, int K, int& a, int& b) {
  a = scene_offset[s];
  b = scene_offset[s + 1];
  return a >= 0 && b > a && b <= K && b - a <= kMaxRank;
}

__global__ void __launch_bounds__(256) k_scene_clear(unsigned long long* zbuf, size_t n, uint32_t* qcount,
                                                     uint32_t* inst_scene, int32_t* visible, int K) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *qcount = 0u;
  if (i < (size_t)K) {
    inst_scene[i] = kNoScene;
    visible[i] = 0;
  }
  if (2 * i + 1 < n) {
    *(ulonglong2*)(zbuf + 2 * i) = make_ulonglong2(kEmpty, kEmpty);
  } else if (2 * i < n) {
    zbuf[2 * i] = kEmpty;
  }
}

__global__ void __launch_bounds__(256)
    k_scene_setup(const float* __restrict__ poses, const int32_t* __restrict__ scene_offset, int K, int S, float fx,
                  float fy, float px, float py, uint32_t* __restrict__ inst_scene, float* __restrict__ logz,
                  float2* __restrict__ centers) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < K) {
    const float tx = poses[(size_t)i * 7 + 4], ty = poses[(size_t)i * 7 + 5], tz = poses[(size_t)i * 7 + 6];
    centers[i] = make_float2(fx * (tx / tz) + px, fy * (ty / tz) + py);
    logz[i] = (float)log((double)tz);
  }
  if (i < S) {
    int a, b;
    if (scene_rows(scene_offset, i, K, a, b))
      for (int k = a; k < b; ++k) atomicMin(inst_scene + k, (uint32_t)i);
  }
}

// The triangle passes' target of instance k (render_common.h): its scene's
// z-buffer and its rank above the face in the key; false when no valid scene
// holds it.
struct SceneTarget {
  const uint32_t* inst_scene;
  const int32_t* scene_offset;
  int S;
  __device__ __forceinline__ bool operator()(int k, RasterTarget& t) const {
    const uint32_t s = inst_scene[k];
    if (s >= (uint32_t)S) return false;
    const int rank = k - scene_offset[s];
    if (rank < 0 || rank >= kMaxRank) return false;
    t.image = s;
    t.prefix = (unsigned)rank << 24;
    return true;
  }
};

// pcnn_render_scenes's resolve: no colour attachment.
struct NoShade {
  __device__ __forceinline__ float4 pixel(int, int, const MeshRef&, const Tri&, const RVert*, float, float,
                                          float) const {
    return make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __device__ __forceinline__ void store(size_t, float4) const {}
};

// Shade: `float4 pixel(s, k, mesh, tri, the instance's RVert rows, la, lb, lc)`
// gives a covered pixel's attachment value from the winner's weights, and
// `store(i, value)` writes scene pixel i's (zero off the models).
template <class Shade>
__global__ void __launch_bounds__(256)
    k_scene_resolve(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                    const int32_t* __restrict__ vert_offset, const int32_t* __restrict__ face_offset, int M,
                    int V_total, int F_total, int F_max, const int32_t* __restrict__ mesh_index,
                    const int32_t* __restrict__ class_id, const uint32_t* __restrict__ inst_scene,
                    const int32_t* __restrict__ scene_offset, int K, const RVert* __restrict__ verts,
                    const unsigned long long* __restrict__ zbuf, const float* __restrict__ logz,
                    const float2* __restrict__ centers, int H, int W, size_t total, int32_t* __restrict__ label,
                    float* __restrict__ depth, F3* __restrict__ vertmap, F3* __restrict__ vertex3,
                    int32_t* __restrict__ inst_id, int32_t* __restrict__ visible, Shade shade) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const float nan = __uint_as_float(0x7fc00000u);
  F3 vm = {nan, nan, nan}, v3 = {0.f, 0.f, 0.f};
  float4 col = make_float4(0.f, 0.f, 0.f, 0.f);
  float d = 0.f;
  int lab = 0, id = -1;
  if (i < total) {
    const size_t hw = (size_t)H * W;
    const int s = (int)(i / hw);
    const int pix = (int)(i - (size_t)s * hw);
    const unsigned long long key = zbuf[i];
    int a, b;
    if (key != kEmpty && scene_rows(scene_offset, s, K, a, b)) {
      const int k = a + (int)(((uint32_t)key) >> 24);
      const int f = (int)((uint32_t)key & 0xffffffu);
      MeshRef m;
      Tri t;
      if (k < b && inst_scene[k] == (uint32_t)s &&
          mesh_of(mesh_index, vert_offset, face_offset, M, V_total, F_total, F_max, k, m) && f < m.nf &&
          tri_setup(verts + (size_t)k * V_total, faces + (size_t)(m.f0 + f) * 3, m.nv, t)) {
        const int y = pix / W, x = pix - y * W;
        float la, lb, lc;
        const float Z = tri_weights(t, x, y, la, lb, lc);
        const float* ma = vertices + (size_t)(m.v0 + t.ia) * 3;
        const float* mb = vertices + (size_t)(m.v0 + t.ib) * 3;
        const float* mc = vertices + (size_t)(m.v0 + t.ic) * 3;
        lab = class_id[k];
        vm.x = ((la * ma[0] + lb * mb[0]) + lc * mc[0]) + (float)lab;  // synthesize.cpp:267-274
        vm.y = (la * ma[1] + lb * mb[1]) + lc * mc[1];
        vm.z = (la * ma[2] + lb * mb[2]) + lc * mc[2];
        d = Z;
        id = k;
        const float2 c = centers[k];
        const double rx = (double)c.x - (double)x, ry = (double)c.y - (double)y;  // minibatch.py:560
        const double nrm = sqrt(rx * rx + ry * ry) + 1e-10;                       // :562
        v3.x = (float)(rx / nrm);                                                 // :564-567
        v3.y = (float)(ry / nrm);
        v3.z = logz[k];                                                           // :568
        col = shade.pixel(s, k, m, t, verts + (size_t)k * V_total, la, lb, lc);
      }
    }
    label[i] = lab;
    depth[i] = d;
    vertmap[i] = vm;
    vertex3[i] = v3;
    if (inst_id) inst_id[i] = id;
    shade.store(i, col);
  }
  // visible: one atomic per wave and distinct winning instance
  bool pending = id >= 0;
  unsigned long long mask;
  while ((mask = __ballot(pending)) != 0ull) {
    const int leader = __ffsll((long long)mask) - 1;
    const int kk = __shfl(id, leader, 64);
    const bool same = pending && id == kk;
    const unsigned long long group = __ballot(same);
    if (lane_id() == leader) atomicAdd(visible + kk, (int32_t)__popcll(group));
    pending = pending && !same;
  }
}

struct SceneWs {
  unsigned long long* zbuf;
  RVert* verts;
  uint2* queue;
  uint32_t* qcount;
  uint32_t* inst_scene;
  float* logz;
  size_t bytes;
};

inline SceneWs carve_scene(void* ws, int S, int K, int H, int W, int V_total, int F_max) {
  Carve c(ws);
  SceneWs r;
  r.zbuf = c.take<unsigned long long>((size_t)S * H * W);
  r.verts = c.take<RVert>((size_t)K * V_total);
  r.queue = c.take<uint2>((size_t)K * F_max);
  r.qcount = c.take<uint32_t>(1);
  r.inst_scene = c.take<uint32_t>((size_t)K);
  r.logz = c.take<float>((size_t)K);
  r.bytes = align_up(c.off, 256);
  return r;
}

inline bool scene_dims_ok(int S, int K, int H, int W, int V_total, int F_max) {
  return S > 0 && K > 0 && H > 0 && W > 0 && V_total > 0 && F_max > 0 && F_max <= kMaxFaces && K <= 65535 &&
         S <= (1 << 20) && H <= (1 << 20) && W <= (1 << 20) && (size_t)H * W <= 0x7fffffffull &&
         (size_t)S * H * W <= (1ull << 38) && (size_t)K * F_max <= 0xffffffffull &&
         (size_t)K * V_total <= (1ull << 32);
}

// The whole op on `stream`: the passes of render_scene.hip's list, the resolve
// with `shade`.  The caller has checked the pointers and the workspace's size.
template <class Shade>
int run_scene_passes(const float* vertices, const float* normals, const int32_t* faces, const int32_t* vert_offset,
                     const int32_t* face_offset, int M, int V_total, int F_total, int F_max,
                     const int32_t* mesh_index, const int32_t* class_id, const float* poses, int K,
                     const int32_t* scene_offset, int S, int H, int W, float fx, float fy, float px, float py,
                     float znear, float zfar, int32_t* label, float* depth, float* vertmap, float* vertex3,
                     int32_t* inst_id, int32_t* visible, float* centers, const SceneWs& ws, Shade shade,
                     hipStream_t st) {
  const size_t total = (size_t)S * H * W;
  const size_t clear_n = total / 2 + 1 > (size_t)K ? total / 2 + 1 : (size_t)K;
  k_scene_clear<<<dim3((unsigned)((clear_n + 255) / 256)), 256, 0, st>>>(ws.zbuf, total, ws.qcount, ws.inst_scene,
                                                                         visible, K);
  PCNN_CHECK_LAUNCH();
  k_scene_setup<<<dim3((unsigned)(((K > S ? K : S) + 255) / 256)), 256, 0, st>>>(
      poses, scene_offset, K, S, fx, fy, px, py, ws.inst_scene, ws.logz, (float2*)centers);
  PCNN_CHECK_LAUNCH();
  k_render_vertex<<<dim3((unsigned)((V_total + 255) / 256), (unsigned)K), 256, 0, st>>>(
      vertices, normals, vert_offset, face_offset, M, V_total, F_total, F_max, mesh_index, poses, fx, fy, px, py,
      znear, ws.verts);
  PCNN_CHECK_LAUNCH();
  const SceneTarget target{ws.inst_scene, scene_offset, S};
  k_render_triangle<<<dim3((unsigned)((F_max + 255) / 256), (unsigned)K), 256, 0, st>>>(
      faces, vert_offset, face_offset, M, V_total, F_total, F_max, mesh_index, target, ws.verts, H, W, zfar,
      small_max(), ws.zbuf, ws.queue, ws.qcount);
  PCNN_CHECK_LAUNCH();
  k_render_large<<<dim3(kLargeBlocks), 256, 0, st>>>(faces, vert_offset, face_offset, M, V_total, F_total, F_max,
                                                     mesh_index, target, ws.verts, K, H, W, zfar, ws.zbuf, ws.queue,
                                                     ws.qcount, (uint32_t)((size_t)K * F_max));
  PCNN_CHECK_LAUNCH();
  k_scene_resolve<<<dim3((unsigned)((total + 255) / 256)), 256, 0, st>>>(
      vertices, faces, vert_offset, face_offset, M, V_total, F_total, F_max, mesh_index, class_id, ws.inst_scene,
      scene_offset, K, ws.verts, ws.zbuf, ws.logz, (const float2*)centers, H, W, total, label, depth, (F3*)vertmap,
      (F3*)vertex3, inst_id, visible, shade);
  PCNN_CHECK_LAUNCH();
  return PCNN_OK;
}

}  // namespace
}  // namespace pcnn
