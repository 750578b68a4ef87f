// Triangle-mesh rasteriser for the pose-refinement maps (pcnn_render_meshes,
// include/posecnn_hip.h): the role of the reference's OpenGL pass
// (lib/synthesize/synthesize.cpp:2103-2139 with the canonicalVerts.* and
// vertsAndNorms.* shaders of lib/kinect_fusion/shaders).  K problems, one mesh
// and one pose each, into pred_vertices / pred_normals (K,H,W,4), vertmap
// (K,H,W,3) and optionally depth / tri_id (K,H,W).
//
// Geometry rules (DESIGN.md "Mesh rasteriser" restates them)
//  Sampling   pixel (x, y) samples the image-plane point u = x, v = y, with
//             u = fx X / Z + px, v = fy Y / Z + py (the box ray-caster's rays;
//             ProjectionMatrixRDF_TopLeft(..., px + 0.5, ...) under GL's
//             half-pixel centres).
//  Coverage   exact and order-independent.  Projected vertices are snapped to
//             1/256 px (rint(u * 256) as an integer) and the edge functions
//             are evaluated in int64.  A triangle is oriented so that its
//             integer area is positive in the x-right, y-down frame; area 0 is
//             dropped.  For an edge a -> b, d = b - a,
//             e(p) = d.x (p.y - a.y) - d.y (p.x - a.x); the edge covers p when
//             e > 0, or e = 0 and (d.y < 0 or (d.y = 0 and d.x > 0)).  A pixel
//             is covered when all three edges cover it, so a pixel centre on
//             an edge shared by two triangles belongs to exactly one of them.
//  Culling    no back-face culling (the reference enables none).  A triangle
//             is dropped whole when a vertex has Z < znear (a narrowing: no
//             near-plane clipping; objects at 0.25-6 m never cross the plane),
//             when a vertex has |u| or |v| above 2^20 px, or when its snapped
//             bounding box holds no pixel centre of the viewport.  A fragment
//             with Z > zfar (or a Z that is not a positive number) is discarded.
//  Values     float32 from the UNSNAPPED projected vertices: the three float
//             edge functions at the pixel centre, each divided by its vertex's
//             Z, normalised by their sum (perspective-correct weights); every
//             attribute and the depth are interpolated with those weights.
//             Snapping moves coverage only, never values.  The vertex pass
//             works in double and keeps the unsnapped position as the snapped
//             one plus a float residual (|r| <= 1/512 px); the per-pixel
//             arithmetic is float32.  (With u itself held in a float, its
//             rounding -- 8e-6 px at u = 100 -- reached the weights of sliver
//             triangles at a silhouette: interpolated normals were off by
//             5.1e-6 against float64; in this form 1.8e-7, see DESIGN.md.)
//  Visibility the nearest camera Z wins, an equal Z goes to the lower face
//             index: a 64-bit atomicMin of (float_bits(Z) << 32) | face (Z > 0,
//             so its bits order like its value).  A render is bitwise
//             reproducible and the same alone or inside a batch.
//
// Passes (one stream, nothing allocated, nothing read back, capturable):
//  clear      z-buffer keys to all-ones, large-triangle queue count to 0
//  vertex     one thread per (problem, vertex), in double: R from the
//             normalised quaternion, camera position, u / v, snapped u / v and
//             the residuals, rotated normal
//  triangle   one thread per (problem, face): setup, culls; a clipped bounding
//             box of at most `small_max` pixel centres is rasterised by the
//             thread, larger ones are queued (one aggregated atomic per wave)
//  large      a fixed grid of waves over the queue (count read on the device),
//             one row band (an eighth of the bounding box) of one triangle
//             per wave, lanes striding the band
//  resolve    one thread per pixel: the winning face's weights recomputed,
//             every map written (background included) with vector stores
//
// The vertex pass, the two triangle passes and the per-triangle /
// per-fragment helpers live in render_common.h, shared with the scene
// renderer (render_scene.hip); clear and resolve are this file's.
#include "render_common.h"

namespace pcnn {
namespace {

__global__ void __launch_bounds__(256) k_render_clear(unsigned long long* zbuf, size_t n, uint32_t* qcount) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *qcount = 0u;
  if (2 * i + 1 < n) {
    *(ulonglong2*)(zbuf + 2 * i) = make_ulonglong2(kEmpty, kEmpty);
  } else if (2 * i < n) {
    zbuf[2 * i] = kEmpty;
  }
}

// The triangle passes' target of problem k (render_common.h): image k, the
// face alone in the key's low word.
struct ImagePerProblem {
  __device__ __forceinline__ bool operator()(int k, RasterTarget& t) const {
    t.image = (uint32_t)k;
    t.prefix = 0u;
    return true;
  }
};

__global__ void __launch_bounds__(256)
    k_render_resolve(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                     const int32_t* __restrict__ vert_offset, const int32_t* __restrict__ face_offset, int M,
                     int V_total, int F_total, int F_max, const int32_t* __restrict__ mesh_index,
                     const int32_t* __restrict__ class_id, const RVert* __restrict__ verts,
                     const unsigned long long* __restrict__ zbuf, int H, int W, size_t total,
                     float4* __restrict__ pred_vertices, float4* __restrict__ pred_normals, F3* __restrict__ vertmap,
                     float* __restrict__ depth, int32_t* __restrict__ tri_id) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const size_t hw = (size_t)H * W;
  const int k = (int)(i / hw);
  const int pix = (int)(i - (size_t)k * hw);
  const unsigned long long key = zbuf[i];
  float4 pv = make_float4(0.f, 0.f, 0.f, 0.f), pn = pv;
  const float nan = __uint_as_float(0x7fc00000u);
  F3 vm = {nan, nan, nan};
  float d = 0.f;
  int id = -1;
  MeshRef m;
  if (key != kEmpty && mesh_of(mesh_index, vert_offset, face_offset, M, V_total, F_total, F_max, k, m)) {
    const int f = (int)(uint32_t)key;
    const RVert* vs = verts + (size_t)k * V_total;
    Tri t;
    if (f < m.nf && tri_setup(vs, faces + (size_t)(m.f0 + f) * 3, m.nv, t)) {
      const int y = pix / W, x = pix - y * W;
      float la, lb, lc;
      const float Z = tri_weights(t, x, y, la, lb, lc);
      const float4 ca = vs[t.ia].cam, cb = vs[t.ib].cam, cc = vs[t.ic].cam;
      const float4 na = vs[t.ia].nrm, nb = vs[t.ib].nrm, nc = vs[t.ic].nrm;
      const float* ma = vertices + (size_t)(m.v0 + t.ia) * 3;
      const float* mb = vertices + (size_t)(m.v0 + t.ib) * 3;
      const float* mc = vertices + (size_t)(m.v0 + t.ic) * 3;
      pv = make_float4((la * ca.x + lb * cb.x) + lc * cc.x, (la * ca.y + lb * cb.y) + lc * cc.y, Z, 1.f);
      pn = make_float4((la * na.x + lb * nb.x) + lc * nc.x, (la * na.y + lb * nb.y) + lc * nc.y,
                       (la * na.z + lb * nb.z) + lc * nc.z, 0.f);
      vm.x = ((la * ma[0] + lb * mb[0]) + lc * mc[0]) + (float)class_id[k];  // synthesize.cpp:267-274
      vm.y = (la * ma[1] + lb * mb[1]) + lc * mc[1];
      vm.z = (la * ma[2] + lb * mb[2]) + lc * mc[2];
      d = Z;
      id = f;
    }
  }
  pred_vertices[i] = pv;
  pred_normals[i] = pn;
  vertmap[i] = vm;
  if (depth) depth[i] = d;
  if (tri_id) tri_id[i] = id;
}

struct RenderWs {
  unsigned long long* zbuf;
  RVert* verts;
  uint2* queue;
  uint32_t* qcount;
  size_t bytes;
};

RenderWs carve_render(void* ws, int K, int H, int W, int V_total, int F_max) {
  Carve c(ws);
  RenderWs r;
  r.zbuf = c.take<unsigned long long>((size_t)K * H * W);
  r.verts = c.take<RVert>((size_t)K * V_total);
  r.queue = c.take<uint2>((size_t)K * F_max);
  r.qcount = c.take<uint32_t>(1);
  r.bytes = align_up(c.off, 256);
  return r;
}

bool dims_ok(int K, int H, int W, int V_total, int F_max) {
  return K > 0 && H > 0 && W > 0 && V_total > 0 && F_max > 0 && K <= 65535 && H <= (1 << 20) && W <= (1 << 20) &&
         (size_t)H * W <= 0x7fffffffull &&
         (size_t)K * H * W <= (1ull << 38) && (size_t)K * F_max <= 0xffffffffull;
}

}  // namespace
}  // namespace pcnn

extern "C" size_t pcnn_render_workspace_size(int K, int H, int W, int V_total, int F_max) {
  if (!pcnn::dims_ok(K, H, W, V_total, F_max)) return 0;
  return pcnn::carve_render(nullptr, K, H, W, V_total, F_max).bytes;
}

extern "C" int pcnn_render_meshes(const float* vertices, const float* normals, const int32_t* faces,
                                  const int32_t* vert_offset, const int32_t* face_offset, int M, int V_total,
                                  int F_total, int F_max, const int32_t* mesh_index, const int32_t* class_id,
                                  const float* poses, int K, int H, int W, float fx, float fy, float px, float py,
                                  float znear, float zfar, float* pred_vertices, float* pred_normals, float* vertmap,
                                  float* depth, int32_t* tri_id, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  using namespace pcnn;
  PCNN_REQUIRE(vertices && normals && faces && vert_offset && face_offset && mesh_index && class_id && poses);
  PCNN_REQUIRE(pred_vertices && pred_normals && vertmap && workspace);
  PCNN_REQUIRE(M > 0 && F_total > 0 && F_max <= F_total && dims_ok(K, H, W, V_total, F_max));
  PCNN_REQUIRE(znear > 0.f && zfar >= znear);  // Z > 0: the depth's bits order like its value
  PCNN_REQUIRE(((uintptr_t)pred_vertices & 15) == 0 && ((uintptr_t)pred_normals & 15) == 0 &&
               ((uintptr_t)workspace & 15) == 0);
  const RenderWs ws = carve_render(workspace, K, H, W, V_total, F_max);
  if (workspace_bytes < ws.bytes) return PCNN_ECAPACITY;
  hipStream_t st = (hipStream_t)stream;
  const size_t total = (size_t)K * H * W;
  k_render_clear<<<dim3((unsigned)((total / 2 + 256) / 256)), 256, 0, st>>>(ws.zbuf, total, ws.qcount);
  PCNN_CHECK_LAUNCH();
  k_render_vertex<<<dim3((unsigned)((V_total + 255) / 256), (unsigned)K), 256, 0, st>>>(
      vertices, normals, vert_offset, face_offset, M, V_total, F_total, F_max, mesh_index, poses, fx, fy, px, py,
      znear, ws.verts);
  PCNN_CHECK_LAUNCH();
  k_render_triangle<<<dim3((unsigned)((F_max + 255) / 256), (unsigned)K), 256, 0, st>>>(
      faces, vert_offset, face_offset, M, V_total, F_total, F_max, mesh_index, ImagePerProblem{}, ws.verts, H, W, zfar,
      small_max(), ws.zbuf, ws.queue, ws.qcount);
  PCNN_CHECK_LAUNCH();
  k_render_large<<<dim3(kLargeBlocks), 256, 0, st>>>(faces, vert_offset, face_offset, M, V_total, F_total, F_max,
                                                     mesh_index, ImagePerProblem{}, ws.verts, K, H, W, zfar, ws.zbuf,
                                                     ws.queue, ws.qcount, (uint32_t)((size_t)K * F_max));
  PCNN_CHECK_LAUNCH();
  k_render_resolve<<<dim3((unsigned)((total + 255) / 256)), 256, 0, st>>>(
      vertices, faces, vert_offset, face_offset, M, V_total, F_total, F_max, mesh_index, class_id, ws.verts, ws.zbuf,
      H, W, total, (float4*)pred_vertices, (float4*)pred_normals, (pcnn::F3*)vertmap, depth, tri_id);
  PCNN_CHECK_LAUNCH();
  return PCNN_OK;
}
