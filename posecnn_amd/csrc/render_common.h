// The mesh rasterisers' shared geometry: the vertex pass, triangle set-up,
// coverage, weights and the z-buffer key of one fragment, used by
// pcnn_render_meshes (render.hip, one object per image) and pcnn_render_scenes
// (render_scene.hip, several objects depth-tested in one image).  The rules
// are written at the top of render.hip; this is their only statement in code.
#pragma once
#include <stdlib.h>

#include "pcnn_common.h"

namespace pcnn {
namespace {

constexpr double kMaxPx = 1048576.;  // 2^20: snapped coordinates stay below 2^29, edge products below 2^60
constexpr unsigned long long kEmpty = ~0ull;
// bounding-box pixel centres up to which the triangle's own thread rasterises
// it (DESIGN.md "Mesh rasteriser": the A/B behind the value)
constexpr int kSmallMaxDefault = 64;
constexpr int kLargeBlocks = 1024;  // x 4 waves: the large-triangle pass's fixed grid
constexpr int kBands = 8;           // row bands of a queued triangle's bounding box, one wave each

// Experiments only: PCNN_RENDER_SMALL_MAX overrides the path threshold (the
// result is the same bits on either path).
inline int small_max() {
  const char* s = getenv("PCNN_RENDER_SMALL_MAX");
  return s && *s ? atoi(s) : kSmallMaxDefault;
}

struct F3 {
  float x, y, z;
};

struct RVert {     // per (problem, vertex) record of the vertex pass, 48 B
  float4 cam;      // X, Y, Z, 1 if drawable (Z >= znear, |u|, |v| <= 2^20) else 0
  float4 nrm;      // R n / |R n| (zero length left as is), 0
  int2 s;          // snapped projection, 1/256 px
  float2 r;        // unsnapped projection minus the snapped one, px (|r| <= 1/512)
};

struct MeshRef {
  int v0, nv, f0, nf;
};

// Problem k's mesh; false (nothing is drawn) for a mesh_index outside [0, M)
// or offsets that do not fit the packed arrays and the workspace's slabs.
__device__ __forceinline__ bool mesh_of(const int32_t* mesh_index, const int32_t* vert_offset,
                                        const int32_t* face_offset, int M, int V_total, int F_total, int F_max, int k,
                                        MeshRef& m) {
  const int mi = mesh_index[k];
  if (mi < 0 || mi >= M) return false;
  const int v0 = vert_offset[mi], v1 = vert_offset[mi + 1];
  const int f0 = face_offset[mi], f1 = face_offset[mi + 1];
  if (v0 < 0 || v1 < v0 || v1 > V_total || f0 < 0 || f1 < f0 || f1 > F_total || f1 - f0 > F_max) return false;
  m.v0 = v0;
  m.nv = v1 - v0;
  m.f0 = f0;
  m.nf = f1 - f0;
  return true;
}

__global__ void __launch_bounds__(256)
    k_render_vertex(const float* __restrict__ vertices, const float* __restrict__ normals,
                    const int32_t* __restrict__ vert_offset, const int32_t* __restrict__ face_offset, int M,
                    int V_total, int F_total, int F_max, const int32_t* __restrict__ mesh_index,
                    const float* __restrict__ poses, float fx, float fy, float px, float py, float znear,
                    RVert* __restrict__ verts) {
  const int k = blockIdx.y;
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  MeshRef m;
  if (!mesh_of(mesh_index, vert_offset, face_offset, M, V_total, F_total, F_max, k, m) || v >= m.nv) return;
  // double throughout: the projection's rounding (an ulp of a float u is
  // 8e-6 px at u = 100) would otherwise reach the weights of sliver triangles
  const float* qf = poses + (size_t)k * 7;
  double qw = qf[0], qx = qf[1], qy = qf[2], qz = qf[3];
  const double qn = sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz);
  qw = qw / qn;
  qx = qx / qn;
  qy = qy / qn;
  qz = qz / qn;
  const double r00 = 1. - 2. * (qy * qy + qz * qz), r01 = 2. * (qx * qy - qz * qw), r02 = 2. * (qx * qz + qy * qw);
  const double r10 = 2. * (qx * qy + qz * qw), r11 = 1. - 2. * (qx * qx + qz * qz), r12 = 2. * (qy * qz - qx * qw);
  const double r20 = 2. * (qx * qz - qy * qw), r21 = 2. * (qy * qz + qx * qw), r22 = 1. - 2. * (qx * qx + qy * qy);
  const float* pf = vertices + (size_t)(m.v0 + v) * 3;
  const float* nf = normals + (size_t)(m.v0 + v) * 3;
  const double p0 = pf[0], p1 = pf[1], p2 = pf[2], n0 = nf[0], n1 = nf[1], n2 = nf[2];
  const double X = ((r00 * p0 + r01 * p1) + r02 * p2) + (double)qf[4];
  const double Y = ((r10 * p0 + r11 * p1) + r12 * p2) + (double)qf[5];
  const double Z = ((r20 * p0 + r21 * p1) + r22 * p2) + (double)qf[6];
  double nx = (r00 * n0 + r01 * n1) + r02 * n2;
  double ny = (r10 * n0 + r11 * n1) + r12 * n2;
  double nz = (r20 * n0 + r21 * n1) + r22 * n2;
  const double len = sqrt((nx * nx + ny * ny) + nz * nz);
  if (len > 0.) {  // vertsAndNorms.vert: a zero-length normal is left as is
    nx = nx / len;
    ny = ny / len;
    nz = nz / len;
  }
  const double u = (double)fx * X / Z + (double)px;
  const double w = (double)fy * Y / Z + (double)py;
  // NaN (a zero quaternion, Z = 0) fails every comparison: not drawable
  const bool ok = Z >= (double)znear && fabs(u) <= kMaxPx && fabs(w) <= kMaxPx;
  RVert o;
  o.cam = make_float4((float)X, (float)Y, (float)Z, ok ? 1.f : 0.f);
  o.nrm = make_float4((float)nx, (float)ny, (float)nz, 0.f);
  o.s = make_int2(0, 0);
  o.r = make_float2(0.f, 0.f);
  if (ok) {
    const double su = rint(u * 256.), sw = rint(w * 256.);
    o.s = make_int2((int)su, (int)sw);
    o.r = make_float2((float)(u - su / 256.), (float)(w - sw / 256.));
  }
  verts[(size_t)k * V_total + v] = o;
}

struct Tri {          // a set-up triangle, vertices a, b, c in the positive orientation
  int ia, ib, ic;     // local vertex indices
  int2 sa, sb, sc;    // snapped positions
  float2 ra, rb, rc;  // unsnapped minus snapped positions, px
  float za, zb, zc;   // camera Z
};

// Face f of problem's mesh: false when an index is out of range, a vertex is
// not drawable or the integer area is 0.
__device__ __forceinline__ bool tri_setup(const RVert* __restrict__ vs, const int32_t* __restrict__ face, int nv,
                                          Tri& t) {
  int ia = face[0], ib = face[1], ic = face[2];
  if ((unsigned)ia >= (unsigned)nv || (unsigned)ib >= (unsigned)nv || (unsigned)ic >= (unsigned)nv) return false;
  float4 ca = vs[ia].cam, cb = vs[ib].cam, cc = vs[ic].cam;
  if (ca.w == 0.f || cb.w == 0.f || cc.w == 0.f) return false;
  int2 sa = vs[ia].s, sb = vs[ib].s, sc = vs[ic].s;
  const int64_t area = (int64_t)(sb.x - sa.x) * (int64_t)(sc.y - sa.y) - (int64_t)(sb.y - sa.y) * (int64_t)(sc.x - sa.x);
  if (area == 0) return false;
  if (area < 0) {  // swap b and c
    int ti = ib; ib = ic; ic = ti;
    int2 ts = sb; sb = sc; sc = ts;
    float4 tc = cb; cb = cc; cc = tc;
  }
  t.ia = ia; t.ib = ib; t.ic = ic;
  t.sa = sa; t.sb = sb; t.sc = sc;
  t.ra = vs[ia].r; t.rb = vs[ib].r; t.rc = vs[ic].r;
  t.za = ca.z; t.zb = cb.z; t.zc = cc.z;
  return true;
}

// floor / ceil of a snapped coordinate in pixels (|s| < 2^29)
__device__ __forceinline__ int px_floor(int s) { return s >> 8; }
__device__ __forceinline__ int px_ceil(int s) { return (s + 255) >> 8; }

// Pixel-centre bounding box clipped to the viewport; false when empty.
__device__ __forceinline__ bool tri_bbox(const Tri& t, int H, int W, int& x0, int& x1, int& y0, int& y1) {
  x0 = max(px_ceil(min(t.sa.x, min(t.sb.x, t.sc.x))), 0);
  x1 = min(px_floor(max(t.sa.x, max(t.sb.x, t.sc.x))), W - 1);
  y0 = max(px_ceil(min(t.sa.y, min(t.sb.y, t.sc.y))), 0);
  y1 = min(px_floor(max(t.sa.y, max(t.sb.y, t.sc.y))), H - 1);
  return x0 <= x1 && y0 <= y1;
}

__device__ __forceinline__ bool edge_covers(int2 a, int2 b, int64_t x, int64_t y) {
  const int64_t dx = (int64_t)b.x - a.x, dy = (int64_t)b.y - a.y;
  const int64_t e = dx * (y - a.y) - dy * (x - a.x);
  return e > 0 || (e == 0 && (dy < 0 || (dy == 0 && dx > 0)));
}

__device__ __forceinline__ bool tri_covers(const Tri& t, int x, int y) {
  const int64_t X = (int64_t)x * 256, Y = (int64_t)y * 256;
  return edge_covers(t.sa, t.sb, X, Y) && edge_covers(t.sb, t.sc, X, Y) && edge_covers(t.sc, t.sa, X, Y);
}

// Float edge function of the unsnapped edge a -> b at the pixel centre whose
// snapped coordinates are (x, y): every difference is taken as the (exact
// integer) snapped difference plus the difference of the residuals, so its
// error is relative to its own size and not to the coordinates'.
__device__ __forceinline__ float edge_f(int2 sa, float2 ra, int2 sb, float2 rb, int x, int y) {
  const float k = 1.f / 256.f;
  const float dx = (float)(sb.x - sa.x) * k + (rb.x - ra.x), dy = (float)(sb.y - sa.y) * k + (rb.y - ra.y);
  const float qx = (float)(x - sa.x) * k - ra.x, qy = (float)(y - sa.y) * k - ra.y;
  return dx * qy - dy * qx;
}

// Perspective-correct weights of a, b, c at pixel centre (x, y) and the depth.
__device__ __forceinline__ float tri_weights(const Tri& t, int x, int y, float& la, float& lb, float& lc) {
  const int X = x * 256, Y = y * 256;  // |x|, |y| < 2^22: the viewport
  const float ba = edge_f(t.sb, t.rb, t.sc, t.rc, X, Y) / t.za;
  const float bb = edge_f(t.sc, t.rc, t.sa, t.ra, X, Y) / t.zb;
  const float bc = edge_f(t.sa, t.ra, t.sb, t.rb, X, Y) / t.zc;
  const float s = (ba + bb) + bc;
  la = ba / s;
  lb = bb / s;
  lc = bc / s;
  return (la * t.za + lb * t.zb) + lc * t.zc;
}

// One fragment into the image's z-buffer zk: `low` is the key's low word, the
// face index (the scene renderer puts the instance's rank into its top 8 bits).
__device__ __forceinline__ void raster_pixel(const Tri& t, int x, int y, float zfar, unsigned low,
                                             unsigned long long* __restrict__ zk, int W) {
  if (!tri_covers(t, x, y)) return;
  float la, lb, lc;
  const float Z = tri_weights(t, x, y, la, lb, lc);
  if (!(Z > 0.f && Z <= zfar)) return;
  atomicMin(zk + (size_t)y * W + x, ((unsigned long long)__float_as_uint(Z) << 32) | low);
}

// Where problem k's fragments go: the image (z-buffer slab of H x W keys) and
// the bits set above the face index in the key's low word.  The two ops give
// the triangle passes a functor `bool target_of(int k, RasterTarget&)`, false
// when k draws nothing: pcnn_render_meshes image k and no prefix,
// pcnn_render_scenes the instance's scene and its rank << 24.
struct RasterTarget {
  uint32_t image;
  unsigned prefix;
};

// One thread per (problem, face): setup, culls; a clipped bounding box of at
// most `small_max` pixel centres is rasterised here, a larger triangle is
// queued for k_render_large (one aggregated atomic per wave).
template <class TargetOf>
__global__ void __launch_bounds__(256)
    k_render_triangle(const int32_t* __restrict__ faces, const int32_t* __restrict__ vert_offset,
                      const int32_t* __restrict__ face_offset, int M, int V_total, int F_total, int F_max,
                      const int32_t* __restrict__ mesh_index, TargetOf target_of, const RVert* __restrict__ verts,
                      int H, int W, float zfar, int small_max, unsigned long long* __restrict__ zbuf,
                      uint2* __restrict__ queue, uint32_t* __restrict__ qcount) {
  const int k = blockIdx.y;
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  MeshRef m;
  RasterTarget tg;
  bool big = false;
  if (target_of(k, tg) && mesh_of(mesh_index, vert_offset, face_offset, M, V_total, F_total, F_max, k, m) &&
      f < m.nf) {
    Tri t;
    int x0, x1, y0, y1;
    if (tri_setup(verts + (size_t)k * V_total, faces + (size_t)(m.f0 + f) * 3, m.nv, t) &&
        tri_bbox(t, H, W, x0, x1, y0, y1)) {
      if ((int64_t)(x1 - x0 + 1) * (y1 - y0 + 1) <= small_max) {
        unsigned long long* zk = zbuf + (size_t)tg.image * H * W;
        for (int y = y0; y <= y1; ++y)
          for (int x = x0; x <= x1; ++x) raster_pixel(t, x, y, zfar, tg.prefix | (unsigned)f, zk, W);
      } else {
        big = true;
      }
    }
  }
  // one queue reservation per wave
  const unsigned long long mask = __ballot(big);
  if (mask) {
    const int leader = __ffsll((long long)mask) - 1;
    uint32_t base = 0;
    if (lane_id() == leader) base = atomicAdd(qcount, (uint32_t)__popcll(mask));
    base = __shfl(base, leader, 64);
    if (big) queue[base + __popcll(mask & lanemask_lt())] = make_uint2((unsigned)k, (unsigned)f);
  }
}

// A fixed grid of waves over the queue (count read on the device): one row
// band (1 / kBands of the bounding box) of one triangle per wave, lanes
// striding the band.
template <class TargetOf>
__global__ void __launch_bounds__(256)
    k_render_large(const int32_t* __restrict__ faces, const int32_t* __restrict__ vert_offset,
                   const int32_t* __restrict__ face_offset, int M, int V_total, int F_total, int F_max,
                   const int32_t* __restrict__ mesh_index, TargetOf target_of, const RVert* __restrict__ verts, int K,
                   int H, int W, float zfar, unsigned long long* __restrict__ zbuf, const uint2* __restrict__ queue,
                   const uint32_t* __restrict__ qcount, uint32_t capacity) {
  const uint64_t n = (uint64_t)min(*qcount, capacity) * kBands;
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, waves = (gridDim.x * blockDim.x) >> 6;
  const int lane = lane_id();
  for (uint64_t i = wave; i < n; i += waves) {
    const uint2 e = queue[i / kBands];
    const int band = (int)(i % kBands);
    const int k = (int)e.x, f = (int)e.y;
    MeshRef m;
    RasterTarget tg;
    if (k >= K || !target_of(k, tg) ||
        !mesh_of(mesh_index, vert_offset, face_offset, M, V_total, F_total, F_max, k, m) || f >= m.nf)
      continue;
    Tri t;
    int x0, x1, y0, y1;
    if (!tri_setup(verts + (size_t)k * V_total, faces + (size_t)(m.f0 + f) * 3, m.nv, t) ||
        !tri_bbox(t, H, W, x0, x1, y0, y1))
      continue;
    unsigned long long* zk = zbuf + (size_t)tg.image * H * W;
    const int rows = y1 - y0 + 1;  // this wave's rows: [ya, yb)
    const int ya = y0 + (int)((int64_t)rows * band / kBands), yb = y0 + (int)((int64_t)rows * (band + 1) / kBands);
    const int nx = x1 - x0 + 1, cnt = nx * (yb - ya);
    for (int j = lane; j < cnt; j += 64) {
      const int r = j / nx;
      raster_pixel(t, x0 + (j - r * nx), ya + r, zfar, tg.prefix | (unsigned)f, zk, W);
    }
  }
}

}  // namespace
}  // namespace pcnn
