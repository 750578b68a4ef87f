// The network's input side (include/posecnn_image.h): pcnn_render_scenes_lit,
// the scene renderer with a Phong-lit colour attachment -- the colour pass of
// the reference's Synthesizer::render (lib/synthesize/synthesize.cpp:473-536,
// 575-590, shaders canonicalVertsAndColor.*) -- and pcnn_image_blob, the
// picture -> input-blob pass of _get_image_blob (lib/gt_synthesize_layer/
// minibatch.py:132-187, lib/utils/blob.py:74-129).
//
//  Lit render the passes of render_scene.hip, unchanged (render_scene_common.h);
//             the resolve is given Phong, which shades the pixel from the
//             winner's weights: P, N and the surface colour interpolated like
//             every other map, then the shader's ApplyLight in float32, every
//             operation rounded separately, sums as (x + y) + z.  One 16-byte
//             store (b, g, r, 1) per pixel; (0, 0, 0, 0) off the models.
//  Blob       one thread per four consecutive pixels of the batch: quantise,
//             paste the background where alpha is 0, HLS jitter, Gaussian
//             noise, mean subtraction (the rules are in the header; their numpy
//             restatement is tests/image_ref.py).  Every step is a correctly
//             rounded float32 or an integer operation but the deviate, which is
//             evaluated in double and rounded once.  NHWC: three float4 stores
//             per thread; NCHW: one float4 per channel plane when H W is a
//             multiple of 4, scalar stores otherwise and in the batch's tail.
#include "../../include/posecnn_image.h"
#include "pcnn_philox.h"
#include "render_scene_common.h"

namespace pcnn {
namespace {

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
  return (ax * bx + ay * by) + az * bz;
}

// The surface colour at the pixel: the interpolated vertex colour.  A texture
// fetch at interpolated texture coordinates would replace this function alone.
__device__ __forceinline__ F3 surface_color(const float* __restrict__ colors, const MeshRef& m, const Tri& t, float la,
                                            float lb, float lc) {
  const float* ca = colors + (size_t)(m.v0 + t.ia) * 3;
  const float* cb = colors + (size_t)(m.v0 + t.ib) * 3;
  const float* cc = colors + (size_t)(m.v0 + t.ic) * 3;
  return F3{(la * ca[0] + lb * cb[0]) + lc * cc[0], (la * ca[1] + lb * cb[1]) + lc * cc[1],
            (la * ca[2] + lb * cb[2]) + lc * cc[2]};
}

// The resolve's colour attachment (render_scene_common.h, `Shade`).
struct Phong {
  const float* colors;     // (V_total,3) RGB
  const float* shininess;  // (K)
  const float* lights;     // (S,8)
  float4* color;           // (S,H,W) BGRA

  __device__ __forceinline__ float4 pixel(int s, int k, const MeshRef& m, const Tri& t, const RVert* __restrict__ vs,
                                          float la, float lb, float lc) const {
    const float4 pa = vs[t.ia].cam, pb = vs[t.ib].cam, pc = vs[t.ic].cam;
    const float4 na = vs[t.ia].nrm, nb = vs[t.ib].nrm, nc = vs[t.ic].nrm;
    const float Px = (la * pa.x + lb * pb.x) + lc * pc.x;
    const float Py = (la * pa.y + lb * pb.y) + lc * pc.y;
    const float Pz = (la * pa.z + lb * pb.z) + lc * pc.z;
    float Nx = (la * na.x + lb * nb.x) + lc * nc.x;
    float Ny = (la * na.y + lb * nb.y) + lc * nc.y;
    float Nz = (la * na.z + lb * nb.z) + lc * nc.z;
    const float nlen = sqrtf(dot3(Nx, Ny, Nz, Nx, Ny, Nz));
    if (nlen > 0.f) {
      Nx = Nx / nlen;
      Ny = Ny / nlen;
      Nz = Nz / nlen;
    }
    const F3 c = surface_color(colors, m, t, la, lb, lc);
    const float4 lp = *(const float4*)(lights + (size_t)s * 8);
    const float4 lq = *(const float4*)(lights + (size_t)s * 8 + 4);  // intensity, attenuation, ambient, 0
    float Dx = lp.x, Dy = lp.y, Dz = lp.z, att = 1.f;
    if (lp.w != 0.f) {  // a point light
      Dx = lp.x - Px;
      Dy = lp.y - Py;
      Dz = lp.z - Pz;
      att = 1.f / (1.f + lq.y * dot3(Dx, Dy, Dz, Dx, Dy, Dz));
    }
    const float dlen = sqrtf(dot3(Dx, Dy, Dz, Dx, Dy, Dz));
    if (dlen > 0.f) {
      Dx = Dx / dlen;
      Dy = Dy / dlen;
      Dz = Dz / dlen;
    }
    float Vx = -Px, Vy = -Py, Vz = -Pz;
    const float vlen = sqrtf(dot3(Vx, Vy, Vz, Vx, Vy, Vz));
    if (vlen > 0.f) {
      Vx = Vx / vlen;
      Vy = Vy / vlen;
      Vz = Vz / vlen;
    }
    const float nl = dot3(Nx, Ny, Nz, Dx, Dy, Dz);
    const float diffuse = fmaxf(0.f, nl);
    float specular = 0.f;
    if (diffuse > 0.f) {
      const float k2 = 2.f * nl;
      const float Rx = k2 * Nx - Dx, Ry = k2 * Ny - Dy, Rz = k2 * Nz - Dz;  // reflect(-L, N)
      specular = powf(fmaxf(0.f, dot3(Vx, Vy, Vz, Rx, Ry, Rz)), shininess[k]);
    }
    const float I = lq.x, ka = lq.z, sI = specular * I;
    const float r = (ka * c.x) * I + att * ((diffuse * c.x) * I + sI);
    const float g = (ka * c.y) * I + att * ((diffuse * c.y) * I + sI);
    const float b = (ka * c.z) * I + att * ((diffuse * c.z) * I + sI);
    return make_float4(b, g, r, 1.f);
  }
  __device__ __forceinline__ void store(size_t i, float4 v) const { color[i] = v; }
};

// ---- image blob ----
constexpr uint32_t kTagImage = 0x494D4731u;  // "IMG1": the noise's Philox stream, apart from dropout's

struct U8x3 {
  int b, g, r;
};

// Step 1: (uint8)min(max(255 c, 0), 255), truncated; NaN -> 0.
__device__ __forceinline__ int quantise(float c) { return (int)fminf(fmaxf(255.f * c, 0.f), 255.f); }

__device__ __forceinline__ int sat8(float x) { return (int)fminf(fmaxf(rintf(255.f * x), 0.f), 255.f); }

// Step 3: BGR -> HLS (8-bit), the jitter, HLS -> BGR (8-bit).
__device__ __forceinline__ U8x3 chromatic(U8x3 p, float d_h, float d_l, float d_s) {
  const float b = (float)p.b / 255.f, g = (float)p.g / 255.f, r = (float)p.r / 255.f;
  const float vmax = fmaxf(fmaxf(r, g), b), vmin = fminf(fminf(r, g), b);
  const float d = vmax - vmin;
  const float l = (vmax + vmin) * 0.5f;
  float h = 0.f, s = 0.f;
  if (d > 0.f) {
    s = l < 0.5f ? d / (vmax + vmin) : d / ((2.f - vmax) - vmin);
    if (vmax == r) {
      h = (60.f * (g - b)) / d;
    } else if (vmax == g) {
      h = (60.f * (b - r)) / d + 120.f;
    } else {
      h = (60.f * (r - g)) / d + 240.f;
    }
    if (h < 0.f) h = h + 360.f;
  }
  int H8 = (int)rintf(h * 0.5f);
  if (H8 >= 180) H8 -= 180;
  const int L8 = (int)rintf(255.f * l), S8 = (int)rintf(255.f * s);
  // the jitter: hue modulo 180, the others clipped; all truncated to 8 bits
  float th = (float)H8 + d_h;
  th = th - 180.f * floorf(th / 180.f);
  int Hn = (int)fminf(fmaxf(th, 0.f), 180.f);
  if (Hn >= 180) Hn -= 180;
  const int Ln = (int)fminf(fmaxf((float)L8 + d_l, 0.f), 255.f);
  const int Sn = (int)fminf(fmaxf((float)S8 + d_s, 0.f), 255.f);
  // back
  const float l2 = (float)Ln / 255.f, s2 = (float)Sn / 255.f;
  float ob = l2, og = l2, orr = l2;
  if (Sn > 0) {
    const float p2 = l2 <= 0.5f ? l2 * (1.f + s2) : (l2 + s2) - l2 * s2;
    const float p1 = 2.f * l2 - p2;
    const int sector = Hn / 30;
    const float f = (float)(Hn - 30 * sector) / 30.f;
    const float up = p1 + (p2 - p1) * f, down = p1 + (p2 - p1) * (1.f - f);
    switch (sector) {
      case 0: orr = p2; og = up; ob = p1; break;
      case 1: orr = down; og = p2; ob = p1; break;
      case 2: orr = p1; og = p2; ob = up; break;
      case 3: orr = p1; og = down; ob = p2; break;
      case 4: orr = up; og = p1; ob = p2; break;
      default: orr = p2; og = p1; ob = down; break;
    }
  }
  return U8x3{sat8(ob), sat8(og), sat8(orr)};
}

// Step 4's deviate of pixel `pix` of global image `gi`.
__device__ __forceinline__ float deviate(uint32_t pix, uint64_t gi, uint32_t k0, uint32_t k1) {
  const pcnn_philox::U4 o =
      pcnn_philox::philox4x32_10(pcnn_philox::U4{pix, 0u, (uint32_t)gi, (uint32_t)(gi >> 32)}, k0, k1);
  const double u1 = ((double)o.x + 1.0) * (1.0 / 4294967296.0);  // (0, 1]
  const double u2 = (double)o.y * (1.0 / 4294967296.0);          // [0, 1)
  return (float)(sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2));
}

__global__ void __launch_bounds__(256)
    k_image_blob(const float4* __restrict__ color, const uint8_t* __restrict__ backgrounds, int N_bg,
                 const int32_t* __restrict__ bg_index, const float4* __restrict__ jitter,
                 const float* __restrict__ pixel_means, uint32_t k0, uint32_t k1, uint64_t image_offset, size_t total,
                 uint32_t hw, int flags, float* __restrict__ blob) {
  const size_t i0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i0 >= total) return;
  const float mb = pixel_means[0], mg = pixel_means[1], mr = pixel_means[2];
  float ob[4], og[4], orr[4];
  size_t img = i0 / hw;
  uint32_t pix = (uint32_t)(i0 - img * hw);
  const int n = total - i0 < 4 ? (int)(total - i0) : 4;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    ob[j] = og[j] = orr[j] = 0.f;
    if (j < n) {
      const float4 c = color[i0 + j];  // b, g, r, alpha
      U8x3 p = {quantise(c.x), quantise(c.y), quantise(c.z)};
      if (c.w == 0.f) {
        const int bi = bg_index[img];
        p = U8x3{0, 0, 0};
        if (bi >= 0 && bi < N_bg) {
          const uint8_t* q = backgrounds + ((size_t)bi * hw + pix) * 3;
          p = U8x3{(int)q[0], (int)q[1], (int)q[2]};
        }
      }
      const float4 jt = jitter[img];  // d_h, d_l, d_s, sigma
      if (flags & PCNN_IMAGE_CHROMATIC) p = chromatic(p, jt.x, jt.y, jt.z);
      float vb = (float)p.b, vg = (float)p.g, vr = (float)p.r;
      if (flags & PCNN_IMAGE_NOISE) {
        const float e = jt.w * deviate(pix, image_offset + img, k0, k1);
        vb = fminf(fmaxf(vb + e, 0.f), 255.f);
        vg = fminf(fmaxf(vg + e, 0.f), 255.f);
        vr = fminf(fmaxf(vr + e, 0.f), 255.f);
      }
      ob[j] = vb - mb;
      og[j] = vg - mg;
      orr[j] = vr - mr;
      if (++pix == hw) {
        pix = 0;
        ++img;
      }
    }
  }
  if (!(flags & PCNN_IMAGE_NCHW)) {
    float* o = blob + i0 * 3;
    if (n == 4) {
      *(float4*)(o + 0) = make_float4(ob[0], og[0], orr[0], ob[1]);
      *(float4*)(o + 4) = make_float4(og[1], orr[1], ob[2], og[2]);
      *(float4*)(o + 8) = make_float4(orr[2], ob[3], og[3], orr[3]);
    } else {
      for (int j = 0; j < n; ++j) {
        o[3 * j + 0] = ob[j];
        o[3 * j + 1] = og[j];
        o[3 * j + 2] = orr[j];
      }
    }
  } else {
    img = i0 / hw;
    pix = (uint32_t)(i0 - img * hw);
    if (n == 4 && (hw & 3u) == 0u) {  // the four pixels lie in one image, 16-byte aligned in each plane
      float* o = blob + img * 3 * hw + pix;
      *(float4*)(o) = make_float4(ob[0], ob[1], ob[2], ob[3]);
      *(float4*)(o + hw) = make_float4(og[0], og[1], og[2], og[3]);
      *(float4*)(o + 2 * (size_t)hw) = make_float4(orr[0], orr[1], orr[2], orr[3]);
    } else {
      for (int j = 0; j < n; ++j) {
        float* o = blob + img * 3 * hw + pix;
        o[0] = ob[j];
        o[hw] = og[j];
        o[2 * (size_t)hw] = orr[j];
        if (++pix == hw) {
          pix = 0;
          ++img;
        }
      }
    }
  }
}

}  // namespace
}  // namespace pcnn

extern "C" size_t pcnn_render_scenes_lit_workspace_size(int S, int K, int H, int W, int V_total, int F_max) {
  if (!pcnn::scene_dims_ok(S, K, H, W, V_total, F_max)) return 0;
  return pcnn::carve_scene(nullptr, S, K, H, W, V_total, F_max).bytes;
}

extern "C" int pcnn_render_scenes_lit(const float* vertices, const float* normals, const float* colors,
                                      const int32_t* faces, const int32_t* vert_offset, const int32_t* face_offset,
                                      int M, int V_total, int F_total, int F_max, const int32_t* mesh_index,
                                      const int32_t* class_id, const float* poses, const float* shininess, int K,
                                      const int32_t* scene_offset, const float* lights, int S, int H, int W, float fx,
                                      float fy, float px, float py, float znear, float zfar, int32_t* label,
                                      float* depth, float* vertmap, float* vertex3, int32_t* inst_id,
                                      int32_t* visible, float* centers, float* color, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  using namespace pcnn;
  PCNN_REQUIRE(vertices && normals && faces && vert_offset && face_offset && mesh_index && class_id && poses);
  PCNN_REQUIRE(scene_offset && label && depth && vertmap && vertex3 && visible && centers && workspace);
  PCNN_REQUIRE(colors && shininess && lights && color);
  PCNN_REQUIRE(M > 0 && F_total > 0 && F_max <= F_total && scene_dims_ok(S, K, H, W, V_total, F_max));
  PCNN_REQUIRE(znear > 0.f && zfar >= znear);  // Z > 0: the depth's bits order like its value
  PCNN_REQUIRE(((uintptr_t)label & 3) == 0 && ((uintptr_t)depth & 3) == 0 && ((uintptr_t)vertmap & 3) == 0 &&
               ((uintptr_t)vertex3 & 3) == 0 && ((uintptr_t)inst_id & 3) == 0 && ((uintptr_t)visible & 3) == 0 &&
               ((uintptr_t)centers & 7) == 0 && ((uintptr_t)workspace & 15) == 0);
  PCNN_REQUIRE(((uintptr_t)colors & 3) == 0 && ((uintptr_t)shininess & 3) == 0 && ((uintptr_t)lights & 15) == 0 &&
               ((uintptr_t)color & 15) == 0);
  const SceneWs ws = carve_scene(workspace, S, K, H, W, V_total, F_max);
  if (workspace_bytes < ws.bytes) return PCNN_ECAPACITY;
  return run_scene_passes(vertices, normals, faces, vert_offset, face_offset, M, V_total, F_total, F_max, mesh_index,
                          class_id, poses, K, scene_offset, S, H, W, fx, fy, px, py, znear, zfar, label, depth, vertmap,
                          vertex3, inst_id, visible, centers, ws, Phong{colors, shininess, lights, (float4*)color},
                          (hipStream_t)stream);
}

extern "C" int pcnn_image_blob(const float* color, const uint8_t* backgrounds, int N_bg, const int32_t* bg_index,
                               const float* jitter, const float* pixel_means, uint64_t seed, int64_t image_offset,
                               int B, int H, int W, int flags, float* blob, void* stream) {
  using namespace pcnn;
  PCNN_REQUIRE(color && bg_index && jitter && pixel_means && blob && (backgrounds || N_bg == 0));
  PCNN_REQUIRE(B > 0 && H > 0 && W > 0 && N_bg >= 0 && B <= (1 << 20) && (size_t)H * W <= 0x7fffffffull);
  PCNN_REQUIRE((flags & ~(PCNN_IMAGE_CHROMATIC | PCNN_IMAGE_NOISE | PCNN_IMAGE_NCHW)) == 0);
  PCNN_REQUIRE(((uintptr_t)color & 15) == 0 && ((uintptr_t)blob & 15) == 0 && ((uintptr_t)jitter & 15) == 0 &&
               ((uintptr_t)bg_index & 3) == 0 && ((uintptr_t)pixel_means & 3) == 0);
  const size_t total = (size_t)B * H * W;
  PCNN_REQUIRE(total <= (1ull << 38));
  k_image_blob<<<dim3((unsigned)(((total + 3) / 4 + 255) / 256)), 256, 0, (hipStream_t)stream>>>(
      (const float4*)color, backgrounds, N_bg, bg_index, (const float4*)jitter, pixel_means,
      (uint32_t)seed ^ kTagImage, (uint32_t)(seed >> 32), (uint64_t)image_offset, total, (uint32_t)((size_t)H * W),
      flags, blob);
  PCNN_CHECK_LAUNCH();
  return PCNN_OK;
}
