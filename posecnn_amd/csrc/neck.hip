// The embedding neck of vgg16_convs (include/posecnn_neck.h): what stands
// between conv4_3 / conv5_3 and the two heads (lib/networks/vgg16_convs.py:
// 128-137 and :152-161) around its two 1x1 convs, which are GEMMs
// (z4 = x4 W4, z5 = x5 W5, N = U + V columns: the score branch's U with ReLU,
// then the vertex branch's V without):
//
//     t4 = act(z4 + b4)                     score_conv4(_vertex)
//     t5 = act(z5 + b5)                     score_conv5(_vertex)
//     up = stride-2 bilinear taps of t5     upscore_conv5(_vertex)
//     a  = t4 + up                          add_score(_vertex)
//     out = (a / keep_prob) * keep          dropout(_vertex), tf.nn.dropout
//
//  k_neck_fwd   a thread per (pixel, channel quad): one 16-byte load of z4,
//               the four taps of z5 (a quarter of z4's size: it stays in
//               cache), one Philox block for the quad's four keep bits, one
//               16-byte store into the branch's own contiguous map and one
//               4-byte store of the keep bytes.  Consecutive lanes walk the
//               channels, then the pixels: z4 is one contiguous stream.
//  k_neck_bwd   a thread per (low-res pixel, channel quad) gathers the 4 x 4
//               window of g = (d / keep_prob) * keep that taps the pixel (the
//               transpose of the forward's taps, row-major, a fixed order) for
//               dz5, and writes dz4 for the 2 x 2 pixels of the window that no
//               other low-res pixel owns.  A thread's column quad is the same
//               for all its pixels, so the bias sums are per-thread registers;
//               the block's thread rows are added in row order through LDS
//               (16 bytes per lane, lane-linear: no bank conflict) into one
//               partial per block.
//  k_neck_fold  adds the partials in block order (kFoldWaves contiguous groups,
//               each in order, then the groups in order).
//
// No floating-point atomics, every order fixed: two runs give the same bits.
// float32 throughout, every op rounded separately.
#include "pcnn_common.h"
#include "pcnn_philox.h"
#include "../../include/posecnn_neck.h"

namespace {

using pcnn::lane_id;
using pcnn_philox::keep_quad;

constexpr int kThreads = 256;
constexpr int kFoldWaves = 16;
constexpr int kMaxBlocks = 2048;  // forward: grid-stride beyond this
constexpr int kPix = 4;           // low-res pixels of a backward thread

// The stride-2 taps of output coordinate y along an axis of low-res extent n (upscore.hip tap_of at s = 2).
struct Tap {
  int i1;        // i0 = i1 - 1
  float w0, w1;  // weights of i0, i1
  bool p0, p1;   // present
};

__device__ __forceinline__ Tap tap2(int y, int n) {
  const int t = y + 1;
  Tap r;
  r.i1 = t >> 1;
  const int k = t & 1;
  r.w1 = (float)(2 * k + 1) * 0.25f;
  r.w0 = (float)(3 - 2 * k) * 0.25f;
  r.p0 = r.i1 >= 1;
  r.p1 = r.i1 < n;
  return r;
}

// Weight of window position u in [0, 4) of a low-res pixel: rows (columns) 2 i - 1 + u.
__device__ __forceinline__ float window_weight2(int u) { return (u == 0 || u == 3) ? 0.25f : 0.75f; }

// The pinned sum of upscore.hip's generic forward: ((t00 + t01) + t10) + t11 over the present taps.
struct Acc {
  float v;
  bool have;
  __device__ __forceinline__ void add(bool present, float x, float wgt) {
    if (present) {
      const float t = x * wgt;
      v = have ? v + t : t;
      have = true;
    }
  }
};

__device__ __forceinline__ float relu_if(bool relu, float v) { return relu ? (v > 0.f ? v : 0.f) : v; }

__device__ __forceinline__ void load4(float (&o)[4], const float* p) {
  const float4 v = *(const float4*)p;
  o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w;
}

__device__ __forceinline__ void store4(float* p, const float (&v)[4]) {
  *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
}

// z4 (M4, N), z5 (M5, N); out_s (M4, U), out_v (M4, V), keep_s, keep_v likewise (NULL at keep == 1).
__global__ void __launch_bounds__(kThreads) k_neck_fwd(const float* __restrict__ z4, const float* __restrict__ z5,
                                                       const float* __restrict__ b4, const float* __restrict__ b5,
                                                       int B, int h, int w, int U, int V, float keep, uint32_t k0,
                                                       uint32_t k1, const int64_t* __restrict__ step_dev,
                                                       uint32_t sid_s, uint32_t sid_v, float* __restrict__ out_s,
                                                       float* __restrict__ out_v, uint8_t* __restrict__ keep_s,
                                                       uint8_t* __restrict__ keep_v) {
  const int N = U + V, nq = N >> 2, uq = U >> 2, vq = V >> 2;
  const int hl = h >> 1, wl = w >> 1;
  const int total = B * h * w * nq;  // < 2^29 (checked by the host)
  const bool drop = keep != 1.f;
  const uint32_t step = (drop && step_dev) ? (uint32_t)(uint64_t)*step_dev : 0u;
  for (int e = blockIdx.x * kThreads + threadIdx.x; e < total; e += gridDim.x * kThreads) {
    const int p = e / nq, cq = e - p * nq;
    const int x = p % w;
    const int t = p / w;
    const int y = t % h;
    const int b = t / h;
    const int c = cq * 4;
    const bool sc = cq < uq;  // the score branch: ReLU
    float bb4[4], bb5[4], t4[4];
    load4(bb4, b4 + c);
    load4(bb5, b5 + c);
    load4(t4, z4 + (size_t)e * 4);
    const Tap r = tap2(y, hl), cl = tap2(x, wl);
    float tp[4][4];  // [tap 00, 01, 10, 11][channel]
#pragma unroll
    for (int a = 0; a < 4; a++) {
      const bool pr = (a >> 1 ? r.p1 : r.p0) && (a & 1 ? cl.p1 : cl.p0);
      const int i = r.i1 - 1 + (a >> 1), j = cl.i1 - 1 + (a & 1);
      if (pr) {
        load4(tp[a], z5 + ((size_t)(b * hl + i) * wl + j) * N + c);
      } else {
#pragma unroll
        for (int v = 0; v < 4; v++) tp[a][v] = 0.f;
      }
    }
    float o[4];
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const float a4 = relu_if(sc, t4[v] + bb4[v]);
      Acc up = {0.f, false};
      up.add(r.p0 && cl.p0, relu_if(sc, tp[0][v] + bb5[v]), r.w0 * cl.w0);
      up.add(r.p0 && cl.p1, relu_if(sc, tp[1][v] + bb5[v]), r.w0 * cl.w1);
      up.add(r.p1 && cl.p0, relu_if(sc, tp[2][v] + bb5[v]), r.w1 * cl.w0);
      up.add(r.p1 && cl.p1, relu_if(sc, tp[3][v] + bb5[v]), r.w1 * cl.w1);
      o[v] = a4 + up.v;
    }
    const int ld = sc ? U : V, co = sc ? c : c - U;
    const size_t at = (size_t)p * ld + co;
    if (drop) {
      // element quad of a dense (M4, U) or (M4, V) mask, as pcnn_dropout_mask counts them
      const uint64_t quad = (uint64_t)p * (uint64_t)(sc ? uq : vq) + (uint64_t)(co >> 2);
      const uint32_t bits = keep_quad(quad, k0, k1, sc ? sid_s : sid_v, step, keep);
#pragma unroll
      for (int v = 0; v < 4; v++) o[v] = (o[v] / keep) * (float)((bits >> (8 * v)) & 1u);
      *(uint32_t*)((sc ? keep_s : keep_v) + at) = bits;
    }
    store4((sc ? out_s : out_v) + at, o);
  }
}

// The thread grid of a backward block: CQ column quads x R rows of threads (CQ R <= kThreads); a block owns
// PB = R kPix consecutive low-res pixels, thread row r the pixels r, r + R, ...; blockIdx.y: the column chunk.
struct BwdTiling {
  int CQ, ncc, R, PB, nblk;
};

// part: [nblk][2 N] bias partials, the block's column sums of dz4 then of dz5.
__global__ void __launch_bounds__(kThreads) k_neck_bwd(const float* __restrict__ d_s, const float* __restrict__ d_v,
                                                       const uint8_t* __restrict__ keep_s,
                                                       const uint8_t* __restrict__ keep_v,
                                                       const float* __restrict__ z4, const float* __restrict__ z5,
                                                       const float* __restrict__ b4, const float* __restrict__ b5,
                                                       int B, int h, int w, int U, int V, float keep, BwdTiling tl,
                                                       float* __restrict__ dz4, float* __restrict__ dz5,
                                                       float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float red[2][kThreads][4];
  const int N = U + V, nq = N >> 2, uq = U >> 2;
  const int hl = h >> 1, wl = w >> 1;
  const int M5 = B * hl * wl;
  const bool drop = keep != 1.f;
  const int tid = threadIdx.x;
  const int r = tid / tl.CQ;
  const int cq = blockIdx.y * tl.CQ + (tid - r * tl.CQ);
  const int c = cq * 4;
  float s4[4] = {0.f, 0.f, 0.f, 0.f}, s5[4] = {0.f, 0.f, 0.f, 0.f};
  if (r < tl.R && cq < nq) {
    const bool sc = cq < uq;
    const float* __restrict__ d = sc ? d_s : d_v;
    const uint8_t* __restrict__ kp = sc ? keep_s : keep_v;
    const int ld = sc ? U : V, co = sc ? c : c - U;
    float bb4[4], bb5[4];
    load4(bb4, b4 + c);
    load4(bb5, b5 + c);
    for (int k = 0; k < kPix; k++) {
      const int q = blockIdx.x * tl.PB + k * tl.R + r;
      if (q >= M5) break;
      const int j = q % wl;
      const int t = q / wl;
      const int i = t % hl;
      const int b = t / hl;
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int yy = 2 * i - 1 + u;
        if (yy < 0 || yy >= h) continue;
#pragma unroll
        for (int v = 0; v < 4; v++) {
          const int xx = 2 * j - 1 + v;
          if (xx < 0 || xx >= w) continue;
          const size_t p = (size_t)(b * h + yy) * w + xx;
          float g[4];
          load4(g, d + p * ld + co);
          if (drop) {
            const uint32_t bits = *(const uint32_t*)(kp + p * ld + co);
#pragma unroll
            for (int e = 0; e < 4; e++) g[e] = (g[e] / keep) * (float)((bits >> (8 * e)) & 1u);
          }
          const float wgt = window_weight2(u) * window_weight2(v);
#pragma unroll
          for (int e = 0; e < 4; e++) acc[e] = acc[e] + wgt * g[e];
          if ((u == 1 || u == 2) && (v == 1 || v == 2)) {  // pixel (2 i + u - 1, 2 j + v - 1): this thread's alone
            if (sc) {
              float z[4];
              load4(z, z4 + p * N + c);
#pragma unroll
              for (int e = 0; e < 4; e++) g[e] = z[e] + bb4[e] > 0.f ? g[e] : 0.f;
            }
            store4(dz4 + p * N + c, g);
#pragma unroll
            for (int e = 0; e < 4; e++) s4[e] = s4[e] + g[e];
          }
        }
      }
      if (sc) {
        float z[4];
        load4(z, z5 + (size_t)q * N + c);
#pragma unroll
        for (int e = 0; e < 4; e++) acc[e] = z[e] + bb5[e] > 0.f ? acc[e] : 0.f;
      }
      store4(dz5 + (size_t)q * N + c, acc);
#pragma unroll
      for (int e = 0; e < 4; e++) s5[e] = s5[e] + acc[e];
    }
  }
  store4(red[0][tid], s4);
  store4(red[1][tid], s5);
  __syncthreads();
  if (r == 0 && cq < nq) {
#pragma unroll
    for (int a = 0; a < 2; a++) {
      float s[4];
      load4(s, red[a][tid]);
      for (int rr = 1; rr < tl.R; rr++) {
        float o[4];
        load4(o, red[a][rr * tl.CQ + tid]);
#pragma unroll
        for (int e = 0; e < 4; e++) s[e] = s[e] + o[e];
      }
      store4(part + (size_t)blockIdx.x * 2 * N + a * N + c, s);
    }
  }
}

// out[e] = the P partials' element e added in block order: one element per lane, a contiguous group of the
// blocks per wave, then the groups in order.  Elements [0, N) go to db4, [N, 2 N) to db5.
__global__ void __launch_bounds__(kFoldWaves * 64) k_neck_fold(const float* __restrict__ part, int P, int N,
                                                               float* __restrict__ db4, float* __restrict__ db5) {
  __shared__ float red[kFoldWaves][64];
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  const int n = 2 * N;
  const int e = blockIdx.x * 64 + lane;
  const int per = (P + kFoldWaves - 1) / kFoldWaves;
  const int p0 = wave * per, p1 = (p0 + per < P) ? p0 + per : P;
  float s = 0.f;
  if (e < n) {
#pragma unroll 8
    for (int p = p0; p < p1; p++) s = s + part[(size_t)p * n + e];
  }
  red[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && e < n) {
    float v = red[0][lane];
    for (int wv = 1; wv < kFoldWaves; wv++) v = v + red[wv][lane];
    if (e < N) db4[e] = v;
    else db5[e - N] = v;
  }
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

inline bool dims_ok(int B, int h, int w, int U, int V, float keep_prob) {
  if (B <= 0 || h <= 0 || w <= 0 || (h & 1) || (w & 1)) return false;
  if (U < 0 || V < 0 || (U & 3) || (V & 3) || (long)U + V <= 0 || (long)U + V >= (1l << 31)) return false;
  if (!(keep_prob > 0.f && keep_prob <= 1.f)) return false;
  return (long)B * h * w * ((long)U + V) < (1l << 31);  // element counts, the largest map's
}

inline BwdTiling bwd_tiling(int B, int h, int w, int U, int V) {
  BwdTiling t;
  const int nq = (U + V) >> 2;
  t.CQ = nq < kThreads ? nq : kThreads;
  t.ncc = (nq + t.CQ - 1) / t.CQ;
  t.R = kThreads / t.CQ;
  t.PB = t.R * kPix;
  const long M5 = (long)B * (h >> 1) * (w >> 1);
  t.nblk = (int)((M5 + t.PB - 1) / t.PB);
  return t;
}

}  // namespace

// 1: pcnn_neck_fwd, pcnn_neck_bwd_workspace_size, pcnn_neck_bwd
extern "C" int pcnn_neck_abi_version(void) { return 1; }

extern "C" int pcnn_neck_fwd(const float* z4, const float* z5, const float* b4, const float* b5, int B, int h, int w,
                             int U, int V, float keep_prob, uint64_t seed, const int64_t* step_dev,
                             int stream_id_score, int stream_id_vertex, float* add_score, float* add_score_vertex,
                             uint8_t* keep_score, uint8_t* keep_vertex, void* stream) {
  PCNN_REQUIRE(dims_ok(B, h, w, U, V, keep_prob));
  PCNN_REQUIRE(z4 && z5 && b4 && b5 && (add_score || U == 0) && (add_score_vertex || V == 0));
  PCNN_REQUIRE(aligned(z4, 16) && aligned(z5, 16) && aligned(b4, 16) && aligned(b5, 16) && aligned(add_score, 16) &&
               aligned(add_score_vertex, 16));
  if (keep_prob != 1.f) {
    PCNN_REQUIRE((keep_score || U == 0) && (keep_vertex || V == 0) && aligned(keep_score, 4) &&
                 aligned(keep_vertex, 4) && aligned(step_dev, 8) && stream_id_score >= 0 && stream_id_vertex >= 0);
  }
  const long quads = (long)B * h * w * ((U + V) / 4);
  long grid = (quads + kThreads - 1) / kThreads;
  if (grid > kMaxBlocks) grid = kMaxBlocks;
  pcnn::launch_last(k_neck_fwd, dim3((unsigned)grid), dim3(kThreads), 0, (hipStream_t)stream, z4, z5, b4, b5, B, h, w,
                    U, V, keep_prob, (uint32_t)seed, (uint32_t)(seed >> 32), step_dev, (uint32_t)stream_id_score,
                    (uint32_t)stream_id_vertex, add_score, add_score_vertex, keep_score, keep_vertex);
  PCNN_CHECK_LAUNCH();
  return PCNN_OK;
}

extern "C" size_t pcnn_neck_bwd_workspace_size(int B, int h, int w, int U, int V) {
  if (!dims_ok(B, h, w, U, V, 1.f)) return 0;
  const BwdTiling tl = bwd_tiling(B, h, w, U, V);
  return pcnn::align_up((size_t)tl.nblk * 2 * (U + V) * sizeof(float), 256);
}

extern "C" int pcnn_neck_bwd(const float* d_add_score, const float* d_add_score_vertex, const uint8_t* keep_score,
                             const uint8_t* keep_vertex, const float* z4, const float* z5, const float* b4,
                             const float* b5, int B, int h, int w, int U, int V, float keep_prob, float* dz4,
                             float* dz5, float* db4, float* db5, void* workspace, size_t workspace_bytes,
                             void* stream) {
  PCNN_REQUIRE(dims_ok(B, h, w, U, V, keep_prob));
  PCNN_REQUIRE((d_add_score || U == 0) && (d_add_score_vertex || V == 0) && z4 && z5 && b4 && b5 && dz4 && dz5 &&
               db4 && db5 && workspace);
  PCNN_REQUIRE(aligned(d_add_score, 16) && aligned(d_add_score_vertex, 16) && aligned(z4, 16) && aligned(z5, 16) &&
               aligned(b4, 16) && aligned(b5, 16) && aligned(dz4, 16) && aligned(dz5, 16) && aligned(db4, 4) &&
               aligned(db5, 4) && aligned(workspace, 16));
  if (keep_prob != 1.f) {
    PCNN_REQUIRE((keep_score || U == 0) && (keep_vertex || V == 0) && aligned(keep_score, 4) &&
                 aligned(keep_vertex, 4));
  }
  if (workspace_bytes < pcnn_neck_bwd_workspace_size(B, h, w, U, V)) return PCNN_ECAPACITY;
  const BwdTiling tl = bwd_tiling(B, h, w, U, V);
  const int N = U + V;
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)workspace;
  hipLaunchKernelGGL(k_neck_bwd, dim3(tl.nblk, tl.ncc), dim3(kThreads), 0, st, d_add_score, d_add_score_vertex,
                     keep_score, keep_vertex, z4, z5, b4, b5, B, h, w, U, V, keep_prob, tl, dz4, dz5, part);
  PCNN_CHECK_LAUNCH();
  pcnn::launch_last(k_neck_fold, dim3((2 * N + 63) / 64), dim3(kFoldWaves * 64), 0, st, (const float*)part, tl.nblk,
                    N, db4, db5);
  PCNN_CHECK_LAUNCH();
  return PCNN_OK;
}
