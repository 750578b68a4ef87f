// The two dense-map terms of the training objective (lib/fcn/train.py:489-515),
// forward and backward:
//
//  pcnn_seg_loss       log-softmax / softmax / argmax / Hardlabel / weighted
//                      cross entropy of the segmentation head fused over the
//                      (B,H,W,C) score map (vgg16_convs.py:140-149,
//                      network.py:475-506, train.py:455-465), and its gradient.
//  pcnn_cross_entropy  loss_cross_entropy_single_frame (train.py:455-465) on
//                      already-formed (n_pix,C) maps.
//  pcnn_vertex_loss    smooth_l1_loss_vertex (train.py:565-574) on the
//                      (B,H,W,3C) blobs.
//  pcnn_vertex_loss_compact  the same loss from label + the (B,H,W,3) vote
//                      target, reading only the 3 live channels of a pixel.
//
// Every op is forward-reduce -> k_loss_final -> (optional) gradient: the
// normaliser (hard-pixel count, weight sum) is known only after a full pass.
// (The dense vertex op sums the weights alone first when the gradient is
// wanted, so that the loss and the gradient share one pass over the blobs.)
// Reductions have a fixed order (lane, butterfly over the wave, the four waves
// of a workgroup in order, the workgroups' partials in the workspace summed in
// a fixed order by one workgroup): no floating-point atomics, so two runs give
// the same bits.  Loss sums are double; per-element arithmetic is float32 with
// every op rounded separately.
#include "pcnn_common.h"
#include <math.h>

namespace {

using pcnn::lane_id;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
// Classes staged through LDS: 4 waves * 64 rows * (C | 1) floats stays under
// the 64 KiB a kernel gets without opting in to more.
constexpr int kSegStagedMaxC = 63;
constexpr int kFlatMaxBlocks = 2048;

struct SegOut {
  float* log_prob;
  float* prob;
  int32_t* label;
  float* weight;
};

struct SmoothL1 {
  float c_inv, c_half, c_off, c_s2;  // 1/sigma^2, sigma^2/2, 0.5/sigma^2, sigma^2
};

// Row stride of the staged rows: odd, so that the 64 lanes' reads of one
// column fall on distinct banks.
__host__ __device__ inline int padded(int C) { return C | 1; }

// The wave's npx rows of C floats, contiguous at src, into LDS rows of stride
// Cp.  A whole group (64 rows) starts 16-byte aligned and is read as float4.
__device__ __forceinline__ void stage_in(const float* __restrict__ src, float* stage, int npx, int C, int Cp,
                                         float rcpC) {
  const int lane = lane_id();
  const int n = npx * C;
  if (npx == 64) {
    const float4* s4 = (const float4*)src;
    for (int i = lane; i < n / 4; i += 64) {
      const float4 v = s4[i];
      const float x[4] = {v.x, v.y, v.z, v.w};
      const int e = 4 * i;
      int r = (int)(((float)e + 0.5f) * rcpC);  // e / C: e < 64 C, the quotient is off an integer by >= 0.5 / C
      int c = e - r * C;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        stage[r * Cp + c] = x[j];
        if (++c == C) { c = 0; ++r; }
      }
    }
  } else {
    for (int i = lane; i < n; i += 64) {
      const int r = i / C;
      stage[r * Cp + (i - r * C)] = src[i];
    }
  }
}

__device__ __forceinline__ void stream_out(float* __restrict__ dst, const float* stage, int npx, int C, int Cp,
                                           float rcpC) {
  const int lane = lane_id();
  const int n = npx * C;
  if (npx == 64) {
    float4* d4 = (float4*)dst;
    for (int i = lane; i < n / 4; i += 64) {
      const int e = 4 * i;
      int r = (int)(((float)e + 0.5f) * rcpC);
      int c = e - r * C;
      float x[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        x[j] = stage[r * Cp + c];
        if (++c == C) { c = 0; ++r; }
      }
      d4[i] = make_float4(x[0], x[1], x[2], x[3]);
    }
  } else {
    for (int i = lane; i < n; i += 64) {
      const int r = i / C;
      dst[i] = stage[r * Cp + (i - r * C)];
    }
  }
}

// argmax_classes (hough_common.h: the first maximum, a NaN at its first occurrence) fed one value at a time
struct ArgmaxScan {
  float bv;
  int best;
  bool done;
  __device__ __forceinline__ void init(float v) { bv = v; best = 0; done = v != v; }
  __device__ __forceinline__ void step(float v, int c) {
    if (done) return;
    if (v != v) { best = c; done = true; }
    else if (v > bv) { bv = v; best = c; }
  }
};

// hard_label_at (label_producer.hip) for the pixel as a whole: p0 = prob_normalized[0]
__device__ __forceinline__ bool is_hard(int g, int C, float p0, float threshold) {
  return g >= 0 && g < C && (g > 0 || p0 < threshold);
}

// (a, b) summed over the workgroup in a fixed order -> partials[blockIdx.x]
__device__ __forceinline__ void block_partial(double a, double b, double2* __restrict__ partials) {
  __shared__ double2 red[kWaves];
  a = pcnn::wave_sum(a);
  b = pcnn::wave_sum(b);
  if (lane_id() == 0) red[threadIdx.x >> 6] = make_double2(a, b);
  __syncthreads();
  if (threadIdx.x == 0) {
    double sa = red[0].x, sb = red[0].y;
    for (int w = 1; w < kWaves; w++) { sa += red[w].x; sb += red[w].y; }
    partials[blockIdx.x] = make_double2(sa, sb);
  }
}

// loss = (float)(A / (wmul * Bsum + 1e-10)), inv = grad_scale / ((float)(wmul * Bsum) + 1e-10f)
__global__ void __launch_bounds__(kThreads) k_loss_final(const double2* __restrict__ partials, int nb, double wmul,
                                                         float grad_scale, float* __restrict__ loss,
                                                         float* __restrict__ fin) {
  __shared__ double2 red[kWaves];
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < nb; i += kThreads) {
    const double2 v = partials[i];
    a += v.x;
    b += v.y;
  }
  a = pcnn::wave_sum(a);
  b = pcnn::wave_sum(b);
  if (lane_id() == 0) red[threadIdx.x >> 6] = make_double2(a, b);
  __syncthreads();
  if (threadIdx.x == 0) {
    double sa = red[0].x, sb = red[0].y;
    for (int w = 1; w < kWaves; w++) { sa += red[w].x; sb += red[w].y; }
    const double wsum = wmul * sb;
    loss[0] = (float)(sa / (wsum + 1e-10));
    fin[0] = grad_scale / ((float)wsum + 1e-10f);
  }
}

// ---------------------------------------------------------------------------
// Segmentation head.  One lane per pixel, one 64-pixel group per wave.

// Forward.  Staged rows are overwritten in place: scores -> e_c -> p_c.
__global__ void __launch_bounds__(kThreads) k_seg_fwd(const float* __restrict__ score, const int32_t* __restrict__ gt,
                                                      int n_pix, int C, float threshold, SegOut o,
                                                      float2* __restrict__ ms, double2* __restrict__ partials) {
  extern __shared__ __attribute__((aligned(16))) float stage_all[];
  const int lane = lane_id();
  const int p0 = blockIdx.x * kThreads + (threadIdx.x & ~63);
  const int p = p0 + lane;
  const bool live = p < n_pix;
  const int g = live ? gt[p] : -1;
  const bool valid = g >= 0 && g < C;
  const bool want_p = o.label || o.prob;
  float m = 0.f, s = 1.f, logs = 0.f, sg = 0.f;
  bool hard = false;
  if (C <= kSegStagedMaxC) {  // uniform
    const int Cp = padded(C);
    const float rcpC = 1.f / (float)C;
    float* stage = stage_all + (threadIdx.x >> 6) * 64 * Cp;
    float* row = stage + lane * Cp;
    const int npx = n_pix - p0 < 64 ? (n_pix - p0 > 0 ? n_pix - p0 : 0) : 64;
    const size_t goff = (size_t)p0 * C;
    stage_in(score + goff, stage, npx, C, Cp, rcpC);
    __syncthreads();
    if (live) {
      m = row[0];
      for (int c = 1; c < C; c++) { const float x = row[c]; m = x > m ? x : m; }
      if (valid) sg = row[g];
      float e = expf(row[0] - m);
      row[0] = e;
      s = e;
      for (int c = 1; c < C; c++) {
        e = expf(row[c] - m);
        row[c] = e;
        s = s + e;
      }
      logs = logf(s);
      const float pz = row[0] / s;
      hard = is_hard(g, C, pz, threshold);
      if (want_p) {
        ArgmaxScan am;
        am.init(pz);
        row[0] = pz;
        for (int c = 1; c < C; c++) {
          const float pc = row[c] / s;
          row[c] = pc;
          am.step(pc, c);
        }
        if (o.label) o.label[p] = am.best;
      }
    }
    __syncthreads();
    if (o.prob) stream_out(o.prob + goff, stage, npx, C, Cp, rcpC);
    if (o.weight) {
      __syncthreads();
      if (live)
        for (int c = 0; c < C; c++) row[c] = (hard && c == g) ? 1.f : 0.f;
      __syncthreads();
      stream_out(o.weight + goff, stage, npx, C, Cp, rcpC);
    }
    if (o.log_prob) {
      __syncthreads();
      stage_in(score + goff, stage, npx, C, Cp, rcpC);
      __syncthreads();
      if (live)
        for (int c = 0; c < C; c++) row[c] = (row[c] - m) - logs;
      __syncthreads();
      stream_out(o.log_prob + goff, stage, npx, C, Cp, rcpC);
    }
  } else if (live) {  // rows read from global memory, outputs written straight out
    const size_t off = (size_t)p * C;
    const float* x = score + off;
    m = x[0];
    for (int c = 1; c < C; c++) { const float v = x[c]; m = v > m ? v : m; }
    if (valid) sg = x[g];
    const float ez = expf(x[0] - m);
    s = ez;
    for (int c = 1; c < C; c++) s = s + expf(x[c] - m);
    logs = logf(s);
    const float pz = ez / s;
    hard = is_hard(g, C, pz, threshold);
    if (want_p) {
      ArgmaxScan am;
      am.init(pz);
      if (o.prob) o.prob[off] = pz;
      for (int c = 1; c < C; c++) {
        const float pc = expf(x[c] - m) / s;
        if (o.prob) o.prob[off + c] = pc;
        am.step(pc, c);
      }
      if (o.label) o.label[p] = am.best;
    }
    if (o.weight)
      for (int c = 0; c < C; c++) o.weight[off + c] = (hard && c == g) ? 1.f : 0.f;
    if (o.log_prob)
      for (int c = 0; c < C; c++) o.log_prob[off + c] = (x[c] - m) - logs;
  }
  if (live) ms[p] = make_float2(m, s);
  const float nlp = -((sg - m) - logs);  // -log_prob[gt]
  block_partial(hard ? (double)nlp : 0.0, hard ? 1.0 : 0.0, partials);
}

// Backward: d_score_c = (p_c - [c == gt]) * inv on hard pixels, 0 elsewhere,
// with (m, s) of the forward pass.
__global__ void __launch_bounds__(kThreads) k_seg_bwd(const float* __restrict__ score, const int32_t* __restrict__ gt,
                                                      int n_pix, int C, float threshold,
                                                      const float2* __restrict__ ms, const float* __restrict__ fin,
                                                      float* __restrict__ d_score) {
  extern __shared__ __attribute__((aligned(16))) float stage_all[];
  const int lane = lane_id();
  const int p0 = blockIdx.x * kThreads + (threadIdx.x & ~63);
  const int p = p0 + lane;
  const bool live = p < n_pix;
  const int g = live ? gt[p] : -1;
  const float inv = fin[0];
  const float2 v = live ? ms[p] : make_float2(0.f, 1.f);
  const float m = v.x, s = v.y;
  if (C <= kSegStagedMaxC) {  // uniform
    const int Cp = padded(C);
    const float rcpC = 1.f / (float)C;
    float* stage = stage_all + (threadIdx.x >> 6) * 64 * Cp;
    float* row = stage + lane * Cp;
    const int npx = n_pix - p0 < 64 ? (n_pix - p0 > 0 ? n_pix - p0 : 0) : 64;
    const size_t goff = (size_t)p0 * C;
    stage_in(score + goff, stage, npx, C, Cp, rcpC);
    __syncthreads();
    if (live) {
      const float pz = expf(row[0] - m) / s;
      if (is_hard(g, C, pz, threshold)) {
        row[0] = (pz - (g == 0 ? 1.f : 0.f)) * inv;
        for (int c = 1; c < C; c++) {
          const float pc = expf(row[c] - m) / s;
          row[c] = (pc - (c == g ? 1.f : 0.f)) * inv;
        }
      } else {
        for (int c = 0; c < C; c++) row[c] = 0.f;
      }
    }
    __syncthreads();
    stream_out(d_score + goff, stage, npx, C, Cp, rcpC);
  } else if (live) {
    const size_t off = (size_t)p * C;
    const float* x = score + off;
    const float pz = expf(x[0] - m) / s;
    if (is_hard(g, C, pz, threshold)) {
      for (int c = 0; c < C; c++) {
        const float pc = expf(x[c] - m) / s;
        d_score[off + c] = (pc - (c == g ? 1.f : 0.f)) * inv;
      }
    } else {
      for (int c = 0; c < C; c++) d_score[off + c] = 0.f;
    }
  }
}

// ---------------------------------------------------------------------------
// Flat streams: float4 per thread over a persistent grid, the < 4 element tail
// by the first threads of workgroup 0.

__global__ void __launch_bounds__(kThreads) k_ce_fwd(const float* __restrict__ scores,
                                                     const float* __restrict__ labels, int n,
                                                     double2* __restrict__ partials) {
  double a = 0.0, b = 0.0;
  const int n4 = n / 4;
  for (int q = blockIdx.x * kThreads + threadIdx.x; q < n4; q += gridDim.x * kThreads) {
    const float4 sc = ((const float4*)scores)[q], lb = ((const float4*)labels)[q];
    a += (double)(-(lb.x * sc.x));
    b += (double)lb.x;
    a += (double)(-(lb.y * sc.y));
    b += (double)lb.y;
    a += (double)(-(lb.z * sc.z));
    b += (double)lb.z;
    a += (double)(-(lb.w * sc.w));
    b += (double)lb.w;
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < n - 4 * n4) {
    const int i = 4 * n4 + threadIdx.x;
    a += (double)(-(labels[i] * scores[i]));
    b += (double)labels[i];
  }
  block_partial(a, b, partials);
}

__global__ void __launch_bounds__(kThreads) k_ce_bwd(const float* __restrict__ labels, int n,
                                                     const float* __restrict__ fin, float* __restrict__ d) {
  const float inv = fin[0];
  const int n4 = n / 4;
  for (int q = blockIdx.x * kThreads + threadIdx.x; q < n4; q += gridDim.x * kThreads) {
    const float4 lb = ((const float4*)labels)[q];
    ((float4*)d)[q] = make_float4(-lb.x * inv, -lb.y * inv, -lb.z * inv, -lb.w * inv);
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < n - 4 * n4) {
    const int i = 4 * n4 + threadIdx.x;
    d[i] = -labels[i] * inv;
  }
}

__device__ __forceinline__ float sl1_in(float w, float pred, float tgt, SmoothL1 k, float& diff, bool& near) {
  diff = w * (pred - tgt);
  const float a = fabsf(diff);
  near = a < k.c_inv;
  return near ? (diff * diff) * k.c_half : a - k.c_off;
}

__device__ __forceinline__ float sl1_grad(float w, float diff, bool near, SmoothL1 k, float inv) {
  const float sgn = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
  return (w * (near ? diff * k.c_s2 : sgn)) * inv;
}

// sum of the weights alone: the gradient's normaliser, ahead of the fused pass
__global__ void __launch_bounds__(kThreads) k_weight_sum(const float* __restrict__ wt, int n,
                                                         double2* __restrict__ partials) {
  double b = 0.0;
  const int n4 = n / 4;
  for (int q = blockIdx.x * kThreads + threadIdx.x; q < n4; q += gridDim.x * kThreads) {
    const float4 w = ((const float4*)wt)[q];
    b += (double)w.x;
    b += (double)w.y;
    b += (double)w.z;
    b += (double)w.w;
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < n - 4 * n4) b += (double)wt[4 * n4 + threadIdx.x];
  block_partial(0.0, b, partials);
}

// (sum of in_loss, sum of w); kGrad: d_pred in the same pass, inv from k_weight_sum's sum
template <bool kGrad>
__global__ void __launch_bounds__(kThreads) k_vertex(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                     const float* __restrict__ wt, int n, SmoothL1 k,
                                                     const float* __restrict__ fin, float* __restrict__ d,
                                                     double2* __restrict__ partials) {
  const float inv = kGrad ? fin[0] : 0.f;
  double a = 0.0, b = 0.0;
  const int n4 = n / 4;
  for (int q = blockIdx.x * kThreads + threadIdx.x; q < n4; q += gridDim.x * kThreads) {
    const float4 p4 = ((const float4*)pred)[q], t4 = ((const float4*)tgt)[q], w4 = ((const float4*)wt)[q];
    const float p[4] = {p4.x, p4.y, p4.z, p4.w}, t[4] = {t4.x, t4.y, t4.z, t4.w}, w[4] = {w4.x, w4.y, w4.z, w4.w};
    float g[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      float diff;
      bool near;
      a += (double)sl1_in(w[j], p[j], t[j], k, diff, near);
      b += (double)w[j];
      if (kGrad) g[j] = sl1_grad(w[j], diff, near, k, inv);
    }
    if (kGrad) ((float4*)d)[q] = make_float4(g[0], g[1], g[2], g[3]);
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < n - 4 * n4) {
    const int i = 4 * n4 + threadIdx.x;
    float diff;
    bool near;
    a += (double)sl1_in(wt[i], pred[i], tgt[i], k, diff, near);
    b += (double)wt[i];
    if (kGrad) d[i] = sl1_grad(wt[i], diff, near, k, inv);
  }
  block_partial(a, b, partials);
}

// ---------------------------------------------------------------------------
// Class-compact vertex loss: a pixel with label l in [1, C) carries weight
// w_inside and target vertex3 on channels 3l..3l+2, every other element of
// the blob pair is (0, 0) and adds nothing to the loss or the gradient.

// channel j of pixel p's prediction at class l
__device__ __forceinline__ size_t pred_at(int p, int l, int j, int pred_ch) {
  return pred_ch == 3 ? (size_t)p * 3 + j : (size_t)p * pred_ch + 3 * l + j;
}

// one thread per pixel: (sum of in_loss, live pixels)
__global__ void __launch_bounds__(kThreads) k_vc_fwd(const int32_t* __restrict__ label,
                                                     const float* __restrict__ vertex3,
                                                     const float* __restrict__ pred, int pred_ch, int n_pix, int C,
                                                     float w, SmoothL1 k, double2* __restrict__ partials) {
  double a = 0.0, b = 0.0;
  float diff;
  bool near;
  for (int p = blockIdx.x * kThreads + threadIdx.x; p < n_pix; p += gridDim.x * kThreads) {
    const int l = label[p];
    if (l >= 1 && l < C) {
#pragma unroll
      for (int j = 0; j < 3; j++)
        a += (double)sl1_in(w, pred[pred_at(p, l, j, pred_ch)], vertex3[(size_t)p * 3 + j], k, diff, near);
      b += 1.0;
    }
  }
  block_partial(a, b, partials);
}

// One thread per pixel.  d_ch = 3: every pixel's three values; d_ch = 3C: the
// labelled pixels' three channels into a map the op has zeroed.
__global__ void __launch_bounds__(kThreads) k_vc_bwd(const int32_t* __restrict__ label,
                                                     const float* __restrict__ vertex3,
                                                     const float* __restrict__ pred, int pred_ch, int n_pix, int C,
                                                     float w, SmoothL1 k, const float* __restrict__ fin,
                                                     float* __restrict__ d, int d_ch) {
  const float inv = fin[0];
  for (int p = blockIdx.x * kThreads + threadIdx.x; p < n_pix; p += gridDim.x * kThreads) {
    const int l = label[p];
    const bool on = l >= 1 && l < C;
    if (!on && d_ch != 3) continue;
#pragma unroll
    for (int j = 0; j < 3; j++) {
      float g = 0.f;
      if (on) {
        float diff;
        bool near;
        sl1_in(w, pred[pred_at(p, l, j, pred_ch)], vertex3[(size_t)p * 3 + j], k, diff, near);
        g = sl1_grad(w, diff, near, k, inv);
      }
      d[pred_at(p, l, j, d_ch)] = g;
    }
  }
}

// ---------------------------------------------------------------------------
// host side

struct LossWs {
  float* fin;         // [0] = inv
  double2* partials;  // [nb]
  float2* ms;         // [n_pix] (segmentation only)
  size_t bytes;
};

LossWs carve_loss(void* ws, int nb, size_t n_ms) {
  pcnn::Carve c(ws);
  LossWs r;
  r.fin = c.take<float>(4);
  r.partials = c.take<double2>((size_t)nb);
  r.ms = n_ms ? c.take<float2>(n_ms) : nullptr;
  r.bytes = pcnn::align_up(c.off, 256);
  return r;
}

inline int flat_blocks(long work) {
  long b = (work + kThreads - 1) / kThreads;
  if (b > kFlatMaxBlocks) b = kFlatMaxBlocks;
  return b < 1 ? 1 : (int)b;
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

inline bool seg_dims_ok(int B, int H, int W, int C) {
  return B > 0 && H > 0 && W > 0 && C > 0 && (long)B * H * W * C < (1l << 31);
}
inline int seg_blocks(long n_pix) { return (int)((n_pix + kThreads - 1) / kThreads); }
inline size_t seg_lds(int C) { return C <= kSegStagedMaxC ? (size_t)kThreads * padded(C) * sizeof(float) : 0; }

inline SmoothL1 smooth_l1_constants(float sigma) {
  const double s2 = (double)sigma * (double)sigma;
  return SmoothL1{(float)(1.0 / s2), (float)(s2 / 2.0), (float)(0.5 / s2), (float)s2};
}

}  // namespace

extern "C" size_t pcnn_seg_loss_workspace_size(int B, int H, int W, int C) {
  if (!seg_dims_ok(B, H, W, C)) return 0;
  const long n_pix = (long)B * H * W;
  return carve_loss(nullptr, seg_blocks(n_pix), (size_t)n_pix).bytes;
}

extern "C" int pcnn_seg_loss(const float* score, const int32_t* gt_label, int B, int H, int W, int C, float threshold,
                             float grad_scale, float* log_prob, float* prob_normalized, int32_t* label_2d,
                             float* gt_label_weight, float* d_score, float* loss, void* workspace,
                             size_t workspace_bytes, void* stream) {
  PCNN_REQUIRE(score && gt_label && loss && workspace);
  PCNN_REQUIRE(seg_dims_ok(B, H, W, C));
  PCNN_REQUIRE(threshold > 0.f);
  PCNN_REQUIRE(aligned(score, 16) && aligned(log_prob, 16) && aligned(prob_normalized, 16) &&
               aligned(gt_label_weight, 16) && aligned(d_score, 16) && aligned(workspace, 16));
  PCNN_REQUIRE(aligned(gt_label, 4) && aligned(label_2d, 4) && aligned(loss, 4));
  const int n_pix = B * H * W;
  const int nb = seg_blocks(n_pix);
  const LossWs ws = carve_loss(workspace, nb, (size_t)n_pix);
  if (workspace_bytes < ws.bytes) return PCNN_ECAPACITY;
  hipStream_t st = (hipStream_t)stream;
  const SegOut o{log_prob, prob_normalized, label_2d, gt_label_weight};
  hipLaunchKernelGGL(k_seg_fwd, dim3(nb), dim3(kThreads), seg_lds(C), st, score, gt_label, n_pix, C, threshold, o,
                     ws.ms, ws.partials);
  PCNN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_loss_final, dim3(1), dim3(kThreads), 0, st, ws.partials, nb, 1.0, grad_scale, loss, ws.fin);
  PCNN_CHECK_LAUNCH();
  if (d_score) {
    hipLaunchKernelGGL(k_seg_bwd, dim3(nb), dim3(kThreads), seg_lds(C), st, score, gt_label, n_pix, C, threshold,
                       ws.ms, ws.fin, d_score);
    PCNN_CHECK_LAUNCH();
  }
  return PCNN_OK;
}

extern "C" size_t pcnn_cross_entropy_workspace_size(int n_pix, int C) {
  if (n_pix <= 0 || C <= 0 || (long)n_pix * C >= (1l << 31)) return 0;
  return carve_loss(nullptr, flat_blocks(((long)n_pix * C + 3) / 4), 0).bytes;
}

extern "C" int pcnn_cross_entropy(const float* scores, const float* labels, int n_pix, int C, float grad_scale,
                                  float* d_scores, float* loss, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  PCNN_REQUIRE(scores && labels && loss && workspace);
  PCNN_REQUIRE(n_pix > 0 && C > 0 && (long)n_pix * C < (1l << 31));
  PCNN_REQUIRE(aligned(scores, 16) && aligned(labels, 16) && aligned(d_scores, 16) && aligned(workspace, 16) &&
               aligned(loss, 4));
  const int n = n_pix * C;
  const int nb = flat_blocks(((long)n + 3) / 4);
  const LossWs ws = carve_loss(workspace, nb, 0);
  if (workspace_bytes < ws.bytes) return PCNN_ECAPACITY;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_ce_fwd, dim3(nb), dim3(kThreads), 0, st, scores, labels, n, ws.partials);
  PCNN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_loss_final, dim3(1), dim3(kThreads), 0, st, ws.partials, nb, 1.0, grad_scale, loss, ws.fin);
  PCNN_CHECK_LAUNCH();
  if (d_scores) {
    hipLaunchKernelGGL(k_ce_bwd, dim3(nb), dim3(kThreads), 0, st, labels, n, ws.fin, d_scores);
    PCNN_CHECK_LAUNCH();
  }
  return PCNN_OK;
}

extern "C" size_t pcnn_vertex_loss_workspace_size(long n) {
  if (n <= 0 || n >= (1l << 31)) return 0;
  return carve_loss(nullptr, flat_blocks((n + 3) / 4), 0).bytes;
}

extern "C" int pcnn_vertex_loss(const float* vertex_pred, const float* vertex_targets, const float* vertex_weights,
                                long n, float sigma, float grad_scale, float* d_pred, float* loss, void* workspace,
                                size_t workspace_bytes, void* stream) {
  PCNN_REQUIRE(vertex_pred && vertex_targets && vertex_weights && loss && workspace);
  PCNN_REQUIRE(n > 0 && n < (1l << 31));
  PCNN_REQUIRE(sigma > 0.f);
  PCNN_REQUIRE(aligned(vertex_pred, 16) && aligned(vertex_targets, 16) && aligned(vertex_weights, 16) &&
               aligned(d_pred, 16) && aligned(workspace, 16) && aligned(loss, 4));
  const int nb = flat_blocks((n + 3) / 4);
  const LossWs ws = carve_loss(workspace, nb, 0);
  if (workspace_bytes < ws.bytes) return PCNN_ECAPACITY;
  const SmoothL1 k = smooth_l1_constants(sigma);
  hipStream_t st = (hipStream_t)stream;
  if (d_pred) {  // the normaliser first (one read of the weights), then loss and gradient in one pass
    hipLaunchKernelGGL(k_weight_sum, dim3(nb), dim3(kThreads), 0, st, vertex_weights, (int)n, ws.partials);
    PCNN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_loss_final, dim3(1), dim3(kThreads), 0, st, ws.partials, nb, 1.0, grad_scale, loss, ws.fin);
    PCNN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_vertex<true>, dim3(nb), dim3(kThreads), 0, st, vertex_pred, vertex_targets, vertex_weights,
                       (int)n, k, ws.fin, d_pred, ws.partials);
  } else {
    hipLaunchKernelGGL(k_vertex<false>, dim3(nb), dim3(kThreads), 0, st, vertex_pred, vertex_targets, vertex_weights,
                       (int)n, k, ws.fin, d_pred, ws.partials);
  }
  PCNN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_loss_final, dim3(1), dim3(kThreads), 0, st, ws.partials, nb, 1.0, grad_scale, loss, ws.fin);
  PCNN_CHECK_LAUNCH();
  return PCNN_OK;
}

extern "C" size_t pcnn_vertex_loss_compact_workspace_size(int B, int H, int W, int C) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || (long)B * H * W * 3 * C >= (1l << 31)) return 0;
  return carve_loss(nullptr, flat_blocks((long)B * H * W), 0).bytes;
}

extern "C" int pcnn_vertex_loss_compact(const int32_t* label, const float* vertex3, const float* vertex_pred,
                                        int pred_ch, int B, int H, int W, int C, float w_inside, float sigma,
                                        float grad_scale, float* d_pred, int d_ch, float* loss, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  PCNN_REQUIRE(label && vertex3 && vertex_pred && loss && workspace);
  PCNN_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && (long)B * H * W * 3 * C < (1l << 31));
  PCNN_REQUIRE(sigma > 0.f);
  PCNN_REQUIRE(pred_ch == 3 || pred_ch == 3 * C);
  PCNN_REQUIRE(!d_pred || d_ch == 3 || d_ch == 3 * C);
  PCNN_REQUIRE(aligned(vertex_pred, 16) && aligned(d_pred, 16) && aligned(workspace, 16) && aligned(label, 4) &&
               aligned(vertex3, 4) && aligned(loss, 4));
  const int n_pix = B * H * W;
  const int nb = flat_blocks(n_pix);
  const LossWs ws = carve_loss(workspace, nb, 0);
  if (workspace_bytes < ws.bytes) return PCNN_ECAPACITY;
  const SmoothL1 k = smooth_l1_constants(sigma);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_vc_fwd, dim3(nb), dim3(kThreads), 0, st, label, vertex3, vertex_pred, pred_ch, n_pix, C,
                     w_inside, k, ws.partials);
  PCNN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_loss_final, dim3(1), dim3(kThreads), 0, st, ws.partials, nb, (double)w_inside * 3.0,
                     grad_scale, loss, ws.fin);
  PCNN_CHECK_LAUNCH();
  if (d_pred) {
    if (d_ch != 3 && hipMemsetAsync(d_pred, 0, (size_t)n_pix * d_ch * sizeof(float), st) != hipSuccess)
      return PCNN_EHIP;
    hipLaunchKernelGGL(k_vc_bwd, dim3(nb), dim3(kThreads), 0, st, label, vertex3, vertex_pred, pred_ch, n_pix, C,
                       w_inside, k, ws.fin, d_pred, d_ch);
    PCNN_CHECK_LAUNCH();
  }
  return PCNN_OK;
}
