// Backward of the class-compact vertex_pred layer: the
// 1x1 conv 128 -> 3C plus bias of lib/networks/vgg16_convs.py:152-163
// (network.py:168-185) evaluated only at each pixel's own class
// (k_vertex_pred_compact, label_producer.hip).  With g = d_vertex3[p] and
// l = label[p], a pixel is live if 0 <= l < C:
//
//  d_feat[p][k]       = (g0 * w[k][3l] + g1 * w[k][3l+1]) + g2 * w[k][3l+2], 0 if not live
//  d_weights[k][3l+j] = sum over the live pixels of class l of feat[p][k] * g_j
//  d_bias[3l+j]       = sum over the live pixels of class l of g_j
//
//  k_vp_dfeat    a pure write stream of B*H*W*K floats.  A wave takes tiles of
//                64 pixels: each lane loads one pixel's label and gradient
//                (the next tile's while this one is written), then the wave
//                walks the tile's 64 * K / 4 float4s, consecutive lanes at
//                consecutive float4s, so that a store instruction covers
//                1 KiB of whole pixel rows; a lane takes its pixel's (l, g)
//                from the lane that loaded it.  The weights sit in LDS
//                transposed, [3C][K]: the lanes of a pixel read a class column
//                as contiguous float4s, conflict-free (the forward's [K][3C]
//                image read along k strides by 3C floats: four scalar reads in
//                place of each float4, and at 3C = 66 lanes k and k + 16 of a
//                32-lane ds_read_b32 group share a bank).
//  k_vp_partial  one workgroup per range of kRange pixels, one thread per two
//                columns (lanes along k).  Per sub-chunk the waves list, in pixel
//                order, the live pixels whose gradient is not all zero, with
//                their (l, g); only those rows of feat are read, two batches
//                of kBatch loads in flight per thread (the list is padded to
//                whole batches with rows that add zeros).  A thread sums a run
//                of equal labels in registers and adds the run into the
//                workgroup's private [3C][K] image in LDS; the image goes to
//                the workspace.
//  k_vp_fold     adds the ranges' partials in range order (kFoldWaves
//                contiguous groups of ranges, each in order, then the groups
//                in order) and writes d_weights in the weights' [K][3C] layout.
//
// No floating-point atomics and a fixed order throughout: two runs give the
// same bits.  float32 products and sums, every op rounded separately.
#include "pcnn_common.h"

namespace {

using pcnn::lane_id;

constexpr int kDfThreads = 256;
constexpr int kDfMaxBlocks = 256 * 4;  // persistent: the weights are staged once per workgroup
constexpr int kRange = 2048;           // pixels per first-stage partial
constexpr int kSeg = 256;              // pixels a wave lists per sub-chunk
constexpr int kBatch = 16;             // feat rows of one batch; two batches in flight per thread
constexpr int kFoldWaves = 16;
constexpr int kPartialMaxLds = 96 * 1024;

struct PixGrad {
  int l;  // -1: not live
  float g0, g1, g2;
};

__device__ __forceinline__ PixGrad load_pix(const int32_t* __restrict__ label, const float* __restrict__ d3, int p,
                                            int n_pix, int C) {
  PixGrad r = {-1, 0.f, 0.f, 0.f};
  if (p < n_pix) {
    const int l = label[p];
    r.l = (l >= 0 && l < C) ? l : -1;
    r.g0 = d3[(size_t)p * 3 + 0];
    r.g1 = d3[(size_t)p * 3 + 1];
    r.g2 = d3[(size_t)p * 3 + 2];
  }
  return r;
}

__global__ void __launch_bounds__(kDfThreads) k_vp_dfeat(const float* __restrict__ w,
                                                         const int32_t* __restrict__ label,
                                                         const float* __restrict__ d3, int n_pix, int K, int C,
                                                         float* __restrict__ d_feat) {
  extern __shared__ __attribute__((aligned(16))) float wt[];  // [3C][K]
  const int NC3 = 3 * C;
  for (int i = threadIdx.x; i < K * NC3; i += kDfThreads) {
    const int c = i / K;
    const int k = i - c * K;
    wt[i] = w[k * NC3 + c];
  }
  __syncthreads();
  const int lane = lane_id();
  const int K4 = K / 4;
  const int n_tiles = (n_pix + 63) / 64;
  const int n_waves = gridDim.x * (kDfThreads / 64);
  const int dpl = 64 / K4, dk = 64 - dpl * K4;  // a step of 64 float4s in (pixel, k4)
  const int pl0 = lane / K4, k40 = lane - pl0 * K4;
  int tile = blockIdx.x * (kDfThreads / 64) + (threadIdx.x >> 6);
  PixGrad nxt = load_pix(label, d3, tile < n_tiles ? tile * 64 + lane : n_pix, n_pix, C);
  for (; tile < n_tiles; tile += n_waves) {
    const PixGrad cur = nxt;
    nxt = load_pix(label, d3, tile + n_waves < n_tiles ? (tile + n_waves) * 64 + lane : n_pix, n_pix, C);
    const int npl = n_pix - tile * 64 < 64 ? n_pix - tile * 64 : 64;
    const int nq = npl * K4;  // float4s of this tile
    float4* dst = (float4*)d_feat + (size_t)tile * 64 * K4;
    int pl = pl0, k4 = k40;
    for (int base = 0; base < nq; base += 64) {  // every lane runs every step: the shuffles need them all
      const bool active = base + lane < nq;
      const int src = active ? pl : 0;
      const int l = __shfl(cur.l, src, 64);
      const float g0 = __shfl(cur.g0, src, 64), g1 = __shfl(cur.g1, src, 64), g2 = __shfl(cur.g2, src, 64);
      const float* col = wt + 3 * (l < 0 ? 0 : l) * K + 4 * (active ? k4 : 0);
      const float4 a = *(const float4*)col, b = *(const float4*)(col + K), c = *(const float4*)(col + 2 * K);
      float4 o;
      o.x = (g0 * a.x + g1 * b.x) + g2 * c.x;
      o.y = (g0 * a.y + g1 * b.y) + g2 * c.y;
      o.z = (g0 * a.z + g1 * b.z) + g2 * c.z;
      o.w = (g0 * a.w + g1 * b.w) + g2 * c.w;
      if (l < 0) o = make_float4(0.f, 0.f, 0.f, 0.f);
      if (active) dst[base + lane] = o;
      pl += dpl;
      k4 += dk;
      if (k4 >= K4) { k4 -= K4; pl++; }
    }
  }
}

// The run of equal labels a thread is summing: columns k, k + 1 of the class's
// three weight gradients, and (lanes 0..2 of the first wave) one bias gradient.
struct Run {
  int cur;
  float2 a0, a1, a2;
  float ab;
  __device__ __forceinline__ void reset(int l) {
    cur = l;
    a0 = a1 = a2 = make_float2(0.f, 0.f);
    ab = 0.f;
  }
  // bias_j >= 0: this lane sums the bias gradient of channel j
  __device__ __forceinline__ void flush(float* acc, float* accb, int K, int k, bool col_w, int bias_j) {
    if (cur < 0) return;
    if (col_w) {
      float* col = acc + 3 * cur * K + k;
      float2 v = *(float2*)col;
      *(float2*)col = make_float2(v.x + a0.x, v.y + a0.y);
      v = *(float2*)(col + K);
      *(float2*)(col + K) = make_float2(v.x + a1.x, v.y + a1.y);
      v = *(float2*)(col + 2 * K);
      *(float2*)(col + 2 * K) = make_float2(v.x + a2.x, v.y + a2.y);
    }
    if (bias_j >= 0) accb[3 * cur + bias_j] = accb[3 * cur + bias_j] + ab;
  }
};

// The listed pixels of a sub-chunk, in pixel order.
struct PixList {
  int* idx;
  int* l;
  float *g0, *g1, *g2;
};

// kBatch rows of the list in flight: lane u % kBatch holds row i + u's (pixel, l, g), which every lane takes
// with a readlane -- one LDS round trip per batch, not one per row.  Every lane of the wave runs these.
struct Rows {
  float2 f[kBatch];
  int idx, l;
  float g0, g1, g2;
  __device__ __forceinline__ void load(const PixList& ls, int i, const float* __restrict__ feat, int K, int k,
                                       bool want_w) {
    const int e = i + (lane_id() & (kBatch - 1));
    idx = ls.idx[e];
    l = ls.l[e];
    g0 = ls.g0[e];
    g1 = ls.g1[e];
    g2 = ls.g2[e];
#pragma unroll
    for (int u = 0; u < kBatch; u++)
      f[u] = want_w ? *(const float2*)(feat + (size_t)__builtin_amdgcn_readlane(idx, u) * K + k)
                    : make_float2(0.f, 0.f);
  }
  __device__ __forceinline__ void add_row(int u, bool wave_bias, int bias_j, Run& r) const {
    const float h0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(g0), u));
    const float h1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(g1), u));
    const float h2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(g2), u));
    r.a0.x = r.a0.x + f[u].x * h0;
    r.a0.y = r.a0.y + f[u].y * h0;
    r.a1.x = r.a1.x + f[u].x * h1;
    r.a1.y = r.a1.y + f[u].y * h1;
    r.a2.x = r.a2.x + f[u].x * h2;
    r.a2.y = r.a2.y + f[u].y * h2;
    if (wave_bias) r.ab = r.ab + (bias_j == 0 ? h0 : (bias_j == 1 ? h1 : h2));
  }
  // the sums, in list order; wave_bias: this wave holds the bias lanes (wave-uniform)
  __device__ __forceinline__ void sum(int K, int k, bool col_w, bool wave_bias, int bias_j, float* acc, float* accb,
                                      Run& r) const {
    if (__ballot(l >= 0 && l != r.cur) == 0) {  // the whole batch continues the run: no per-row branch
#pragma unroll
      for (int u = 0; u < kBatch; u++) add_row(u, wave_bias, bias_j, r);
      return;
    }
#pragma unroll
    for (int u = 0; u < kBatch; u++) {
      const int lu = __builtin_amdgcn_readlane(l, u);
      if (lu >= 0 && lu != r.cur) {  // wave-uniform; lu < 0: a padding row, which stays in the run
        r.flush(acc, accb, K, k, col_w, bias_j);
        r.reset(lu);
      }
      add_row(u, wave_bias, bias_j, r);
    }
  }
};

// part[blockIdx.x] = [3C][K] weight partial, then [3C] bias partial
__global__ void __launch_bounds__(256) k_vp_partial(const float* __restrict__ feat, const int32_t* __restrict__ label,
                                                    const float* __restrict__ d3, int n_pix, int K, int C,
                                                    int want_w, int want_b, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int NC3 = 3 * C;
  const int T = blockDim.x, nw = T >> 6;
  const int tid = threadIdx.x, wave = tid >> 6, lane = lane_id();
  float* acc = lds;             // [3C][K]
  float* accb = acc + NC3 * K;  // [3C]
  const int cap = nw * kSeg;    // pixels per sub-chunk
  PixList ls;
  ls.idx = (int*)(accb + NC3);
  ls.l = ls.idx + cap;
  ls.g0 = (float*)(ls.l + cap);
  ls.g1 = ls.g0 + cap;
  ls.g2 = ls.g1 + cap;
  int* cnt = (int*)(ls.g2 + cap);  // [nw]
  for (int i = tid; i < NC3 * (K + 1); i += T) lds[i] = 0.f;
  const int r0 = blockIdx.x * kRange;
  const int r1 = n_pix - r0 < kRange ? n_pix : r0 + kRange;
  const int k2_end = want_w ? K / 2 : 1;  // column pairs; bias only: the first wave still walks the rows
  // the wave's kSeg pixels of a sub-chunk, loaded one sub-chunk ahead of the walk
  PixGrad px[kSeg / 64];
#pragma unroll
  for (int it = 0; it < kSeg / 64; it++) {
    const int p = r0 + wave * kSeg + it * 64 + lane;
    px[it] = load_pix(label, d3, p < r1 ? p : n_pix, n_pix, C);
  }
  for (int s0 = r0; s0 < r1; s0 += cap) {
    // which of them are listed, and where in the wave's part of the list
    int pos[kSeg / 64];
    int n = 0;
#pragma unroll
    for (int it = 0; it < kSeg / 64; it++) {
      const bool keep = px[it].l >= 0 && !(px[it].g0 == 0.f && px[it].g1 == 0.f && px[it].g2 == 0.f);
      const uint64_t m = __ballot(keep);
      pos[it] = keep ? n + __popcll(m & pcnn::lanemask_lt()) : -1;
      n += __popcll(m);
    }
    __syncthreads();  // the image is zeroed / the previous list is consumed
    if (lane == 0) cnt[wave] = n;
    __syncthreads();
    int first = 0, total = 0;
    for (int w = 0; w < nw; w++) {
      const int c = cnt[w];
      if (w < wave) first += c;
      total += c;
    }
#pragma unroll
    for (int it = 0; it < kSeg / 64; it++) {
      if (pos[it] >= 0) {
        const int e = first + pos[it];
        ls.idx[e] = s0 + wave * kSeg + it * 64 + lane;
        ls.l[e] = px[it].l;
        ls.g0[e] = px[it].g0;
        ls.g1[e] = px[it].g1;
        ls.g2[e] = px[it].g2;
      }
      const int p = s0 + cap + wave * kSeg + it * 64 + lane;  // the next sub-chunk's
      px[it] = load_pix(label, d3, p < r1 ? p : n_pix, n_pix, C);
    }
    // pad the list to whole batches with rows that add zeros: the sub-chunk's first pixel (its feat row is
    // valid memory), no label of their own, a zero gradient
    const int padded = (total + kBatch - 1) / kBatch * kBatch;  // <= cap, a multiple of kBatch
    if (tid < padded - total) {
      const int e = total + tid;
      ls.idx[e] = s0;
      ls.l[e] = -1;
      ls.g0[e] = ls.g1[e] = ls.g2[e] = 0.f;
    }
    __syncthreads();
    // whole waves walk the list (the readlanes need every lane): a lane past the last column pair reads
    // columns 0, 1 and keeps nothing
    for (int kb = wave * 64; kb < k2_end; kb += T) {
      const bool mine = want_w && 2 * (kb + lane) < K;
      const int k = mine ? 2 * (kb + lane) : 0;
      const bool wave_bias = want_b && kb == 0;  // the first wave, once
      const int bias_j = wave_bias && lane < 3 ? lane : -1;
      Run r;
      r.reset(-1);
      Rows a, b;  // two batches in flight
      if (padded > 0) a.load(ls, 0, feat, K, k, want_w);
      for (int i = 0; i < padded; i += 2 * kBatch) {
        const bool two = i + kBatch < padded;
        if (two) b.load(ls, i + kBatch, feat, K, k, want_w);
        a.sum(K, k, mine, wave_bias, bias_j, acc, accb, r);
        if (two) {
          if (i + 2 * kBatch < padded) a.load(ls, i + 2 * kBatch, feat, K, k, want_w);
          b.sum(K, k, mine, wave_bias, bias_j, acc, accb, r);
        }
      }
      r.flush(acc, accb, K, k, mine, bias_j);
    }
  }
  __syncthreads();
  float* out = part + (size_t)blockIdx.x * NC3 * (K + 1);
  const int lo = want_w ? 0 : NC3 * K, hi = want_b ? NC3 * (K + 1) : NC3 * K;
  for (int i = lo + tid; i < hi; i += T) out[i] = lds[i];
}

// One element of a partial per lane, a contiguous group of the ranges per wave.
__global__ void __launch_bounds__(kFoldWaves * 64) k_vp_fold(const float* __restrict__ part, int P, int K, int C,
                                                             int lo, int hi, float* __restrict__ d_weights,
                                                             float* __restrict__ d_bias) {
  __shared__ float red[kFoldWaves][64];
  const int NC3 = 3 * C;
  const int PS = NC3 * (K + 1);
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  const int e = lo + blockIdx.x * 64 + lane;
  const int per = (P + kFoldWaves - 1) / kFoldWaves;
  const int p0 = wave * per, p1 = (p0 + per < P) ? p0 + per : P;
  float s = 0.f;
  if (e < hi) {
#pragma unroll 8
    for (int p = p0; p < p1; p++) s = s + part[(size_t)p * PS + e];
  }
  red[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && e < hi) {
    float v = red[0][lane];
    for (int w = 1; w < kFoldWaves; w++) v = v + red[w][lane];
    if (e < NC3 * K) {
      const int c = e / K;
      d_weights[(e - c * K) * NC3 + c] = v;
    } else {
      d_bias[e - NC3 * K] = v;
    }
  }
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

inline bool dims_ok(int B, int H, int W, int K, int C) {
  if (B <= 0 || H <= 0 || W <= 0 || K <= 0 || C <= 0 || K % 4) return false;
  if ((long)K * 3 * C * 4 > 64 * 1024) return false;
  return (long)B * H * W * K < (1l << 31);
}

inline int n_ranges(long n_pix) { return (int)((n_pix + kRange - 1) / kRange); }

// one thread per pair of columns
inline int partial_threads(int K) { return K >= 512 ? 256 : (K / 2 + 63) / 64 * 64; }

inline size_t partial_lds(int K, int C, int T) {
  return (size_t)3 * C * (K + 1) * sizeof(float) + (size_t)(T / 64) * (5 * kSeg + 1) * sizeof(int);
}

// k_vp_partial's image, bias row and list can pass the 64 KiB a kernel gets
// without asking: raise its limit once per device.
inline bool allow_partial_lds() {
  static bool done[pcnn::kMaxDevices] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= pcnn::kMaxDevices) return false;
  if (!done[dev]) {
    if (hipFuncSetAttribute((const void*)k_vp_partial, hipFuncAttributeMaxDynamicSharedMemorySize,
                            kPartialMaxLds) != hipSuccess)
      return false;
    done[dev] = true;
  }
  return true;
}

}  // namespace

extern "C" int pcnn_vertex_pred_compact_bwd_partials(int B, int H, int W, int K, int C) {
  return dims_ok(B, H, W, K, C) ? n_ranges((long)B * H * W) : 0;
}

extern "C" size_t pcnn_vertex_pred_compact_bwd_workspace_size(int B, int H, int W, int K, int C) {
  if (!dims_ok(B, H, W, K, C)) return 0;
  return pcnn::align_up((size_t)n_ranges((long)B * H * W) * 3 * C * (K + 1) * sizeof(float), 256);
}

extern "C" int pcnn_vertex_pred_compact_bwd(const float* feat, const float* weights, const int32_t* label,
                                            const float* d_vertex3, int B, int H, int W, int K, int C, float* d_feat,
                                            float* d_weights, float* d_bias, void* workspace, size_t workspace_bytes,
                                            void* stream) {
  PCNN_REQUIRE(d_feat || d_weights || d_bias);
  PCNN_REQUIRE(label && d_vertex3 && (feat || !d_weights) && (weights || !d_feat));
  PCNN_REQUIRE(dims_ok(B, H, W, K, C));
  PCNN_REQUIRE(aligned(feat, 16) && aligned(d_vertex3, 16) && aligned(d_feat, 16) && aligned(weights, 4) &&
               aligned(d_weights, 4) && aligned(d_bias, 4) && aligned(label, 4));
  const int n_pix = B * H * W;
  const int NC3 = 3 * C;
  hipStream_t st = (hipStream_t)stream;
  const bool sums = d_weights || d_bias;
  if (sums) {
    PCNN_REQUIRE(workspace && aligned(workspace, 16));
    if (workspace_bytes < pcnn_vertex_pred_compact_bwd_workspace_size(B, H, W, K, C)) return PCNN_ECAPACITY;
  }
  if (d_feat) {
    const int tiles = (n_pix + 63) / 64;
    int blocks = (tiles + kDfThreads / 64 - 1) / (kDfThreads / 64);
    if (blocks > kDfMaxBlocks) blocks = kDfMaxBlocks;
    hipLaunchKernelGGL(k_vp_dfeat, dim3(blocks), dim3(kDfThreads), (size_t)K * NC3 * sizeof(float), st, weights, label,
                       d_vertex3, n_pix, K, C, d_feat);
    PCNN_CHECK_LAUNCH();
  }
  if (sums) {
    const int P = n_ranges(n_pix);
    const int T = partial_threads(K);
    const size_t lds = partial_lds(K, C, T);
    if (lds > 48 * 1024 && !allow_partial_lds()) return PCNN_EHIP;
    float* part = (float*)workspace;
    hipLaunchKernelGGL(k_vp_partial, dim3(P), dim3(T), lds, st, feat, label, d_vertex3, n_pix, K, C,
                       d_weights ? 1 : 0, d_bias ? 1 : 0, part);
    PCNN_CHECK_LAUNCH();
    const int lo = d_weights ? 0 : NC3 * K, hi = d_bias ? NC3 * (K + 1) : NC3 * K;
    hipLaunchKernelGGL(k_vp_fold, dim3((hi - lo + 63) / 64), dim3(kFoldWaves * 64), 0, st, part, P, K, C, lo, hi,
                       d_weights, d_bias);
    PCNN_CHECK_LAUNCH();
  }
  return PCNN_OK;
}
