// The reference's fixed bilinear transposed conv (`upscore`, `upscore_vertex`:
// 16x16 at stride 8, lib/networks/vgg16_convs.py:138,162; `upscore_conv5(_vertex)`:
// 4x4 at stride 2, :122,130,154; filter network.py:141-157, layer :207-222), and
// its class-compact form folded behind the 1x1 conv it feeds: both are linear
// and the upscore is depthwise, so vertex_pred(upscore(x)) = upscore(x W) + b
// and the (B,H,W,128) map between them need not exist.
//
// Geometry, stride s in {2,4,8,16}, kernel 2s x 2s, SAME padding, output
// (B, H = s h, W = s w, Ch).  An output row y has the taps
//     i1 = (y + s/2) div s, k = y + s/2 - s i1, i0 = i1 - 1,
//     weight (2k+1)/(2s) at i1 and (2s-1-2k)/(2s) at i0,
// a tap with i0 < 0 or i1 >= h is absent (zero padding), columns alike; a 2-D
// weight is the product of the two (exact: dyadic fractions).  The band of i1
// is the s rows [s i1 - s/2, s i1 + s/2) (s/2 rows at both borders), so a
// low-res row i is tapped by the 2s rows [s i - s/2, s i + 3s/2): as i1 by the
// first s of them, as i0 by the rest.
//
//  k_up_fwd      generic forward, a write stream.  A workgroup takes one row
//                band x a run of column bands x a channel chunk, stages the
//                two low-res rows it taps in LDS once, then walks the band's
//                output rows: consecutive lanes at consecutive channels and
//                pixels, 16-, 8- or 4-byte stores by Ch % 4, Ch % 2.
//  k_upc_fwd     class-compact forward: a thread per output pixel gathers the
//                four taps of its own class's three channels from z (small:
//                it stays in cache) with the generic forward's arithmetic.
//  k_up_bwd      generic backward.  A workgroup owns a tile of low-res pixels
//                (a strip of rows x a run of columns) and reads the full-res
//                rows over it once, band by band: each thread sums its
//                (column, channel) over a band's rows under both row weights
//                (16-byte loads wherever a tile's row of pixels is a whole
//                number of them), which completes the low-res row above in
//                LDS; then a thread per low-res (pixel, channel) sums 2s of
//                those with the column weights.  The bias partial is the
//                unweighted sum over the pixels the tile owns.
//  k_upc_bwd     class-compact backward: a wave per low-res pixel holds its
//                2s x 2s window in registers and walks the distinct classes
//                present in ascending order; per class a masked sum per lane
//                and a butterfly over the lanes, zeros written for the
//                classes between.  Bias sums likewise over the owned pixels,
//                added per wave in LDS, per workgroup into a partial.
//  k_up_fold     adds the partials in range order (kFoldWaves contiguous
//                groups, each in order, then the groups in order).
//
// No floating-point atomics, every order fixed: two runs give the same bits.
// float32 products and sums, every op rounded separately.
#include "pcnn_common.h"

#include <limits.h>

namespace {

using pcnn::lane_id;

constexpr int kThreads = 256;
constexpr int kFoldWaves = 16;
constexpr int kFwdLdsFloats = 8192;   // two staged low-res rows of a forward tile
constexpr int kBwdLdsFloats = 12288;  // a backward tile's three arrays of column sums
constexpr int kBwdRows = 4;           // low-res rows of a backward strip: 5 bands read for 4 rows
constexpr int kCbPix = 32;            // low-res pixels of a compact-backward workgroup (4 waves, 8 each)
constexpr int kCbMaxC = 1024;         // 4 waves x 3C bias sums in LDS

// The taps of output coordinate y along one axis of low-res extent n.
struct Tap {
  int i1;        // i0 = i1 - 1
  float w0, w1;  // weights of i0, i1
  bool p0, p1;   // present
};

__device__ __forceinline__ Tap tap_of(int y, int ls, int n) {
  const int s = 1 << ls;
  const int t = y + (s >> 1);
  Tap r;
  r.i1 = t >> ls;
  const int k = t - (r.i1 << ls);
  const float inv = 1.f / (float)(2 * s);
  r.w1 = (float)(2 * k + 1) * inv;
  r.w0 = (float)(2 * s - 1 - 2 * k) * inv;
  r.p0 = r.i1 >= 1;
  r.p1 = r.i1 < n;
  return r;
}

// Weight of window position u in [0, 2s) of a low-res pixel: rows (columns)
// s i - s/2 + u; the first s tap it as i1, the rest as i0.
__device__ __forceinline__ float window_weight(int u, int s) {
  const float inv = 1.f / (float)(2 * s);
  return (float)(u < s ? 2 * u + 1 : 4 * s - 1 - 2 * u) * inv;
}

// The pinned sum: ((t00 + t01) + t10) + t11, absent taps skipped, the first
// present term starts the sum; then bias, then ReLU.
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

__device__ __forceinline__ float up_value(float x00, float x01, float x10, float x11, const Tap& r, const Tap& c,
                                          bool has_bias, float bias, bool relu) {
  Acc a = {0.f, false};
  a.add(r.p0 && c.p0, x00, r.w0 * c.w0);
  a.add(r.p0 && c.p1, x01, r.w0 * c.w1);
  a.add(r.p1 && c.p0, x10, r.w1 * c.w0);
  a.add(r.p1 && c.p1, x11, r.w1 * c.w1);
  float v = a.v;
  if (has_bias) v = v + bias;
  if (relu) v = v > 0.f ? v : 0.f;
  return v;
}

template <int V>
struct Vec;
template <>
struct Vec<1> { using T = float; };
template <>
struct Vec<2> { using T = float2; };
template <>
struct Vec<4> { using T = float4; };

struct Tiling {
  int nj;   // column bands (forward) or low-res columns (backward) of a tile
  int ntj;  // tiles along the columns
  int cc;   // channels of a chunk
  int ncc;  // chunks
};

template <int V>
__global__ void __launch_bounds__(kThreads) k_up_fwd(const float* __restrict__ x, const float* __restrict__ bias,
                                                     int B, int h, int w, int Ch, int ls, int relu, Tiling tl,
                                                     float* __restrict__ y) {
  extern __shared__ __attribute__((aligned(16))) float lo[];  // [2][ncol][ccn]
  const int s = 1 << ls, H = h << ls, W = w << ls;
  int blk = blockIdx.x;
  const int tc = blk % tl.ncc;
  blk /= tl.ncc;
  const int tj = blk % tl.ntj;
  blk /= tl.ntj;
  const int i1 = blk % (h + 1);
  const int b = blk / (h + 1);
  const int c0 = tc * tl.cc;
  const int ccn = Ch - c0 < tl.cc ? Ch - c0 : tl.cc;
  const int jb0 = tj * tl.nj;                                        // first column band
  const int njt = w + 1 - jb0 < tl.nj ? w + 1 - jb0 : tl.nj;         // column bands here
  const int ncol = njt + 1;                                          // low-res columns jb0 - 1 .. jb0 + njt - 1
  const int tid = threadIdx.x;
  for (int idx = tid; idx < 2 * ncol * ccn; idx += kThreads) {
    const int r = idx / (ncol * ccn);
    const int rem = idx - r * ncol * ccn;
    const int cl = rem / ccn;
    const int ch = rem - cl * ccn;
    const int i = i1 - 1 + r, j = jb0 - 1 + cl;
    float v = 0.f;
    if (i >= 0 && i < h && j >= 0 && j < w) v = x[((size_t)(b * h + i) * w + j) * Ch + c0 + ch];
    lo[idx] = v;
  }
  __syncthreads();
  const int ya = i1 * s - (s >> 1) < 0 ? 0 : i1 * s - (s >> 1);
  const int yb = i1 * s + (s >> 1) > H ? H : i1 * s + (s >> 1);
  const int xa = jb0 * s - (s >> 1) < 0 ? 0 : jb0 * s - (s >> 1);
  const int xb = (jb0 + njt) * s - (s >> 1) > W ? W : (jb0 + njt) * s - (s >> 1);
  const int nvec = (xb - xa) * ccn / V;
  const float* lo1 = lo + ncol * ccn;
  for (int e = tid; e < nvec; e += kThreads) {
    const int f = e * V;
    const int xl = f / ccn;
    const int ch = f - xl * ccn;
    const int xo = xa + xl;
    const Tap c = tap_of(xo, ls, w);
    const int cl1 = c.i1 - jb0 + 1;  // in [1, njt]; column cl1 - 1 holds j0 (zeros where absent)
    float x00[V], x01[V], x10[V], x11[V], bv[V];
#pragma unroll
    for (int v = 0; v < V; v++) {
      x00[v] = lo[(cl1 - 1) * ccn + ch + v];
      x01[v] = lo[cl1 * ccn + ch + v];
      x10[v] = lo1[(cl1 - 1) * ccn + ch + v];
      x11[v] = lo1[cl1 * ccn + ch + v];
      bv[v] = bias ? bias[c0 + ch + v] : 0.f;
    }
    float* dst = y + ((size_t)(b * H + ya) * W + xo) * Ch + c0 + ch;
    for (int yo = ya; yo < yb; yo++, dst += (size_t)W * Ch) {
      const Tap r = tap_of(yo, ls, h);
      float o[V];
#pragma unroll
      for (int v = 0; v < V; v++) o[v] = up_value(x00[v], x01[v], x10[v], x11[v], r, c, bias != nullptr, bv[v], relu);
      if constexpr (V == 4) *(float4*)dst = make_float4(o[0], o[1], o[2], o[3]);
      else if constexpr (V == 2) *(float2*)dst = make_float2(o[0], o[1]);
      else *dst = o[0];
    }
  }
}

__global__ void __launch_bounds__(kThreads) k_upc_fwd(const float* __restrict__ z, const float* __restrict__ bias,
                                                      const int32_t* __restrict__ label, int B, int h, int w, int C,
                                                      int ls, float* __restrict__ v3) {
  const int H = h << ls, W = w << ls;
  const int n_pix = B * H * W;
  const int p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= n_pix) return;
  const int xo = p % W;
  const int t = p / W;
  const int yo = t % H;
  const int b = t / H;
  const int l = label[p];
  float o0 = 0.f, o1 = 0.f, o2 = 0.f;
  if (l >= 0 && l < C) {
    const Tap r = tap_of(yo, ls, h), c = tap_of(xo, ls, w);
    const int NC3 = 3 * C;
    float v[4][3];
#pragma unroll
    for (int a = 0; a < 4; a++) {
      const bool pr = (a >> 1 ? r.p1 : r.p0) && (a & 1 ? c.p1 : c.p0);
      const int i = r.i1 - 1 + (a >> 1), j = c.i1 - 1 + (a & 1);
      const float* src = z + ((size_t)(b * h + (pr ? i : 0)) * w + (pr ? j : 0)) * NC3 + 3 * l;
#pragma unroll
      for (int k = 0; k < 3; k++) v[a][k] = pr ? src[k] : 0.f;
    }
    o0 = up_value(v[0][0], v[1][0], v[2][0], v[3][0], r, c, true, bias[3 * l + 0], false);
    o1 = up_value(v[0][1], v[1][1], v[2][1], v[3][1], r, c, true, bias[3 * l + 1], false);
    o2 = up_value(v[0][2], v[1][2], v[2][2], v[3][2], r, c, true, bias[3 * l + 2], false);
  }
  float* dst = v3 + (size_t)p * 3;
  dst[0] = o0;
  dst[1] = o1;
  dst[2] = o2;
}

// A workgroup takes a strip of up to kBwdRows low-res rows [ia, ib) x a run of low-res columns x a channel chunk
// and walks the row bands ia .. ib over it.  Band bb taps low-res row bb as i1 and row bb - 1 as i0, so with
// A(bb), Z(bb) its rows' sums under the two weights, low-res row i has the column sums A(i) + Z(i + 1): A waits
// in `carry` for the next band.  part: [B * nstrips * ntj][Ch] bias partials, NULL without d_bias.  yv: the
// forward's output (ReLU mask), or NULL.
template <int V>
__global__ void __launch_bounds__(kThreads) k_up_bwd(const float* __restrict__ dy, const float* __restrict__ yv, int B,
                                                     int h, int w, int Ch, int ls, Tiling tl, float* __restrict__ d_x,
                                                     float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  using VT = typename Vec<V>::T;
  const int s = 1 << ls, H = h << ls, W = w << ls;
  const int nstr = (h + kBwdRows - 1) / kBwdRows;
  int blk = blockIdx.x;
  const int tc = blk % tl.ncc;
  blk /= tl.ncc;
  const int sp = blk;  // the spatial tile: (b, strip, tj)
  const int tj = blk % tl.ntj;
  blk /= tl.ntj;
  const int ia = (blk % nstr) * kBwdRows;
  const int ib = ia + kBwdRows < h ? ia + kBwdRows : h;
  const int b = blk / nstr;
  const int c0 = tc * tl.cc;
  const int ccn = Ch - c0 < tl.cc ? Ch - c0 : tl.cc;
  const int jc0 = tj * tl.nj;
  const int njt = w - jc0 < tl.nj ? w - jc0 : tl.nj;
  const int x0 = jc0 * s - (s >> 1);
  const int xa = x0 < 0 ? 0 : x0;
  const int xb = (jc0 + njt) * s + (s >> 1) > W ? W : (jc0 + njt) * s + (s >> 1);
  const int nx = xb - xa;
  float* cs = lds;                // [nx][ccn] a low-res row's sums over its 2s rows with the row weights
  float* carry = cs + nx * ccn;   // [nx][ccn] A of the band before
  float* ub = carry + nx * ccn;   // [nx][ccn] plain sums over the strip's own rows [s ia, s ib)
  const int tid = threadIdx.x;
  const size_t row = (size_t)W * Ch;
  const float inv = 1.f / (float)(2 * s);
  for (int bb = ia; bb <= ib; bb++) {
    const int r0 = bb * s - (s >> 1);  // the band's first row, -s/2 for band 0
    const int ra = r0 < 0 ? 0 : r0;
    const int rb = r0 + s > H ? H : r0 + s;
    // each element of the three arrays belongs to one thread in every band: no barrier around carry and ub
    for (int e = tid; e < nx * ccn / V; e += kThreads) {
      const int f = e * V;
      const int xl = f / ccn;
      const int ch = f - xl * ccn;
      const size_t base = ((size_t)(b * H + ra) * W + xa + xl) * Ch + c0 + ch;
      float a[V], z[V], u[V];
#pragma unroll
      for (int v = 0; v < V; v++) a[v] = z[v] = u[v] = 0.f;
#pragma unroll 8
      for (int yo = ra; yo < rb; yo++) {
        const size_t at = base + (size_t)(yo - ra) * row;
        float g[V];
        *(VT*)g = *(const VT*)(dy + at);
        if (yv) {
          float m[V];
          *(VT*)m = *(const VT*)(yv + at);
#pragma unroll
          for (int v = 0; v < V; v++) g[v] = m[v] > 0.f ? g[v] : 0.f;
        }
        const int k = yo - r0;
        const float w1 = (float)(2 * k + 1) * inv, w0 = (float)(2 * s - 1 - 2 * k) * inv;
        const bool own = yo >= ia * s && yo < ib * s;
#pragma unroll
        for (int v = 0; v < V; v++) {
          a[v] = a[v] + w1 * g[v];
          z[v] = z[v] + w0 * g[v];
          if (own) u[v] = u[v] + g[v];
        }
      }
#pragma unroll
      for (int v = 0; v < V; v++) {
        if (bb > ia) cs[f + v] = carry[f + v] + z[v];
        carry[f + v] = a[v];
        if (part) ub[f + v] = bb > ia ? ub[f + v] + u[v] : u[v];
      }
    }
    if (bb == ia) continue;
    __syncthreads();
    const int i = bb - 1;
    for (int o = tid; o < njt * ccn; o += kThreads) {
      const int jl = o / ccn;
      const int ch = o - jl * ccn;
      const int j = jc0 + jl;
      const int wx0 = j * s - (s >> 1);
      float acc = 0.f;
      for (int u = 0; u < 2 * s; u++) {
        const int xo = wx0 + u;
        if (xo < 0 || xo >= W) continue;
        acc = acc + window_weight(u, s) * cs[(xo - xa) * ccn + ch];
      }
      d_x[((size_t)(b * h + i) * w + j) * Ch + c0 + ch] = acc;
    }
    __syncthreads();  // cs is rewritten by the next band; after the last, ub is complete
  }
  if (part) {
    for (int ch = tid; ch < ccn; ch += kThreads) {
      float acc = 0.f;
      for (int xo = jc0 * s; xo < (jc0 + njt) * s; xo++) acc = acc + ub[(xo - xa) * ccn + ch];
      part[(size_t)sp * Ch + c0 + ch] = acc;
    }
  }
}

__device__ __forceinline__ int wave_min_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int t = __shfl_xor(v, o, 64);
    v = t < v ? t : v;
  }
  return v;
}

// A fixed tree over the lanes; float addition commutes, so every lane ends with the same bits.
__device__ __forceinline__ float wave_tree_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
  return v;
}

// The window of a low-res pixel in registers: position e = r * 64 + lane of the 2S x 2S window, row-major.
template <int S>
struct Window {
  static constexpr int NP = (4 * S * S + 63) / 64;
  int lab[NP];  // -1: outside the image or not live
  float g0[NP], g1[NP], g2[NP];
  __device__ __forceinline__ void load(const int32_t* __restrict__ label, const float* __restrict__ d3, int q,
                                       int n_low, int h, int w, int C) {
    const int H = h * S, W = w * S;
    const int j = q % w;
    const int t = q / w;
    const int i = t % h;
    const int b = t / h;
#pragma unroll
    for (int r = 0; r < NP; r++) {
      const int e = r * 64 + lane_id();
      const int yo = i * S - S / 2 + e / (2 * S), xo = j * S - S / 2 + e % (2 * S);
      lab[r] = -1;
      g0[r] = g1[r] = g2[r] = 0.f;
      if (q < n_low && e < 4 * S * S && yo >= 0 && yo < H && xo >= 0 && xo < W) {
        const size_t p = (size_t)(b * H + yo) * W + xo;
        const int l = label[p];
        if (l >= 0 && l < C) {
          lab[r] = l;
          g0[r] = d3[p * 3 + 0];
          g1[r] = d3[p * 3 + 1];
          g2[r] = d3[p * 3 + 2];
        }
      }
    }
  }
};

// part: [gridDim.x][3C] bias partials, NULL without d_bias; d_z may be NULL.
template <int S>
__global__ void __launch_bounds__(kThreads) k_upc_bwd(const int32_t* __restrict__ label, const float* __restrict__ d3,
                                                      int B, int h, int w, int C, float* __restrict__ d_z,
                                                      float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float accb[];  // [4][3C]
  constexpr int NP = Window<S>::NP;
  const int NC3 = 3 * C;
  const int n_low = B * h * w;
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  float* mine = accb + wave * NC3;
  if (part)
    for (int ch = lane; ch < NC3; ch += 64) mine[ch] = 0.f;
  // per lane, the same for every pixel: the 2-D weights of its window positions, and which of them a pixel owns
  float wt[NP];
  bool own[NP];
#pragma unroll
  for (int r = 0; r < NP; r++) {
    const int e = r * 64 + lane;
    const int wy = e / (2 * S), wx = e % (2 * S);
    wt[r] = e < 4 * S * S ? window_weight(wy, S) * window_weight(wx, S) : 0.f;
    own[r] = wy >= S / 2 && wy < S / 2 + S && wx >= S / 2 && wx < S / 2 + S;
  }
  const int q0 = blockIdx.x * kCbPix + wave;
  Window<S> nxt;
  nxt.load(label, d3, q0, n_low, h, w, C);
  for (int q = q0; q < (blockIdx.x + 1) * kCbPix && q < n_low; q += kThreads / 64) {
    const Window<S> cur = nxt;
    nxt.load(label, d3, q + kThreads / 64 < (blockIdx.x + 1) * kCbPix ? q + kThreads / 64 : n_low, n_low, h, w, C);
    float* dz = d_z ? d_z + (size_t)q * NC3 : nullptr;
    int last = -1;
    for (;;) {
      int m = INT_MAX;
#pragma unroll
      for (int r = 0; r < NP; r++) m = (cur.lab[r] > last && cur.lab[r] < m) ? cur.lab[r] : m;
      m = wave_min_int(m);  // wave-uniform: the next class present
      const int stop = m == INT_MAX ? NC3 : 3 * m;
      if (dz)
        for (int ch = 3 * (last + 1) + lane; ch < stop; ch += 64) dz[ch] = 0.f;  // the classes between have no pixel
      if (m == INT_MAX) break;
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, b0 = 0.f, b1 = 0.f, b2 = 0.f;
#pragma unroll
      for (int r = 0; r < NP; r++) {
        if (cur.lab[r] == m) {
          a0 = a0 + wt[r] * cur.g0[r];
          a1 = a1 + wt[r] * cur.g1[r];
          a2 = a2 + wt[r] * cur.g2[r];
          if (own[r]) {
            b0 = b0 + cur.g0[r];
            b1 = b1 + cur.g1[r];
            b2 = b2 + cur.g2[r];
          }
        }
      }
      if (dz) {
        a0 = wave_tree_sum(a0);
        a1 = wave_tree_sum(a1);
        a2 = wave_tree_sum(a2);
        if (lane == 0) {
          dz[3 * m + 0] = a0;
          dz[3 * m + 1] = a1;
          dz[3 * m + 2] = a2;
        }
      }
      if (part) {
        b0 = wave_tree_sum(b0);
        b1 = wave_tree_sum(b1);
        b2 = wave_tree_sum(b2);
        if (lane == 0) {  // this lane alone reads and writes the sums until the barrier below
          mine[3 * m + 0] = mine[3 * m + 0] + b0;
          mine[3 * m + 1] = mine[3 * m + 1] + b1;
          mine[3 * m + 2] = mine[3 * m + 2] + b2;
        }
      }
      last = m;
    }
  }
  if (part) {
    __syncthreads();
    for (int ch = threadIdx.x; ch < NC3; ch += kThreads) {
      float v = accb[ch];
      for (int wv = 1; wv < kThreads / 64; wv++) v = v + accb[wv * NC3 + ch];
      part[(size_t)blockIdx.x * NC3 + ch] = v;
    }
  }
}

// out[e] = the P partials' element e added in range order: one element per lane, a contiguous group of the
// ranges per wave, then the groups in order.
__global__ void __launch_bounds__(kFoldWaves * 64) k_up_fold(const float* __restrict__ part, int P, int n,
                                                             float* __restrict__ out) {
  __shared__ float red[kFoldWaves][64];
  const int lane = lane_id(), wave = threadIdx.x >> 6;
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
    out[e] = v;
  }
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

inline int log2_stride(int s) { return s == 2 ? 1 : s == 4 ? 2 : s == 8 ? 3 : s == 16 ? 4 : 0; }

inline int vec_of(int Ch) { return Ch % 4 == 0 ? 4 : Ch % 2 == 0 ? 2 : 1; }

inline bool dims_ok(int B, int h, int w, int Ch, int s) {
  if (B <= 0 || h <= 0 || w <= 0 || Ch <= 0 || !log2_stride(s)) return false;
  if (h > INT_MAX / s || w > INT_MAX / s) return false;
  const long H = (long)h * s, W = (long)w * s;
  if (H * W >= (1l << 31) || B * H * W >= (1l << 31)) return false;
  return B * H * W * (Ch > 3 ? Ch : 3) < (1l << 31);
}

// the compact pair: C classes, 3C channels at low resolution
inline bool compact_dims_ok(int B, int h, int w, int C, int s) {
  if (C <= 0 || C > kCbMaxC) return false;
  if (!dims_ok(B, h, w, 3, s)) return false;
  return (long)B * h * w * 3 * C < (1l << 31);
}

inline Tiling fwd_tiling(int w, int Ch, int s) {
  Tiling t;
  t.cc = Ch < 2048 ? Ch : 2048;
  t.ncc = (Ch + t.cc - 1) / t.cc;
  int nj = kFwdLdsFloats / 2 / t.cc - 1;  // (nj + 1) columns of two rows in LDS
  const int by_row = 8192 / (s * t.cc);   // about 8192 floats per output row of a tile
  if (nj > by_row) nj = by_row;
  if (nj < 1) nj = 1;
  if (nj > w + 1) nj = w + 1;
  t.nj = nj;
  t.ntj = (w + 1 + nj - 1) / nj;
  return t;
}

inline Tiling bwd_tiling(int w, int Ch, int s) {
  Tiling t;
  const int per_col = kBwdLdsFloats / 3 / s;  // channels x (nj + 1) each of the three LDS arrays holds
  t.cc = 2 * Ch <= per_col ? Ch : per_col / 2 / 4 * 4;
  t.ncc = (Ch + t.cc - 1) / t.cc;
  int nj = per_col / t.cc - 1;
  if (nj < 1) nj = 1;
  if (nj > w) nj = w;
  t.nj = nj;
  t.ntj = (w + nj - 1) / nj;
  return t;
}

inline int bwd_strips(int h) { return (h + kBwdRows - 1) / kBwdRows; }

inline int compact_blocks(int B, int h, int w) { return (int)(((long)B * h * w + kCbPix - 1) / kCbPix); }

template <int V>
void launch_fwd(const float* x, const float* bias, int B, int h, int w, int Ch, int ls, int relu, const Tiling& tl,
                float* y, hipStream_t st) {
  const int grid = B * (h + 1) * tl.ntj * tl.ncc;
  const uint32_t lds = (uint32_t)(2 * (tl.nj + 1) * tl.cc * sizeof(float));
  pcnn::launch_last(k_up_fwd<V>, dim3(grid), dim3(kThreads), lds, st, x, bias, B, h, w, Ch, ls, relu, tl, y);
}

template <int V>
void launch_bwd(bool last, const float* dy, const float* yv, int B, int h, int w, int Ch, int ls, const Tiling& tl,
                float* d_x, float* part, hipStream_t st) {
  const int grid = B * bwd_strips(h) * tl.ntj * tl.ncc;
  const uint32_t lds = (uint32_t)(3 * (tl.nj + 1) * (1 << ls) * tl.cc * sizeof(float));
  if (last) pcnn::launch_last(k_up_bwd<V>, dim3(grid), dim3(kThreads), lds, st, dy, yv, B, h, w, Ch, ls, tl, d_x, part);
  else hipLaunchKernelGGL(k_up_bwd<V>, dim3(grid), dim3(kThreads), lds, st, dy, yv, B, h, w, Ch, ls, tl, d_x, part);
}

template <int S>
void launch_compact_bwd(bool last, const int32_t* label, const float* d3, int B, int h, int w, int C, float* d_z,
                        float* part, hipStream_t st) {
  const int grid = compact_blocks(B, h, w);
  const uint32_t lds = (uint32_t)((kThreads / 64) * 3 * C * sizeof(float));
  if (last) pcnn::launch_last(k_upc_bwd<S>, dim3(grid), dim3(kThreads), lds, st, label, d3, B, h, w, C, d_z, part);
  else hipLaunchKernelGGL(k_upc_bwd<S>, dim3(grid), dim3(kThreads), lds, st, label, d3, B, h, w, C, d_z, part);
}

}  // namespace

extern "C" int pcnn_upscore_fwd(const float* x, int B, int h, int w, int Ch, int stride, const float* bias, int relu,
                                float* y, void* stream) {
  PCNN_REQUIRE(x && y);
  PCNN_REQUIRE(dims_ok(B, h, w, Ch, stride));
  const int V = vec_of(Ch);
  PCNN_REQUIRE(aligned(x, 4) && aligned(bias, 4) && aligned(y, 16));
  const Tiling tl = fwd_tiling(w, Ch, stride);
  const int ls = log2_stride(stride);
  hipStream_t st = (hipStream_t)stream;
  if (V == 4) launch_fwd<4>(x, bias, B, h, w, Ch, ls, relu ? 1 : 0, tl, y, st);
  else if (V == 2) launch_fwd<2>(x, bias, B, h, w, Ch, ls, relu ? 1 : 0, tl, y, st);
  else launch_fwd<1>(x, bias, B, h, w, Ch, ls, relu ? 1 : 0, tl, y, st);
  PCNN_CHECK_LAUNCH();
  return PCNN_OK;
}

extern "C" size_t pcnn_upscore_bwd_workspace_size(int B, int h, int w, int Ch, int stride) {
  if (!dims_ok(B, h, w, Ch, stride)) return 0;
  const Tiling tl = bwd_tiling(w, Ch, stride);
  return pcnn::align_up((size_t)B * bwd_strips(h) * tl.ntj * Ch * sizeof(float), 256);
}

extern "C" int pcnn_upscore_bwd(const float* d_y, const float* y, int B, int h, int w, int Ch, int stride, float* d_x,
                                float* d_bias, void* workspace, size_t workspace_bytes, void* stream) {
  PCNN_REQUIRE(d_y && d_x);
  PCNN_REQUIRE(dims_ok(B, h, w, Ch, stride));
  PCNN_REQUIRE(aligned(d_y, 16) && aligned(y, 16) && aligned(d_x, 4) && aligned(d_bias, 4));
  if (d_bias) {
    PCNN_REQUIRE(workspace && aligned(workspace, 16));
    if (workspace_bytes < pcnn_upscore_bwd_workspace_size(B, h, w, Ch, stride)) return PCNN_ECAPACITY;
  }
  const Tiling tl = bwd_tiling(w, Ch, stride);
  // the sums over the rows do not look at pixel borders: with all channels in one chunk a tile's row is one
  // run of floats, read 16 bytes at a time wherever every run starts and ends on a multiple of four floats
  const int V = (tl.ncc == 1 && (stride / 2) * Ch % 4 == 0) ? 4 : vec_of(Ch);
  const int ls = log2_stride(stride);
  hipStream_t st = (hipStream_t)stream;
  float* part = d_bias ? (float*)workspace : nullptr;
  if (V == 4) launch_bwd<4>(!d_bias, d_y, y, B, h, w, Ch, ls, tl, d_x, part, st);
  else if (V == 2) launch_bwd<2>(!d_bias, d_y, y, B, h, w, Ch, ls, tl, d_x, part, st);
  else launch_bwd<1>(!d_bias, d_y, y, B, h, w, Ch, ls, tl, d_x, part, st);
  PCNN_CHECK_LAUNCH();
  if (d_bias) {
    pcnn::launch_last(k_up_fold, dim3((Ch + 63) / 64), dim3(kFoldWaves * 64), 0, st, (const float*)part,
                      B * bwd_strips(h) * tl.ntj, Ch, d_bias);
    PCNN_CHECK_LAUNCH();
  }
  return PCNN_OK;
}

extern "C" int pcnn_upscore_compact_fwd(const float* z, const float* bias, const int32_t* label, int B, int h, int w,
                                        int C, int stride, float* vertex3, void* stream) {
  PCNN_REQUIRE(z && bias && label && vertex3);
  PCNN_REQUIRE(compact_dims_ok(B, h, w, C, stride));
  PCNN_REQUIRE(aligned(z, 4) && aligned(bias, 4) && aligned(label, 4) && aligned(vertex3, 4));
  const long n_pix = (long)B * h * w * stride * stride;
  pcnn::launch_last(k_upc_fwd, dim3((unsigned)((n_pix + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                    (hipStream_t)stream, z, bias, label, B, h, w, C, log2_stride(stride), vertex3);
  PCNN_CHECK_LAUNCH();
  return PCNN_OK;
}

extern "C" size_t pcnn_upscore_compact_bwd_workspace_size(int B, int h, int w, int C, int stride) {
  if (!compact_dims_ok(B, h, w, C, stride)) return 0;
  return pcnn::align_up((size_t)compact_blocks(B, h, w) * 3 * C * sizeof(float), 256);
}

extern "C" int pcnn_upscore_compact_bwd(const int32_t* label, const float* d_vertex3, int B, int h, int w, int C,
                                        int stride, float* d_z, float* d_bias, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  PCNN_REQUIRE(d_z || d_bias);
  PCNN_REQUIRE(label && d_vertex3);
  PCNN_REQUIRE(compact_dims_ok(B, h, w, C, stride));
  PCNN_REQUIRE(aligned(label, 4) && aligned(d_vertex3, 4) && aligned(d_z, 4) && aligned(d_bias, 4));
  if (d_bias) {
    PCNN_REQUIRE(workspace && aligned(workspace, 16));
    if (workspace_bytes < pcnn_upscore_compact_bwd_workspace_size(B, h, w, C, stride)) return PCNN_ECAPACITY;
  }
  hipStream_t st = (hipStream_t)stream;
  float* part = d_bias ? (float*)workspace : nullptr;
  switch (stride) {
    case 2: launch_compact_bwd<2>(!d_bias, label, d_vertex3, B, h, w, C, d_z, part, st); break;
    case 4: launch_compact_bwd<4>(!d_bias, label, d_vertex3, B, h, w, C, d_z, part, st); break;
    case 8: launch_compact_bwd<8>(!d_bias, label, d_vertex3, B, h, w, C, d_z, part, st); break;
    default: launch_compact_bwd<16>(!d_bias, label, d_vertex3, B, h, w, C, d_z, part, st); break;
  }
  PCNN_CHECK_LAUNCH();
  if (d_bias) {
    pcnn::launch_last(k_up_fold, dim3((3 * C + 63) / 64), dim3(kFoldWaves * 64), 0, st, (const float*)part,
                      compact_blocks(B, h, w), 3 * C, d_bias);
    PCNN_CHECK_LAUNCH();
  }
  return PCNN_OK;
}
