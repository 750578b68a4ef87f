// ADD / ADD-S pose loss for PoseCNN on MI355X (gfx950).
//
// Replaces AveragedistanceForwardLaucher / AveragedistanceBackwardLaucher
// (lib/average_distance_loss/average_distance_loss_op_gpu.cu.cc:34-377).
//
// The reference runs one thread per (row, point), re-deriving the row's six
// 3x3 matrices per point into a (R, P, 54) global scratch and the per-point
// gradient into a (R, P, 4C) scratch (~0.64 GB at R = 432), sums both
// sequentially per row, and reduces the row losses with thrust + a host copy.
//
// Here a workgroup owns (row, chunk of kPts points), one lane per point: the
// matrices live in registers; for symmetric classes the GT-rotated model
// points are staged once per workgroup in LDS (float4) and each lane scans
// them in index order as wave-uniform broadcasts (cu.cc:150-172, first
// minimum, strict <) — the reference's per-point loop, vectorised over points
// (by default that scan is replaced, item by item, by a bf16 MFMA filter and an
// exact re-check of the few candidates it leaves, with the same picks: "The
// filtered search" below).  Per-point loss and the four gradient terms use
// the reference's expressions and operation order (cu.cc:174-203) and are
// reduced in a fixed tree -> (R, chunks, 5) partials; one workgroup folds the
// partials per row and the rows into the scalar loss, in fixed order
// (deterministic; fp32 sums agree with the reference's sequential sums to
// ~1e-6 relative).
#include "pcnn_common.h"
#include "head_common.h"
#include <atomic>
#include <cfloat>
#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace {

#ifndef ADD_LANES
#define ADD_LANES 64
#endif
constexpr int kSymLanes = ADD_LANES;           // symmetric rows: lanes per candidate group
#ifndef ADD_GRID
#define ADD_GRID 1024
#endif
#ifndef ADD_PPL
#define ADD_PPL 4
#endif
constexpr int kPPL = ADD_PPL;                  // query points per lane (independent min chains)
constexpr int kPts = kSymLanes * kPPL;         // query points per (row, chunk) item
constexpr int kMaxPointsLds = 8192;            // float4 candidates in LDS (128 KB)

__device__ __forceinline__ int rows_of(const int32_t* dev, int cap) {
  if (!dev) return cap;
  int r = *dev;
  return r < cap ? r : cap;
}

// cu.cc:63-71 (unnormalised quaternion -> rotation)
__device__ __forceinline__ void quat2rot(float s, float u, float v, float w, float* r) {
  r[0] = s * s + u * u - v * v - w * w;
  r[1] = 2 * (u * v - s * w);
  r[2] = 2 * (u * w + s * v);
  r[3] = 2 * (u * v + s * w);
  r[4] = s * s - u * u + v * v - w * w;
  r[5] = 2 * (v * w - s * u);
  r[6] = 2 * (u * w - s * v);
  r[7] = 2 * (v * w + s * u);
  r[8] = s * s - u * u - v * v + w * w;
}

// x / b correctly rounded, for a b fixed per launch (the loss normaliser),
// from r = RN(1 / b): y0 = RN(x r) is within ~2 ulp of x / b; one fma
// correction y1 = RN(y0 + r (x - b y0)) leaves a relative error of ~2u^2 on
// top of its own rounding, so y1 is a faithful quotient; then its remainder
// x - b y1 is exact in one fma and RN(y1 + r (x - b y1)) is the correctly
// rounded x / b (Markstein's theorem: faithful y, r = RN(1/b), no underflow
// at these magnitudes) -- the reference's IEEE division (cu.cc:181,196-202)
// in five instructions instead of the ten of the generic division sequence.
// (One correction from y0 alone is not enough: y0 need not be faithful when
// x / b has its mantissa near 2.)  pcnn_div_rn_check exposes it to the tests.
// Same for the double form.
__device__ __forceinline__ float div_rn(float x, float b, float r) {
  const float y0 = x * r;
  const float y1 = fmaf(fmaf(-y0, b, x), r, y0);
  return fmaf(fmaf(-y1, b, x), r, y1);
}
__device__ __forceinline__ double div_rn(double x, double b, double r) {
  const double y0 = x * r;
  const double y1 = fma(fma(-y0, b, x), r, y0);
  return fma(fma(-y1, b, x), r, y1);
}

__global__ void k_div_rn_check(const float* __restrict__ x, float b, int n, int dbl, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (dbl) {
    const double bd = (double)b, rd = 1.0 / bd;
    out[i] = (float)div_rn((double)x[i], bd, rd);
  } else {
    out[i] = div_rn(x[i], b, 1.f / b);
  }
}

__device__ __forceinline__ int row_class(const float* __restrict__ weight, int n, int C) {
  // first class with weight > 0 (cu.cc:47-52); the row's weights are loaded
  // eight at a time with independent loads, not one dependent load per class
  const float* w = weight + (size_t)n * 4 * C;
  for (int i0 = 0; i0 < C; i0 += 8) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = i0 + j < C ? w[4 * (i0 + j)] : 0.f;
#pragma unroll
    for (int j = 0; j < 8; j++)
      if (v[j] > 0) return i0 + j;
  }
  return -1;
}

// One point's loss and gradient terms (cu.cc:174-203, the reference's
// expressions and operation order) added to acc[5]: X the model point,
// (x1, y1, z1) its rotation by the prediction (s, u, v, w), (x2, y2, z2) the
// GT-rotated point it is matched with; bn / ln the gradient's and the loss's
// normalisers with their reciprocals (div_rn).
__device__ __forceinline__ void add_point_terms(float X0, float X1, float X2, float x1, float y1, float z1, float x2,
                                                float y2, float z2, float s, float u, float v, float w, float margin,
                                                float bn, float rbn, double ln, double rln, float* acc) {
  const float dist = (x1 - x2) * (x1 - x2) + (y1 - y2) * (y1 - y2) + (z1 - z2) * (z1 - z2);
  if (dist < margin) return;  // cu.cc:178-179
  acc[0] += (float)div_rn((double)(dist - margin), ln, rln);  // cu.cc:181
  // derivative matrices of Rp w.r.t. (s, u, v, w) (cu.cc:97-139)
  const float d0[9] = {2 * s, -2 * w, 2 * v, 2 * w, 2 * s, -2 * u, -2 * v, 2 * u, 2 * s};
  const float d1[9] = {2 * u, 2 * v, 2 * w, 2 * v, -2 * u, -2 * s, 2 * w, 2 * s, -2 * u};
  const float d2[9] = {-2 * v, 2 * u, 2 * s, 2 * u, 2 * v, 2 * w, -2 * s, 2 * w, -2 * v};
  const float d3[9] = {-2 * w, -2 * s, 2 * u, 2 * s, -2 * w, 2 * v, 2 * u, 2 * v, 2 * w};
  const float X[3] = {X0, X1, X2};
  const float df[3] = {x1 - x2, y1 - y2, z1 - z2};
  float e0 = 0.f, e1 = 0.f, e2 = 0.f, e3 = 0.f;  // this point's terms, reference order
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) {  // cu.cc:183-203, same operation order
      e0 += div_rn(df[a] * X[b] * d0[a * 3 + b], bn, rbn);
      e1 += div_rn(df[a] * X[b] * d1[a * 3 + b], bn, rbn);
      e2 += div_rn(df[a] * X[b] * d2[a * 3 + b], bn, rbn);
      e3 += div_rn(df[a] * X[b] * d3[a * 3 + b], bn, rbn);
    }
  acc[1] += e0; acc[2] += e1; acc[3] += e2; acc[4] += e3;
}

// Non-symmetric rows (and rows without weight): kPts threads per row, points
// strided over them; the per-point arithmetic is k_add_rows' (cu.cc:140-203).
// Run as the tail items of k_add_rows' queue, after the symmetric items, so
// they fill the workgroups that finish the O(P^2) items early.  kRows = 1: the
// workgroup is kPts threads and takes row n0.  kRows = 2 (the 2 kPts-thread
// workgroup of the filtered search): its halves take rows n0 and n0 + 1, each
// with the summation geometry of kRows = 1 (points strided by kPts, one
// partial per wave, the row's four waves in order), so a row's sums have the
// same bits either way; the halves meet at one barrier, so nothing returns
// before it.
template <int kRows>
__device__ __forceinline__ void add_plain_rows(int n0, const float* __restrict__ pred,
                                               const float* __restrict__ target, const float* __restrict__ points,
                                               const float* __restrict__ symmetry, int R, int C, int P, float margin,
                                               int norm_rows, const int32_t* __restrict__ norm_rows_dev, int nchunk,
                                               const int32_t* __restrict__ rcls, float* __restrict__ partial,
                                               float (*red)[5]) {
  const int half = kRows == 2 ? (int)(threadIdx.x / kPts) : 0, tid = (int)(threadIdx.x % kPts);
  const int n = n0 + half;
  const bool live = n < R;
  const int cls = live ? rcls[n] : -1;
  const bool sym = cls >= 0 && symmetry[cls] > 0;  // the symmetric items own such a row
  float* out = partial + (size_t)(live ? n : 0) * nchunk * 5;
  if (live && !sym)
    for (int i = tid; i < nchunk * 5; i += kPts) out[i] = 0.f;
  const bool work = live && !sym && cls >= 0;
  float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (work) {
    const int PC = 4 * C;
    const float* tq = target + (size_t)n * PC + 4 * cls;
    const float* pq = pred + (size_t)n * PC + 4 * cls;
    float Rg[9], Rp[9];
    quat2rot(tq[0], tq[1], tq[2], tq[3], Rg);
    const float s = pq[0], u = pq[1], v = pq[2], w = pq[3];
    quat2rot(s, u, v, w, Rp);
    const int Rn = norm_rows_dev ? *norm_rows_dev : (norm_rows > 0 ? norm_rows : R);
    const float bn = (float)(Rn * P), rbn = 1.f / bn;
    const double ln = 2.0 * (double)Rn * (double)P, rln = 1.0 / ln;
    const float* pts = points + (size_t)cls * P * 3;
    for (int p = tid; p < P; p += kPts) {
      const float X0 = pts[p * 3 + 0], X1 = pts[p * 3 + 1], X2 = pts[p * 3 + 2];
      const float x1 = Rp[0] * X0 + Rp[1] * X1 + Rp[2] * X2;
      const float y1 = Rp[3] * X0 + Rp[4] * X1 + Rp[5] * X2;
      const float z1 = Rp[6] * X0 + Rp[7] * X1 + Rp[8] * X2;
      const float x2 = Rg[0] * X0 + Rg[1] * X1 + Rg[2] * X2;
      const float y2 = Rg[3] * X0 + Rg[4] * X1 + Rg[5] * X2;
      const float z2 = Rg[6] * X0 + Rg[7] * X1 + Rg[8] * X2;
      add_point_terms(X0, X1, X2, x1, y1, z1, x2, y2, z2, s, u, v, w, margin, bn, rbn, ln, rln, acc);
    }
  }
#pragma unroll
  for (int q = 0; q < 5; q++) acc[q] = pcnn::wave_sum(acc[q]);
  if (pcnn::lane_id() == 0)
    for (int q = 0; q < 5; q++) red[threadIdx.x >> 6][q] = acc[q];
  __syncthreads();
  if (work && tid < 5) {
    float t = 0.f;
    for (int i = 0; i < kPts / 64; i++) t += red[half * (kPts / 64) + i][tid];
    out[tid] = t;
  }
}

// Symmetric rows: a 256-thread workgroup owns (row, chunk of kPts = 256 query
// points); its four one-wave groups scan disjoint quarters of the candidate
// list for the same query points (kPPL = 4 chains per lane: each broadcast
// candidate read serves four distances), then merge in LDS in group order
// with a strict < — a later range wins only with a strictly smaller
// distance, which is exactly the reference's sequential first minimum
// (cu.cc:150-172).  Round 6 geometry sweep of the whole op on the bench's
// rows (scripts/add_bench.py, one box, profiles/r06/add_geometry_sweep.log):
// 8 groups / 768 workgroups 143-148 us; 4 groups 126-130 us (kept, with a
// 1024-workgroup grid: 124-130 us); kPPL 2 129-134 us; 16 groups, kPPL 8,
// blocks of 16: slower.  Half the workgroup, twice as many in flight: the
// merge and per-item staging cost less, and more items overlap the scans.
// Measured and dropped: a pruned search (Morton-ordered blocks of 8 points
// with bounding spheres, wave-uniform skips) visited 16 % of the blocks, but
// its sphere tests are a latency-bound chain: 314 us against this scan's
// 212 us on the bench's rows, at the geometry of the time (last in the tree
// at commit 5eb95d4).
#ifndef ADD_GROUPS
#define ADD_GROUPS 4
#endif
constexpr int kSymGroups = ADD_GROUPS;
constexpr int kSymThreads = kSymLanes * kSymGroups;
#ifndef ADD_BLK
#define ADD_BLK 8
#endif
constexpr int kBlk = ADD_BLK;  // candidates per block of the running-minimum scan

// ---------------------------------------------------------------------------
// The filtered search of a symmetric item (PCNN_ADD_SEARCH unset): the few
// candidates that can be a query's first minimum are found with bf16 MFMA,
// and only those are evaluated with the scan's fp32 expression.
//
// Filter value.  d(i, j) = |q_i|^2 + s(i, j), s(i, j) = |c_j|^2 - 2 q_i . c_j,
// so for one query the minimum of s is the minimum of d.  s~ is one
// v_mfma_f32_32x32x16_bf16 per (32 candidates x 32 queries): candidates are
// the M index (A operand, the LDS image), queries the N index (B operand, in
// registers), K = 16 slots per pair:
//   k = 4 a + {0, 1, 2, 3}, a = x, y, z:  A = c_h, c_h, c_m, c_m;  B = b_h, b_m, b_h, b_m
//   k = 12, 13, 14:  A = n_h, n_m, n_l;  B = 1;      k = 15: 0
// with b = -2 q, n = fl(|c|^2), x_h = bf16(x), x_m = bf16(x - x_h),
// x_l = bf16(x - x_h - x_m).  The result tile has the query on the lane
// (lane & 31) and candidates (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) of the
// block in the lane's 16 registers, so lanes l and l + 32 hold the two halves
// of a block for one query.
//
// Window.  With M^2 the item's largest |c_j|^2 or |q_i|^2 (fp32), u = 2^-8:
//  (a) |s~ - s| <= 6.8e-5 M^2:  x_h + x_m is x to 2^-16 relative, so the four
//      products of a coordinate miss c b by (2^-15 + 2^-32) |c_a| |b_a|, over
//      the three coordinates 2^-15 |c| |b| <= 2^-14 M^2 = 6.11e-5 M^2
//      (Cauchy-Schwarz, |b| = 2 |q|); n_h + n_m + n_l is n exactly and n is
//      |c|^2 to 4 * 2^-24; the 15 products are exact in fp32 and their sum,
//      in any order, rounded or truncated per step, is off by at most
//      16 * 2^-23 * (sum of magnitudes <= 1.02 (2 |c| |q| + |c|^2) <= 3.06 M^2)
//      = 5.9e-6 M^2;
//  (b) |d_fp32 - d| <= 5 * 2^-24 d <= 20 * 2^-24 M^2 = 1.2e-6 M^2 (three
//      rounded differences squared and summed, all terms >= 0, d <= 4 M^2).
// Let j* be the scan's pick and j^ the filter's minimum m~ = s~(j^):
//   s~(j*) <= s(j*) + a = d(j*) - |q|^2 + a <= d_fp32(j*) + b - |q|^2 + a
//          <= d_fp32(j^) + a + b - |q|^2 <= s(j^) + a + 2 b <= m~ + 2 (a + b),
// so the pick lies within 2 (a + b) = 1.39e-4 M^2 of m~; the window is
// kFiltWin M^2 = 2.8e-4 M^2, a safety factor of 2 (it also covers the rounding
// of m~ + window).  Proved for finite inputs with 2^-40 <= M^2 <= 2^40: no
// product or sum overflows, and what a bf16 plane or a product loses to
// underflow (< 2^-100) is far below the window; any other item (non-finite,
// all-zero, out of range) takes the exact scan.
//
// One pass of MFMAs: each lane keeps the minimum of every 32 x 32 tile it sees
// (8 v_min3 per MFMA) in registers; the minimum over them, merged over the
// lane pair and the workgroup's eight waves, which split the candidate
// blocks, gives the threshold, and one bit per block marks where the lane's
// tile minimum is within the window (a second pass of the same MFMAs, which
// would give the same bits, is what the registers save).  Walking the
// 16 values where a lane passes would diverge the wave at almost every MFMA
// (about 0.8 passing lanes per MFMA), so the passing (query, block, half)
// triples go to an LDS list instead and the whole workgroup evaluates them,
// one thread per triple (its 16 candidates, a superset of the candidates inside
// the window), with dist_to's expression; the winner is the minimum of
// (distance bits, index) as one 64-bit key -- the smaller distance, then the
// smaller index: the scan's sequential strict-< first minimum in any arrival
// order (distances are finite and >= +0 here, so their bits order as
// integers).  A full list is drained and refilled.
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kFiltWaves = 8;           // two waves per SIMD: one's v_min3 issue beside the other's MFMA
constexpr int kFiltThreads = 64 * kFiltWaves;
constexpr int kFiltMaxPoints = 2816;    // both images and the static arrays within 160 KB; <= 32 blocks a wave
constexpr int kFiltList = 1024;         // (query, block, half) triples per drain
constexpr int kFiltBlk = ((kFiltMaxPoints + 31) / 32 + kFiltWaves - 1) / kFiltWaves;  // blocks of 32 per wave
constexpr float kFiltWin = 2.8e-4f;     // window / M^2 (above)
constexpr float kFiltM2Min = 0x1p-40f, kFiltM2Max = 0x1p40f;
constexpr unsigned kFiltPadNorm = 0x7180u;  // bf16 2^100: a pad row's |c|^2 never passes a threshold

template <bool F>
struct FiltLds {};
template <>
struct FiltLds<true> {
  float4 sq[kPts];                // the item's query points
  float smin[kFiltWaves][kPts];   // the waves' minima per query
  unsigned long long skey[kPts];  // (distance bits, index) minima of the exact stage
  unsigned list[kFiltList];
  int cnt, m2;
};

__device__ __forceinline__ unsigned bf16_rn(float x) {  // finite x, round to nearest even
  const unsigned b = __float_as_uint(x);
  return (b + 0x7fffu + ((b >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ float bf16_val(unsigned h) { return __uint_as_float(h << 16); }
__device__ __forceinline__ void bf16_split2(float x, unsigned& h, unsigned& m) {
  h = bf16_rn(x);
  m = bf16_rn(x - bf16_val(h));  // the difference is exact
}

// A-operand row of candidate c (n = fl(|c|^2)): slots 0..7 and 8..15
__device__ __forceinline__ void filt_candidate(const float4& c, float n, u32x4& k0, u32x4& k8) {
  unsigned xh, xm, yh, ym, zh, zm;
  bf16_split2(c.x, xh, xm);
  bf16_split2(c.y, yh, ym);
  bf16_split2(c.z, zh, zm);
  const unsigned nh = bf16_rn(n);
  const float r1 = n - bf16_val(nh);
  const unsigned nm = bf16_rn(r1);
  const unsigned nl = bf16_rn(r1 - bf16_val(nm));
  k0 = (u32x4){xh | xh << 16, xm | xm << 16, yh | yh << 16, ym | ym << 16};
  k8 = (u32x4){zh | zh << 16, zm | zm << 16, nh | nm << 16, nl};
}

// minimum of m and a result tile's 16 values: 8 v_min3 in two independent
// chains (a dependent v_min3 does not issue back to back)
__device__ __forceinline__ float filt_min17(float m, const f32x16& v) {
  float a = fminf(fminf(v[0], v[1]), v[2]);
  float b = fminf(fminf(v[3], v[4]), v[5]);
  a = fminf(fminf(a, v[6]), v[7]);
  b = fminf(fminf(b, v[8]), v[9]);
  a = fminf(fminf(a, v[10]), v[11]);
  b = fminf(fminf(b, v[12]), v[13]);
  a = fminf(fminf(a, v[14]), v[15]);
  return fminf(fminf(m, a), b);
}

// Picks of the item's nq query points into s_imin (NF fragments of 32
// queries); returns the number of (query, block, half) triples evaluated.
template <int NF>
__device__ __forceinline__ int filter_search(FiltLds<true>& fl, const float4* gpts, const char* cimg, int P, int nq,
                                             float win, int* s_imin) {
  const int lane = pcnn::lane_id(), r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // uniform: scalar loop control
  // this wave's candidate blocks (<= 32), the remainder spread over the first waves
  const int nblk = (P + 31) >> 5, bq = nblk / kFiltWaves, brem = nblk % kFiltWaves;
  const int b0 = wave * bq + min(wave, brem), b1 = b0 + bq + (wave < brem ? 1 : 0);
  bf16x8 qb[NF];
#pragma unroll
  for (int f = 0; f < NF; f++) {
    const float4 q = fl.sq[f * 32 + r];
    unsigned xh, xm, yh, ym, zh, zm;
    bf16_split2(-2.f * q.x, xh, xm);
    bf16_split2(-2.f * q.y, yh, ym);
    bf16_split2(-2.f * q.z, zh, zm);
    const u32x4 w = h == 0 ? (u32x4){xh | xm << 16, xh | xm << 16, yh | ym << 16, yh | ym << 16}
                           : (u32x4){zh | zm << 16, zh | zm << 16, 0x3f803f80u, 0x00003f80u};
    qb[f] = __builtin_bit_cast(bf16x8, w);
  }
  const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const char* ap = cimg + r * 32 + h * 16;  // A fragment: row lane & 31, k = 8 (lane >> 5) .. + 7
  // One MFMA pass.  Each lane keeps the minimum of every (block, fragment)
  // tile it sees -- at most kFiltBlk x NF registers, the block loop unrolled
  // so that they are indexed statically -- so the threshold test needs no
  // second pass of the same MFMAs.  The MFMA of fragment f + 1 is issued
  // before the minimum of fragment f's tile, and the next block's A fragment
  // is read a block ahead, so the eight v_min3 of a tile run under the next
  // MFMA (the scheduling barriers keep that order; left alone the compiler
  // puts each tile's minimum right behind its MFMA, in the same registers,
  // and waits out the MFMA every time).
  float bmin[kFiltBlk][NF];
  bf16x8 a = *(const bf16x8*)(ap + min(b0, nblk - 1) * 1024);
#pragma unroll
  for (int k = 0; k < kFiltBlk; k++) {
    if (b0 + k < b1) {  // wave-uniform
      const bf16x8 an = *(const bf16x8*)(ap + min(b0 + k + 1, nblk - 1) * 1024);
      f32x16 v = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, qb[0], zero, 0, 0, 0);
#pragma unroll
      for (int f = 0; f < NF; f++) {
        f32x16 vn = v;
        if (f + 1 < NF) vn = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, qb[f + 1], zero, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        bmin[k][f] = filt_min17(FLT_MAX, v);
        __builtin_amdgcn_sched_barrier(0);
        v = vn;
      }
      a = an;
    } else {
#pragma unroll
      for (int f = 0; f < NF; f++) bmin[k][f] = FLT_MAX;  // no block: never within a window
    }
  }
  // the lane's minimum, merged over the lane pair and the waves
#pragma unroll
  for (int f = 0; f < NF; f++) {
    float m = bmin[0][f];
#pragma unroll
    for (int k = 1; k < kFiltBlk; k++) m = fminf(m, bmin[k][f]);
    m = fminf(m, __shfl_xor(m, 32, 64));
    if (h == 0) fl.smin[wave][f * 32 + r] = m;
  }
  __syncthreads();
  // one bit per block whose minimum is within the window of the query's minimum
  unsigned mask[NF];
#pragma unroll
  for (int f = 0; f < NF; f++) {
    float t = fl.smin[0][f * 32 + r];
#pragma unroll
    for (int g = 1; g < kFiltWaves; g++) t = fminf(t, fl.smin[g][f * 32 + r]);
    const float thr = t + win;
    unsigned mk = 0u;
#pragma unroll
    for (int k = 0; k < kFiltBlk; k++) mk |= bmin[k][f] <= thr ? 1u << k : 0u;
    mask[f] = mk;
  }
#pragma unroll
  for (int f = 0; f < NF; f++)
    if (f * 32 + r >= nq) mask[f] = 0u;  // the slots past a short chunk's queries
  int nrec = 0;
  for (;;) {
    // the wave's triples take consecutive list slots: one counter add per
    // wave (a prefix sum of the lanes' counts), not one per triple
    int mine = 0;
#pragma unroll
    for (int f = 0; f < NF; f++) mine += __popc(mask[f]);
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    const int total = __shfl(incl, 63, 64);
    int base = 0;
    if (lane == 0 && total > 0) base = atomicAdd(&fl.cnt, total);
    int pos = __shfl(base, 0, 64) + incl - mine;
    int pending = 0;
#pragma unroll
    for (int f = 0; f < NF; f++) {
      unsigned mk = mask[f];
      while (mk && pos < kFiltList) {  // a full list: the bits left stay for the next round
        const int bit = __ffs(mk) - 1;
        mk &= mk - 1;
        fl.list[pos++] = (unsigned)(f * 32 + r) << 16 | (unsigned)(b0 + bit) << 1 | (unsigned)h;
      }
      mask[f] = mk;
      pending |= mk != 0u;
    }
    __syncthreads();
    const int n = min(fl.cnt, kFiltList);
    // one thread per triple: its 16 candidates in index order, dist_to's
    // expression (no contraction), then one 64-bit minimum on the query's key
    for (int w = threadIdx.x; w < n; w += blockDim.x) {
      const unsigned rec = fl.list[w];
      const int qi = rec >> 16;
      const int i0 = (int)((rec >> 1) & 0x7fffu) * 32 + 4 * (int)(rec & 1u);
      const float4 q = fl.sq[qi];
      unsigned long long best = ~0ull;
#pragma unroll
      for (int reg = 0; reg < 16; reg++) {  // (unconditional clamped reads: all 16 in flight at once)
        const int idx = i0 + (reg & 3) + 8 * (reg >> 2);
        const float4 c = gpts[min(idx, P - 1)];
        const float d = (q.x - c.x) * (q.x - c.x) + (q.y - c.y) * (q.y - c.y) + (q.z - c.z) * (q.z - c.z);
        const unsigned long long key = (unsigned long long)__float_as_uint(d) << 32 | (unsigned long long)(unsigned)idx;
        if (idx < P && d < FLT_MAX && key < best) best = key;
      }
      if (best != ~0ull) atomicMin(&fl.skey[qi], best);
    }
    nrec += n;
    pending = __syncthreads_or(pending);
    if (!pending) break;
    if (threadIdx.x == 0) fl.cnt = 0;
    __syncthreads();
  }
  if (threadIdx.x < kPts) {
    const unsigned long long key = fl.skey[threadIdx.x];
    s_imin[threadIdx.x] = key == ~0ull ? -1 : (int)(unsigned)(key & 0xffffffffull);
  }
  return nrec;
}

template <bool kFilt>
__global__ void __launch_bounds__(kFilt ? kFiltThreads : kSymThreads) k_add_rows(const float* __restrict__ pred,
                                                           const float* __restrict__ target,
                                                           const float* __restrict__ weight,
                                                           const float* __restrict__ points,
                                                           const float* __restrict__ symmetry, int R_cap,
                                                           const int32_t* __restrict__ num_rois_dev, int C, int P,
                                                           float margin, int norm_rows,
                                                           const int32_t* __restrict__ norm_rows_dev, int nchunk,
                                                           const int32_t* __restrict__ rcls,
                                                           const int32_t* __restrict__ sym_rows,
                                                           const int32_t* __restrict__ nsym,
                                                           int32_t* __restrict__ queue,
                                                           int32_t* __restrict__ stats,
                                                           float* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) float4 gpts[];  // [P] GT-rotated points (+ the bf16 image)
  __shared__ FiltLds<kFilt> fl;
  __shared__ float mdist[kSymGroups - 1][kPts];                   // range minima of groups 1..kSymGroups-1
  __shared__ int midx[kSymGroups - 1][kPts];
  __shared__ float red[(kFilt ? kFiltThreads : kSymThreads) / 64][5];
  __shared__ int s_imin[kPts];
  const int R = rows_of(num_rois_dev, R_cap);
  const int sym_items = *nsym * nchunk;
  // then the plain rows (add_plain_rows): one per item, two in the filtered search's wider workgroup
  constexpr int kPlain = kFilt ? kFiltThreads / kPts : 1;
  const int items = sym_items + (R + kPlain - 1) / kPlain;
  const int grp = threadIdx.x / kSymLanes, lt = threadIdx.x % kSymLanes;
  const int quarter = ((P + kSymGroups - 1) / kSymGroups + kBlk - 1) / kBlk * kBlk;
  const int c0 = grp * quarter, c1 = min(P, c0 + quarter);
  // items are handed out by an atomic counter (zeroed by k_add_prep), so a
  // workgroup that finishes early takes the next (row, chunk)
  __shared__ int s_item;
  // (triples, not evaluations: an item has at most 256 x 88 x 2 = 45056 of them,
  // so the int32 sum holds for R_cap x chunks up to 47 000 even when every
  // half block of every item passes; 16 evaluations each)
  int st_filter = 0, st_scan = 0, st_triples = 0;
  for (;;) {
  __syncthreads();
  if (threadIdx.x == 0) {
    s_item = atomicAdd(queue, 1);
    if constexpr (kFilt) { fl.cnt = 0; fl.m2 = 0; }
  }
  __syncthreads();
  const int item = s_item;
  if (item >= items) break;
  if (item >= sym_items) {  // workgroup-uniform
    add_plain_rows<kPlain>((item - sym_items) * kPlain, pred, target, points, symmetry, R, C, P, margin, norm_rows,
                           norm_rows_dev, nchunk, rcls, partial, red);
    continue;  // the loop head synchronises before red is reused
  }
  // full chunks of every symmetric row first, the rows' short last chunks
  // (P % kPts points: cheaper, see the scan below) after them, so the short
  // ones fill the tail of the queue instead of opening a second round of
  // full-cost items
  const int nfull = P / kPts, nsym_rows = *nsym;
  int n, chunk, slot;
  if (item < nsym_rows * nfull) {
    slot = item / nfull;
    chunk = item % nfull;
  } else {
    slot = item - nsym_rows * nfull;
    chunk = nfull;
  }
  n = sym_rows[slot];
  const int PC = 4 * C;
  const int cls = rcls[n];
  float* out = partial + ((size_t)n * nchunk + chunk) * 5;
  const float* tq = target + (size_t)n * PC + 4 * cls;
  const float* pq = pred + (size_t)n * PC + 4 * cls;
  float Rg[9], Rp[9];
  quat2rot(tq[0], tq[1], tq[2], tq[3], Rg);
  const float s = pq[0], u = pq[1], v = pq[2], w = pq[3];
  quat2rot(s, u, v, w, Rp);
  const float* pts = points + (size_t)cls * P * 3;
  const int nq = min(kPts, P - chunk * kPts);  // query points of this item
  bool searched = false;
  int nrec = 0;  // kFilt: the search's (query, block, half) triples
  float Xt0 = 0.f, Xt1 = 0.f, Xt2 = 0.f;  // kFilt: this thread's query model point, kept for the tail
  if constexpr (kFilt) {
    // the fp32 image as below, the bf16 K = 16 image beside it and the item's
    // query points; the largest squared norm and whether all of them are in
    // the range the window is proved for
    char* cimg = (char*)gpts + (((size_t)P * sizeof(float4) + 31) & ~(size_t)31);
    const int Ppad = (P + 31) & ~31;
    float mx = 0.f;
    int bad = 0;
    // every load of the thread's model points is issued before the first is
    // used: one memory latency per item, not one per 512 points (a workgroup
    // has the CU to itself here, so nothing else would hide them)
    constexpr int kStage = (kFiltMaxPoints + kFiltThreads - 1) / kFiltThreads;
    float Xs[kStage][3];
#pragma unroll
    for (int k = 0; k < kStage; k++) {
      const int i = (int)threadIdx.x + k * kFiltThreads;
      const int ii = i < P ? i : 0;
      Xs[k][0] = pts[ii * 3 + 0]; Xs[k][1] = pts[ii * 3 + 1]; Xs[k][2] = pts[ii * 3 + 2];
    }
#pragma unroll
    for (int k = 0; k < kStage; k++) {
      const int i = (int)threadIdx.x + k * kFiltThreads;
      if (i >= Ppad) continue;
      u32x4 k0 = {0u, 0u, 0u, 0u}, k8 = {0u, 0u, kFiltPadNorm, 0u};  // a pad row: |c|^2 = 2^100
      if (i < P) {
        const float X0 = Xs[k][0], X1 = Xs[k][1], X2 = Xs[k][2];
        const float4 c = make_float4(Rg[0] * X0 + Rg[1] * X1 + Rg[2] * X2, Rg[3] * X0 + Rg[4] * X1 + Rg[5] * X2,
                                     Rg[6] * X0 + Rg[7] * X1 + Rg[8] * X2, 0.f);
        gpts[i] = c;
        const float nn = c.x * c.x + c.y * c.y + c.z * c.z;
        bad |= !(nn <= kFiltM2Max);  // also NaN
        mx = fmaxf(mx, nn);
        filt_candidate(c, nn, k0, k8);
      }
      *(u32x4*)(cimg + (size_t)i * 32) = k0;
      *(u32x4*)(cimg + (size_t)i * 32 + 16) = k8;
    }
    if (threadIdx.x < kPts) {
      const int p = chunk * kPts + (int)threadIdx.x;
      const int pp = p < P ? p : 0;
      const float X0 = pts[pp * 3 + 0], X1 = pts[pp * 3 + 1], X2 = pts[pp * 3 + 2];
      Xt0 = X0; Xt1 = X1; Xt2 = X2;
      const float4 q = make_float4(Rp[0] * X0 + Rp[1] * X1 + Rp[2] * X2, Rp[3] * X0 + Rp[4] * X1 + Rp[5] * X2,
                                   Rp[6] * X0 + Rp[7] * X1 + Rp[8] * X2, 0.f);  // = the tail's (x1, y1, z1)
      fl.sq[threadIdx.x] = q;
      const float nn = q.x * q.x + q.y * q.y + q.z * q.z;
      bad |= !(nn <= kFiltM2Max);
      mx = fmaxf(mx, nn);
      fl.skey[threadIdx.x] = ~0ull;
    }
    mx = pcnn::wave_max(mx);
    if (pcnn::lane_id() == 0) atomicMax(&fl.m2, __float_as_int(mx));  // >= 0: ordered as integers
    bad = __syncthreads_or(bad);
    const float m2 = __int_as_float(fl.m2);
    if (!bad && m2 >= kFiltM2Min) {  // workgroup-uniform
      nrec = nq > 64 ? filter_search<8>(fl, gpts, cimg, P, nq, kFiltWin * m2, s_imin)
                     : filter_search<2>(fl, gpts, cimg, P, nq, kFiltWin * m2, s_imin);
      searched = true;
    }
  } else {
  for (int i = threadIdx.x; i < P; i += blockDim.x) {
    const float X0 = pts[i * 3 + 0], X1 = pts[i * 3 + 1], X2 = pts[i * 3 + 2];
    gpts[i] = make_float4(Rg[0] * X0 + Rg[1] * X1 + Rg[2] * X2, Rg[3] * X0 + Rg[4] * X1 + Rg[5] * X2,
                          Rg[6] * X0 + Rg[7] * X1 + Rg[8] * X2, 0.f);
  }
  __syncthreads();
  }
  if (!searched) {  // the exact scan: forced, or an item outside the filter's range
  // kPPL query points per lane (points p0 + k*kSymLanes): each broadcast
  // candidate read serves kPPL distances and the lane carries kPPL
  // independent first-minimum chains
  float qx[kPPL], qy[kPPL], qz[kPPL], Xq[kPPL][3];
  int pq_[kPPL];
#pragma unroll
  for (int k = 0; k < kPPL; k++) {
    const int p = chunk * kPts + k * kSymLanes + lt;
    pq_[k] = p;
    const int pp = p < P ? p : 0;
    Xq[k][0] = pts[pp * 3 + 0]; Xq[k][1] = pts[pp * 3 + 1]; Xq[k][2] = pts[pp * 3 + 2];
    qx[k] = Rp[0] * Xq[k][0] + Rp[1] * Xq[k][1] + Rp[2] * Xq[k][2];
    qy[k] = Rp[3] * Xq[k][0] + Rp[4] * Xq[k][1] + Rp[5] * Xq[k][2];
    qz[k] = Rp[6] * Xq[k][0] + Rp[7] * Xq[k][1] + Rp[8] * Xq[k][2];
  }
  // Nearest GT-rotated model point of this group's range [c0, c1) with the
  // reference's first-minimum semantics (strict <, index order, NaN never
  // wins; cu.cc:150-172), in two exact steps: a running minimum over blocks
  // of kBlk candidates (block minimum by v_min3 -- fminf drops NaN like the
  // strict < does; the running minimum updates only on a strictly smaller
  // block minimum, remembering the block), then the first index of that block
  // whose distance, recomputed by the same expression, equals the minimum.
  // The per-candidate compare/select pair of a direct scan becomes ~1/2 min
  // (kBlk 8: one compare + two selects per 8 candidates instead of per 4).
  auto dist_to = [&](int k, const float4& c) {
    return (qx[k] - c.x) * (qx[k] - c.x) + (qy[k] - c.y) * (qy[k] - c.y) + (qz[k] - c.z) * (qz[k] - c.z);
  };
  float dmin[kPPL];
  int iblk[kPPL];
#pragma unroll
  for (int k = 0; k < kPPL; k++) { dmin[k] = FLT_MAX; iblk[k] = -1; }
  // query points in pairs (k, k + 1): every sub / mul / add of a distance is
  // one packed-fp32 instruction over two evaluations, in the scalar
  // expression's association order (bitwise the same as dist_to)
  typedef float f2 __attribute__((ext_vector_type(2)));
  f2 px[kPPL / 2], py[kPPL / 2], pz[kPPL / 2];
#pragma unroll
  for (int h = 0; h < kPPL / 2; h++) {
    px[h] = (f2){qx[2 * h], qx[2 * h + 1]};
    py[h] = (f2){qy[2 * h], qy[2 * h + 1]};
    pz[h] = (f2){qz[2 * h], qz[2 * h + 1]};
  }
  // NP query pairs per lane: an item whose queries fit in the first
  // 2 * kSymLanes lanes' slots (a row's short last chunk) scans with one pair
  auto scan = [&](auto np_c) {
    constexpr int NP = decltype(np_c)::value;
    int i = c0;
    for (; i + kBlk <= c1; i += kBlk) {
      float4 c[kBlk];
#pragma unroll
      for (int j = 0; j < kBlk; j++) c[j] = gpts[i + j];
#pragma unroll
      for (int h = 0; h < NP; h++) {
        f2 d[kBlk];
#pragma unroll
        for (int j = 0; j < kBlk; j++) {
          const f2 ex = px[h] - c[j].x, ey = py[h] - c[j].y, ez = pz[h] - c[j].z;
          d[j] = ex * ex + ey * ey + ez * ez;
        }
#pragma unroll
        for (int e = 0; e < 2; e++) {
          const int k = 2 * h + e;
          float bm = fminf(d[0][e], d[1][e]);  // min3 chains: (kBlk - 1) / 2 instructions
#pragma unroll
          for (int j = 2; j < kBlk; j += 2) bm = fminf(bm, fminf(d[j][e], d[j + 1][e]));
          if (bm < dmin[k]) { dmin[k] = bm; iblk[k] = i; }
        }
      }
    }
    for (; i < c1; i++) {  // ragged tail: blocks of one
      const float4 c = gpts[i];
#pragma unroll
      for (int k = 0; k < 2 * NP; k++) {
        const float d = dist_to(k, c);
        if (d < dmin[k]) { dmin[k] = d; iblk[k] = i; }
      }
    }
  };
  if (nq > 2 * kSymLanes) scan(std::integral_constant<int, kPPL / 2>{});
  else scan(std::integral_constant<int, 1>{});
  if (grp > 0 && grp < kSymGroups) {  // (kFilt: the workgroup's waves past the scan's groups have empty ranges)
#pragma unroll
    for (int k = 0; k < kPPL; k++) {
      mdist[grp - 1][k * kSymLanes + lt] = dmin[k];
      midx[grp - 1][k * kSymLanes + lt] = iblk[k];
    }
  }
  __syncthreads();
  if (grp == 0) {
#pragma unroll
    for (int k = 0; k < kPPL; k++) {
#pragma unroll
      for (int g = 0; g < kSymGroups - 1; g++) {  // group order, strict <: the earliest range wins ties
        const float d = mdist[g][k * kSymLanes + lt];
        if (d < dmin[k]) { dmin[k] = d; iblk[k] = midx[g][k * kSymLanes + lt]; }
      }
      int im = -1;
      if (iblk[k] >= 0) {
        const int e = min(iblk[k] + kBlk, P);
        for (int j = iblk[k]; j < e; j++)
          if (dist_to(k, gpts[j]) == dmin[k]) { im = j; break; }
      }
      s_imin[k * kSymLanes + lt] = im;
    }
  }
  }
  __syncthreads();
  // per-point loss and gradient terms (cu.cc:174-203), one point per thread
  // over the whole workgroup
  float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (int jj = threadIdx.x; jj < kPts; jj += blockDim.x) {
    const int p = chunk * kPts + jj;
    if (p >= P) continue;
    const int im = s_imin[jj] < 0 ? p : s_imin[jj];  // no finite distance (index_min unset in the reference)
    static_assert(kPts == kSymThreads, "one tail point per thread: jj == threadIdx.x");
    const float X0 = kFilt ? Xt0 : pts[p * 3 + 0], X1 = kFilt ? Xt1 : pts[p * 3 + 1], X2 = kFilt ? Xt2 : pts[p * 3 + 2];
    const float x1 = Rp[0] * X0 + Rp[1] * X1 + Rp[2] * X2;  // = the scan's query point, same expression
    const float y1 = Rp[3] * X0 + Rp[4] * X1 + Rp[5] * X2;
    const float z1 = Rp[6] * X0 + Rp[7] * X1 + Rp[8] * X2;
    const float4 cm = gpts[im];
    const int Rn = norm_rows_dev ? *norm_rows_dev : (norm_rows > 0 ? norm_rows : R);
    const float bn = (float)(Rn * P), rbn = 1.f / bn;
    const double ln = 2.0 * (double)Rn * (double)P, rln = 1.0 / ln;
    add_point_terms(X0, X1, X2, x1, y1, z1, cm.x, cm.y, cm.z, s, u, v, w, margin, bn, rbn, ln, rln, acc);
  }
#pragma unroll
  for (int q = 0; q < 5; q++) acc[q] = pcnn::wave_sum(acc[q]);
  if (pcnn::lane_id() == 0 && threadIdx.x < kSymThreads)
    for (int q = 0; q < 5; q++) red[threadIdx.x >> 6][q] = acc[q];
  __syncthreads();
  if (threadIdx.x < 5) {  // fixed order over the waves
    float t = 0.f;
    for (int i = 0; i < kSymThreads / 64; i++) t += red[i][threadIdx.x];
    out[threadIdx.x] = t;
  }
  if (searched) {  // the search counters: kept by the workgroup, added once when it leaves
    st_filter++;
    st_triples += nrec;
  } else {
    st_scan++;
  }
  __syncthreads();  // red / gpts / mdist reused by the next item
  }
  if (threadIdx.x == 0) {
    if (st_filter) atomicAdd(stats + 0, st_filter);
    if (st_scan) atomicAdd(stats + 1, st_scan);
    if (st_triples) atomicAdd(stats + 2, st_triples);
  }
}

// Row classes once (first class with weight > 0, cu.cc:47-52) and the
// ascending list of symmetric rows (ballot scan, one workgroup: deterministic).
__global__ void __launch_bounds__(1024) k_add_prep(const float* __restrict__ weight, const float* __restrict__ symmetry,
                                                    int R_cap, const int32_t* __restrict__ num_rois_dev, int C,
                                                    int32_t* __restrict__ rcls, int32_t* __restrict__ sym_rows,
                                                    int32_t* __restrict__ nsym, int32_t* __restrict__ queue,
                                                    int32_t* __restrict__ stats) {
  __shared__ int wcount[16];
  __shared__ int base;
  const int R = rows_of(num_rois_dev, R_cap);
  const int lane = pcnn::lane_id(), wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) base = 0;
  __syncthreads();
  for (int n0 = 0; n0 < R; n0 += blockDim.x) {
    const int n = n0 + threadIdx.x;
    int cls = -1;
    if (n < R) {
      cls = row_class(weight, n, C);
      rcls[n] = cls;
    }
    const bool sym = n < R && cls >= 0 && symmetry[cls] > 0;
    const uint64_t m = __ballot(sym);
    if (lane == 0) wcount[wave] = __popcll(m);
    __syncthreads();
    int off = base;
    for (int w = 0; w < wave; w++) off += wcount[w];
    if (sym) sym_rows[off + __popcll(m & pcnn::lanemask_lt())] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
      int t = 0;
      for (int w = 0; w < (int)(blockDim.x >> 6); w++) t += wcount[w];
      base += t;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *nsym = base;
    *queue = 0;
    stats[0] = stats[1] = stats[2] = 0;  // k_add_rows' search counters
  }
}

// Row n's five sums over its chunk partials, by one wave in a fixed tree.
__device__ __forceinline__ void fold_row(int n, int nchunk, const float* __restrict__ partial, int lane, float* s) {
#pragma unroll
  for (int q = 0; q < 5; q++) s[q] = 0.f;
  for (int k = lane; k < nchunk; k += 64)
    for (int q = 0; q < 5; q++) s[q] += partial[((size_t)n * nchunk + k) * 5 + q];
#pragma unroll
  for (int q = 0; q < 5; q++) s[q] = pcnn::wave_sum(s[q]);
}

__device__ __forceinline__ void finish_row(int n, int R, int C, int nchunk, const int32_t* __restrict__ rcls,
                                           const float* __restrict__ partial, float* __restrict__ row_loss,
                                           float* __restrict__ bottom_diff, int lane) {
  if (n >= R) return;
  const int cls = rcls[n];
  float s[5];
  fold_row(n, nchunk, partial, lane, s);
  const int PC = 4 * C;
  for (int col = lane; col < PC; col += 64) {
    float vv = 0.f;
    if (cls >= 0 && col >= 4 * cls && col < 4 * cls + 4) vv = s[1 + col - 4 * cls];
    bottom_diff[(size_t)n * PC + col] = vv;
  }
  if (lane == 0) row_loss[n] = cls >= 0 ? s[0] : 0.f;
}

// One wave per row: fold the chunk partials (fixed tree), write the row of
// bottom_diff (zeros except the class's 4 channels) and the row loss.
// Measured and dropped: the scalar total added by the last workgroup to
// finish (device-scope counter): the agent-scope release fence of each of the
// 288 workgroups writes back the XCD's L2, 12 -> 25 us for the pair of launches.
__global__ void __launch_bounds__(256) k_add_finish_rows(int R_cap, const int32_t* __restrict__ num_rois_dev, int C,
                                                          int nchunk, const int32_t* __restrict__ rcls,
                                                          const float* __restrict__ partial,
                                                          float* __restrict__ row_loss,
                                                          float* __restrict__ bottom_diff) {
  const int R = rows_of(num_rois_dev, R_cap);
  const int n = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  finish_row(n, R, C, nchunk, rcls, partial, row_loss, bottom_diff, pcnn::lane_id());
}

// k_add_finish_rows + the pose head's backward in one pass (the step's fused
// tail, pcnn_add_loss_fwd_head_bwd): the row's four gradient sums go straight
// into d pred (times the ADD gradient op's top_diff[0], cu.cc:346-354) and on
// through tanh * poses_weight -> l2_normalize (pose_head.hip k_head_bwd, the
// same helper), so the d_pred row is never re-read.  4 C <= 256.
__global__ void __launch_bounds__(256) k_add_finish_head(int R_cap, const int32_t* __restrict__ num_rois_dev, int C,
                                                          int nchunk, const int32_t* __restrict__ rcls,
                                                          const float* __restrict__ partial,
                                                          float* __restrict__ row_loss,
                                                          float* __restrict__ bottom_diff,
                                                          const float* __restrict__ t_in,
                                                          const float* __restrict__ pw,
                                                          const float* __restrict__ pred,
                                                          const float* __restrict__ dscale, float* __restrict__ dy8) {
  const int R = rows_of(num_rois_dev, R_cap);
  const int n = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = pcnn::lane_id();
  if (n >= R) return;
  const int cls = rcls[n];
  float s[5];
  fold_row(n, nchunk, partial, lane, s);
  const int PC = 4 * C;
  const float g = dscale ? dscale[0] : 1.f;
  float dp[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int col = lane + 64 * k;
    float vv = 0.f;
    if (cls >= 0 && col >= 4 * cls && col < 4 * cls + 4) vv = s[1 + col - 4 * cls];
    if (col < PC) bottom_diff[(size_t)n * PC + col] = vv;
    dp[k] = col < PC ? g * vv : 0.f;
  }
  if (lane == 0) row_loss[n] = cls >= 0 ? s[0] : 0.f;
  pcnn_head::head_bwd_row(dp, t_in, pw, pred, n, PC, lane, dy8);
}

// Scalar loss: fixed-order sum of the row losses (thrust::reduce, cu.cc:333-334).
__global__ void __launch_bounds__(1024) k_add_total(int R_cap, const int32_t* __restrict__ num_rois_dev,
                                                     const float* __restrict__ row_loss, float* __restrict__ loss) {
  __shared__ float red[16];
  const int R = rows_of(num_rois_dev, R_cap);
  float my = 0.f;
  for (int n = threadIdx.x; n < R; n += blockDim.x) my += row_loss[n];
  my = pcnn::wave_sum(my);
  if (pcnn::lane_id() == 0) red[threadIdx.x >> 6] = my;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int i = 0; i < (int)(blockDim.x >> 6); i++) t += red[i];
    loss[0] = t;
  }
}

__global__ void k_add_bwd(const float* __restrict__ top_diff, const float* __restrict__ bottom_diff, int n,
                          float* __restrict__ out) {
  const float g = top_diff[0];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = g * bottom_diff[i];
}

__global__ void k_add_bwd_rows(const float* __restrict__ top_diff, const float* __restrict__ bottom_diff,
                               const int32_t* __restrict__ num_rois_dev, int R_cap, int row_len,
                               float* __restrict__ out) {
  const float g = top_diff[0];
  const int n = rows_of(num_rois_dev, R_cap) * row_len;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = g * bottom_diff[i];
}

}  // namespace

extern "C" int pcnn_div_rn_check(const float* x, float b, int n, int dbl, float* out, void* stream) {
  PCNN_REQUIRE(x && out && n >= 0 && b != 0.f);
  if (n == 0) return PCNN_OK;
  hipLaunchKernelGGL(k_div_rn_check, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, b, n, dbl, out);
  PCNN_CHECK_LAUNCH();
  return PCNN_OK;
}

// The loss's workspace, carved the same way by every entry point.
struct AddWs {
  float* partial;
  int32_t *rcls, *sym_rows, *nsym, *queue;
  float* row_loss;
  int32_t* stats;  // symmetric items searched by the filter, by the scan; the filter's evaluated triples
  size_t stats_off;
};
static AddWs add_carve(void* workspace, int R_cap, int P, size_t* bytes) {
  const int nchunk = (P + kPts - 1) / kPts;
  const size_t R = (size_t)(R_cap > 0 ? R_cap : 1);
  pcnn::Carve cv(workspace);
  AddWs w;
  w.partial = cv.take<float>(R * nchunk * 5);
  w.rcls = cv.take<int32_t>(R);
  w.sym_rows = cv.take<int32_t>(R);
  w.nsym = cv.take<int32_t>(1);
  w.queue = cv.take<int32_t>(1);
  w.row_loss = cv.take<float>(R);
  w.stats = cv.take<int32_t>(4);
  w.stats_off = cv.off - 4 * sizeof(int32_t);
  if (bytes) *bytes = cv.off + 256;
  return w;
}

extern "C" size_t pcnn_add_loss_workspace_size(int R_cap, int C, int P) {
  (void)C;
  size_t b = 0;
  (void)add_carve(nullptr, R_cap, P, &b);
  return b;
}

// the row classification
static void add_launch_prep(const AddWs& w, const float* weight, const float* symmetry, int R_cap,
                            const int32_t* num_rois_dev, int C, hipStream_t st) {
  hipLaunchKernelGGL(k_add_prep, dim3(1), dim3(1024), 0, st, weight, symmetry, R_cap, num_rois_dev, C, w.rcls,
                     w.sym_rows, w.nsym, w.queue, w.stats);
}

// Dynamic LDS of the filtered search: the float4 image, then the bf16 image
// of the candidates padded to whole blocks of 32.
static size_t add_filter_lds(int P) {
  return (((size_t)P * sizeof(float4) + 31) & ~(size_t)31) + (size_t)((P + 31) & ~31) * 32;
}

// Whether the symmetric items of this launch take the filtered search:
// PCNN_ADD_SEARCH=scan (read at each launch; a test / A-B knob, both give the
// same bits) forces the exact scan, and so does a P whose two images do not
// fit the device's LDS beside the kernel's static arrays.
static bool add_use_filter(int P) {
  const char* mode = getenv("PCNN_ADD_SEARCH");
  if (mode && strcmp(mode, "scan") == 0) return false;
  if (P > kFiltMaxPoints) return false;
  // dynamic LDS the kernel may have; 0 not asked yet, -1 none (atomic: two host
  // threads' first launches may both ask, and store the same answer)
  static std::atomic<int> room[pcnn::kMaxDevices];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= pcnn::kMaxDevices) return false;
  int have = room[dev].load(std::memory_order_acquire);
  if (have == 0) {
    hipFuncAttributes fa;
    int lds = 0;
    have = -1;
    if (hipFuncGetAttributes(&fa, (const void*)k_add_rows<true>) == hipSuccess &&
        hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess &&
        lds > (int)fa.sharedSizeBytes) {
      const int dyn = lds - (int)fa.sharedSizeBytes;
      if (hipFuncSetAttribute((const void*)k_add_rows<true>, hipFuncAttributeMaxDynamicSharedMemorySize, dyn) ==
          hipSuccess)
        have = dyn;
    }
    if (have < 0) (void)hipGetLastError();  // only the error of a query that failed here
    room[dev].store(have, std::memory_order_release);
  }
  return have > 0 && add_filter_lds(P) <= (size_t)have;
}

// the per-point sums: one persistent grid over the symmetric (row, chunk)
// items of the device-side list, then the plain rows
static void add_launch_rows(const AddWs& w, const float* pred, const float* target, const float* weight,
                            const float* points, const float* symmetry, int R_cap, const int32_t* num_rois_dev,
                            int C, int P, float margin, int loss_norm_rows, const int32_t* loss_norm_rows_dev,
                            hipStream_t st) {
  const int nchunk = (P + kPts - 1) / kPts;
  const long items = (long)R_cap * nchunk + R_cap;
  const int grid = (int)(items < ADD_GRID ? items : ADD_GRID);
  if (add_use_filter(P))
    hipLaunchKernelGGL(k_add_rows<true>, dim3(grid), dim3(kFiltThreads), add_filter_lds(P), st, pred, target, weight,
                       points, symmetry, R_cap, num_rois_dev, C, P, margin, loss_norm_rows, loss_norm_rows_dev,
                       nchunk, w.rcls, w.sym_rows, w.nsym, w.queue, w.stats, w.partial);
  else
    hipLaunchKernelGGL(k_add_rows<false>, dim3(grid), dim3(kSymThreads), (size_t)P * sizeof(float4), st, pred,
                       target, weight, points, symmetry, R_cap, num_rois_dev, C, P, margin, loss_norm_rows,
                       loss_norm_rows_dev, nchunk, w.rcls, w.sym_rows, w.nsym, w.queue, w.stats, w.partial);
}

static int add_loss_fwd(const float* pred, const float* target, const float* weight, const float* points,
                        const float* symmetry, int R_cap, const int32_t* num_rois_dev, int C, int P, float margin,
                        int loss_norm_rows, const int32_t* loss_norm_rows_dev, float* loss, float* bottom_diff,
                        void* workspace, size_t workspace_bytes, bool prepared, void* stream) {
  PCNN_REQUIRE(pred && target && weight && points && symmetry && loss && bottom_diff && workspace);
  PCNN_REQUIRE(R_cap > 0 && C > 0 && P > 0 && P <= kMaxPointsLds);
  if (workspace_bytes < pcnn_add_loss_workspace_size(R_cap, C, P)) return PCNN_ECAPACITY;
  hipStream_t st = (hipStream_t)stream;
  const int nchunk = (P + kPts - 1) / kPts;
  const AddWs w = add_carve(workspace, R_cap, P, nullptr);
  if (!prepared) add_launch_prep(w, weight, symmetry, R_cap, num_rois_dev, C, st);
  add_launch_rows(w, pred, target, weight, points, symmetry, R_cap, num_rois_dev, C, P, margin, loss_norm_rows,
                  loss_norm_rows_dev, st);
  hipLaunchKernelGGL(k_add_finish_rows, dim3((R_cap + 3) / 4), dim3(256), 0, st, R_cap, num_rois_dev, C, nchunk,
                     w.rcls, w.partial, w.row_loss, bottom_diff);
  hipLaunchKernelGGL(k_add_total, dim3(1), dim3(1024), 0, st, R_cap, num_rois_dev, w.row_loss, loss);
  PCNN_CHECK_LAUNCH();
  return PCNN_OK;
}

// Byte offset, in the loss workspace, of the three int32 search counters that
// the row classification zeroes and the per-point sums add to.
extern "C" size_t pcnn_add_loss_stats_offset(int R_cap, int C, int P) {
  (void)C;
  return add_carve(nullptr, R_cap, P, nullptr).stats_off;
}

extern "C" int pcnn_add_loss_fwd(const float* pred, const float* target, const float* weight, const float* points,
                                 const float* symmetry, int R_cap, const int32_t* num_rois_dev, int C, int P,
                                 float margin, int loss_norm_rows, const int32_t* loss_norm_rows_dev, float* loss,
                                 float* bottom_diff, void* workspace, size_t workspace_bytes, void* stream) {
  return add_loss_fwd(pred, target, weight, points, symmetry, R_cap, num_rois_dev, C, P, margin, loss_norm_rows,
                      loss_norm_rows_dev, loss, bottom_diff, workspace, workspace_bytes, false, stream);
}

// The row classification of pcnn_add_loss_fwd on its own: it reads only the
// weights (the Hough op's targets), so a caller can run it as soon as they
// exist, on another stream, off the chain that produces the predictions.
extern "C" int pcnn_add_loss_prep(const float* weight, const float* symmetry, int R_cap, const int32_t* num_rois_dev,
                                  int C, int P, void* workspace, size_t workspace_bytes, void* stream) {
  PCNN_REQUIRE(weight && symmetry && workspace && R_cap > 0 && C > 0 && P > 0 && P <= kMaxPointsLds);
  if (workspace_bytes < pcnn_add_loss_workspace_size(R_cap, C, P)) return PCNN_ECAPACITY;
  const AddWs w = add_carve(workspace, R_cap, P, nullptr);
  add_launch_prep(w, weight, symmetry, R_cap, num_rois_dev, C, (hipStream_t)stream);
  PCNN_CHECK_LAUNCH();
  return PCNN_OK;
}

extern "C" int pcnn_add_loss_fwd_prepared(const float* pred, const float* target, const float* weight,
                                          const float* points, const float* symmetry, int R_cap,
                                          const int32_t* num_rois_dev, int C, int P, float margin,
                                          int loss_norm_rows, const int32_t* loss_norm_rows_dev, float* loss,
                                          float* bottom_diff, void* workspace, size_t workspace_bytes,
                                          void* stream) {
  return add_loss_fwd(pred, target, weight, points, symmetry, R_cap, num_rois_dev, C, P, margin, loss_norm_rows,
                      loss_norm_rows_dev, loss, bottom_diff, workspace, workspace_bytes, true, stream);
}

// The loss with the step's backward tail fused in (prepared rows only): the
// per-point sums (k_add_rows), then one pass that finishes each row's
// bottom_diff and runs the pose head's backward on it into d_y8
// (pcnn_pose_head_bwd with d_pred = bottom_diff, d_pred_scale the ADD
// gradient op's top_diff[0]: the same bits as the two separate launches).
// The scalar loss is left to pcnn_add_loss_total on the same workspace --
// nothing on the backward chain reads it, so a caller can run it on another
// stream after this call.  4 C <= 256.
extern "C" int pcnn_add_loss_fwd_head_bwd(const float* pred, const float* target, const float* weight,
                                          const float* points, const float* symmetry, int R_cap,
                                          const int32_t* num_rois_dev, int C, int P, float margin,
                                          int loss_norm_rows, const int32_t* loss_norm_rows_dev, float* bottom_diff,
                                          void* workspace, size_t workspace_bytes, const float* tanh_out,
                                          const float* d_pred_scale, float* d_y8, void* stream) {
  PCNN_REQUIRE(pred && target && weight && points && symmetry && bottom_diff && workspace && tanh_out && d_y8);
  PCNN_REQUIRE(R_cap > 0 && C > 0 && 4 * C <= 256 && P > 0 && P <= kMaxPointsLds);
  if (workspace_bytes < pcnn_add_loss_workspace_size(R_cap, C, P)) return PCNN_ECAPACITY;
  hipStream_t st = (hipStream_t)stream;
  const int nchunk = (P + kPts - 1) / kPts;
  const AddWs w = add_carve(workspace, R_cap, P, nullptr);
  add_launch_rows(w, pred, target, weight, points, symmetry, R_cap, num_rois_dev, C, P, margin, loss_norm_rows,
                  loss_norm_rows_dev, st);
  pcnn::launch_last(k_add_finish_head, dim3((R_cap + 3) / 4), dim3(256), 0, st, R_cap, num_rois_dev, C, nchunk,
                     w.rcls, w.partial, w.row_loss, bottom_diff, tanh_out, weight, pred, d_pred_scale, d_y8);
  PCNN_CHECK_LAUNCH();
  return PCNN_OK;
}

// The scalar loss of a pcnn_add_loss_fwd_head_bwd call (the row losses it left
// in the workspace, summed in the fixed order of pcnn_add_loss_fwd).
extern "C" int pcnn_add_loss_total(int R_cap, const int32_t* num_rois_dev, int C, int P, const void* workspace,
                                   size_t workspace_bytes, float* loss, void* stream) {
  PCNN_REQUIRE(workspace && loss && R_cap > 0 && C > 0 && P > 0);
  if (workspace_bytes < pcnn_add_loss_workspace_size(R_cap, C, P)) return PCNN_ECAPACITY;
  const AddWs w = add_carve(const_cast<void*>(workspace), R_cap, P, nullptr);
  hipLaunchKernelGGL(k_add_total, dim3(1), dim3(1024), 0, (hipStream_t)stream, R_cap, num_rois_dev, w.row_loss,
                     loss);
  PCNN_CHECK_LAUNCH();
  return PCNN_OK;
}

extern "C" int pcnn_add_loss_bwd(const float* top_diff, const float* bottom_diff, int n,
                                 const int32_t* num_rois_dev, int row_len, float* out, void* stream) {
  PCNN_REQUIRE(top_diff && bottom_diff && out && n >= 0);
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) return PCNN_OK;
  const int blocks = (n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024;
  if (num_rois_dev) {
    PCNN_REQUIRE(row_len > 0);
    hipLaunchKernelGGL(k_add_bwd_rows, dim3(blocks), dim3(256), 0, st, top_diff, bottom_diff, num_rois_dev,
                       n / row_len, row_len, out);
  } else {
    hipLaunchKernelGGL(k_add_bwd, dim3(blocks), dim3(256), 0, st, top_diff, bottom_diff, n, out);
  }
  PCNN_CHECK_LAUNCH();
  return PCNN_OK;
}
