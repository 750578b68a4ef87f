// estimatePose3D (synthesize.cpp:1769-1965) on the device.  The label lists,
// object ids and hypothesis bookkeeping are estimatePose2D's (pose_ransac.h,
// shared with pose2d.hip); the 3-D pieces:
//   k_p3d_eye: getEye / pxToEye (:1372-1407), the camera coordinates of the
//       raw depth (float arithmetic; holes at the origin);
//   k_p3d_valid: one bit per class-list position -- depth present -- so
//       that a round's subset can skip holes the way countInliers3D does
//       (:1255-1287: a hole advances to the next pixel without a draw);
//   k_p3d_subset: the rounds' subsets with holes: positions p_{j+1} =
//       next_valid(p_j + gap_j), the same Philox gaps as estimatePose2D.
//       A class without holes takes the parallel gap scan; otherwise one wave
//       walks 64 draws per step from the class's bits in LDS, the lanes up to
//       the first one landing on a hole accepted at once, that lane moved to
//       the next valid position (a wave-wide bit search) and the walk resumed;
//   k_attempts<true> / k_pick<true>: the sampling loop (:1814-1889);
//   k_p3d_count: countInliers3D over the round's subset (1 cm in double),
//       inlier bits per hypothesis;
//   k_select_sum: the partial counts summed, the stable halving (as
//       estimatePose2D);
//   k_p3d_update: updateHyp3D (:1347-1364) for every survivor, one wave
//       each: filterInliers3D (:1308-1322; pick k of round r on its own
//       stream (draw, h, 'F3D', 1024 r + k)), the inlier ranks resolved to
//       subset positions by a popcount prefix, then the rigid transform with
//       the workgroup-tree sums and the 3x3 Jacobi SVD;
//   k_p3d_finish: the survivor's output (:1936-1964): when it has more than
//       minPixels = 10 inliers, filterInliers3D again (r = 8) and
//       refineWithOpt (:1510-1567) -- the bounded Nelder-Mead over the
//       Rodrigues vector and translation (+-10 deg, +-0.1, +-0.1, +-0.5 m,
//       100 evaluations) of optEnergy3D (:1464-1507), one workgroup per
//       object, the energy's float sum in the workgroup tree; the search is
//       pcnn_nm::search (nelder_mead.h).
#include "nelder_mead.h"
#include "pose_ransac.h"

namespace {

// sin / cos / acos from + - * / sqrt only (the oracle's dsincos / dacos):
// quadrant reduction by a two-part pi/2, the fdlibm kernel polynomials; acos
// by the half-angle identity and 6 Newton steps on asin
__device__ void dsincos(double x, double& s, double& c) {
  const double n = floor(x * 0.63661977236758134308 + 0.5);
  const double y = (x - n * 1.57079632673412561417e+00) - n * 6.07710050650619224932e-11;
  const double z = y * y;
  const double ks = y + y * z * (-1.66666666666666324348e-01 + z * (8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 +
                        z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)))));
  const double kc = 1.0 - (0.5 * z - z * z * (4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05 +
                        z * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11))))));
  const int q = ((int)n) & 3;
  s = q == 0 ? ks : q == 1 ? kc : q == 2 ? -ks : -kc;
  c = q == 0 ? kc : q == 1 ? -ks : q == 2 ? -kc : ks;
}

__device__ double dasin_small(double x) {
  double y = x;
  for (int i = 0; i < 6; i++) {
    double s, c;
    dsincos(y, s, c);
    y = y - (s - x) / c;
  }
  return y;
}

__device__ double dacos(double c) {
  if (c >= 0) return 2.0 * dasin_small(sqrt((1.0 - c) * 0.5));
  return 3.14159265358979311600 - 2.0 * dasin_small(sqrt((1.0 + c) * 0.5));
}

// cv::Rodrigues vector -> matrix
__device__ void rod_v2m(const double* r, double* R) {
  const double th = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  if (th < 2.220446049250313e-16) {
    for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    return;
  }
  double s, c;
  dsincos(th, s, c);
  const double c1 = 1.0 - c, it = 1.0 / th;
  const double x = r[0] * it, y = r[1] * it, z = r[2] * it;
  const double rrt[9] = {x * x, x * y, x * z, x * y, y * y, y * z, x * z, y * z, z * z};
  const double rx[9] = {0, -z, y, z, 0, -x, -y, x, 0};
  for (int i = 0; i < 9; i++) R[i] = c * ((i % 4 == 0) ? 1.0 : 0.0) + c1 * rrt[i] + s * rx[i];
}

// cv::Rodrigues matrix -> vector (without cvRodrigues2's re-orthonormalisation)
__device__ void rod_m2v(const double* R, double* r) {
  double rx = R[7] - R[5], ry = R[2] - R[6], rz = R[3] - R[1];
  const double s = sqrt((rx * rx + ry * ry + rz * rz) * 0.25);
  double c = (R[0] + R[4] + R[8] - 1) * 0.5;
  c = c > 1. ? 1. : c < -1. ? -1. : c;
  double th = dacos(c);
  if (s < 1e-5) {
    if (c > 0) {
      rx = ry = rz = 0;
    } else {
      double t = (R[0] + 1) * 0.5;
      rx = sqrt(fmax(t, 0.));
      t = (R[4] + 1) * 0.5;
      ry = sqrt(fmax(t, 0.)) * (R[1] < 0 ? -1. : 1.);
      t = (R[8] + 1) * 0.5;
      rz = sqrt(fmax(t, 0.)) * (R[2] < 0 ? -1. : 1.);
      if (fabs(rx) < fabs(ry) && fabs(rx) < fabs(rz) && (R[5] > 0) != (ry * rz > 0)) rz = -rz;
      th /= sqrt(rx * rx + ry * ry + rz * rz);
      rx *= th;
      ry *= th;
      rz *= th;
    }
  } else {
    double vth = 1 / (2 * s);
    vth *= th;
    rx *= vth;
    ry *= vth;
    rz *= vth;
  }
  r[0] = rx;
  r[1] = ry;
  r[2] = rz;
}

struct P3dWs {
  P2dWs b;
  float* eye;       // (H W 3) camera coordinates
  uint64_t* valid;  // depth-present bits over the concatenated class lists (+ 2 pad words)
  uint64_t* imask;  // (n_hyp, mwords) inlier bits over the round's subset
  int32_t* pick;    // (n_hyp, kMaxInl) pixels of the last refit's correspondences
  int32_t* npick;   // (n_hyp)
  int mwords;
};

constexpr int kMaxInl = 1000;     // maxPixels: filterInliers3D's cap (:1796)
constexpr int kLdsWords = 5120;   // class-list bits kept in LDS by k_p3d_subset (327,680 positions)
constexpr int kSkipMax = 65536;   // class lists up to this long also get the per-position skip bytes
constexpr int kPrefWords = 2048;  // subset words with an LDS popcount prefix in k_p3d_update
constexpr int kFinThreads = 1024;  // k_p3d_finish workgroup (one correspondence per thread)

// the outputs' initial values (one launch instead of five fills)
__global__ void __launch_bounds__(1024) k_p3d_init(int C, int n_hyp, float* __restrict__ poses_out,
                                                   float* __restrict__ energy_out, int32_t* __restrict__ inl_out,
                                                   int32_t* __restrict__ final_out, int32_t* __restrict__ rm) {
  for (int i = threadIdx.x; i < 12 * C; i += 1024) poses_out[i] = 0.f;
  for (int i = threadIdx.x; i < C; i += 1024) {
    energy_out[i] = 0.f;
    rm[i] = 0;
  }
  for (int i = threadIdx.x; i < 3 * C; i += 1024) final_out[i] = -1;
  for (int i = threadIdx.x; i < kRounds * n_hyp; i += 1024) inl_out[i] = -1;
}

__global__ void __launch_bounds__(256) k_p3d_eye(const uint16_t* __restrict__ depth, int H, int W, float fx, float fy,
                                                 float px, float py, float factor, float* __restrict__ eye) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= H * W) return;
  const int x = p % W, y = p / W;
  const unsigned short d = depth[p];
  float e0 = 0.f, e1 = 0.f, e2 = 0.f;
  if (d != 0) {
    e0 = ((float)x - px) * (float)d / fx / factor;
    e1 = ((float)y - py) * (float)d / fy / factor;
    e2 = (float)d / factor;
  }
  eye[(size_t)p * 3] = e0;
  eye[(size_t)p * 3 + 1] = e1;
  eye[(size_t)p * 3 + 2] = e2;
}

// grid valid_blocks(HW): every word a class_word read may touch is written
inline int valid_blocks(int HW) { return (HW + 64 + 255) / 256; }

__global__ void __launch_bounds__(256) k_p3d_valid(int C, P3dWs w3) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int total = w3.b.listoff[C - 1] + w3.b.count[C - 1];
  const bool v = i < total && w3.eye[(size_t)w3.b.lists[i] * 3 + 2] != 0.f;
  const uint64_t b = __ballot(v);
  if (pcnn::lane_id() == 0) w3.valid[i >> 6] = b;
}

// bits [64 k, 64 k + 64) of the class list starting at global bit o, none past N
__device__ __forceinline__ uint64_t class_word(const uint64_t* __restrict__ V, long o, int N, long k) {
  const long b = o + 64 * k;
  const long w = b >> 6;
  const int sh = (int)(b & 63);
  uint64_t v = V[w] >> sh;
  if (sh) v |= V[w + 1] << (64 - sh);
  const long rem = (long)N - 64 * k;
  if (rem < 64) v &= rem <= 0 ? 0ull : ((1ull << rem) - 1);
  return v;
}

__global__ void __launch_bounds__(1024) k_p3d_subset(uint64_t seed, P3dWs w3) {
  __shared__ uint64_t bits[kLdsWords];  // 40 KiB
  __shared__ uint8_t skip[kSkipMax];     // 64 KiB
  __shared__ int wsum[16];
  __shared__ long qrel[1024];
  __shared__ int sh_int[4];
  const P2dWs& ws = w3.b;
  const int c = blockIdx.x, r = blockIdx.y, t = threadIdx.x, lane = pcnn::lane_id(), wave = t >> 6;
  const int N = ws.count[c];
  if (c == 0 || !((float)N > 400.0f)) return;  // not an object (block-uniform)
  int* S = ws.sub + (size_t)kRounds * ws.listoff[c] + (size_t)r * N;
  int* cnt_out = ws.subcnt + c * kRounds + r;
  const long o = ws.listoff[c];
  const int nw = (N + 63) / 64;
  const bool in_lds = nw <= kLdsWords;
  int nv = 0;
  for (int k = t; k < nw; k += 1024) {
    const uint64_t v = class_word(w3.valid, o, N, k);
    if (in_lds) bits[k] = v;
    nv += __popcll(v);
  }
  nv = pcnn::wave_sum(nv);
  if (t == 0) sh_int[0] = 0;
  __syncthreads();
  if (lane == 0) atomicAdd(&sh_int[0], nv);  // integer: order-free
  __syncthreads();
  nv = sh_int[0];
  auto word = [&](long k) -> uint64_t { return in_lds ? bits[k] : class_word(w3.valid, o, N, k); };
  const int maxPixels = 1000 * (r + 1);
  const float rate = maxPixels / (float)N;  // :1250
  if (!(rate < 1)) {  // every valid pixel in list order (:1283-1286)
    long carry = 0;
    for (int base = 0; base < nw; base += 1024) {  // ordered compaction, a word per thread
      const int k = base + t;
      const uint64_t v = k < nw ? word(k) : 0ull;
      const int pc = __popcll(v);
      int incl = pc;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(incl, d, 64);
        if (lane >= d) incl += y;
      }
      if (lane == 63) wsum[wave] = incl;
      __syncthreads();
      long wb = 0, tot = 0;
      for (int w = 0; w < 16; w++) {
        if (w < wave) wb += wsum[w];
        tot += wsum[w];
      }
      long pos = carry + wb + incl - pc;
      for (uint64_t m = v; m; m &= m - 1) S[pos++] = 64 * k + __ffsll((unsigned long long)m) - 1;
      __syncthreads();
      carry += tot;
    }
    if (t == 0) *cnt_out = nv;
    return;
  }
  const double q = 1.0 - (double)rate;
  if (nv == N) {  // no holes: estimatePose2D's subset
    subset_nohole(seed, c, r, N, q, S, cnt_out, wsum);
    return;
  }
  // skip[x] = next_valid(x) - x (0: x valid; 255: 255 or more, resolved by a
  // word search) when the class list fits kSkipMax bytes: one LDS byte per
  // walk step decides both "hole?" and "how far"
  const bool use_skip = N <= kSkipMax;  // block-uniform
  if (use_skip) {
    for (int x = t; x < N; x += 1024) {
      const int k = x >> 6;
      uint64_t w = word(k) >> (x & 63);
      int d = 0;
      if (!(w & 1ull)) {
        if (w) {
          d = __ffsll((unsigned long long)w) - 1;
        } else {
          d = 64 - (x & 63);
          for (int kk = k + 1; d < 255; kk++, d += 64) {
            if (kk >= nw) {
              d = N - x;  // no valid position after x: the walk leaves the list
              break;
            }
            const uint64_t v = word(kk);
            if (v) {
              d += __ffsll((unsigned long long)v) - 1;
              break;
            }
          }
        }
      }
      skip[x] = (uint8_t)(d < 255 ? d : 255);
    }
    __syncthreads();
  }
  long carry = 0;  // q_{j0}: the hole-free position of draw j0
  long D = 0;      // holes skipped so far (wave 0)
  for (int j0 = 0;; j0 += 1024) {
    const int g = p2d_gap(seed, c, r, j0 + t, q);
    int incl = g;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int y = __shfl_up(incl, d, 64);
      if (lane >= d) incl += y;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    long wb = 0, tot = 0;
    for (int w = 0; w < 16; w++) {
      if (w < wave) wb += wsum[w];
      tot += wsum[w];
    }
    qrel[t] = wb + incl - g;
    __syncthreads();
    if (wave == 0 && use_skip) {  // the lean walk: 32-bit positions, one LDS byte per step
      int done = 0, cnt = 0, Di = (int)D;  // D < N <= kSkipMax
      for (int sc = 0; sc < 16 && !done; sc++) {
        const int jl = sc * 64 + lane;
        const long ql = carry + qrel[jl];
        const int qj = ql < N ? (int)ql : N;  // every position at or past N means "past the list"
        int s = 0, pos = 0, nvalid = 64;
        for (;;) {  // wave-uniform; one hole hit resolved per step
          const int x = qj + Di;
          const int hv = x < N ? (int)skip[x] : 0;
          const bool ev = lane >= s && (x >= N || hv != 0);
          const uint64_t b = __ballot(ev);
          const int first = b ? __ffsll((unsigned long long)b) - 1 : 64;
          if (lane >= s && lane < first) pos = x;
          if (first == 64) break;
          const int xs = __builtin_amdgcn_readlane(x, first);
          int hs = __builtin_amdgcn_readlane(hv, first);
          if (xs < N && hs == 255) {  // a run of 255 or more holes: the word search
            long nh = N;
            for (long kb = (xs >> 6); kb < nw; kb += 64) {
              const long k = kb + lane;
              uint64_t v = k < nw ? bits[k] : 0ull;
              if (k == (xs >> 6)) v &= ~0ull << (xs & 63);
              const uint64_t hit = __ballot(v != 0ull);
              if (hit) {
                const int l = __ffsll((unsigned long long)hit) - 1;
                const uint64_t vv = __shfl((unsigned long long)v, l, 64);
                nh = 64 * (kb + l) + __ffsll((unsigned long long)vv) - 1;
                break;
              }
            }
            hs = (int)(nh - xs);
          }
          if (xs >= N || xs + hs >= N) {  // the walk leaves the list
            done = 1;
            cnt = j0 + sc * 64 + first;
            nvalid = first;
            break;
          }
          Di += hs;
          s = first;
        }
        if (lane < nvalid) S[j0 + jl] = pos;
      }
      D = Di;
      if (lane == 0) {
        sh_int[1] = done;
        sh_int[2] = cnt;
      }
    } else if (wave == 0) {  // class lists longer than kSkipMax: the bit walk
      int done = 0, cnt = 0;
      for (int sc = 0; sc < 16 && !done; sc++) {
        const int jl = sc * 64 + lane;
        const long qj = carry + qrel[jl];
        int s = 0;
        for (;;) {  // wave-uniform; one hole hit resolved per step
          const long x = qj + D;
          bool ev = false;
          if (lane >= s) ev = x >= N || !((word(x >> 6) >> (x & 63)) & 1ull);
          const uint64_t b = __ballot(ev);
          const int first = b ? __ffsll((unsigned long long)b) - 1 : 64;
          if (lane >= s && lane < first) S[j0 + jl] = (int)x;
          if (first == 64) break;
          const long xs = __shfl(x, first, 64);
          long nh = N;
          const uint64_t w0 = xs < N ? word(xs >> 6) >> (xs & 63) : 0ull;
          if (w0) {  // the hole run ends in this word (the usual case)
            nh = xs + __ffsll((unsigned long long)w0) - 1;
          } else if (xs < N) {  // the next valid position past this word (wave-wide word search)
            for (long kb = (xs >> 6) + 1; kb < nw; kb += 64) {
              const long k = kb + lane;
              const uint64_t v = k < nw ? word(k) : 0ull;
              const uint64_t hit = __ballot(v != 0ull);
              if (hit) {
                const int l = __ffsll((unsigned long long)hit) - 1;
                const uint64_t vv = __shfl((unsigned long long)v, l, 64);
                nh = 64 * (kb + l) + __ffsll((unsigned long long)vv) - 1;
                break;
              }
            }
          }
          if (nh >= N) {  // the walk leaves the list: draws j0 + sc 64 + first .. are not taken
            done = 1;
            cnt = j0 + sc * 64 + first;
            break;
          }
          D += nh - xs;
          s = first;
        }
      }
      if (lane == 0) {
        sh_int[1] = done;
        sh_int[2] = cnt;
      }
    }
    __syncthreads();
    if (sh_int[1]) {
      if (t == 0) *cnt_out = sh_int[2];
      return;
    }
    carry += tot;
  }
}

// grid (hypothesis slot, object, kCntZ): workgroup z takes the subset chunks
// z, z + kCntZ, ... of kCntChunk entries and writes its partial count (the
// chunks' inlier bits go to the hypothesis's mask)
__global__ void __launch_bounds__(256) k_p3d_count(const float* __restrict__ vm, const float* __restrict__ ext, int C,
                                                   P3dWs w3, int r) {
  __shared__ int part[4];
  const P2dWs& ws = w3.b;
  const int j = blockIdx.x, oi = blockIdx.y, z = blockIdx.z, lane = pcnn::lane_id(), wave = threadIdx.x >> 6;
  if (oi >= *ws.nobj || j >= ws.rm[oi]) return;  // block-uniform
  const int obj = ws.objs[oi];
  const int* L = ws.lists + ws.listoff[obj];
  const int h = ws.rl[oi * kMaxHypBlock + j];
  const int* S = ws.sub + (size_t)kRounds * ws.listoff[obj] + (size_t)r * ws.count[obj];
  const int ns = ws.subcnt[obj * kRounds + r];
  const double* hr = ws.hyp + (size_t)h * 16;
  Pose P;
  for (int i = 0; i < 9; i++) P.R[i] = hr[1 + i];
  for (int i = 0; i < 3; i++) P.t[i] = hr[10 + i];
  uint64_t* M = w3.imask + (size_t)h * w3.mwords;
  int cnt = 0;
  for (int c0 = z * kCntChunk; c0 < ns; c0 += (int)gridDim.z * kCntChunk) {  // countInliers3D (:1255-1287)
    for (int i0 = c0; i0 < c0 + kCntChunk && i0 < ns; i0 += 256) {
      const int i = i0 + threadIdx.x;
      bool in = false;
      if (i < ns) {
        const int p = L[S[i]];
        const F3 e = eye_at(w3.eye, p);
        const F3 o = mode3d(vm, ext, C, obj, p);
        in = nrm(sub(D3{e.x, e.y, e.z}, xform(P, D3{o.x, o.y, o.z}))) < 0.01;
      }
      const uint64_t b = __ballot(in);
      if (lane == 0 && i0 + 64 * wave < ns) M[(i0 >> 6) + wave] = b;
      cnt += in;
    }
  }
  cnt = pcnn::wave_sum(cnt);
  if (lane == 0) part[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) ws.pcnt[((size_t)oi * kMaxHypBlock + j) * kCntZ + z] = part[0] + part[1] + part[2] + part[3];
}

// the subset position of the rank-th set bit of M (pref: exclusive popcount
// prefix per word when the subset has at most kPrefWords words)
__device__ __forceinline__ int select_bit(const uint64_t* __restrict__ M, const int* pref, int nw, int rank) {
  int k = 0;
  if (nw <= kPrefWords) {
    int lo = 0, hi = nw - 1;  // the last word with pref <= rank
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (pref[mid] <= rank) lo = mid; else hi = mid - 1;
    }
    k = lo;
    rank -= pref[k];
  } else {
    for (;; k++) {
      const int pc = __popcll(M[k]);
      if (rank < pc) break;
      rank -= pc;
    }
  }
  uint64_t v = M[k];  // the rank-th set bit of v by halving
  int pos = 0;
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1) {
    const uint64_t low = (1ull << w) - 1;
    const int c = __popcll(v & low);
    if (rank >= c) {
      rank -= c;
      v >>= w;
      pos += w;
    } else {
      v &= low;
    }
  }
  return 64 * k + pos;
}

// one workgroup per survivor: the popcount prefix and the picks spread over
// 1024 threads (each pick on its own stream, one correspondence per thread),
// the centroid and covariance sums in the workgroup tree, the SVD on thread 0
__global__ void __launch_bounds__(1024) k_p3d_update(const float* __restrict__ vm, const float* __restrict__ ext,
                                                     int C, uint64_t seed, P3dWs w3, int r) {
  __shared__ int pref[kPrefWords];
  __shared__ int wsum[16];
  __shared__ double wc[16][6], wv[16][9];
  const P2dWs& ws = w3.b;
  const int j = blockIdx.x, oi = blockIdx.y, t = threadIdx.x, lane = pcnn::lane_id(), wave = t >> 6;
  if (oi >= *ws.nobj || j >= ws.rm[oi]) return;  // block-uniform
  const int n = ws.rc[oi * kMaxHypBlock + j];
  if (n < 4) return;  // :1350-1351
  const int obj = ws.objs[oi];
  const int h = ws.rl[oi * kMaxHypBlock + j];
  const int* L = ws.lists + ws.listoff[obj];
  const int* S = ws.sub + (size_t)kRounds * ws.listoff[obj] + (size_t)r * ws.count[obj];
  const int ns = ws.subcnt[obj * kRounds + r];
  const int nw = (ns + 63) / 64;
  const uint64_t* M = w3.imask + (size_t)h * w3.mwords;
  if (nw <= kPrefWords) {  // block-uniform
    int carry = 0;
    for (int base = 0; base < nw; base += 1024) {
      const int k = base + t;
      const int pc = k < nw ? __popcll(M[k]) : 0;
      int incl = pc;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(incl, d, 64);
        if (lane >= d) incl += y;
      }
      if (lane == 63) wsum[wave] = incl;
      __syncthreads();
      int wb = 0, tot = 0;
      for (int w = 0; w < 16; w++) {
        if (w < wave) wb += wsum[w];
        tot += wsum[w];
      }
      if (k < nw) pref[k] = carry + wb + incl - pc;
      __syncthreads();
      carry += tot;
    }
  }
  const int m = n >= kMaxInl ? kMaxInl : n;  // filterInliers3D (:1308-1322)
  const bool live = t < m;
  double a[3] = {0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
  if (live) {
    int rank = t;
    if (n >= kMaxInl) {
      Stream rs(seed, (uint32_t)h, kTagF3D, (uint32_t)(1024 * r + t));
      rank = rs.uniform(n);
    }
    const int p = L[S[select_bit(M, pref, nw, rank)]];
    const F3 o = mode3d(vm, ext, C, obj, p);
    const F3 e = eye_at(w3.eye, p);
    a[0] = o.x; a[1] = o.y; a[2] = o.z;
    b[0] = e.x; b[1] = e.y; b[2] = e.z;
    w3.pick[(size_t)h * kMaxInl + t] = p;
  }
  if (t == 0) w3.npick[h] = m;
  // Hypothesis::refine (:1359): calcRigidBodyTransform's sums in the tree
  for (int i = 0; i < 3; i++) {
    const double sa = wave_fold(live ? 0.0 + a[i] : 0.0), sb = wave_fold(live ? 0.0 + b[i] : 0.0);
    if (lane == 0) {
      wc[wave][i] = sa;
      wc[wave][3 + i] = sb;
    }
  }
  __syncthreads();
  const double inv = 1.0 / (double)m;
  double cA[3], cB[3];
  for (int i = 0; i < 3; i++) {
    cA[i] = cross_fold<double, 6>(wc, i) * inv;
    cB[i] = cross_fold<double, 6>(wc, 3 + i) * inv;
  }
  for (int rr = 0; rr < 3; rr++)
    for (int cc = 0; cc < 3; cc++) {
      const double v = wave_fold(live ? 0.0 + (a[rr] - cA[rr]) * (b[cc] - cB[cc]) : 0.0);
      if (lane == 0) wv[wave][rr * 3 + cc] = v;
    }
  __syncthreads();
  if (t != 0) return;
  double Hc[9];
  for (int i = 0; i < 9; i++) Hc[i] = cross_fold<double, 9>(wv, i);
  const Pose P = rigid_from_cov_ool(Hc, cA, cB);
  double* hr = ws.hyp + (size_t)h * 16;
  for (int i = 0; i < 9; i++) hr[1 + i] = P.R[i];
  for (int i = 0; i < 3; i++) hr[10 + i] = P.t[i];
}

// optEnergy3D (:1464-1507) as the evaluator of pcnn_nm::search: each thread
// of the 1024 holds one correspondence, and every evaluation sums the
// distances in the workgroup tree (the oracle's order)
struct Energy3dEval {
  static constexpr int kBatch = 1;
  static constexpr bool kBarrierAfterReflection = false;
  bool live;            // this thread has a correspondence
  float co[3], ce[3];   // its object coordinate and camera point
  int m;                // correspondences
  float (*wf)[1];       // LDS: the 16 wave sums
  float* Rf;            // LDS: the point's rotation matrix
  __device__ __forceinline__ double value(const double (*xs)[6], int k) {
    const double* xq = xs[k];  // written by thread 0
    if (threadIdx.x == 0) {
      double Rd[9];
      rod_v2m(xq, Rd);
      for (int i = 0; i < 9; i++) Rf[i] = (float)Rd[i];  // jp::double2float
    }
    __syncthreads();
    float leaf = 0.f;
    if (live) {
      float tr[3];
      for (int rr = 0; rr < 3; rr++) {
        const float mm = Rf[rr * 3 + 0] * co[0] + Rf[rr * 3 + 1] * co[1] + Rf[rr * 3 + 2] * co[2];
        tr[rr] = (float)((double)mm + xq[3 + rr]);
      }
      const double dx = (double)tr[0] - (double)ce[0], dy = (double)tr[1] - (double)ce[1],
                   dz = (double)tr[2] - (double)ce[2];
      leaf = 0.f + (float)sqrt(dx * dx + dy * dy + dz * dz);
    }
    const float sw = wave_fold(leaf);
    if (pcnn::lane_id() == 0) wf[threadIdx.x >> 6][0] = sw;
    __syncthreads();
    // every thread folds the 16 wave sums (the next evaluation's first
    // barrier orders these reads before wf is rewritten)
    return (double)(cross_fold<float, 1>(wf, 0) / (float)m);
  }
  __device__ __forceinline__ bool failed() const { return false; }
};

// one workgroup per object: the final filter, then refineWithOpt as the
// bounded Nelder-Mead of nelder_mead.h over Energy3dEval
__global__ void __launch_bounds__(kFinThreads) k_p3d_finish(const float* __restrict__ vm,
                                                            const float* __restrict__ ext, int C, int n_hyp,
                                                            uint64_t seed, int nm_evals, P3dWs w3,
                                                            int32_t* __restrict__ final_out,
                                                            float* __restrict__ poses_out,
                                                            float* __restrict__ energy_out) {
  constexpr int nd = 6;
  __shared__ float wf[16][1];
  __shared__ pcnn_nm::Simplex<nd> sx;
  __shared__ float Rf[9];
  __shared__ int nh_s;
  const P2dWs& ws = w3.b;
  const int oi = blockIdx.x, t = threadIdx.x, lane = pcnn::lane_id();
  if (oi >= *ws.nobj || ws.rm[oi] == 0) return;  // block-uniform
  const int obj = ws.objs[oi];
  const int h = ws.rl[oi * kMaxHypBlock];
  const int n = ws.rc[oi * kMaxHypBlock];
  if (t == 0) nh_s = 0;
  __syncthreads();
  {
    int nh = 0;
    for (int q = t; q < n_hyp; q += kFinThreads) nh += ws.hyp[(size_t)q * 16] == (double)obj;
    nh = pcnn::wave_sum(nh);
    if (lane == 0) atomicAdd(&nh_s, nh);  // integer: order-free
  }
  const double* hr = ws.hyp + (size_t)h * 16;
  Pose P;
  for (int i = 0; i < 9; i++) P.R[i] = hr[1 + i];
  for (int i = 0; i < 3; i++) P.t[i] = hr[10 + i];
  float en = 0.f;
  if (n > 10) {  // minPixels (:1939); block-uniform
    const int mp = w3.npick[h];
    const int m = mp >= kMaxInl ? kMaxInl : mp;
    Energy3dEval ev{t < m, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, m, wf, Rf};
    if (ev.live) {  // filterInliers3D again (:1942): correspondence t of this thread
      int idx = t;
      if (mp >= kMaxInl) {
        Stream rs(seed, (uint32_t)h, kTagF3D, (uint32_t)(1024 * kRounds + t));
        idx = rs.uniform(mp);
      }
      const int p = w3.pick[(size_t)h * kMaxInl + idx];
      const F3 o = mode3d(vm, ext, C, obj, p);
      const F3 e = eye_at(w3.eye, p);
      ev.co[0] = o.x; ev.co[1] = o.y; ev.co[2] = o.z;
      ev.ce[0] = e.x; ev.ce[1] = e.y; ev.ce[2] = e.z;
    }
    if (t == 0) {  // refineWithOpt (:1510-1567)
      double x0[nd];
      rod_m2v(P.R, x0);
      for (int i = 0; i < 3; i++) x0[3 + i] = P.t[i];
      const double rot = 10 * 3.1415926 / 180;  // rotRange, PI of types.h:33
      const double rng[nd] = {rot, rot, rot, 0.1, 0.1, 0.5};
      for (int i = 0; i < nd; i++) {
        sx.lb[i] = x0[i] - rng[i];
        sx.ub[i] = x0[i] + rng[i];
        sx.pts[0][i] = x0[i];
      }
    }
    pcnn_nm::search(sx, ev, nm_evals);
    if (t == 0) {
      const int bi = pcnn_nm::best(sx);
      double xb[nd];
      for (int e = 0; e < nd; e++) xb[e] = sx.pts[bi][e];
      rod_v2m(xb, P.R);
      for (int i = 0; i < 3; i++) P.t[i] = xb[3 + i];
      en = (float)sx.vals[bi];
    }
  }
  __syncthreads();
  if (t != 0) return;
  final_out[obj * 3] = h;
  final_out[obj * 3 + 1] = n;
  final_out[obj * 3 + 2] = nh_s;
  energy_out[obj] = en;
  for (int y = 0; y < 3; y++)
    for (int x = 0; x < 4; x++) poses_out[obj + C * (y * 4 + x)] = x < 3 ? (float)P.R[y * 3 + x] : (float)P.t[y];
}

// the workspace: estimatePose2D's regions, then the 3-D ones; a null base
// answers the size query (total)
P3dWs layout3(void* base, int H, int W, int C, int n_hyp, size_t& total) {
  pcnn::Carve cv(base);
  P3dWs w3;
  w3.b = carve_base(cv, H, W, C, n_hyp);
  const long HW = (long)H * W;
  w3.mwords = (int)((HW + 63) / 64);
  w3.eye = cv.take<float>((size_t)HW * 3);
  w3.valid = cv.take<uint64_t>((size_t)valid_blocks((int)HW) * 4);
  w3.imask = cv.take<uint64_t>((size_t)n_hyp * w3.mwords);
  w3.pick = cv.take<int32_t>((size_t)n_hyp * kMaxInl);
  w3.npick = cv.take<int32_t>((size_t)n_hyp);
  total = cv.off + 256;
  return w3;
}

}  // namespace

extern "C" size_t pcnn_pose3d_workspace_size(int H, int W, int C, int n_hyp) {
  if (H <= 0 || W <= 0 || C <= 0 || n_hyp <= 0) return 256;
  size_t total;
  layout3(nullptr, H, W, C, n_hyp, total);
  return total;
}

extern "C" int pcnn_pose3d(const int32_t* label, const uint16_t* depth, const float* vertmap, const float* extents,
                           int H, int W, int C, float fx, float fy, float px, float py, float depth_factor,
                           uint64_t seed, int n_hyp, int max_iter, int nm_evals, float* poses_out, float* hyps_out,
                           int32_t* hyp_px, int32_t* inl_out, int32_t* final_out, float* energy_out, float* eye_out,
                           void* workspace, size_t workspace_bytes, void* stream) {
  PCNN_REQUIRE(label && depth && vertmap && extents && poses_out && hyps_out && hyp_px && inl_out && final_out &&
               energy_out);
  // nm_evals >= 7: at least the six-dimensional search's initial simplex (NLopt's
  // maxeval counts it; a smaller budget is refused rather than overrun)
  PCNN_REQUIRE(H > 0 && W > 0 && C > 1 && C <= 64 && n_hyp > 0 && n_hyp <= kMaxHyp && max_iter > 0 && nm_evals >= 7);
  PCNN_REQUIRE((long)H * W < (1l << 28));
  size_t total;
  const P3dWs w3 = layout3(workspace, H, W, C, n_hyp, total);
  if (!workspace || workspace_bytes < total) return PCNN_ECAPACITY;
  const P2dWs& ws = w3.b;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_p3d_init, dim3(1), dim3(1024), 0, st, C, n_hyp, poses_out, energy_out, inl_out, final_out,
                     ws.rm);
  const Cam k{fx, fy, px, py};
  const int HW = H * W;
  hipLaunchKernelGGL(k_p3d_eye, dim3((HW + 255) / 256), dim3(256), 0, st, depth, H, W, fx, fy, px, py, depth_factor,
                     w3.eye);
  hipLaunchKernelGGL(k_p2d_colcount, dim3((W + 3) / 4), dim3(256), 0, st, label, H, W, C, ws.colcnt);
  hipLaunchKernelGGL(k_p2d_scan, dim3(C), dim3(1024), 0, st, ws.colcnt, W, ws.coloff, ws.count);
  hipLaunchKernelGGL(k_p2d_objs, dim3(1), dim3(64), 0, st, C, ws);
  hipLaunchKernelGGL(k_p2d_scatter, dim3((W + 3) / 4), dim3(256), 0, st, label, H, W, C, ws);
  hipLaunchKernelGGL(k_p3d_valid, dim3(valid_blocks(HW)), dim3(256), 0, st, C, w3);
  hipLaunchKernelGGL(k_p3d_subset, dim3(C, kRounds), dim3(1024), 0, st, seed, w3);
  const int T = max_iter < kAttempts ? max_iter : kAttempts;
  const AttArgs A{vertmap, extents, w3.eye, H, W, C, k, seed};
  hipLaunchKernelGGL(k_attempts<true>, dim3((n_hyp * T + 63) / 64), dim3(64), 0, st, A, n_hyp, T, ws);
  hipLaunchKernelGGL(k_pick<true>, dim3(n_hyp), dim3(64), 0, st, A, n_hyp, max_iter, T, ws, hyps_out, hyp_px);
  hipLaunchKernelGGL(k_p2d_collect, dim3(C), dim3(64), 0, st, n_hyp, ws);
  for (int r = 0; r < kRounds; r++) {
    const int gx = std::max(1, n_hyp >> r);  // survivors halve each round (one stays one)
    hipLaunchKernelGGL(k_p3d_count, dim3(gx, C, count_z(r)), dim3(256), 0, st, vertmap, extents, C, w3, r);
    hipLaunchKernelGGL(k_select_sum, dim3(C), dim3(1024), 0, st, ws, r, count_z(r), inl_out);
    hipLaunchKernelGGL(k_p3d_update, dim3(std::max(1, n_hyp >> (r + 1)), C), dim3(1024), 0, st, vertmap, extents, C,
                       seed, w3, r);
  }
  hipLaunchKernelGGL(k_p3d_finish, dim3(C), dim3(kFinThreads), 0, st, vertmap, extents, C, n_hyp, seed, nm_evals, w3, final_out,
                     poses_out, energy_out);
  if (eye_out &&
      hipMemcpyAsync(eye_out, w3.eye, (size_t)HW * 3 * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
    return PCNN_EHIP;
  PCNN_CHECK_LAUNCH();
  return PCNN_OK;
}
