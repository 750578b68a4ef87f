// The VGG16 backbone's forward layers (include/posecnn_backbone.h): 3x3
// convolution + bias + ReLU and 2x2 max-pool, NHWC float32, TF SAME padding
// (lib/networks/vgg16_convs.py:80-97).
//
// k_conv3x3_x6 (Cin % 16 == 0) is an implicit GEMM on v_mfma_f32_32x32x16_bf16
// with the numerics of gemm_x6.hip: both operands split exactly into three bf16
// planes (x_split3), the six kept plane products accumulated smallest first in
// fp32.  M = B H W output pixels, N = Cout, K = 9 Cin with k = (dy 3 + dx) Cin
// + c, so a 16-deep K step is 16 channels of ONE tap and an output pixel's A
// fragment for it is 64 contiguous bytes of the input pixel (y+dy-1, x+dx-1).
// No im2col matrix exists anywhere:
//
//  * a workgroup (512 threads, 8 waves) owns a 16 x 16 patch of output pixels
//    of one image (256 rows of the implicit matrix) and a 64- or 128-column
//    tile; the wave grid is 8 x 1 (32 rows x 64 columns a wave) or 4 x 2
//    (64 rows x 64 columns);
//  * per 16-channel step it stages the patch's 18 x 18 halo slab ONCE, split
//    into its three planes once (not nine times): 324 LDS rows of 48 B per
//    plane (16 bf16 + 16 B of padding, the conflict-free row of gemm_x6.hip).
//    A halo pixel outside the IMAGE is loaded through an out-of-extent buffer
//    offset and is therefore zero: that is the SAME padding.  A halo pixel
//    outside the patch but inside the image is real data.  Row m + 1 of the
//    implicit matrix never enters the addressing: a fragment is found from the
//    pixel's (py + dy, px + dx) position in the slab;
//  * the nine taps then run from shifted rows of that slab (tap (dy, dx) reads
//    slab row (py + dy) 18 + px + dx); only the current tap's 16 x NT weight
//    panel streams through a double buffer, loaded a tap ahead into registers
//    and transposed / split on its way into LDS; the next step's slab is loaded
//    into registers under the nine taps and stored behind the last one;
//  * LDS: slab 3 x 324 x 48 = 46656 B, weight panels 2 x 3 x NT x 48 = 36864 B
//    (NT 128; 83520 B in all, one workgroup per CU) or 18432 B (NT 64; 65088 B,
//    two per CU);
//  * small maps: when patches x column tiles fill less than half the CUs the
//    channel steps are split over up to 16 slices, each writing raw partial sums
//    to the workspace; k_conv_reduce adds the slices in slice order (no float
//    atomics) and applies bias / ReLU.  The plan is a function of the shape
//    alone (conv_plan), so two calls give the same bits.
//
// k_conv3x3_direct (Cin == 3: conv1_1) and k_maxpool2x2 are plain float32
// kernels with the fixed orders the header states.
#include "gemm_common.h"
#include "../../include/posecnn_backbone.h"

using namespace pcnn_gk;

namespace {

constexpr int kP = 16;                        // patch edge (output pixels)
constexpr int kHalo = kP + 2;                 // slab edge
constexpr int kSlabPix = kHalo * kHalo;       // 324
constexpr int kRow = 48;                      // bytes per LDS plane row
constexpr int kSlabPlane = kSlabPix * kRow;   // 15552
constexpr int kSlab = 3 * kSlabPlane;         // 46656
constexpr int kThreads = 512;
constexpr int kSlabLoads = (kSlabPix * 4 + kThreads - 1) / kThreads;  // float4 loads per thread: 3
constexpr int kFillCUs = 256;                 // the planner's CU count (MI355X)
constexpr int kMaxSplit = 16;

template <int NT>
struct CTile {
  static constexpr int wpart = NT * kRow;      // one plane of a weight panel
  static constexpr int wstage = 3 * wpart;
  static constexpr int lds = kSlab + 2 * wstage;
  static constexpr int WN = NT / 64;           // waves along N (64 columns each)
  static constexpr int WM = 8 / WN;            // waves along M
  static constexpr int AM = 8 / WM;            // 32-row accumulator blocks per wave
};

struct ConvPlan {
  int nt;       // column tile: 64 or 128
  int ty, tx;   // patches per image
  int npatch;   // B ty tx
  int ncol;     // column tiles
  int S;        // slices of the channel steps (1: whole contraction, epilogue in the kernel)
  int cps;      // channel steps per slice (no slice is empty)
  int items;    // workgroups
};

struct ConvArgs {
  const float* x;
  const float* w;
  const float* bias;
  float* y;
  float* part;  // [S][M][Cout] when S > 1
  int B, H, W, Cin, Cout, act;
  ConvPlan pl;
};

inline ConvPlan conv_plan(int B, int H, int W, int Cin, int Cout) {
  ConvPlan p;
  p.nt = Cout <= 64 ? 64 : 128;
  p.ty = (H + kP - 1) / kP;
  p.tx = (W + kP - 1) / kP;
  p.npatch = B * p.ty * p.tx;
  p.ncol = (Cout + p.nt - 1) / p.nt;
  const int ncs = Cin / 16;
  const long tiles = (long)p.npatch * p.ncol;
  int S = 1;
  if (tiles < kFillCUs / 2) {
    S = (int)(kFillCUs / tiles);
    if (S > kMaxSplit) S = kMaxSplit;
    if (S > ncs) S = ncs;
  }
  p.cps = (ncs + S - 1) / S;
  p.S = (ncs + p.cps - 1) / p.cps;
  p.items = (int)(tiles * p.S);
  return p;
}

__device__ __forceinline__ f32x2 x_ld2(const XOp& o, unsigned voff, int soff) {
  return __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(o.rs, voff, soff, 0));
}

#define CV_FRAG(ptr) (*(const bf16x8*)(ptr))

template <int NT>
__global__ void __launch_bounds__(kThreads) k_conv3x3_x6(ConvArgs g) {
  using T = CTile<NT>;
  constexpr int AM = T::AM, WSTAGE = T::wstage, WPART = T::wpart;
  extern __shared__ __attribute__((aligned(16))) char cl[];
  char* const slab = cl;
  char* const wb = cl + kSlab;
  const ConvPlan& pl = g.pl;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / T::WN, wn = wave % T::WN;
  const int r = lane & 31, hsel = lane >> 5;
  // item -> (slice z, patch, column tile); the column tiles of a patch are
  // neighbours (they share the slab through L2), XCD-aware as the GEMMs
  int item = xcd_remap((int)blockIdx.x, pl.items);
  const int nc = item % pl.ncol;
  item /= pl.ncol;
  const int patch = item % pl.npatch, z = item / pl.npatch;
  const int b = patch / (pl.ty * pl.tx), pt = patch % (pl.ty * pl.tx);
  const int y0 = (pt / pl.tx) * kP, x0 = (pt % pl.tx) * kP, n0 = nc * NT;
  const int H = g.H, W = g.W, Cin = g.Cin, Cout = g.Cout;
  const int ncs = Cin / 16;
  const int cs_lo = z * pl.cps, cs_hi = min(ncs, cs_lo + pl.cps);
  const int nsteps = (cs_hi - cs_lo) * 9;
  if (nsteps <= 0) return;  // the plan has no empty slice

  const XOp ox = x_op(g.x, 0, (long)g.B * H * W * Cin);
  const XOp ow = x_op(g.w, 0, (long)9 * Cin * Cout);

  // slab staging: float4 idx -> slab pixel idx >> 2, channel quad idx & 3.  A
  // pixel outside the image gets the out-of-extent offset: zeros.
  unsigned s_voff[kSlabLoads];
  int s_lds[kSlabLoads];
#pragma unroll
  for (int q = 0; q < kSlabLoads; q++) {
    const int idx = tid + kThreads * q;
    const int p = idx >> 2, cq = idx & 3;
    const int yy = y0 - 1 + p / kHalo, xx = x0 - 1 + p % kHalo;
    const bool in_slab = idx < kSlabPix * 4;
    const bool ok = in_slab && yy >= 0 && yy < H && xx >= 0 && xx < W;
    s_voff[q] = ok ? (unsigned)(((b * H + yy) * W + xx) * Cin + 4 * cq) * 4u : kXOob;
    s_lds[q] = in_slab ? p * kRow + 8 * cq : -1;
  }
  // weight staging: k pair tid & 7, column pair tid >> 3 of the panel
  const int kp = tid & 7, nh = tid >> 3;
  const bool w_act = nh < NT / 2;
  const unsigned w_voff = (w_act && n0 + 2 * nh < Cout) ? (unsigned)((2 * kp) * Cout + n0 + 2 * nh) * 4u : kXOob;
  const int w_lds = (2 * nh) * kRow + 4 * kp;

  xf4 sv[kSlabLoads];
  f32x2 wv[2];
  auto ld_slab = [&](int cs) {
#pragma unroll
    for (int q = 0; q < kSlabLoads; q++) sv[q] = x_ld4(ox, s_voff[q], cs * 64);
  };
  auto st_slab = [&]() {
#pragma unroll
    for (int q = 0; q < kSlabLoads; q++) {
      if (s_lds[q] >= 0) {
        unsigned h0, m0, l0, h1, m1, l1;
        x_split3(sv[q][0], sv[q][1], h0, m0, l0);
        x_split3(sv[q][2], sv[q][3], h1, m1, l1);
        *(uint2*)(slab + s_lds[q]) = make_uint2(h0, h1);
        *(uint2*)(slab + kSlabPlane + s_lds[q]) = make_uint2(m0, m1);
        *(uint2*)(slab + 2 * kSlabPlane + s_lds[q]) = make_uint2(l0, l1);
      }
    }
  };
  auto ld_w = [&](int cs, int tap) {
    const int soff = ((tap * Cin + cs * 16) * Cout) * 4;
    wv[0] = x_ld2(ow, w_voff, soff);
    wv[1] = x_ld2(ow, w_voff + (unsigned)Cout * 4u, soff);
  };
  auto st_w = [&](char* buf) {
    if (w_act) {
#pragma unroll
      for (int e = 0; e < 2; e++) {
        unsigned h, m, l;
        x_split3(wv[0][e], wv[1][e], h, m, l);
        const int o = w_lds + e * kRow;
        *(unsigned*)(buf + o) = h;
        *(unsigned*)(buf + WPART + o) = m;
        *(unsigned*)(buf + 2 * WPART + o) = l;
      }
    }
  };

  // fragment offsets: lane -> patch pixel row r of block i, k 8 hsel .. +7
  int a_off[AM], b_off[2];
  bool live_i[AM], live_j[2];
#pragma unroll
  for (int i = 0; i < AM; i++) {
    const int p0 = wm * (32 * AM) + i * 32;
    const int p = p0 + r;
    a_off[i] = ((p >> 4) * kHalo + (p & 15)) * kRow + 16 * hsel;
    live_i[i] = y0 + (p0 >> 4) < H;  // the block's first pixel row is in the image
  }
#pragma unroll
  for (int j = 0; j < 2; j++) {
    b_off[j] = (wn * 64 + j * 32 + r) * kRow + 16 * hsel;
    live_j[j] = n0 + wn * 64 + j * 32 < Cout;
  }

  f32x16 acc[AM][2];
#pragma unroll
  for (int i = 0; i < AM; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) acc[i][j] = (f32x16){};

  ld_slab(cs_lo);
  ld_w(cs_lo, 0);
  st_slab();
  st_w(wb);
  __syncthreads();
  int cs = cs_lo, tap = 0;
  for (int s = 0; s < nsteps; s++) {
    const bool more = s + 1 < nsteps;
    int ntap = tap + 1, ncs_ = cs;
    if (ntap == 9) {
      ntap = 0;
      ncs_++;
    }
    if (more) ld_w(ncs_, ntap);
    if (tap == 0 && cs + 1 < cs_hi) ld_slab(cs + 1);
    const char* cur = wb + (s & 1) * WSTAGE;
    const int toff = ((tap / 3) * kHalo + tap % 3) * kRow;
    bf16x8 bh[2], bm[2], bl[2];
#pragma unroll
    for (int j = 0; j < 2; j++) {
      bh[j] = CV_FRAG(cur + b_off[j]);
      bm[j] = CV_FRAG(cur + WPART + b_off[j]);
      bl[j] = CV_FRAG(cur + 2 * WPART + b_off[j]);
    }
#pragma unroll
    for (int i = 0; i < AM; i++) {
      if (!live_i[i]) continue;
      const bf16x8 ah = CV_FRAG(slab + a_off[i] + toff);
      const bf16x8 am = CV_FRAG(slab + kSlabPlane + a_off[i] + toff);
      const bf16x8 al = CV_FRAG(slab + 2 * kSlabPlane + a_off[i] + toff);
#pragma unroll
      for (int j = 0; j < 2; j++) {
        if (!live_j[j]) continue;
        // smallest first, as k_gemm_x6
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh[j], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl[j], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm[j], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh[j], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm[j], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh[j], acc[i][j], 0, 0, 0);
      }
    }
    // the other weight buffer was last read in step s - 1, behind a barrier
    if (more) st_w(wb + ((s + 1) & 1) * WSTAGE);
    __syncthreads();
    if (tap == 8 && more) {  // every wave is done with this step's slab
      st_slab();
      __syncthreads();
    }
    tap = ntap;
    cs = ncs_;
  }

  // epilogue: value q of block (i, j) is patch pixel wm 32 AM + 32 i + 4 hsel +
  // (q & 3) + 8 (q >> 2), column n0 + wn 64 + 32 j + r
  const long M = (long)g.B * H * W;
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const int n = n0 + wn * 64 + j * 32 + r;
    const bool nok = n < Cout;
    const float bv = (pl.S == 1 && g.bias && nok) ? g.bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < AM; i++)
#pragma unroll
      for (int q = 0; q < 16; q++) {
        const int p = wm * (32 * AM) + i * 32 + 4 * hsel + (q & 3) + 8 * (q >> 2);
        const int yy = y0 + (p >> 4), xx = x0 + (p & 15);
        if (nok && yy < H && xx < W) {
          const long m = ((long)b * H + yy) * W + xx;
          float v = acc[i][j][q];
          if (pl.S == 1) {
            v = v + bv;
            if (g.act == 1) v = v > 0.f ? v : 0.f;
            g.y[m * Cout + n] = v;
          } else {
            g.part[((long)z * M + m) * Cout + n] = v;
          }
        }
      }
  }
}

// y = act(sum of the S slices in slice order + bias): one float4 per thread
__global__ void __launch_bounds__(256) k_conv_reduce(const float* __restrict__ part, const float* __restrict__ bias,
                                                     long MN4, int Cout, int S, int act, float* __restrict__ y) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= MN4) return;
  f32x4 s = *(const f32x4*)(part + 4 * i);
  for (int z = 1; z < S; z++) s = s + *(const f32x4*)(part + 4 * ((long)z * MN4 + i));
  if (bias) s = s + *(const f32x4*)(bias + (4 * i) % Cout);
  if (act == 1) {
#pragma unroll
    for (int e = 0; e < 4; e++) s[e] = s[e] > 0.f ? s[e] : 0.f;
  }
  *(f32x4*)(y + 4 * i) = s;
}

// conv1_1: Cin == 3, K = 27.  One thread per (pixel, 4 output channels); the
// order of the header: dy, dx, c nested, product and sum rounded separately
// (fp contract off), taps outside the image skipped, then bias, then ReLU.
__global__ void __launch_bounds__(256) k_conv3x3_direct(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ bias, int B, int H, int W, int Cout,
                                                        int act, float* __restrict__ y) {
  const int nq = Cout >> 2;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * H * W * nq) return;
  const int n = (int)(i % nq) * 4;
  const long m = i / nq;
  const int xx = (int)(m % W), yy = (int)((m / W) % H);
  const long b = m / ((long)W * H);
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  for (int dy = 0; dy < 3; dy++) {
    const int sy = yy + dy - 1;
    if (sy < 0 || sy >= H) continue;
    for (int dx = 0; dx < 3; dx++) {
      const int sx = xx + dx - 1;
      if (sx < 0 || sx >= W) continue;
      const float* px = x + ((b * H + sy) * W + sx) * 3;
      const float* pw = w + (size_t)((dy * 3 + dx) * 3) * Cout + n;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const float xv = px[c];
        const f32x4 wv = *(const f32x4*)(pw + (size_t)c * Cout);
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const float t = xv * wv[e];
          s[e] = s[e] + t;
        }
      }
    }
  }
  if (bias) s = s + *(const f32x4*)(bias + n);
  if (act == 1) {
#pragma unroll
    for (int e = 0; e < 4; e++) s[e] = s[e] > 0.f ? s[e] : 0.f;
  }
  *(f32x4*)(y + m * Cout + n) = s;
}

// 2x2 max-pool, stride 2, SAME: window rows 2 oy, 2 oy + 1 and columns 2 ox,
// 2 ox + 1, the ones inside the map; m = the top-left value, then v > m ? v : m
// over (0,1), (1,0), (1,1).  One float4 of channels per thread.
__global__ void __launch_bounds__(256) k_maxpool2x2(const float* __restrict__ x, int B, int H, int W, int C, int OH,
                                                    int OW, float* __restrict__ y) {
  const int cq = C >> 2;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * OH * OW * cq) return;
  const int c = (int)(i % cq) * 4;
  const long o = i / cq;
  const int ox = (int)(o % OW), oy = (int)((o / OW) % OH);
  const long b = o / ((long)OW * OH);
  const float* p = x + ((b * H + 2 * oy) * W + 2 * ox) * C + c;
  f32x4 m = *(const f32x4*)p;
  const bool right = 2 * ox + 1 < W, down = 2 * oy + 1 < H;
  auto take = [&](const float* q) {
    const f32x4 v = *(const f32x4*)q;
#pragma unroll
    for (int e = 0; e < 4; e++) m[e] = v[e] > m[e] ? v[e] : m[e];
  };
  if (right) take(p + C);
  if (down) take(p + (size_t)W * C);
  if (right && down) take(p + (size_t)W * C + C);
  *(f32x4*)(y + o * C + c) = m;
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

constexpr long kMaxBytes = 1l << 31;

inline bool conv_dims_ok(int B, int H, int W, int Cin, int Cout, int precision) {
  if (precision != 2) return false;
  if (B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1) return false;
  if (Cin != 3 && (Cin & 15)) return false;
  if (Cout & 3) return false;
  const long px = (long)B * H;  // < 2^62
  if (px >= kMaxBytes || px * W >= kMaxBytes) return false;
  if (px * W * Cin * 4 >= kMaxBytes || px * W * Cout * 4 >= kMaxBytes) return false;
  if (9l * Cin * Cout * 4 >= kMaxBytes) return false;
  return true;
}

template <int NT>
void launch_conv(const ConvArgs& g, hipStream_t st) {
  allow_dynamic_lds<&k_conv3x3_x6<NT>>(CTile<NT>::lds);
  if (g.pl.S == 1) pcnn::launch_last(&k_conv3x3_x6<NT>, dim3(g.pl.items), dim3(kThreads), CTile<NT>::lds, st, g);
  else hipLaunchKernelGGL(k_conv3x3_x6<NT>, dim3(g.pl.items), dim3(kThreads), CTile<NT>::lds, st, g);
}

}  // namespace

// 1: pcnn_conv3x3_workspace_size, pcnn_conv3x3_fwd, pcnn_maxpool2x2_fwd
extern "C" int pcnn_backbone_abi_version(void) { return 1; }

extern "C" size_t pcnn_conv3x3_workspace_size(int B, int H, int W, int Cin, int Cout, int precision) {
  if (!conv_dims_ok(B, H, W, Cin, Cout, precision) || Cin == 3) return 0;
  const ConvPlan pl = conv_plan(B, H, W, Cin, Cout);
  if (pl.S == 1) return 0;
  return pcnn::align_up((size_t)pl.S * B * H * W * Cout * sizeof(float), 256);
}

extern "C" int pcnn_conv3x3_fwd(const float* x, const float* weights, const float* bias, int B, int H, int W, int Cin,
                                int Cout, int act, int precision, float* y, void* workspace, size_t workspace_bytes,
                                void* stream) {
  PCNN_REQUIRE(conv_dims_ok(B, H, W, Cin, Cout, precision));
  PCNN_REQUIRE(act == 0 || act == 1);
  PCNN_REQUIRE(x && weights && y && (const float*)y != x);
  PCNN_REQUIRE(aligned(x, 16) && aligned(weights, 16) && aligned(y, 16) && aligned(bias, 16));
  hipStream_t st = (hipStream_t)stream;
  if (Cin == 3) {
    const long quads = (long)B * H * W * (Cout / 4);
    pcnn::launch_last(k_conv3x3_direct, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, st, x, weights, bias, B,
                      H, W, Cout, act, y);
    PCNN_CHECK_LAUNCH();
    return PCNN_OK;
  }
  const size_t need = pcnn_conv3x3_workspace_size(B, H, W, Cin, Cout, precision);
  if (workspace_bytes < need) return PCNN_ECAPACITY;
  PCNN_REQUIRE(need == 0 || (workspace && aligned(workspace, 16)));
  ConvArgs g;
  g.x = x; g.w = weights; g.bias = bias; g.y = y; g.part = (float*)workspace;
  g.B = B; g.H = H; g.W = W; g.Cin = Cin; g.Cout = Cout; g.act = act;
  g.pl = conv_plan(B, H, W, Cin, Cout);
  if (g.pl.nt == 64) launch_conv<64>(g, st);
  else launch_conv<128>(g, st);
  PCNN_CHECK_LAUNCH();
  if (g.pl.S > 1) {
    const long MN4 = (long)B * H * W * Cout / 4;
    pcnn::launch_last(k_conv_reduce, dim3((unsigned)((MN4 + 255) / 256)), dim3(256), 0, st, (const float*)g.part, bias,
                      MN4, Cout, g.pl.S, act, y);
    PCNN_CHECK_LAUNCH();
  }
  return PCNN_OK;
}

extern "C" int pcnn_maxpool2x2_fwd(const float* x, int B, int H, int W, int C, float* y, void* stream) {
  PCNN_REQUIRE(B >= 1 && H >= 1 && W >= 1 && C >= 1 && (C & 3) == 0);
  const long px = (long)B * H;
  PCNN_REQUIRE(px < kMaxBytes && px * W < kMaxBytes && px * W * C * 4 < kMaxBytes);
  PCNN_REQUIRE(x && y && (const float*)y != x && aligned(x, 16) && aligned(y, 16));
  const int OH = (H + 1) / 2, OW = (W + 1) / 2;
  const long quads = (long)B * OH * OW * (C / 4);
  pcnn::launch_last(k_maxpool2x2, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, B, H, W,
                    C, OH, OW, y);
  PCNN_CHECK_LAUNCH();
  return PCNN_OK;
}
