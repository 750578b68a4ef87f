// Shape -> kernel form of the RoI-pool backward (roi_pooling.hip,
// roi_pool_bwd): the generic per-pixel kernel or the entry-list kernel
// k_roi_bwd_ent at one of its two tile shapes.  Plain C++ with no HIP call, so
// the library answers it on a host without a GPU (pcnn_roi_pool_bwd_form).
// Buffer alignment is not part of the plan: roi_pool_bwd checks it at the call.
#pragma once

namespace pcnn_roi {

// 2x4 tiles give fewer workgroups than this -> 1x4 tiles (roi_pool_bwd)
#ifndef PCNN_RBW_NARROW
#define PCNN_RBW_NARROW 8192
#endif
// tile height of the wide form
#ifndef PCNN_RBW_TH
#define PCNN_RBW_TH 2
#endif
static_assert(PCNN_RBW_TH == 1 || PCNN_RBW_TH == 2, "the entry-list forms are 1x4 and 2x4");

constexpr int kBWaves = 1;  // one wave per workgroup: a tile's channel chunks land on different CUs
constexpr int kBChunk = 128 * kBWaves;  // channels per workgroup
constexpr int kBTileW = 4;              // tile width of both entry-list forms
constexpr int kBGroup = 16;             // RoIs expanded per list round
constexpr int kBBins = 49;              // most bins of one RoI a list round has room for (7 x 7)
constexpr int kBCap = kBGroup * kBBins;  // entries of the LDS list

enum BwdForm { kBwdRejected = -1, kBwdGeneric = 0, kBwdEnt1x4 = 1, kBwdEnt2x4 = 2 };

struct BwdPlan {
  int form;  // BwdForm
  int tbh;   // tile height of the entry-list forms (0: generic)
};

// H * W * C < limit (limit <= 2^31), without leaving long
inline bool map_below(int H, int W, int C, long limit) {
  return (long)H * W < limit && (long)H * W * C < limit;
}

// Tile height the shape would run at: 2x4 pixels, or 1x4 when 2x4 tiles would
// leave the chip short of workgroups (conv5_3 at 30x40: 4800 -> 9600
// workgroups, measured 64 -> 50 us; conv4_3 at 60x80 keeps 2x4: 77 vs 88 us
// for 1x4)
inline int bwd_tile_h(int B, int H, int W, int C) {
  const long nchunk = ((long)C + kBChunk - 1) / kBChunk;
  const long wg24 = (long)B * (((long)H + 1) / 2) * (((long)W + 3) / 4) * nchunk;
  return wg24 < PCNN_RBW_NARROW ? 1 : PCNN_RBW_TH;
}

// The entry-list kernel takes NHWC, all channels, two channels per lane; its
// row / column acceptance masks hold pooled_h * tile_h and pooled_w * 4 bits
// in 32, and a list round expands kBGroup RoIs of up to pooled_h * pooled_w
// entries each into the kBCap-entry list (a RoI one pixel wide puts that pixel
// into every bin, so the bound is reached); the element offsets it forms fit
// 32 bits.  Everything else runs the generic kernel, except the pixel-index
// argmax (px), which only the entry-list kernel reads: rejected.
inline BwdPlan bwd_plan(int B, int H, int W, int C, int layout, int pool_channel, int pooled_h, int pooled_w,
                        int R_cap, int px) {
  BwdPlan p = {kBwdRejected, 0};
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || pooled_h <= 0 || pooled_w <= 0 || R_cap < 0 ||
      (layout != 0 && layout != 1) || !map_below(H, W, C, 1l << 31))
    return p;
  const int tbh = bwd_tile_h(B, H, W, C);
  const long bins = (long)pooled_h * pooled_w;
  const bool ent = layout == 0 && !pool_channel && C % 2 == 0 && (long)pooled_h * tbh <= 32 &&
                   (long)pooled_w * kBTileW <= 32 && kBGroup * bins <= kBCap && map_below(H, W, C, 1l << 30) &&
                   R_cap <= ((1l << 29) - 1) / (bins * C);  // R_cap * bins * C < 2^29
  if (px && !(ent && (long)H * W < 0xFFFF)) return p;
  p.form = !ent ? kBwdGeneric : tbh == 1 ? kBwdEnt1x4 : kBwdEnt2x4;
  p.tbh = ent ? tbh : 0;
  return p;
}

}  // namespace pcnn_roi
