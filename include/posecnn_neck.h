/*
 * posecnn_neck.h — C-ABI of the EMBEDDING NECK in libposecnn_hip.so: the two
 * fused passes around the 1x1 convs between conv4_3 / conv5_3 and the two heads
 * (csrc/neck.hip).  A companion of posecnn_hip.h (same library, same
 * conventions and error codes); pcnn_neck_abi_version() versions these entry
 * points on their own, pcnn_abi_version() does not change with them.
 *
 * Conventions (those of posecnn_hip.h)
 *  - every pointer is a DEVICE pointer unless the name ends in _host;
 *  - `stream` is a hipStream_t passed as void* (NULL = legacy default stream);
 *  - nothing allocates: temporaries live in a caller-provided `workspace` whose
 *    size the matching *_workspace_size() query returns;
 *  - nothing synchronises and nothing is read back: every op can be captured in
 *    a hipGraph, and the dropout step counter lives on the device;
 *  - return value 0 = PCNN_OK, otherwise a PCNN_E* code (never exit()).
 */
#ifndef POSECNN_NECK_H
#define POSECNN_NECK_H

#include <stddef.h>
#include <stdint.h>

#include "posecnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: pcnn_neck_fwd, pcnn_neck_bwd_workspace_size, pcnn_neck_bwd */
int pcnn_neck_abi_version(void);

/* ---------------------------------------------------------------------------
 * The layers of lib/networks/vgg16_convs.py:128-137 (score branch) and :152-161
 * (vertex branch), both branches at once.  The four 1x1 convs are two GEMMs the
 * caller runs (pcnn_gemm): with x4 (B,h,w,K) = conv4_3 and x5 (B,h/2,w/2,K) =
 * conv5_3, NHWC, M4 = B h w and M5 = M4 / 4,
 *     z4 (M4,N) = x4 W4        z5 (M5,N) = x5 W5        N = U + V,
 * columns [0, U) the score branch (score_conv4 | score_conv5, ReLU), columns
 * [U, N) the vertex branch (score_conv4_vertex | score_conv5_vertex, no ReLU).
 * Either U or V may be 0; both are multiples of 4; h and w are even.
 *
 * Forward, per output element (b, y, x, c), float32, every operation rounded
 * separately (no FMA), act = ReLU (v > 0 ? v : 0) for c < U, the identity above:
 *     t4      = act(z4 + b4)
 *     t5[tap] = act(z5[tap] + b5)
 *     up      = the stride-2 taps of the fixed bilinear 4x4 deconv
 *               (upscore_conv5): along an axis, output y taps i1 = (y + 1) div 2
 *               with weight (2 k + 1) / 4, k = (y + 1) mod 2, and i0 = i1 - 1
 *               with (3 - 2 k) / 4; a tap outside the map is absent; a 2-D
 *               weight is the product of the two (exact); the terms t5 * weight
 *               are added as ((t00 + t01) + t10) + t11 over the present taps,
 *               the first present term starting the sum: pcnn_upscore_fwd's
 *               order at stride 2;
 *     a       = t4 + up                                     (add_score)
 *     out     = (a / keep_prob) * keep                      (tf.nn.dropout);
 *               keep_prob == 1: out = a, nothing is drawn, the keep maps are
 *               not touched and may be NULL.
 *
 *  add_score (M4,U), add_score_vertex (M4,V) f32   out: two contiguous maps
 *  keep_score (M4,U), keep_vertex (M4,V) uint8     out: the keep bits, 0 / 1
 *
 * The keep bits are those pcnn_dropout_mask writes for a dense (M4,U) mask with
 * (seed, *step_dev, stream_id_score), and for a dense (M4,V) mask with
 * stream_id_vertex.  step_dev (1) int64 is read on the device (NULL: step 0),
 * so a captured graph draws fresh masks once the caller bumps the counter.
 *
 * One launch.  z4, z5, b4, b5 and the two maps 16-byte aligned, the keep maps
 * 4-byte aligned.  A map of a branch with no columns may be NULL.
 * PCNN_EINVAL: B, h or w < 1, odd h or w, U or V negative or not a multiple of
 * 4, U + V = 0, keep_prob outside (0, 1], M4 (U + V) >= 2^31, a NULL z4, z5,
 * b4 or b5, a NULL output of a branch with columns (the keep maps only with
 * keep_prob < 1), a negative stream id, a misaligned pointer.
 * ------------------------------------------------------------------------- */
int pcnn_neck_fwd(const float* z4, const float* z5, const float* b4, const float* b5, int B, int h, int w, int U,
                  int V, float keep_prob, uint64_t seed, const int64_t* step_dev, int stream_id_score,
                  int stream_id_vertex, float* add_score, float* add_score_vertex, uint8_t* keep_score,
                  uint8_t* keep_vertex, void* stream);

/* ---------------------------------------------------------------------------
 * Backward of pcnn_neck_fwd down to the GEMM outputs and the biases; the
 * caller's GEMMs finish it (d_x4 = dz4 W4^T, d_W4 = x4^T dz4, d_x5 = dz5 W5^T,
 * d_W5 = x5^T dz5).  d = d_add_score | d_add_score_vertex by column:
 *     g   = (d / keep_prob) * keep           (keep_prob == 1: g = d, keep maps unused)
 *     dz4 = z4 + b4 > 0 ? g : 0 for c < U,   g above                    (M4,N)
 *     dz5 = the transpose of the forward's taps: low-res pixel (i, j) sums
 *           weight(u) weight(v) * g over its 4x4 window, rows 2 i - 1 + u and
 *           columns 2 j - 1 + v, u, v = 0..3, weights 1/4 3/4 3/4 1/4, row
 *           major (u outer), positions outside the map skipped, each product
 *           rounded and added to a sum that starts at 0; then masked by
 *           z5 + b5 > 0 for c < U                                       (M5,N)
 *     db4 (N) = the column sums of dz4,  db5 (N) = the column sums of dz5.
 *
 * dz4 is one product chain per element.  The sums have a fixed order and use
 * no float atomics: two runs give the same bits.  Bias sums: the thread of a
 * (low-res pixel, column quad) adds the dz4 of its 2x2 full-res pixels row
 * major and its dz5; a block's threads of one column are added in pixel order,
 * the blocks' partials by a second launch in block order.
 *
 * Two launches.  workspace: pcnn_neck_bwd_workspace_size(B, h, w, U, V) bytes
 * (0 for dimensions pcnn_neck_bwd refuses), 16-byte aligned.
 * PCNN_EINVAL: as pcnn_neck_fwd for the dimensions and keep_prob; a NULL z4,
 * z5, b4, b5, dz4, dz5, db4, db5 or workspace, a NULL gradient of a branch
 * with columns (its keep map only with keep_prob < 1), a misaligned pointer.
 * PCNN_ECAPACITY: a workspace that is too small.
 * ------------------------------------------------------------------------- */
size_t pcnn_neck_bwd_workspace_size(int B, int h, int w, int U, int V);
int pcnn_neck_bwd(const float* d_add_score, const float* d_add_score_vertex, const uint8_t* keep_score,
                  const uint8_t* keep_vertex, const float* z4, const float* z5, const float* b4, const float* b5,
                  int B, int h, int w, int U, int V, float keep_prob, float* dz4, float* dz5, float* db4, float* db5,
                  void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* POSECNN_NECK_H */
