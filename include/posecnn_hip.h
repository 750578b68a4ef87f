/*
 * posecnn_hip.h — C-ABI of libposecnn_hip.so, the MI355X (gfx950) replacement
 * for the native launchers behind PoseCNN's custom ops.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless the name ends in _host;
 *  - `stream` is a hipStream_t passed as void* (NULL = legacy default stream);
 *  - nothing allocates: temporaries live in a caller-provided `workspace` whose
 *    size the matching *_workspace_size() query returns;
 *  - nothing synchronises: variable-length results (RoI rows) are written into
 *    capacity-sized buffers with a device-side row count, so a whole
 *    vote -> RoI pool -> FC -> loss step can be captured in a hipGraph;
 *  - return value 0 = PCNN_OK, otherwise a PCNN_E* code (never exit()).
 *
 * Reference seam replaced (mrlooi/PoseCNN): the TF OpKernel::Compute methods
 * call C++ launchers with raw device pointers + an Eigen::GpuDevice stream.
 */
#ifndef POSECNN_HIP_H
#define POSECNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCNN_OK 0
#define PCNN_EINVAL 1    /* bad shape / argument (reference: OP_REQUIRES InvalidArgument) */
#define PCNN_EHIP 2      /* HIP launch error (reference: fprintf + exit(-1)) */
#define PCNN_ECAPACITY 3 /* workspace or output capacity too small */

#define PCNN_MAX_ROI 128 /* hough_voting_gpu_op.cu.cc:14 */

int pcnn_abi_version(void);
const char* pcnn_strerror(int code);

/* Completion event of the next op called on this thread (a created
 * hipEvent_t): the op's last kernel records it through the kernel's own
 * completion signal (hipExtLaunchKernel's stop event), so another stream can
 * be forked off at that point without an event-record marker on the op's
 * stream. Implemented by the fused ADD loss + head backward, the FC GEMMs
 * (precision 2) and the RoI-pool backward; after any other op the event stays
 * pending: pcnn_completion_event_pending() reports it (1) and clears it.
 * (No reference counterpart: a host-side scheduling hook of the pose step.) */
int pcnn_set_completion_event(void* event);
int pcnn_completion_event_pending(void);

/* ---------------------------------------------------------------------------
 * Hough voting (Houghvotinggpu).
 * Replaces HoughVotingLaucher (lib/hough_voting_gpu_layer/hough_voting_gpu_op.cu.cc:615-799)
 * called per image from HoughvotinggpuOp<GPU>::Compute (hough_voting_gpu_op.cc:321-429).
 *  label  (B,H,W) int32          vertex (B,H,W,3C) f32      extents (C,3) f32
 *  meta   (B,num_meta) f32       gt (num_gt,13) f32 [b,cls,0,0,0,0,qw,qx,qy,qz,tx,ty,tz]
 *  outputs, capacity `cap` rows (reference MAX_ROI*9 = 1152):
 *    top_box (cap,7) [b,cls,x1,y1,x2,y2,score]  top_pose (cap,7) [qw,qx,qy,qz,tx,ty,tz]
 *    top_target/top_weight (cap,4C)              top_domain (cap) int32
 *    num_rois (2) int32: [0] = rows emitted, [1] = max(rows, 1) (the op's
 *    output row count; row 0 is the all-zero dummy when rows == 0,
 *    hough_voting_gpu_op.cc:382-383)
 *  batch_base   added to the batch column (image-sharded runs, global image index)
 *  global_batch index_size = PCNN_MAX_ROI / global_batch (cu.cc:734)
 *  inlier_thr = 0.9, label_thr = 500 in the reference (hough_voting_gpu_op.cc:356-357)
 *  vote_thr <= 0: single instance per class (argmax); > 0: Hough-space NMS.
 *  debug_counts (optional, may be NULL): (B, C-1, H, W) int32 vote counts per
 *    present-class slot (slot order = ascending class id), the reference hough_space.
 * ------------------------------------------------------------------------- */
size_t pcnn_hough_voting_workspace_size(int B, int H, int W, int C, int skip_pixels, float vote_thr);

int pcnn_hough_voting(const int32_t* label, const float* vertex, const float* extents, const float* meta,
                      int num_meta, const float* gt, int num_gt, int B, int H, int W, int C, int batch_base,
                      int global_batch, int is_train, float inlier_thr, int label_thr, float vote_thr,
                      float per_thr, int skip_pixels, float* top_box, float* top_pose, float* top_target,
                      float* top_weight, int32_t* top_domain, int32_t* num_rois, int cap, int32_t* debug_counts,
                      void* workspace, size_t workspace_bytes, void* stream);

/* pcnn_hough_voting with the label producer fused in:
 * instead of label_2d the op takes prob_normalized (B,H,W,C) fp32 — the
 * softmax whose argmax is label_2d (argmax_2d, lib/networks/network.py:433-434;
 * graph vgg16_convs.py:144-146 -> :167-170) — labels every pixel inside the
 * compaction pass (first maximum; a NaN wins at its first occurrence, as
 * numpy / tf.argmax) and writes label_out (B,H,W) int32 as a by-product.
 * Outputs are those of pcnn_hough_voting on label_out; same workspace size. */
int pcnn_hough_voting_prob(const float* prob, int32_t* label_out, const float* vertex, const float* extents,
                           const float* meta, int num_meta, const float* gt, int num_gt, int B, int H, int W, int C,
                           int batch_base, int global_batch, int is_train, float inlier_thr, int label_thr,
                           float vote_thr, float per_thr, int skip_pixels, float* top_box, float* top_pose,
                           float* top_target, float* top_weight, int32_t* top_domain, int32_t* num_rois, int cap,
                           int32_t* debug_counts, void* workspace, size_t workspace_bytes, void* stream);

/* pcnn_hough_voting on a class-compact vertex map:
 * vertex3 (B,H,W,3) holds, per pixel, the 3 vertex channels of that pixel's
 * own label class (pcnn_vertex_pred_compact) instead of all 3C. Voters read
 * only their own class's channels (cu.cc:276-280), so the outputs equal
 * pcnn_hough_voting on any full map with those channels. C = num classes. */
int pcnn_hough_voting_compact(const int32_t* label, const float* vertex3, const float* extents, const float* meta,
                              int num_meta, const float* gt, int num_gt, int B, int H, int W, int C, int batch_base,
                              int global_batch, int is_train, float inlier_thr, int label_thr, float vote_thr,
                              float per_thr, int skip_pixels, float* top_box, float* top_pose, float* top_target,
                              float* top_weight, int32_t* top_domain, int32_t* num_rois, int cap,
                              int32_t* debug_counts, void* workspace, size_t workspace_bytes, void* stream);

/* HoughvotinggpuGrad (hough_voting_gpu_op.cc:440-484; set_gradients cu.cc:608-612):
 * zero gradients for label (B,H,W) and vertex (B,H,W,3C). Either may be NULL. */
int pcnn_hough_voting_grad(float* grad_label, float* grad_vertex, int B, int H, int W, int C, void* stream);

/* Diagnostic counters of the last pcnn_hough_voting call on `workspace`:
 * copies [0] = count mismatches between the interval vote and the exact
 * per-voter re-check at emitted maxima (must be 0), [1] = NMS candidate
 * overflows, [2] = RoI rows past the output capacity, [3] = maxima whose
 * distance sum took the one-lane serial chain (hough_peak.hip: the in-order
 * fp32 sum is rebuilt in parallel and verified; the serial chain is the
 * fallback when a verification fails; same bits either way).  Synchronous
 * (reads device memory).  The environment variable PCNN_HOUGH_SUM=serial
 * forces the serial chain for every maximum (A/B and test knob). */
int pcnn_hough_voting_diag(const void* workspace, int B, int H, int W, int C, int skip_pixels, float vote_thr,
                           int32_t* diag_host4, void* stream);

/* ---------------------------------------------------------------------------
 * RoI max pooling (RoiPool / RoiPoolGrad).
 * Replaces ROIPoolForwardLaucher / ROIPoolBackwardLaucher
 * (lib/roi_pooling_layer/roi_pooling_op_gpu.cu.cc:103-131, :232-254;
 *  called from roi_pooling_op.cc:250-254, :358-361).
 *  layout 0 = NHWC data (B,H,W,C), output (R,PH,PW,Cout)  [TF op]
 *  layout 1 = NCHW data (B,C,H,W), output (R,Cout,PH,PW)  [my_tools _RoIPooling]
 *  rois (R_cap, roi_stride) rows [b, cls, x1, y1, x2, y2, ...] (roi_stride >= 6), or
 *       with roi_stride == 5 rows [b, x1, y1, x2, y2] (pth API, class column absent)
 *  batch_base: subtracted from the rows' batch column to index `data` (an
 *       image-sharded rank holds images [batch_base, batch_base + B) of the
 *       global batch and the Hough rows carry the global index; 0 otherwise)
 *  num_rois_dev: optional device int; when non-NULL the row count is
 *       min(*num_rois_dev, R_cap) (rows beyond are not touched)
 *  argmax: flat index within the image, (h*W + w)*C + c (NHWC) or (c*H + h)*W + w (NCHW)
 * ------------------------------------------------------------------------- */
int pcnn_roi_pool_fwd(const float* data, int B, int H, int W, int C, int layout, const float* rois, int R_cap,
                      int roi_stride, int batch_base, const int32_t* num_rois_dev, float spatial_scale, int pooled_h, int pooled_w,
                      int pool_channel, float* top, int32_t* argmax, void* stream);

/* As pcnn_roi_pool_fwd but top += pooled (argmax is written as usual): the
 * second pool of vgg16_convs.py:178-184 produces pool5 + pool4 in place, so
 * the fc6 contraction reads one operand.  Same sum as tf.add(pool5, pool4). */
int pcnn_roi_pool_fwd_accumulate(const float* data, int B, int H, int W, int C, int layout, const float* rois,
                                 int R_cap, int roi_stride, int batch_base, const int32_t* num_rois_dev,
                                 float spatial_scale, int pooled_h, int pooled_w, int pool_channel, float* top,
                                 int32_t* argmax, void* stream);

/* Both pose-head RoI pools in one pass (vgg16_convs.py:177-184): pool5 on
 * data_a (e.g. conv5_3 at 1/16) and pool4 on data_b (conv4_3 at 1/8), NHWC,
 * all channels, C % 4 == 0, 16-B aligned. Writes top_sum = pool_a + pool_b
 * (one fp32 add per element, as pcnn_roi_pool_fwd then _accumulate) and both
 * argmax tensors (R_cap, pooled_h, pooled_w, C). */
int pcnn_roi_pool_fwd_pair(const float* data_a, int Ha, int Wa, float scale_a, const float* data_b, int Hb, int Wb,
                           float scale_b, int B, int C, const float* rois, int R_cap, int roi_stride,
                           int batch_base, const int32_t* num_rois_dev, int pooled_h, int pooled_w, float* top_sum,
                           int32_t* argmax_a, int32_t* argmax_b, void* stream);

/* pcnn_roi_pool_fwd_pair with the compact argmax of the fused pose step: per
 * output element the uint16 pixel index h*W + w of the max within its image
 * (the channel is the element's own; 0xFFFF = empty bin, so H*W < 0xFFFF for
 * both maps), i.e. the reference's flat index argmax = pixel*C + c
 * (roi_pooling_op_gpu.cu.cc:87-97) in half the bytes. argmax 8-B aligned.
 * Consumed by pcnn_roi_pool_bwd_px. */
int pcnn_roi_pool_fwd_pair_px(const float* data_a, int Ha, int Wa, float scale_a, const float* data_b, int Hb,
                              int Wb, float scale_b, int B, int C, const float* rois, int R_cap, int roi_stride,
                              int batch_base, const int32_t* num_rois_dev, int pooled_h, int pooled_w,
                              float* top_sum, uint16_t* argmax_a, uint16_t* argmax_b, void* stream);

size_t pcnn_roi_pool_bwd_workspace_size(int B, int R_cap);

/* Which kernel pcnn_roi_pool_bwd (px 0) / pcnn_roi_pool_bwd_px (px 1) runs for
 * a shape, given 8-B aligned buffers (misaligned ones take the generic kernel):
 * 0 = generic per-pixel kernel, 1 = entry-list kernel on 1x4-pixel tiles,
 * 2 = entry-list kernel on 2x4-pixel tiles, negative = the call is rejected
 * (invalid arguments, or a pixel-index argmax on a shape the entry-list kernel
 * does not take).  The entry list has room for 49 bins per RoI: NHWC,
 * all-channel, even-C shapes with pooled_h * pooled_w <= 49 run it, larger
 * pooled sizes the generic kernel.  Answers on a host without a GPU. */
int pcnn_roi_pool_bwd_form(int B, int H, int W, int C, int layout, int pool_channel, int pooled_h, int pooled_w,
                           int R_cap, int px);

int pcnn_roi_pool_bwd(const float* top_diff, const int32_t* argmax, int B, int H, int W, int C, int layout,
                      const float* rois, int R_cap, int roi_stride, int batch_base, const int32_t* num_rois_dev,
                      float spatial_scale, int pooled_h, int pooled_w, int pool_channel, float* bottom_diff,
                      void* workspace, size_t workspace_bytes, void* stream);

/* pcnn_roi_pool_bwd on the pixel-index argmax of pcnn_roi_pool_fwd_pair_px:
 * NHWC, all channels (pool_channel 0), C even, H*W < 0xFFFF; the same
 * entry-list gather and (RoI, ph, pw) summation order, so bit-equal to
 * pcnn_roi_pool_bwd on the flat argmax. */
int pcnn_roi_pool_bwd_px(const float* top_diff, const uint16_t* argmax_px, int B, int H, int W, int C,
                         const float* rois, int R_cap, int roi_stride, int batch_base, const int32_t* num_rois_dev,
                         float spatial_scale, int pooled_h, int pooled_w, float* bottom_diff, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * ADD / ADD-S pose loss (Averagedistance / AveragedistanceGrad).
 * Replaces AveragedistanceForwardLaucher / AveragedistanceBackwardLaucher
 * (lib/average_distance_loss/average_distance_loss_op_gpu.cu.cc:256-343, :357-377;
 *  called from average_distance_loss_op.cc:228-231, :362-363).
 *  pred/target/weight (R_cap, 4C), points (C,P,3), symmetry (C)
 *  loss (1) f32, bottom_diff (R_cap, 4C); rows counted from num_rois_dev when non-NULL.
 *  loss_norm_rows: when > 0, the normaliser R of (d - m)/(2 R P) and of the
 *       gradient (an image-sharded run passes the global row count so that the
 *       per-rank losses sum to the single-device loss); <= 0 uses the local R.
 *  Symmetric classes (ADD-S): each (row, 256-point chunk) item finds its
 *       nearest GT-rotated points with a bf16 MFMA filter and an exact fp32
 *       re-check of the few candidates inside a proved window (the same picks
 *       and the same bits as the exact scan).  An item with a
 *       non-finite point, with every point zero or with a squared norm outside
 *       [2^-40, 2^40] takes the exact scan, and so does every item when P >
 *       2816 or the device's LDS cannot hold both candidate images.  The
 *       environment variable PCNN_ADD_SEARCH=scan, read at each launch, forces
 *       the exact scan everywhere (a test / A-B knob).
 *  Workspace: pcnn_add_loss_workspace_size grew by one 256-byte slot for three
 *       int32 search counters at byte offset pcnn_add_loss_stats_offset: the
 *       symmetric items searched by the filter, those searched by the scan,
 *       and the filter items' passing (query, block of 32 candidates, half)
 *       triples (16 exact evaluations each; the int32 sum holds for
 *       R_cap x chunks up to 47 000 in the worst case).  The row classification
 *       (pcnn_add_loss_fwd, pcnn_add_loss_prep) zeroes them; the per-point sums add.
 * ------------------------------------------------------------------------- */
size_t pcnn_add_loss_workspace_size(int R_cap, int C, int P);
size_t pcnn_add_loss_stats_offset(int R_cap, int C, int P);

int pcnn_add_loss_fwd(const float* pred, const float* target, const float* weight, const float* points,
                      const float* symmetry, int R_cap, const int32_t* num_rois_dev, int C, int P, float margin,
                      int loss_norm_rows, const int32_t* loss_norm_rows_dev, float* loss, float* bottom_diff,
                      void* workspace, size_t workspace_bytes, void* stream);

/* pcnn_add_loss_fwd split in two: pcnn_add_loss_prep classifies the rows
 * (first class with weight > 0, cu.cc:47-52; the symmetric-row list) from the
 * weights alone, so a caller may run it as soon as the Hough targets exist, on
 * another stream; pcnn_add_loss_fwd_prepared is then pcnn_add_loss_fwd without
 * that step, on the same workspace, weights and row count (ordered after the
 * prep by the caller). */
int pcnn_add_loss_prep(const float* weight, const float* symmetry, int R_cap, const int32_t* num_rois_dev, int C,
                       int P, void* workspace, size_t workspace_bytes, void* stream);
int pcnn_add_loss_fwd_prepared(const float* pred, const float* target, const float* weight, const float* points,
                               const float* symmetry, int R_cap, const int32_t* num_rois_dev, int C, int P,
                               float margin, int loss_norm_rows, const int32_t* loss_norm_rows_dev, float* loss,
                               float* bottom_diff, void* workspace, size_t workspace_bytes, void* stream);

/* The fused pose step's loss tail (posecnn_amd/pipeline.py): the prepared
 * loss's per-point sums, then one pass that finishes each row's bottom_diff
 * and runs the pose head's backward on it (pcnn_pose_head_bwd with
 * d_pred = bottom_diff, scaled by d_pred_scale[0] -- the ADD gradient op,
 * cu.cc:346-354; tanh_out and poses_weight = weight as pcnn_pose_head_fwd
 * used them) into d_y8 (R, 4C): the same bits as pcnn_add_loss_fwd_prepared
 * + pcnn_pose_head_bwd.  The scalar loss is left to pcnn_add_loss_total on
 * the same workspace, which the caller may order on another stream (nothing
 * on the backward chain reads it).  4C <= 256. */
int pcnn_add_loss_fwd_head_bwd(const float* pred, const float* target, const float* weight, const float* points,
                               const float* symmetry, int R_cap, const int32_t* num_rois_dev, int C, int P,
                               float margin, int loss_norm_rows, const int32_t* loss_norm_rows_dev,
                               float* bottom_diff, void* workspace, size_t workspace_bytes, const float* tanh_out,
                               const float* d_pred_scale, float* d_y8, void* stream);
int pcnn_add_loss_total(int R_cap, const int32_t* num_rois_dev, int C, int P, const void* workspace,
                        size_t workspace_bytes, float* loss, void* stream);

/* out[i] = top_diff[0] * bottom_diff[i], n = rows * 4C */
int pcnn_add_loss_bwd(const float* top_diff, const float* bottom_diff, int n, const int32_t* num_rois_dev,
                      int row_len, float* out, void* stream);

/* Self-check of the ADD loss's per-launch division (average_distance.hip
 * div_rn): out[i] = x[i] / b correctly rounded, through the kernels' reciprocal
 * + two fma-correction form, in fp32 (dbl = 0) or in double rounded to fp32
 * (dbl = 1, the loss-sum form of cu.cc:181).  Test infrastructure only. */
int pcnn_div_rn_check(const float* x, float b, int n, int dbl, float* out, void* stream);

/* ---------------------------------------------------------------------------
 * Depth backprojection (Backproject / BackprojectGrad).
 * Replaces BackprojectForwardLaucher / BackprojectBackwardLaucher
 * (lib/backprojecting_layer/backprojecting_op_gpu.cu.cc:129-155, :220-242;
 *  called from backprojecting_op.cc:262-267, :388-390).
 *  data (B,H,W,Ch) label (B,H,W,NC) depth (B,H,W) meta (B,num_meta) label_3d (B,G,G,G,NC)
 *  -> top_data (B,G,G,G,Ch), top_label (B,G,G,G,NC), top_flag (B,G,G,G,Ch)
 * ------------------------------------------------------------------------- */
int pcnn_backproject_fwd(const float* data, const float* label, const float* depth, const float* meta, int num_meta,
                         const float* label_3d, int B, int H, int W, int Ch, int NC, int grid_size,
                         int kernel_size, float threshold, float* top_data, float* top_label, float* top_flag,
                         void* stream);

int pcnn_backproject_bwd(const float* top_diff, const float* depth, const float* meta, int num_meta, int B, int H,
                         int W, int Ch, int grid_size, float* bottom_diff, void* stream);

/* ---------------------------------------------------------------------------
 * Pose-head FC contraction (MFMA).  Replaces the TF matmuls of
 * Network.fc (lib/networks/network.py:393-423) as wired by vgg16_convs.py:186-197:
 *   C[M,N] = epilogue( op(A)[M,K] (+ op(A2)) * op(B)[K,N] )
 *  a_trans: 0 -> A stored (M,K) row-major (lda >= K); 1 -> A stored (K,M) (lda >= M)
 *  b_trans: 0 -> B stored (K,N) (ldb >= N);           1 -> B stored (N,K) (ldb >= K)
 *  A2 (optional): same layout as A, added elementwise (pool5 + pool4 fusion)
 *  M_dev / K_dev (optional device ints): effective M / K = min(*dev, M / K)
 *  epilogue: bias (N) added if non-NULL; act 0 none, 1 relu;
 *            mask (optional, ldm) -> C *= (mask > 0)  (relu backward)
 *  precision: 0 = exact fp32 MFMA (v_mfma_f32_32x32x2_f32),
 *             1 = split-bf16 x3 MFMA (hi*hi + hi*lo + lo*hi: ~2^-16 per product),
 *             2 = exact three-way split-bf16 x6 MFMA (hi/mid/lo planes, six
 *                 products: within 2^-24 |a||b| per product, fp32
 *                 accumulation -- fp32-faithful; the pose step's default).
 *                 Operand range: finite |x| <= 3.3895314e38 (the largest bf16);
 *                 there results track fp32.  An inf / NaN operand, or a finite
 *                 one above that bound (its hi plane rounds to inf), makes the
 *                 output elements it reaches NaN (fp32 would give +-inf or a
 *                 finite value); every other element is unaffected
 *                 (tests/test_gpu_gemm_fc6.py::test_x6_edge_semantics).
 *  Deterministic (split-K partials are reduced in fixed order).
 *  workspace: >= pcnn_gemm_workspace_size() bytes, one per stream.
 * ------------------------------------------------------------------------- */
size_t pcnn_gemm_workspace_size(int M, int N, int K, int m_dynamic, int precision);

int pcnn_gemm(int M, int N, int K, const float* A, const float* A2, int lda, int a_trans, const float* B, int ldb,
              int b_trans, float* Cm, int ldc, const float* bias, int act, const float* mask, int ldm,
              const int32_t* M_dev, const int32_t* K_dev, int precision, void* workspace, size_t workspace_bytes,
              void* stream);

/* pcnn_gemm plus the pose head's dropout (drop6 / drop7, vgg16_convs.py:189,191;
 * Network.dropout = tf.nn.dropout, network.py:574-577; keep_prob 0.5 in
 * training, lib/fcn/train.py:421, 1.0 at test time, test.py:173):
 *  drop (optional, uint8 (M, ldd >= N), 0 / 1): forward, applied after bias / act
 *       as tf.nn.dropout computes it: C = (v / keep_prob) * drop
 *  mask (optional): backward of relu + dropout, with mask = the dropped
 *       forward activation: C = mask > 0 ? v / keep_prob : 0
 *       (TF: ReluGrad(features) of (grad * binary) / keep_prob)
 *  keep_prob in (0, 1]; 1 with drop == NULL is exactly pcnn_gemm. */
int pcnn_gemm_drop(int M, int N, int K, const float* A, const float* A2, int lda, int a_trans, const float* B,
                   int ldb, int b_trans, float* Cm, int ldc, const float* bias, int act, const float* mask, int ldm,
                   const uint8_t* drop, int ldd, float keep_prob, const int32_t* M_dev, const int32_t* K_dev,
                   int precision, void* workspace, size_t workspace_bytes, void* stream);

/* The forward of pcnn_gemm_drop with the keep mask drawn in the epilogue: the
 * reduce pass draws, for every live element (m < effective M, n < N), the bit
 * pcnn_dropout_mask would write for a dense (M, N) mask with the same seed,
 * *step_dev and stream_id, applies C = (v / keep_prob) * bit, and stores the
 * bits into drop_out (uint8 (M, ldd)) for the backward (pcnn_gemm_drop with
 * mask).  Bit-identical to pcnn_dropout_mask (rows_dev = M_dev) followed by
 * pcnn_gemm_drop, without the mask launch.  N % 4 == 0, ldd % 4 == 0. */
int pcnn_gemm_drop_gen(int M, int N, int K, const float* A, const float* A2, int lda, int a_trans, const float* B,
                       int ldb, int b_trans, float* Cm, int ldc, const float* bias, int act, uint8_t* drop_out,
                       int ldd, float keep_prob, uint64_t seed, const int64_t* step_dev, int stream_id,
                       const int32_t* M_dev, const int32_t* K_dev, int precision, void* workspace,
                       size_t workspace_bytes, void* stream);

/* The x6 GEMM on pre-split operands (gemm_tp.hip), bit-identical to pcnn_gemm
 * precision 2 on the same fp32 values, with no split work in its K loop.
 * Tiled planes ("TP") of a rows x K operand: block (rb, ks) of 32 rows x 16 k
 * is 3 KiB at ((rb * ceil(K/16) + ks) * 3) KiB, planes hi / mid / lo (the exact
 * 3-way bf16 split), lane l of a plane holding row 32 rb + (l & 31),
 * k 16 ks + 8 (l >> 5) .. + 7 (the MFMA operand fragment).
 *  pcnn_tp_bytes: storage of one operand.
 *  pcnn_split_tp: dst <- TP of the fp32 view src[row * row_stride + k * k_stride]
 *    (rows, K capacities; effective counts from rows_dev / K_dev if non-NULL,
 *    zeros past them; row blocks past ceil(rows_eff / 32) and K steps past
 *    ceil(K_eff / 16) are never multiplied and not written).
 *  pcnn_gemm_tp: C[M,N] = epilogue(A · B) with A_tp = TP of op(A) (M x K) and
 *    B_tp = TP of op(B)^T (N x K), both stored at capacity K; epilogue, M_dev /
 *    K_dev, dropout and workspace as pcnn_gemm_drop at precision 2. */
size_t pcnn_tp_bytes(int rows, int K);
int pcnn_split_tp(const float* src, long row_stride, long k_stride, int rows, const int32_t* rows_dev, int K,
                  const int32_t* K_dev, void* dst, size_t dst_bytes, void* stream);
int pcnn_gemm_tp(int M, int N, int K, const void* A_tp, const void* B_tp, float* Cm, int ldc, const float* bias,
                 int act, const float* mask, int ldm, const uint8_t* drop, int ldd, float keep_prob,
                 const int32_t* M_dev, const int32_t* K_dev, void* workspace, size_t workspace_bytes, void* stream);

/* Dropout keep masks (the binary tensor of tf.nn.dropout: floor(keep_prob + U[0,1))):
 * mask[r, c] for r < min(*rows_dev, rows) (rows_dev may be NULL), c < cols, row
 * pitch ld >= cols bytes.  U comes from Philox4x32-10 (key = seed, counter =
 * (element quad index, *step_dev)) in TF's uint32 -> float construction
 * ((x & 0x7fffff) | 0x3f800000 as a float, minus 1).  The draw is keyed on the
 * device-side step counter, so a captured HIP graph draws new masks on every
 * replay.  TF's own stream assignment is not reproducible (parity unpinned:
 * the masks are i.i.d. Bernoulli(keep_prob) either way); several masks of one
 * step take distinct `stream_id`s.  cols % 4 == 0 and ld % 4 == 0. */
int pcnn_dropout_mask(uint8_t* mask, int rows, int cols, int ld, const int32_t* rows_dev, uint64_t seed,
                      const int64_t* step_dev, int stream_id, float keep_prob, void* stream);

/* Philox4x32-10 self-check (test infrastructure): out[4 i .. 4 i + 3] = philox(ctr[4 i .. 4 i + 3], key[2 i .. 2 i + 1]). */
int pcnn_philox_check(const uint32_t* ctr, const uint32_t* key, int n, uint32_t* out, void* stream);

/* ---------------------------------------------------------------------------
 * RGB-only pose estimation (the RANSAC half).
 * Replaces Synthesizer::estimatePose2D (lib/synthesize/synthesize.cpp:1571-1766;
 * synthesizer.pyx:74-82 estimate_poses_2d, called from lib/fcn/test.py:1364).
 *  label (H,W) int32, vertmap (H,W,3C) object coordinates scaled to [0,1] by the
 *  class extents (getMode3D, :1052-1071), extents (C,3), pinhole fx fy px py.
 *  Preemptive RANSAC: n_hyp (1..256; 256 = the reference's ransacIterations,
 *  :1601) hypotheses, each from 4 pixels of one object (> 400 pixels) through
 *  P3P; attempt a of hypothesis h draws on its own Philox stream (h, a) of
 *  `seed`, h keeps its first accepted attempt (at most max_iter attempts); 8
 *  rounds of inlier counting (< 10 px) over pixel subsets with the
 *  reference's skip law max(1, G), G geometric with p = 1000 r / N (drawn
 *  from Philox streams (j, class, round) of `seed`), keeping the better
 *  half.  Outputs (device): poses_out (3,4,C) [R | t] per class (the reference's
 *  layout; classes without a hypothesis 0); hyps_out (n_hyp,13) [objID or -1 |
 *  R | t]; hyp_px (n_hyp,4) sampled pixel indices; inl_out (n_hyp,8) inliers per
 *  round (-1: not queued); final_out (C,3) [h, inliers, hypotheses] (-1: none).
 *  Asynchronous on `stream`: object lists and subsets are built on the device. */
size_t pcnn_pose2d_workspace_size(int H, int W, int C, int n_hyp);
int pcnn_pose2d(const int32_t* label, const float* vertmap, const float* extents, int H, int W, int C, float fx,
                float fy, float px, float py, uint64_t seed, int n_hyp, int max_iter, float* poses_out,
                float* hyps_out, int32_t* hyp_px, int32_t* inl_out, int32_t* final_out, void* workspace,
                size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Depth-based pose estimation (the cfg.TEST.VERTEX_REG_3D
 * branch).  Replaces Synthesizer::estimatePose3D (lib/synthesize/synthesize.cpp:
 * 1769-1965; synthesizer.pyx:86-95 estimate_poses_3d, called from
 * lib/fcn/test.py:1385, its poses then refined by solveICP, test.py:1403-1416).
 *  label, vertmap, extents, fx fy px py as pcnn_pose2d; depth (H,W) uint16 raw
 *  depth, camera coordinates = pxToEye (:1372-1389) with depth_factor.
 *  Preemptive RANSAC over 3-D / 3-D correspondences: n_hyp (1..256) hypotheses,
 *  each from 3 pixels of one object with depth through the rigid (Kabsch)
 *  transform, 1 cm reconstruction and 400 px box-area checks (attempt a of
 *  hypothesis h on Philox stream (h, 'P3D', a)); 8 rounds of inlier counting
 *  (< 1 cm) over hole-skipping pixel subsets (the pcnn_pose2d skip law), the
 *  better half kept, then updateHyp3D's refit on at most 1000 inliers
 *  (filterInliers3D picks on streams (h, 'F3D', 1024 r + k)); the survivor with
 *  more than 10 inliers refined by a bounded Nelder-Mead (nm_evals evaluations,
 *  100 in the reference) of optEnergy3D over (Rodrigues vector, t).
 *  Outputs (device): poses_out (3,4,C); hyps_out (n_hyp,13); hyp_px (n_hyp,3);
 *  inl_out (n_hyp,8); final_out (C,3) as pcnn_pose2d; energy_out (C) the
 *  refined optEnergy3D (0: not refined); eye_out (H,W,3) camera coordinates,
 *  optional (NULL: not written).  Asynchronous on `stream`. */
size_t pcnn_pose3d_workspace_size(int H, int W, int C, int n_hyp);
int pcnn_pose3d(const int32_t* label, const uint16_t* depth, const float* vertmap, const float* extents, int H, int W,
                int C, float fx, float fy, float px, float py, float depth_factor, uint64_t seed, int n_hyp,
                int max_iter, int nm_evals, float* poses_out, float* hyps_out, int32_t* hyp_px, int32_t* inl_out,
                int32_t* final_out, float* energy_out, float* eye_out, void* workspace, size_t workspace_bytes,
                void* stream);

/* Column sums over the first min(*M_dev, M) rows: out[n] = sum_m X[m, n] (bias gradients). */
int pcnn_colsum(const float* X, int M, int N, int ldx, const int32_t* M_dev, float* out, void* stream);

/* Pose-head tail (vgg16_convs.py:193-197): T = tanh(Y8); Mw = T * poses_weight;
 * pred = Mw / sqrt(max(sum(Mw^2), 1e-12)) (tf.nn.l2_normalize, dim 1).  Rows (R_cap, D). */
int pcnn_pose_head_fwd(const float* y8, const float* poses_weight, int R_cap, const int32_t* num_rois_dev, int D,
                       float* tanh_out, float* pred, void* stream);

/* Backward of the tail: d_pred -> d_y8 (through l2_normalize, multiply, tanh).
 * d_pred_scale (optional device scalar): d_pred is taken as d_pred_scale[0] * d_pred,
 * i.e. the ADD-loss gradient op (AveragedistanceBackward, average_distance_loss_op_gpu.cu.cc:346-354:
 * top_diff[0] * bottom_diff) folded into this pass; NULL = d_pred as given. */
int pcnn_pose_head_bwd(const float* d_pred, const float* d_pred_scale, const float* tanh_out,
                       const float* poses_weight, const float* pred, int R_cap, const int32_t* num_rois_dev, int D,
                       float* d_y8, void* stream);

/* The fc7 -> fc8 -> pose head chain of the pose step with fc8 (4C = D <= 128
 * columns) fused into the split-K reduces around it (fc8_fused.hip).  Bit for
 * bit pcnn_gemm_drop_gen / pcnn_gemm_drop (fc7 forward) -> pcnn_gemm (fc8
 * forward) -> pcnn_pose_head_fwd, and pcnn_gemm_drop (fc8 dX), at precision 2.
 *
 * pcnn_gemm_partial: pcnn_gemm's GEMM kernel without the reduce pass that
 *  would follow it: split-K partial slabs [S][M][N] stay in `workspace` (when
 *  the plan runs whole tiles, C holds bias / act applied).
 * pcnn_fc8_fwd_fused: after pcnn_gemm_partial of the fc7 forward (M, N7, K7,
 *  same M_dev, fc7_workspace): forms y7 (M, ld7) = dropout(act7(sum of slabs +
 *  b7)) -- keep bits given in `drop`, or drawn into it (drop_gen: seed,
 *  *step_dev, stream_id as pcnn_gemm_drop_gen), or none (keep_prob 1, drop
 *  NULL) -- while staging it as the A operand of y7 @ W8 (N7, ldb >= D), and
 *  leaves fc8's split-K partials in fc8_workspace (at least
 *  pcnn_gemm_workspace_size(M, D, N7, M_dev != NULL, 2) bytes, distinct from
 *  fc7_workspace).  N7 % 4 == 0, 16-byte aligned rows.
 * pcnn_fc8_reduce_head_fwd: y8 (R_cap, D) = slabs of fc8_workspace in slice
 *  order + b8, then pcnn_pose_head_fwd's row pass on it.  K = N7.
 * pcnn_fc8_dx_skinny: dy7 (M, ldc >= N7) = (mask > 0 ? dy8 (M, lda >= D) @
 *  W8 (N7, ldb >= D)^T : 0) / keep_prob; D % 4 == 0.  Takes the completion
 *  event (pcnn_set_completion_event). */
int pcnn_gemm_partial(int M, int N, int K, const float* A, const float* A2, int lda, int a_trans, const float* B,
                      int ldb, int b_trans, float* Cm, int ldc, const float* bias, int act, const int32_t* M_dev,
                      const int32_t* K_dev, int precision, void* workspace, size_t workspace_bytes, void* stream);
int pcnn_fc8_fwd_fused(int M, int N7, int K7, const void* fc7_workspace, size_t fc7_workspace_bytes, const float* b7,
                       int act7, float* y7, int ld7, uint8_t* drop, int ldd, float keep_prob, int drop_gen,
                       uint64_t seed, const int64_t* step_dev, int stream_id, const float* W8, int ldb, int D,
                       const int32_t* M_dev, void* fc8_workspace, size_t fc8_workspace_bytes, void* stream);
int pcnn_fc8_reduce_head_fwd(const void* fc8_workspace, size_t fc8_workspace_bytes, const float* b8, int R_cap, int K,
                             int D, const int32_t* num_rois_dev, const float* poses_weight, float* y8,
                             float* tanh_out, float* pred, void* stream);
int pcnn_fc8_dx_skinny(const float* dy8, int lda, const float* W8, int ldb, const float* mask, int ldm,
                       float keep_prob, float* dy7, int ldc, int M, int D, int N7, const int32_t* M_dev,
                       void* stream);

/* ---------------------------------------------------------------------------
 * Class-aware greedy box NMS + pose combination (inference consumer of the
 * Hough rows).
 * Replaces lib/utils/nms.py:3-32 (numpy, on the host after a D2H copy) and the
 * pose combination of lib/fcn/test.py:197-211.
 *  rois (R_cap, roi_stride >= 7) [b,cls,x1,y1,x2,y2,score], row count from
 *  num_rois_dev (may be NULL: R_cap rows), R_cap <= 1152 (MAX_ROI * 9).
 *  keep (R_cap) int32: kept row indices, score descending (ties: lower row
 *  first — numpy argsort()[::-1] leaves tie order unspecified); num_keep (1).
 *  Optional (NULL to skip): rois_out (R_cap,7) = rois[keep]; poses_out (R_cap,7)
 *  = poses_init[keep] with [:4] = poses_pred[keep, 4*cls : 4*cls+4] for cls >= 0
 *  (poses_pred rows of pred_dim floats). Overlap test and areas in float32 in
 *  nms.py's operation order; suppression needs ovr > thresh and equal class.
 * ------------------------------------------------------------------------- */
int pcnn_box_nms(const float* rois, int R_cap, int roi_stride, const int32_t* num_rois_dev, float thresh,
                 int32_t* keep, int32_t* num_keep, const float* poses_init, const float* poses_pred, int pred_dim,
                 float* rois_out, float* poses_out, void* stream);

/* ---------------------------------------------------------------------------
 * Label producers.
 * argmax_2d: label (B,H,W) int32 = argmax over the last axis of prob (B,H,W,C)
 *   (lib/networks/network.py:433-434 `tf.to_int32(tf.argmax(input, 3))`);
 *   first maximum, a NaN wins at its first occurrence (numpy / tf.argmax).
 * Hardlabel: replaces HardlabelForwardLaucher / HardlabelBackwardLaucher
 *   (lib/hard_label_layer/hard_label_op_gpu.cu.cc:17-29,32-52,56-90; op
 *   hard_label_op.cc:30-44). top (B,H,W,C) = one-hot of gt where gt != -1 and
 *   (gt > 0 or prob[gt] < threshold), else 0; threshold > 0 (the op's attr
 *   check). gt outside [-1, C) (out-of-row store in the reference) -> zero row.
 *   Backward: zero gradients for prob (B,H,W,C) and gt (B,H,W) (either NULL).
 * ------------------------------------------------------------------------- */
int pcnn_argmax_2d(const float* prob, int B, int H, int W, int C, int32_t* label, void* stream);
int pcnn_hard_label_fwd(const float* prob, const int32_t* gt, int B, int H, int W, int C, float threshold,
                        float* top, void* stream);
int pcnn_hard_label_bwd(float* grad_prob, float* grad_gt, int B, int H, int W, int C, void* stream);

/* vertex_pred (vgg16_convs.py:152-163: 1x1 conv K -> 3C + bias_add,
 * network.py:168-185) evaluated only at each pixel's label class (SURVEY
 * §8(f) row 3): feat (B,H,W,K) NHWC, K % 4 == 0, weights (K,3C) as the
 * reference's [1,1,K,3C] kernel, bias (3C), label (B,H,W) -> vertex3 (B,H,W,3)
 * = (sum_k feat[k] * w[k][3l+j] in k order) + bias[3l+j]; zeros for labels
 * outside [0, C). K * 3C * 4 B <= 64 KiB. */
int pcnn_vertex_pred_compact(const float* feat, const float* weights, const float* bias, const int32_t* label, int B,
                             int H, int W, int K, int C, float* vertex3, void* stream);

/* ---------------------------------------------------------------------------
 * Test-time pose refinement: the numerical core of
 * Synthesizer::solveICP (lib/synthesize/synthesize.cpp:2052-2395, reached from
 * lib/fcn/test.py:1316-1351 via synthesizer.icp_python, synthesizer.pyx:60-75).
 * Maps are row-major (H,W,ch) f32; the rendered maps (the reference's OpenGL
 * pass, synthesize.cpp:2106-2137) are inputs: pred_vertices / pred_normals
 * (H,W,4) per problem (renderer_vn_ textures), vertmap (H,W,3) canonical model
 * coordinates with the class id in the integer part of x (renderer_ texture).
 * Poses are (qw,qx,qy,qz,tx,ty,tz); input quaternions are normalised as
 * Sophus' SE3(quaternion, translation) constructor does.
 *
 * pcnn_icp_live_vertices: live (L,H,W,3) = df::backproject of the masked depth
 *   (synthesize.cpp:2140-2160; backprojection.cu:10-27, Poly3 camera at zero
 *   distortion): d = depth / factor where label == obj_ids[l], else 0;
 *   vertex = ((x-px)/fx*d, (y-py)/fy*d, d). depth (H,W) uint16, H*W % 4 == 0.
 * pcnn_icp: df::icp (lib/kinect_fusion/src/optimization/icp.cpp:20-106 +
 *   icp.cu:22-245) for N problems: `iterations` Gauss-Newton steps of the
 *   projective point-to-plane residual (border 2 px, ray/normal test 0.1,
 *   |error| <= max_error, weight 1/live depth), each solving JTJ x = JTr
 *   (Eigen LDLT) and left-multiplying SE3::exp(x) into the accumulated update.
 *   live (num_live,H,W,3) with live_index (N) selecting problem n's map (NULL:
 *   n; an index outside [0, num_live) contributes no pixel);
 *   update (N,7); pose_in / pose_out (N,7) optional: pose_out = update * pose_in
 *   (refinePose, synthesize.cpp:2023-2025); systems (N,iterations,28) optional:
 *   per iteration the 21 upper-triangle JTJ entries, 6 JTr and the pixel count.
 * pcnn_icp_center: the translation re-centring of solveICP
 *   (synthesize.cpp:2163-2219) for L objects: out (L,4) = mean(live - model) over
 *   the object's pixels with depth > 0, finite vertmap and |n.(live - pred)| <
 *   max_error, and the count; pose_out = pose_in with t = (rx Tz, ry Tz, Tz),
 *   rx = tx / tz of pose_in, when the count is > 0.
 * pcnn_pose_energy: optEnergy (synthesize.cpp:2474-2526) of K poses: mean
 *   |T p - v| over the object's pixels with finite T p and both depths inside
 *   (znear, zfar); energy (K).
 * ------------------------------------------------------------------------- */
int pcnn_icp_live_vertices(const uint16_t* depth, const int32_t* label, int H, int W, const int32_t* obj_ids, int L,
                           float factor, float fx, float fy, float px, float py, float* live, void* stream);
size_t pcnn_icp_workspace_size(int N, int H, int W);
int pcnn_icp(const float* live, int num_live, const int32_t* live_index, const float* pred_vertices,
             const float* pred_normals, int N, int H, int W, float fx, float fy, float px, float py, float znear, float zfar, float max_error,
             int iterations, const float* pose_in, float* update, float* pose_out, float* systems, void* workspace,
             size_t workspace_bytes, void* stream);
size_t pcnn_icp_reduce_workspace_size(int L, int H, int W);
int pcnn_icp_center(const float* live, const int32_t* label, const int32_t* obj_ids, int L, const float* vertmap,
                    const float* pred_vertices, const float* pred_normals, int H, int W, float max_error,
                    const float* pose_in, float* out, float* pose_out, void* workspace, size_t workspace_bytes,
                    void* stream);
/* Nelder-Mead on optEnergy on the device (round 5): solveICP's refinePose
 * search (synthesize.cpp:2221-2250 -> poseWithOpt :2529-2573, NLopt
 * LN_NELDERMEAD over 7 parameters, optEnergy :2476-2526).
 *  pcnn_energy_records: for problem i (N), the pixels with label ==
 *  prob_obj[i] whose live vertex (live (n_live,H,W,3)[prob_live[i]]) has z in
 *  (znear, zfar), in raster order, as records (rendered vertex
 *  pred_vertices (N,H,W,4)[i] xyz, live xyz) -> records (N, H*W, 6), counts (N).
 *  pcnn_energy_rec: optEnergy of K poses (K,7), pose k over problem
 *  pose_prob[k]'s records (stride = records per problem, H*W).
 *  pcnn_nelder_mead_energy: N bounded Nelder-Mead searches (x0, lb, ub (N,7)
 *  float64, at most max_eval evaluations; the operation order of
 *  posecnn_amd/synthesize/icp.py nelder_mead_steps), one workgroup each, the
 *  energy of every trial point as pcnn_energy_rec computes it (the same bits)
 *  -> x_out (N,7), f_out (N) float64, nev_out (N). Asynchronous. */
size_t pcnn_energy_records_workspace_size(int N, int H, int W);
int pcnn_energy_records(const float* live, int n_live, const int32_t* label, const float* pred_vertices, int H, int W,
                        float znear, float zfar, int N, const int32_t* prob_obj, const int32_t* prob_live,
                        float* records, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream);
int pcnn_energy_rec(const float* records, const int32_t* counts, int stride, const float* poses,
                    const int32_t* pose_prob, int K, float znear, float zfar, float* energy, void* stream);
int pcnn_nelder_mead_energy(const float* records, const int32_t* counts, int stride, int N, const double* x0,
                            const double* lb, const double* ub, int max_eval, float znear, float zfar, double* x_out,
                            double* f_out, int32_t* nev_out, void* stream);

/* pcnn_nelder_mead_energy with 8 cooperating workgroups per evaluated point
 * (the evaluation's records spread over 8 CUs, one arrive-and-wait per round
 * through the workspace), launched cooperatively; the same bits.  N <= 32:
 * speculative rounds (an iteration's reflection, expansion and both
 * contractions evaluated together by 4 x 8 workgroups, the search counting
 * only those it uses); N <= 128: one point per round.  The workspace holds
 * the wave sums, one arrival counter and one failure flag per problem
 * (zeroed by the call).  nev_out = -1 marks a problem one of whose
 * cross-workgroup waits gave up: every workgroup of it stops at its next
 * barrier and its x / f are invalid.  max_eval >= 8 (the initial simplex;
 * NLopt's maxeval, which poseWithOpt / refineWithOpt set, counts it too).
 * The _path form pins the kernel (force_path 1 speculative, 2 cooperative,
 * 3 one workgroup; 0 the first that launches) and reports the one that ran
 * in *path_out (host int, may be NULL); PCNN_EHIP if a forced one cannot
 * launch. */
size_t pcnn_nelder_mead_energy_workspace_size(int N);
int pcnn_nelder_mead_energy_coop(const float* records, const int32_t* counts, int stride, int N, const double* x0,
                                 const double* lb, const double* ub, int max_eval, float znear, float zfar,
                                 double* x_out, double* f_out, int32_t* nev_out, void* workspace,
                                 size_t workspace_bytes, void* stream);
int pcnn_nelder_mead_energy_coop_path(const float* records, const int32_t* counts, int stride, int N,
                                      const double* x0, const double* lb, const double* ub, int max_eval,
                                      float znear, float zfar, double* x_out, double* f_out, int32_t* nev_out,
                                      void* workspace, size_t workspace_bytes, int force_path, int32_t* path_out,
                                      void* stream);

/* pcnn_icp_score: the SegICP hypothesis score of solveICP (synthesize.cpp:2288-2330):
 *   over the object's pixels with depth > 0 and a finite vertmap, each model
 *   point (vertmap, class offset dropped) moved by hypothesis j takes its
 *   nearest live point within `radius` (squared distance < radius^2; ties ->
 *   lowest raster index); score (J) = distinct live points taken / model points;
 *   choose (1) = first best hypothesis (0 when the object has no such pixel).
 *   J <= 64. */
size_t pcnn_icp_score_workspace_size(int J, int H, int W);
int pcnn_icp_score(const float* live, const int32_t* label, int obj, const float* vertmap, int H, int W,
                   const float* hyps, int J, float radius, float* score, int32_t* choose, void* workspace,
                   size_t workspace_bytes, void* stream);
int pcnn_pose_energy(const float* live, const int32_t* label, int obj, const float* pred_vertices, int H, int W,
                     float znear, float zfar, const float* poses, int K, float* energy, void* workspace,
                     size_t workspace_bytes, void* stream);

/* Batched optEnergy: pose k (of K) is scored for object pose_obj[k] against live
 * map pose_live[k] (of n_live, (H,W,3) each) and rendered vertices pose_pv[k]
 * (of n_pv, (H,W,4) each) -- one launch for the Nelder-Mead simplices of every
 * RoI of solveICP (synthesize.cpp:2529-2573), which the reference evaluates one
 * pose at a time.  workspace: pcnn_icp_reduce_workspace_size(K, H, W). */
int pcnn_pose_energy_batch(const float* live, int n_live, const int32_t* label, const float* pred_vertices, int n_pv,
                           int H, int W, float znear, float zfar, const float* poses, int K, const int32_t* pose_obj,
                           const int32_t* pose_live, const int32_t* pose_pv, float* energy, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Mesh rasteriser: the rendered maps the refinement ops above take as inputs,
 * i.e. the role of the reference's OpenGL pass (synthesize.cpp:2103-2139 with
 * lib/kinect_fusion/shaders canonicalVerts.* and vertsAndNorms.*).  K problems,
 * one mesh and one pose each, no texture, colour or lighting.
 *  packed mesh set (M meshes): vertices / normals (V_total,3) f32 model frame,
 *    faces (F_total,3) int32 vertex indices LOCAL to their mesh, vert_offset /
 *    face_offset (M+1) int32 row ranges of each mesh; F_max >= the largest
 *    mesh's face count.
 *  per problem: mesh_index (K) int32, class_id (K) int32, poses (K,7)
 *    (quaternion normalised here).  A mesh_index outside [0, M), or offsets
 *    that do not fit (V_total, F_total, F_max), render nothing for that problem.
 *  fx, fy, px, py: pixel (x, y) samples u = x, v = y, u = fx X / Z + px;
 *    0 < znear <= zfar: a triangle with a vertex at Z < znear is dropped whole
 *    (no near-plane clipping), a fragment with Z > zfar is discarded.
 *  outputs, every pixel written (the caller never clears them):
 *    pred_vertices (K,H,W,4) camera-frame position of the nearest surface
 *      point, perspective-correct, w = 1; all 0 off the model
 *    pred_normals (K,H,W,4) interpolated R n / |R n| (not renormalised), w = 0;
 *      all 0 off the model
 *    vertmap (K,H,W,3) interpolated model-frame position, class_id added to x
 *      (synthesize.cpp:267-274); NaN off the model (glClearColor(nan), :2113)
 *    depth (K,H,W) f32 camera Z, 0 off the model (optional, may be NULL)
 *    tri_id (K,H,W) int32 winning face within its mesh, -1 off the model
 *      (optional, may be NULL)
 *    pred_vertices, pred_normals and the workspace are 16-byte aligned.
 *  Coverage is exact (vertices snapped to 1/256 px, int64 edge functions, a
 *  tie rule that gives a shared edge to one triangle), values are float32
 *  from the unsnapped vertices, the nearest Z wins and an equal Z goes to the
 *  lower face index: bitwise reproducible, alone or in a batch (rules at the
 *  top of csrc/render.hip).  The z-buffer is cleared inside the op.
 *  PCNN_EINVAL: a NULL required pointer, K, H, W, M, V_total or F_max <= 0,
 *  K > 65535, znear <= 0; PCNN_ECAPACITY: a short workspace.
 * ------------------------------------------------------------------------- */
size_t pcnn_render_workspace_size(int K, int H, int W, int V_total, int F_max);
int pcnn_render_meshes(const float* vertices, const float* normals, const int32_t* faces, const int32_t* vert_offset,
                       const int32_t* face_offset, int M, int V_total, int F_total, int F_max,
                       const int32_t* mesh_index, const int32_t* class_id, const float* poses, int K, int H, int W,
                       float fx, float fy, float px, float py, float znear, float zfar, float* pred_vertices,
                       float* pred_normals, float* vertmap, float* depth, int32_t* tri_id, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Scene renderer: the ground truth of synthetic training frames, i.e. the role
 * of Synthesizer::render (synthesize.cpp:345-609), of the label / visibility
 * steps of the render worker (tools/train_net.py:209-230) and of
 * _generate_vertex_targets (gt_synthesize_layer/minibatch.py:517-575).  S
 * scenes, K object instances in all, each scene depth-tested across its
 * instances; no texture, colour or lighting.
 *  packed mesh set, mesh_index / class_id / poses (K): as pcnn_render_meshes.
 *  scene_offset (S+1) int32 on the device: scene s holds the instance rows
 *    [scene_offset[s], scene_offset[s+1]) (a CSR; valid ranges are meant to be
 *    disjoint, a row named by two valid scenes is drawn in the lower-numbered
 *    one).  Checked on the device: an empty range, a decreasing one, one that
 *    leaves [0, K] or one of more than 256 rows renders an all-background
 *    scene.  An instance with an invalid mesh slot draws nothing.
 *  Visibility: per scene pixel the nearest Z wins; an equal Z goes to the
 *    lower rank (the instance's position inside its scene), then to the lower
 *    face (one 64-bit atomicMin of (Z bits << 32) | (rank << 24) | face, so
 *    F_max <= 2^24).  Coverage, culling and values are pcnn_render_meshes's: a
 *    scene of one instance gives that op's bits for the instance.
 *  outputs, every element written (the caller never clears them):
 *    label (S,H,W) int32 the winner's class_id, 0 off the models
 *    depth (S,H,W) f32 camera Z, 0 off the models
 *    vertmap (S,H,W,3) f32 model coordinates, class_id added to x; NaN off
 *    vertex3 (S,H,W,3) f32 class-compact vote target of the winning instance
 *      (the layout pcnn_hough_voting_compact reads), 0 off the models:
 *      c = (fx (tx / tz) + px, fy (ty / tz) + py) in f32 (synthesize.cpp:558-562);
 *      channels 0, 1 = (c - (x, y)) / (|c - (x, y)| + 1e-10), difference, norm
 *      and quotient in double, rounded to f32 (minibatch.py:556-567); channel
 *      2 = (float)log((double)tz) (:568).  Each pixel uses its own instance's
 *      centre: the reference's target when a class occurs once per scene.
 *    inst_id (S,H,W) int32 the winning instance's row in [0, K), -1 off the
 *      models (optional, may be NULL)
 *    visible (K) int32 pixels each instance won (train_net.py:222-230), an
 *      integer sum, zeroed inside the op
 *    centers (K,2) f32 the c above (8-byte aligned)
 *  The workspace is 16-byte aligned.  Nothing is allocated or read back; the
 *  op runs on `stream` and can be captured in a HIP graph.
 *  PCNN_EINVAL: a NULL required pointer, S, K, H, W, M, V_total or F_max <= 0,
 *  K > 65535, F_max > 2^24, znear <= 0, misalignment; PCNN_ECAPACITY: a short
 *  workspace.
 *
 * pcnn_vertex_targets_expand: the compact target back into the reference's
 * blobs.  label (B,H,W) int32, vertex3 (B,H,W,3) -> vertex_targets and
 * vertex_weights (B,H,W,3C), 16-byte aligned: a pixel with label l in [1, C)
 * gets vertex3 at channels 3l..3l+2 and w_inside (VERTEX_W_INSIDE,
 * lib/fcn/config.py:64) at the same channels of the weights; everything else
 * is 0 (minibatch.py:253-254, 566-574).  Every element is written.
 * ------------------------------------------------------------------------- */
size_t pcnn_render_scenes_workspace_size(int S, int K, int H, int W, int V_total, int F_max);
int pcnn_render_scenes(const float* vertices, const float* normals, const int32_t* faces, const int32_t* vert_offset,
                       const int32_t* face_offset, int M, int V_total, int F_total, int F_max,
                       const int32_t* mesh_index, const int32_t* class_id, const float* poses, int K,
                       const int32_t* scene_offset, int S, int H, int W, float fx, float fy, float px, float py,
                       float znear, float zfar, int32_t* label, float* depth, float* vertmap, float* vertex3,
                       int32_t* inst_id, int32_t* visible, float* centers, void* workspace, size_t workspace_bytes,
                       void* stream);
int pcnn_vertex_targets_expand(const int32_t* label, const float* vertex3, int B, int H, int W, int C, float w_inside,
                               float* vertex_targets, float* vertex_weights, void* stream);

/* ---------------------------------------------------------------------------
 * Segmentation and vertex-regression losses, forward and backward: loss_cls
 * and loss_vertex of the training objective (lib/fcn/train.py:489-515).
 * Common to the four ops: float32 per-element arithmetic with every op rounded
 * separately, loss sums in double, reductions in a fixed order without
 * floating-point atomics (two runs give the same bits); `loss` (1) is always
 * written and every element of every requested output is written; optional
 * outputs may be NULL; float maps and the workspace are 16-byte aligned; the
 * ops run on `stream`, allocate nothing, read nothing back and can be captured
 * in a HIP graph.  grad_scale multiplies the gradient only (the incoming
 * d loss).  PCNN_EINVAL: a NULL required pointer, a non-positive dimension, an
 * element count >= 2^31, threshold <= 0, sigma <= 0, misalignment;
 * PCNN_ECAPACITY: a short workspace.  The *_workspace_size queries return 0
 * for dimensions the op rejects.
 *
 * pcnn_seg_loss: the segmentation head (vgg16_convs.py:140-149,
 * network.py:475-506, train.py:455-465) from score (B,H,W,C) f32 and gt_label
 * (B,H,W) int32.  Per pixel: m = max_c score_c, d_c = score_c - m,
 * e_c = expf(d_c), s = e_0 + e_1 + ... in class order;
 *    log_prob (B,H,W,C)         d_c - logf(s)
 *    prob_normalized (B,H,W,C)  e_c / s
 *    label_2d (B,H,W) int32     first maximum of prob_normalized (pcnn_argmax_2d's rule)
 *    gt_label_weight (B,H,W,C)  pcnn_hard_label_fwd of (prob_normalized, gt_label, threshold)
 *    loss = (float)(S / (n + 1e-10)): n the pixels with a non-zero weight row
 *      (an integer count), S the double sum of -log_prob[gt] over them
 *    d_score (B,H,W,C)          (prob_normalized_c - [c == gt]) * inv on those
 *      pixels, 0 elsewhere, inv = grad_scale / ((float)n + 1e-10f): Hardlabel's
 *      gradient is zero, so the denominator is a constant of the graph.
 * A gt outside [-1, C) gives a zero weight row.  The workspace keeps (m, s)
 * per pixel (8 B/px) for the gradient pass.  NaN or infinite scores are
 * outside the numerical contract (no out-of-bounds access follows).
 *
 * pcnn_cross_entropy: loss_cross_entropy_single_frame (train.py:455-465) on
 * scores and labels, both (n_pix, C): loss = (float)(sum(-(labels * scores)) /
 * (sum(labels) + 1e-10)), the product in f32, both sums in double;
 * d_scores (n_pix, C) = -labels * inv, inv = grad_scale / ((float)sum(labels) + 1e-10f).
 *
 * pcnn_vertex_loss: smooth_l1_loss_vertex (train.py:565-574) on n elements of
 * vertex_pred, vertex_targets and vertex_weights.  With c_inv = 1/sigma^2,
 * c_half = sigma^2/2, c_off = 0.5/sigma^2, c_s2 = sigma^2 computed in double
 * and rounded to f32: diff = w * (pred - tgt), a = |diff|, near = a < c_inv,
 * in = near ? (diff * diff) * c_half : a - c_off;
 *    loss = (float)(sum(in) / (Wsum + 1e-10)), Wsum = sum(w), both in double
 *    d_pred (n) = (w * (near ? diff * c_s2 : sign(diff))) * inv, sign(0) = 0,
 *      inv = grad_scale / ((float)Wsum + 1e-10f)
 * The caller multiplies by VERTEX_W (config.py:63).
 *
 * pcnn_vertex_loss_compact: the same loss on the blob pair that
 * pcnn_vertex_targets_expand(label, vertex3, w_inside) would have written,
 * without forming it: a pixel with label l in [1, C) contributes its three
 * channels with weight w_inside, Wsum = (double)w_inside * 3 * count.
 *    label (B,H,W) int32, vertex3 (B,H,W,3) (pcnn_render_scenes's layout)
 *    vertex_pred (B,H,W,pred_ch): pred_ch = 3C reads channels 3l..3l+2,
 *      pred_ch = 3 is pcnn_vertex_pred_compact evaluated at `label`
 *    d_pred (B,H,W,d_ch), d_ch = 3 or 3C; with 3C every element is written,
 *      zeros included.  vertex_pred and d_pred are 16-byte aligned.
 * ------------------------------------------------------------------------- */
size_t pcnn_seg_loss_workspace_size(int B, int H, int W, int C);
int pcnn_seg_loss(const float* score, const int32_t* gt_label, int B, int H, int W, int C, float threshold,
                  float grad_scale, float* log_prob, float* prob_normalized, int32_t* label_2d,
                  float* gt_label_weight, float* d_score, float* loss, void* workspace, size_t workspace_bytes,
                  void* stream);
size_t pcnn_cross_entropy_workspace_size(int n_pix, int C);
int pcnn_cross_entropy(const float* scores, const float* labels, int n_pix, int C, float grad_scale, float* d_scores,
                       float* loss, void* workspace, size_t workspace_bytes, void* stream);
size_t pcnn_vertex_loss_workspace_size(long n);
int pcnn_vertex_loss(const float* vertex_pred, const float* vertex_targets, const float* vertex_weights, long n,
                     float sigma, float grad_scale, float* d_pred, float* loss, void* workspace,
                     size_t workspace_bytes, void* stream);
size_t pcnn_vertex_loss_compact_workspace_size(int B, int H, int W, int C);
int pcnn_vertex_loss_compact(const int32_t* label, const float* vertex3, const float* vertex_pred, int pred_ch, int B,
                             int H, int W, int C, float w_inside, float sigma, float grad_scale, float* d_pred,
                             int d_ch, float* loss, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Backward of the class-compact vertex_pred layer: pcnn_vertex_pred_compact,
 * the 1x1 conv K -> 3C plus bias of lib/networks/vgg16_convs.py:152-163
 * (conv2d then bias_add, network.py:168-185) evaluated at each pixel's own
 * class.  Inputs in the forward's layouts: feat (B,H,W,K) f32 NHWC, weights
 * (K,3C) f32, label (B,H,W) int32, d_vertex3 (B,H,W,3) f32; the forward's
 * domain: K % 4 == 0, K * 3C * 4 B <= 64 KiB, B*H*W*K < 2^31; feat, d_vertex3
 * and d_feat 16-byte aligned.  With g = d_vertex3[p], l = label[p], a pixel is
 * live if 0 <= l < C:
 *    d_feat (B,H,W,K)   t = g0 * w[k][3l]; t = t + g1 * w[k][3l+1];
 *                       t = t + g2 * w[k][3l+2], every op rounded separately;
 *                       zeros at a pixel that is not live
 *    d_weights (K,3C)   d_weights[k][3l+j] = sum of feat[p][k] * g_j over the
 *                       live pixels of class l
 *    d_bias (3C)        d_bias[3l+j] = sum of g_j over the same pixels
 * With `label` the ground-truth label map these are the reference's gradients
 * under the loss's own mask (smooth_l1_loss_vertex, train.py:565-574, whose
 * vertex_weights are zero off the ground-truth class's three channels).
 * Sums: float32 products and float32 sums in a fixed order without
 * floating-point atomics: each range of 2048 pixels is summed into a partial
 * in the workspace (pcnn_vertex_pred_compact_bwd_partials of them) and the
 * partials are added in range order, so two runs give the same bits.  A pixel
 * whose three gradients are all zero is skipped without reading feat, so NaN
 * or infinite inputs are outside the numerical contract (no out-of-bounds
 * access follows) and the sign of a zero result is not pinned.  Every element
 * of every requested output is written, zeros for a class with no pixel.
 * Each output may be NULL, at least one is required; feat may be NULL when
 * d_weights is, weights when d_feat is, the workspace when only d_feat is
 * asked for.  The op runs on `stream`, allocates nothing, reads nothing back
 * and can be captured in a HIP graph.  PCNN_EINVAL: a NULL required pointer,
 * a non-positive or out-of-domain dimension, misalignment; PCNN_ECAPACITY: a
 * short workspace.  The two queries return 0 for dimensions the op rejects.
 * ------------------------------------------------------------------------- */
size_t pcnn_vertex_pred_compact_bwd_workspace_size(int B, int H, int W, int K, int C);
int pcnn_vertex_pred_compact_bwd_partials(int B, int H, int W, int K, int C);
int pcnn_vertex_pred_compact_bwd(const float* feat, const float* weights, const int32_t* label,
                                 const float* d_vertex3, int B, int H, int W, int K, int C, float* d_feat,
                                 float* d_weights, float* d_bias, void* workspace, size_t workspace_bytes,
                                 void* stream);

/* ---------------------------------------------------------------------------
 * The upscore layers: the reference's fixed bilinear transposed conv
 * (`upscore`, `upscore_vertex`: 16x16 at stride 8, lib/networks/
 * vgg16_convs.py:138,162; `upscore_conv5(_vertex)`: 4x4 at stride 2,
 * :122,130,154; filter network.py:141-157, layer :207-222), generic and
 * folded behind the 1x1 conv it feeds.
 *
 * x (B,h,w,Ch) f32 NHWC, stride s in {2,4,8,16}, kernel 2s x 2s, SAME padding:
 * y (B, H = s h, W = s w, Ch).  Output row yo has the taps
 *    i1 = (yo + s/2) div s,  k = yo + s/2 - s i1,  i0 = i1 - 1,
 *    weight (2k+1)/(2s) at i1, (2s-1-2k)/(2s) at i0;
 * a tap with i0 < 0 or i1 >= h is absent (zero padding, not clamping);
 * columns alike; a 2-D weight is the product of its row and column weights
 * (exact).  The generic forward's pinned order, every op rounded separately:
 *    acc = ((t00 + t01) + t10) + t11,  t = x[tap] * weight,
 * taps in the order (i0,j0), (i0,j1), (i1,j0), (i1,j1), absent taps skipped,
 * the first present term starts the sum; then acc + bias[ch] if bias is not
 * NULL; then acc > 0 ? acc : 0 if relu.
 *
 * pcnn_upscore_fwd         the layer above.
 * pcnn_upscore_bwd         d_x[i,j,ch] = sum of weight * m * d_y over the at
 *                          most (2s)^2 outputs that tap (i,j), m = (y > 0)
 *                          with y the forward's output, m = 1 if y is NULL;
 *                          d_bias[ch] = sum of m * d_y (NULL: not computed;
 *                          the workspace may then be NULL).  The order of the
 *                          sums is the device's own and fixed: rows then
 *                          columns for d_x, per-workgroup partials added in
 *                          range order for d_bias.
 * pcnn_upscore_compact_fwd z (B,h,w,3C), bias (3C), label (B,H,W) int32 ->
 *                          vertex3 (B,H,W,3): vertex3[p][j] is the generic
 *                          forward of z with bias and without ReLU at channel
 *                          3l+j for l = label[p] in [0,C), bit for bit; zeros
 *                          for any other label.  With z = x W this is
 *                          vertex_pred(upscore_vertex(x)) at the pixel's own
 *                          class with the two linear layers commuted: equal
 *                          in exact arithmetic, different by float32 rounding.
 * pcnn_upscore_compact_bwd d_z[i,j,3c+k] = sum over the pixels p of the
 *                          window of (i,j) with label[p] = c of weight *
 *                          d_vertex3[p][k]; every one of the 3C channels is
 *                          written, zeros for a class without a pixel there.
 *                          d_bias[3c+k] = sum of d_vertex3[p][k] over the
 *                          pixels of class c.  Either output may be NULL, not
 *                          both; the workspace may be NULL without d_bias.
 *
 * Domain: B, h, w, Ch (C) > 0; B*H*W*max(Ch,3) < 2^31 (compact: Ch = 3, and
 * B*h*w*3C < 2^31, C <= 1024).  The generic pair's full-resolution maps (y,
 * d_y and the mask) are 16-byte aligned.  No floating-point atomics:
 * two runs give the same bits.  NaN or infinite inputs are outside the
 * numerical contract (no out-of-bounds access follows); the sign of a zero
 * sum of the backward ops is not pinned.  Every element of every requested
 * output is written.  The ops run on `stream`, allocate nothing, read nothing
 * back and can be captured in a HIP graph.  PCNN_EINVAL: a NULL required
 * pointer, a stride not in {2,4,8,16}, a non-positive or out-of-domain
 * dimension, misalignment; PCNN_ECAPACITY: a short workspace.  The workspace
 * queries return 0 for dimensions the ops reject.
 * ------------------------------------------------------------------------- */
int pcnn_upscore_fwd(const float* x, int B, int h, int w, int Ch, int stride, const float* bias, int relu, float* y,
                     void* stream);
size_t pcnn_upscore_bwd_workspace_size(int B, int h, int w, int Ch, int stride);
int pcnn_upscore_bwd(const float* d_y, const float* y, int B, int h, int w, int Ch, int stride, float* d_x,
                     float* d_bias, void* workspace, size_t workspace_bytes, void* stream);
int pcnn_upscore_compact_fwd(const float* z, const float* bias, const int32_t* label, int B, int h, int w, int C,
                             int stride, float* vertex3, void* stream);
size_t pcnn_upscore_compact_bwd_workspace_size(int B, int h, int w, int C, int stride);
int pcnn_upscore_compact_bwd(const int32_t* label, const float* d_vertex3, int B, int h, int w, int C, int stride,
                             float* d_z, float* d_bias, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* POSECNN_HIP_H */
