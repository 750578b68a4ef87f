/*
 * posecnn_eval.h — C-ABI of the EVALUATION side in libposecnn_hip.so: the pose
 * errors ADD, ADD-S, re, te and reproj of (estimate, ground truth) pairs, their
 * per-class tally, and the confusion matrix of two label maps
 * (csrc/pose_eval.hip).  A companion of posecnn_hip.h (same library, same
 * conventions and error codes); pcnn_eval_abi_version() versions these entry
 * points on their own, pcnn_abi_version() does not change with them.
 *
 * Conventions (those of posecnn_hip.h)
 *  - every pointer is a DEVICE pointer unless the name ends in _host;
 *  - `stream` is a hipStream_t passed as void* (NULL = legacy default stream);
 *  - nothing allocates: temporaries live in a caller-provided `workspace` whose
 *    size the matching *_workspace_size() query returns;
 *  - nothing synchronises and nothing is read back: every op can be captured in
 *    a hipGraph, and the counts accumulate on the device;
 *  - return value 0 = PCNN_OK, otherwise a PCNN_E* code (never exit()).
 */
#ifndef POSECNN_EVAL_H
#define POSECNN_EVAL_H

#include <stddef.h>
#include <stdint.h>

#include "posecnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: pcnn_pose_errors_chunk, pcnn_pose_errors_workspace_size, pcnn_pose_errors,
 *    pcnn_pose_tally, pcnn_confusion */
int pcnn_eval_abi_version(void);

/* ---------------------------------------------------------------------------
 * Pose errors: the reference's lib/utils/pose_error.py add, adi, re, te and
 * reproj (as lib/datasets/lov.py:582-607 calls them), one scored row per
 * (estimate, ground truth) pair.
 *
 *  cls        (N_cap) int32       class of each row
 *  rt_est, rt_gt (N_cap,3,4) f32  estimated and ground-truth [R | t], row major
 *  num_rows_dev (1) int32 or NULL number of rows (clamped to [0, N_cap]); NULL: N_cap
 *  points     (C,P,3) f32         model points; entries past num_points[c] are
 *                                 padding and are never read
 *  num_points (C) int32           valid points per class (clamped to P)
 *  K          (3,3) f32           intrinsics, row major
 *  errors     (N_cap,5) f32       out: [ADD, ADD-S, re in degrees, te, reproj]
 *
 * A row is scored when it is below the row count and has 0 < cls < C and
 * num_points[cls] > 0; it gets all five values.  Every other row of the N_cap
 * gets -1 in all five columns.  Memory beyond N_cap rows is not touched.
 *
 * Arithmetic: float32, every operation rounded separately (no FMA), so that
 * numpy restates it bit for bit (tests/pose_eval_ref.py).  With n =
 * num_points[cls] and p_i = (x, y, z) the class's points, i < n:
 *  - a transformed point, per coordinate and for both poses,
 *        X = ((r0 x + r1 y) + r2 z) + t;
 *  - a squared distance d2(a, b) = (dx dx + dy dy) + dz dz;
 *  - ADD   = mean_i sqrtf(d2(est_i, gt_i));
 *  - ADD-S = mean_i sqrtf(min_j d2(gt_i, est_j)), pose_error.adi's direction:
 *    for every ground-truth-transformed point the nearest estimate-transformed
 *    point (the minimum of float32 values does not depend on the scan order);
 *  - reproj = mean_i sqrtf(du du + dv dv), du = u_est - u_gt, dv likewise, with
 *        u = ((k00 X + k01 Y) + k02 Z) / ((k20 X + k21 Y) + k22 Z)
 *        v = ((k10 X + k11 Y) + k12 Z) / ((k20 X + k21 Y) + k22 Z)
 *    (correctly rounded divisions and square roots);
 *  - the three means in float64, in a fixed order (no atomics: two runs give
 *    the same bits).  A chunk is pcnn_pose_errors_chunk() = 256 consecutive
 *    points, one per thread of a 256-thread block; a point past n counts 0.
 *    The 64 lanes of a wave add their widened values as a butterfly,
 *    v += v[lane ^ o] for o = 32, 16, 8, 4, 2, 1; the four waves' sums as
 *    ((s0 + s1) + s2) + s3; the row's ceil(n / 256) chunk sums are added to 0
 *    in index order; mean = (float)(sum / (double)n), rounded once;
 *  - te = (float)sqrt((dx dx + dy dy) + dz dz), d = (double)t_est - (double)t_gt;
 *  - re = (float)((acos(c) * 180.0) / pi), c = 0.5 (tr - 1) clamped to [-1, 1],
 *    tr = the sum over the nine entries, row major, added to 0 in float64, of
 *    (double)R_est[i][j] (double)R_gt[i][j] = trace(R_est R_gt^T).  The device's
 *    acos may differ from the host libm's in its last bit.
 *    NARROWING: the reference evaluates trace(R_est inv(R_gt)); the transpose
 *    stands in for the inverse here.  The two agree when R_gt is a rotation.
 *
 * Two launches: (row, chunk) blocks that stage the estimate-transformed
 * candidates in LDS (whole up to 8192 points, in tiles of 8192 above) and scan
 * them for 256 query points, then one thread per row that folds the chunk sums
 * and computes re and te.
 *
 * workspace: pcnn_pose_errors_workspace_size(N_cap, P) bytes, 8-byte aligned.
 * PCNN_EINVAL: N_cap < 0, C < 1, P < 1, N_cap * ceil(P / 256) >= 2^31, a NULL
 * cls, rt_est, rt_gt, points, num_points, K, errors or workspace with
 * N_cap > 0, a workspace that is too small or misaligned.  N_cap = 0 launches
 * nothing.
 * ------------------------------------------------------------------------- */
int pcnn_pose_errors_chunk(void);
size_t pcnn_pose_errors_workspace_size(int N_cap, int P);
int pcnn_pose_errors(const int32_t* cls, const float* rt_est, const float* rt_gt, const int32_t* num_rows_dev,
                     int N_cap, const float* points, const int32_t* num_points, int C, int P, const float* K,
                     float* errors, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Tally of a block of scored rows (lov.py:582-607's bookkeeping), accumulated
 * into caller-owned int64 tensors, so a whole test set sums up on the device.
 *
 *  errors     (N_cap,5) f32   as pcnn_pose_errors wrote them
 *  cls        (N_cap) int32
 *  num_rows_dev (1) int32 or NULL
 *  symmetry   (C) f32         > 0: the class is scored by ADD-S, else by ADD
 *  thresholds (C) f32         the class's bound (0.1 |extents| in the reference)
 *  curve_thr  (T) f32         ascending thresholds of the accuracy curves
 *  scored, correct (C) int64          +=
 *  first_add, first_adds (C,T+1) int64  +=
 *
 * A row counts when it is below the row count, has 0 < cls < C and its ADD is
 * >= 0 (the rows pcnn_pose_errors did not score hold -1).  For such a row of
 * class c: scored[c] += 1; correct[c] += 1 if its metric < thresholds[c]
 * (strict, lov.py:606); first_add[c][t] += 1 for the first t with
 * ADD < curve_thr[t], t = T if there is none; first_adds likewise with ADD-S.
 * Comparisons and integer atomics only: exact, and independent of the order.
 * PCNN_EINVAL: N_cap < 0, C < 1, T < 0, a NULL errors, cls, symmetry,
 * thresholds, scored, correct, first_add or first_adds with N_cap > 0, a NULL
 * curve_thr with T > 0.
 * ------------------------------------------------------------------------- */
int pcnn_pose_tally(const float* errors, const int32_t* cls, const int32_t* num_rows_dev, int N_cap,
                    const float* symmetry, const float* thresholds, int C, const float* curve_thr, int T,
                    int64_t* scored, int64_t* correct, int64_t* first_add, int64_t* first_adds, void* stream);

/* ---------------------------------------------------------------------------
 * Confusion matrix: the reference's imdb.fast_hist (lib/datasets/imdb.py:
 * 123-125), hist[gt][pred] += 1 over n pixels.
 *
 *  gt, pred (n) int32     4-byte aligned; int4 loads where both reach 16-byte
 *                         alignment after the same number (< 4) of elements
 *  hist     (C,C) int64   +=
 *  skipped  (1) int64     +=
 *
 * A pixel counts when 0 <= gt < C.  NARROWING: a counted pixel whose pred lies
 * outside [0, C) is not binned and adds 1 to skipped; the reference's
 * bincount(C * gt + pred) would spill it into a neighbouring row.
 * The lanes of a wave that hold the same (gt, pred) add once, by their count.
 * With C <= 128 a block counts in a C x C int32 table in LDS and adds it to
 * hist once; above, every wave adds to hist directly.  Exact.
 * PCNN_EINVAL: n < 0 or n >= 2^31, C < 1 or C > 32768, a NULL gt, pred, hist
 * or skipped with n > 0.  n = 0 launches nothing.
 * ------------------------------------------------------------------------- */
int pcnn_confusion(const int32_t* gt, const int32_t* pred, long n, int C, int64_t* hist, int64_t* skipped,
                   void* stream);

#ifdef __cplusplus
}
#endif

#endif /* POSECNN_EVAL_H */
