"""numpy restatement of the evaluation ops (include/posecnn_eval.h,
csrc/pose_eval.hip, posecnn_amd/evaluate.py) -- the specification the GPU
tests compare with, bit for bit: the float32 per-point arithmetic with every
operation rounded separately, the device's float64 summation order, the tally
and the confusion matrix (np.bincount).  pose_errors64 is a second, float64
form of the five errors written from the formulas (ADD-S by
scipy.spatial.cKDTree): the measure of what the float32 order costs."""
import numpy as np

F = np.float32
CHUNK = 256  # pcnn_pose_errors_chunk(): points per block, one per thread
WAVE = 64


def xform32(rt, pts):
    """((r0 x + r1 y) + r2 z) + t per coordinate, float32; rt (3, 4), pts (n, 3) -> (n, 3)."""
    rt, pts = np.asarray(rt, F), np.asarray(pts, F)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    return np.stack([((rt[i, 0] * x + rt[i, 1] * y) + rt[i, 2] * z) + rt[i, 3] for i in range(3)], axis=1)


def dist2_32(a, b):
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def project32(K, p):
    K = np.asarray(K, F)
    X, Y, Z = p[:, 0], p[:, 1], p[:, 2]
    w = (K[2, 0] * X + K[2, 1] * Y) + K[2, 2] * Z
    return ((K[0, 0] * X + K[0, 1] * Y) + K[0, 2] * Z) / w, ((K[1, 0] * X + K[1, 1] * Y) + K[1, 2] * Z) / w


def nearest2_32(queries, cands):
    """min_j d2(queries[i], cands[j]) in float32 (the minimum does not depend on the order)."""
    out = np.empty(len(queries), F)
    for i0 in range(0, len(queries), CHUNK):
        q = queries[i0:i0 + CHUNK]
        out[i0:i0 + len(q)] = dist2_32(q[:, None, :], cands[None, :, :]).min(axis=1)
    return out


def mean64(values):
    """The device's mean of n float32 values: chunks of 256, one value per
    thread (0 past n), widened; per wave the butterfly v += v[lane ^ o], o =
    32 .. 1; the four waves ((s0 + s1) + s2) + s3; the chunks added to 0 in
    order; divided by n in float64 and rounded to float32 once."""
    values = np.asarray(values, F)
    n = len(values)
    nch = (n + CHUNK - 1) // CHUNK
    v = np.zeros(nch * CHUNK, np.float64)
    v[:n] = values
    v = v.reshape(nch, CHUNK // WAVE, WAVE)
    lanes = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lanes ^ o]
    w = v[:, :, 0]
    total = np.float64(0.0)
    for ch in range(nch):
        total = total + (((w[ch, 0] + w[ch, 1]) + w[ch, 2]) + w[ch, 3])
    return F(total / np.float64(n))


def re_te(rt_est, rt_gt):
    e, g = np.asarray(rt_est, F).astype(np.float64), np.asarray(rt_gt, F).astype(np.float64)
    tr = np.float64(0.0)
    for i in range(3):
        for j in range(3):
            tr = tr + e[i, j] * g[i, j]
    c = min(1.0, max(-1.0, 0.5 * (tr - 1.0)))
    d = e[:, 3] - g[:, 3]
    return F((np.arccos(c) * 180.0) / np.pi), F(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))


def pose_errors_row(rt_est, rt_gt, pts, K):
    """[ADD, ADD-S, re, te, reproj] of one row over the valid points pts (n, 3), n >= 1."""
    est, gt = xform32(rt_est, pts), xform32(rt_gt, pts)
    add = mean64(np.sqrt(dist2_32(est, gt)))
    adds = mean64(np.sqrt(nearest2_32(gt, est)))
    ue, ve = project32(K, est)
    ug, vg = project32(K, gt)
    du, dv = ue - ug, ve - vg
    rep = mean64(np.sqrt(du * du + dv * dv))
    re, te = re_te(rt_est, rt_gt)
    return np.array([add, adds, re, te, rep], F)


def pose_errors(cls, rt_est, rt_gt, points, num_points, K, num_rows=None):
    """(N, 5) float32; rows that are not scored hold -1.  Padding of `points` is never read."""
    cls = np.asarray(cls)
    N, (C, P, _) = len(cls), points.shape
    rows = N if num_rows is None else max(0, min(int(num_rows), N))
    out = np.full((N, 5), -1, F)
    for i in range(rows):
        c = int(cls[i])
        if not 0 < c < C:
            continue
        n = min(int(num_points[c]), P)
        if n > 0:
            out[i] = pose_errors_row(rt_est[i], rt_gt[i], points[c, :n], K)
    return out


def pose_errors64(rt_est, rt_gt, pts, K):
    """The five errors in float64 from the formulas (ADD-S by a kd-tree):
    mean |est_i - gt_i|; mean over the gt points of the distance to the
    nearest est point; the angle of R_est R_gt^T in degrees; |t_est - t_gt|;
    mean pixel distance of the projections."""
    from scipy.spatial import cKDTree
    e, g, K = np.asarray(rt_est, np.float64), np.asarray(rt_gt, np.float64), np.asarray(K, np.float64)
    pts = np.asarray(pts, np.float64)
    est, gt = pts @ e[:, :3].T + e[:, 3], pts @ g[:, :3].T + g[:, 3]
    add = np.linalg.norm(est - gt, axis=1).mean()
    adds = cKDTree(est).query(gt, k=1)[0].mean()
    c = np.clip(0.5 * (np.trace(e[:, :3] @ g[:, :3].T) - 1.0), -1.0, 1.0)
    pe, pg = est @ K.T, gt @ K.T
    rep = np.linalg.norm(pe[:, :2] / pe[:, 2:] - pg[:, :2] / pg[:, 2:], axis=1).mean()
    return np.array([add, adds, np.degrees(np.arccos(c)), np.linalg.norm(e[:, 3] - g[:, 3]), rep])


def tally(errors, cls, symmetry, thresholds, curve_thr, num_rows=None, into=None):
    """(scored, correct, first_add, first_adds), int64; `into`: the same four to add to."""
    errors, cls = np.asarray(errors, F), np.asarray(cls)
    C, T = len(symmetry), len(curve_thr)
    curve_thr = np.asarray(curve_thr, F)
    scored, correct, first_add, first_adds = into if into is not None else (
        np.zeros(C, np.int64), np.zeros(C, np.int64), np.zeros((C, T + 1), np.int64), np.zeros((C, T + 1), np.int64))
    rows = len(cls) if num_rows is None else max(0, min(int(num_rows), len(cls)))
    for i in range(rows):
        c = int(cls[i])
        if not 0 < c < C or not errors[i, 0] >= 0:
            continue
        scored[c] += 1
        metric = errors[i, 1] if symmetry[c] > 0 else errors[i, 0]
        correct[c] += bool(metric < F(thresholds[c]))
        # thresholds ascend: the first t with err < thr[t] is the number of thr[t] <= err
        first_add[c, np.searchsorted(curve_thr, errors[i, 0], side="right")] += 1
        first_adds[c, np.searchsorted(curve_thr, errors[i, 1], side="right")] += 1
    return scored, correct, first_add, first_adds


def confusion(gt, pred, C):
    """(hist (C, C) int64, skipped): fast_hist's bincount over the pixels with
    0 <= gt < C, with the pixels whose pred is out of range counted apart."""
    gt, pred = np.asarray(gt).ravel().astype(np.int64), np.asarray(pred).ravel().astype(np.int64)
    k = (gt >= 0) & (gt < C)
    inr = (pred >= 0) & (pred < C)
    hist = np.bincount(C * gt[k & inr] + pred[k & inr], minlength=C * C).reshape(C, C).astype(np.int64)
    return hist, int((k & ~inr).sum())


def quat_poses_to_rt(poses):
    """(R, 7) [qw qx qy qz tx ty tz] -> (R, 3, 4) float32, in float64 and rounded once."""
    p = np.asarray(poses).astype(np.float64)
    w, x, y, z = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.sqrt(((w * w + x * x) + y * y) + z * z)
        w, x, y, z = w / n, x / n, y / n, z / n
    rt = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), p[:, 4],
                   2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w), p[:, 5],
                   2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y), p[:, 6]], axis=1)
    return rt.astype(F).reshape(-1, 3, 4)


class Evaluator:
    """posecnn_amd.evaluate.PoseEvaluator on the host, pair by pair."""

    def __init__(self, points, num_points, symmetry, extents, K, curve_max=0.1, curve_bins=1000):
        self.points, self.num_points, self.symmetry, self.K = points, num_points, symmetry, np.asarray(K, F)
        C, T = len(points), int(curve_bins)
        self.C, self.T = C, T
        self.thresholds = np.array([0.1 * np.linalg.norm(np.asarray(extents, F)[c]) for c in range(C)], F)
        self.curve_thr = ((np.arange(T, dtype=np.float64) + 1.0) * float(curve_max) / max(T, 1)).astype(F)
        self.count_all = np.zeros(C, np.int64)
        self.counts = tally(np.zeros((0, 5), F), [], symmetry, self.thresholds, self.curve_thr)
        self.hist, self.skipped = np.zeros((C, C), np.int64), 0

    def update(self, rois, poses, gt, num_rois=None):
        rois, poses, gt = np.asarray(rois, F), np.asarray(poses, F), np.asarray(gt, F)
        R = len(rois) if num_rois is None else int(num_rois)
        est, ref = quat_poses_to_rt(poses), quat_poses_to_rt(gt[:, 6:13])
        for j in range(len(gt)):
            c = int(gt[j, 1])
            if not 0 < c < self.C:
                continue
            self.count_all[c] += 1
            for k in range(R):
                if int(rois[k, 1]) == c and rois[k, 0] == gt[j, 0]:
                    e = pose_errors([c], est[k:k + 1], ref[j:j + 1], self.points, self.num_points, self.K)
                    tally(e, [c], self.symmetry, self.thresholds, self.curve_thr, into=self.counts)

    def update_segmentation(self, gt_label, pred_label):
        h, s = confusion(gt_label, pred_label, self.C)
        self.hist += h
        self.skipped += s

    def summary(self):
        scored, correct, first_add, first_adds = self.counts
        T = self.T
        hist = self.hist.astype(np.float64)
        diag = np.diag(hist)
        with np.errstate(divide="ignore", invalid="ignore"):
            den = self.count_all.astype(np.float64)
            out = dict(count_all=self.count_all, count_scored=scored, count_correct=correct, accuracy=correct / den,
                       add_curve=np.cumsum(first_add[:, :T], axis=1) / den[:, None],
                       adds_curve=np.cumsum(first_adds[:, :T], axis=1) / den[:, None],
                       curve_thr=self.curve_thr, thresholds=self.thresholds, hist=self.hist, skipped=self.skipped)
            out["add_auc"] = out["add_curve"].mean(axis=1) if T else np.full(self.C, np.nan)
            out["adds_auc"] = out["adds_curve"].mean(axis=1) if T else np.full(self.C, np.nan)
            acc = diag / hist.sum(1)
            iu = diag / (hist.sum(1) + hist.sum(0) - diag)
            freq = hist.sum(1) / hist.sum()
            out.update(overall_accuracy=diag.sum() / hist.sum(), class_accuracy=acc,
                       mean_accuracy=np.nanmean(acc) if np.isfinite(acc).any() else np.nan, iu=iu,
                       mean_iu=np.nanmean(iu) if np.isfinite(iu).any() else np.nan,
                       fwavacc=(freq[freq > 0] * iu[freq > 0]).sum() if hist.sum() > 0 else np.nan)
        return out
