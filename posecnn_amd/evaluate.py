"""Scoring of poses and label maps on the device, backed by libposecnn_hip.so
(csrc/pose_eval.hip, include/posecnn_eval.h): what the reference's test driver
ends in, imdb.evaluate_segmentations (lib/datasets/lov.py:518-680) with
lib/utils/pose_error.py and imdb.fast_hist (lib/datasets/imdb.py:123-125).

pose_errors(cls, rt_est, rt_gt, points, num_points, K)  (N, 5) [ADD, ADD-S, re (degrees), te, reproj]
                                                        per (estimate, ground truth) row
pose_tally(errors, cls, symmetry, thresholds, ...)      per-class counts and the accuracy-curve
                                                        histograms, += into int64 tensors
confusion(gt_label, pred_label, num_classes)            hist[gt][pred] += 1, int64
quat_poses_to_rt(poses)                                 (R, 7) [qw qx qy qz tx ty tz] -> (R, 3, 4)
PoseEvaluator(points, num_points, symmetry, extents, K) accumulates a test set from the project's own
                                                        formats (RoIs, poses, the Hough op's gt rows,
                                                        label maps); nothing is read back before summary()

The arithmetic (float32 per point, float64 means in a fixed order) is stated
in the header; tests/pose_eval_ref.py restates all of it in numpy.
"""
import ctypes

import numpy as np
import torch

from . import _lib

_v, _i = ctypes.c_void_p, ctypes.c_int
# include/posecnn_eval.h: name -> (restype, argtypes); v = device pointer or stream
SIGS = {
    "pcnn_eval_abi_version": (_i, []),
    "pcnn_pose_errors_chunk": (_i, []),
    "pcnn_pose_errors_workspace_size": (ctypes.c_size_t, [_i, _i]),
    "pcnn_pose_errors": (_i, [_v, _v, _v, _v, _i, _v, _v, _i, _i, _v, _v, _v, ctypes.c_size_t, _v]),
    "pcnn_pose_tally": (_i, [_v, _v, _v, _i, _v, _v, _i, _v, _i, _v, _v, _v, _v, _v]),
    "pcnn_confusion": (_i, [_v, _v, ctypes.c_long, _i, _v, _v, _v]),
}
_bound = None
I32, I64, F32 = torch.int32, torch.int64, torch.float32


def _load():
    """_lib.load()'s handle with this module's prototypes set on it (once).  A
    library without the entry points is an error: there is no other path."""
    global _bound
    lib = _lib.load()
    if isinstance(lib, ctypes.CDLL) and lib is not _bound:
        for name, (res, args) in SIGS.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:
                raise _lib.PcnnError(f"{_lib.LIB_PATH} has no {name}; rebuild it: __graft_entry__.build()") from None
            fn.restype = res
            fn.argtypes = args
        _bound = lib
    return lib


def _same_device(who, first, **tensors):
    for name, t in tensors.items():
        if t is not None and t.device != first.device:
            raise ValueError(f"{who}: {name}: on {t.device}, expected {first.device}")


def pose_errors(cls, rt_est, rt_gt, points, num_points, K, num_rows=None, out=None, stream=None):
    """errors (N, 5) float32 = [ADD, ADD-S, re in degrees, te, reproj] of the N
    rows (cls[i], rt_est[i], rt_gt[i]); rows that are not scored (at or past
    num_rows, cls outside (0, C), num_points[cls] = 0) hold -1.

    cls (N) int32; rt_est, rt_gt (N, 3, 4) float32 [R | t]; points (C, P, 3)
    float32 with num_points (C) int32 valid points per class (the rest is
    padding and is never read); K (3, 3) float32; num_rows: an optional (1,)
    int32 device counter; out: an (N, 5) float32 tensor to write.  Two
    launches on `stream` (default: the current one), no sync."""
    who = "pose_errors"
    _lib.require(cls, I32, (None,), name=f"{who}: cls")
    N = cls.shape[0]
    _lib.require(rt_est, F32, (N, 3, 4), name=f"{who}: rt_est")
    _lib.require(rt_gt, F32, (N, 3, 4), name=f"{who}: rt_gt")
    _lib.require(points, F32, (None, None, 3), name=f"{who}: points")
    C, P = int(points.shape[0]), int(points.shape[1])
    if C < 1 or P < 1:
        raise ValueError(f"{who}: points: expected at least one class and one point, got shape {tuple(points.shape)}")
    _lib.require(num_points, I32, (C,), name=f"{who}: num_points")
    _lib.require(K, F32, (3, 3), name=f"{who}: K")
    _lib.require_counter(num_rows, f"{who}: num_rows")
    if out is None:
        out = torch.empty((N, 5), dtype=F32, device=cls.device)
    _lib.require(out, F32, (N, 5), name=f"{who}: out")
    _same_device(who, cls, rt_est=rt_est, rt_gt=rt_gt, points=points, num_points=num_points, K=K, num_rows=num_rows,
                 out=out)
    lib = _load()
    need = lib.pcnn_pose_errors_workspace_size(N, P)
    ws = _lib.workspace(need, cls.device, tag="pose_eval", stream=stream)
    rc = lib.pcnn_pose_errors(_lib.ptr(cls), _lib.ptr(rt_est), _lib.ptr(rt_gt), _lib.ptr(num_rows), N,
                              _lib.ptr(points), _lib.ptr(num_points), C, P, _lib.ptr(K), _lib.ptr(out), _lib.ptr(ws),
                              need, _lib.stream_ptr(stream))
    _lib.check(rc, who)
    return out


def pose_tally(errors, cls, symmetry, thresholds, curve_thr, scored, correct, first_add, first_adds, num_rows=None,
               stream=None):
    """Add the rows of `errors` (N, 5) that pose_errors scored to the per-class
    int64 counts: scored (C), correct (C) -- the metric (ADD-S where
    symmetry[c] > 0, else ADD) strictly below thresholds[c] -- and first_add,
    first_adds (C, T + 1), the histograms of the first t with error <
    curve_thr[t] (slot T: none).  symmetry, thresholds (C) and curve_thr (T,
    ascending) are float32.  One launch, exact, no sync."""
    who = "pose_tally"
    _lib.require(errors, F32, (None, 5), name=f"{who}: errors")
    N = errors.shape[0]
    _lib.require(cls, I32, (N,), name=f"{who}: cls")
    _lib.require(symmetry, F32, (None,), name=f"{who}: symmetry")
    C = int(symmetry.shape[0])
    if C < 1:
        raise ValueError(f"{who}: symmetry: expected at least one class")
    _lib.require(thresholds, F32, (C,), name=f"{who}: thresholds")
    _lib.require(curve_thr, F32, (None,), name=f"{who}: curve_thr")
    T = int(curve_thr.shape[0])
    _lib.require(scored, I64, (C,), name=f"{who}: scored")
    _lib.require(correct, I64, (C,), name=f"{who}: correct")
    _lib.require(first_add, I64, (C, T + 1), name=f"{who}: first_add")
    _lib.require(first_adds, I64, (C, T + 1), name=f"{who}: first_adds")
    _lib.require_counter(num_rows, f"{who}: num_rows")
    _same_device(who, errors, cls=cls, symmetry=symmetry, thresholds=thresholds, curve_thr=curve_thr, scored=scored,
                 correct=correct, first_add=first_add, first_adds=first_adds, num_rows=num_rows)
    rc = _load().pcnn_pose_tally(_lib.ptr(errors), _lib.ptr(cls), _lib.ptr(num_rows), N, _lib.ptr(symmetry),
                                 _lib.ptr(thresholds), C, _lib.ptr(curve_thr), T, _lib.ptr(scored), _lib.ptr(correct),
                                 _lib.ptr(first_add), _lib.ptr(first_adds), _lib.stream_ptr(stream))
    _lib.check(rc, who)


def confusion(gt_label, pred_label, num_classes, hist=None, skipped=None, stream=None):
    """hist[gt][pred] += 1 over the pixels of two int32 label maps of the same
    shape (any number of dimensions, contiguous): the reference's fast_hist.
    A pixel counts when 0 <= gt < num_classes; a counted pixel whose pred is
    outside [0, num_classes) is not binned and adds 1 to skipped (the
    reference's bincount would spill it into a neighbouring row).  hist
    (C, C) and skipped (1,) are int64 and are created zeroed if not given.
    Returns (hist, skipped).  One launch, exact, no sync."""
    who = "confusion"
    _lib.require(gt_label, I32, name=f"{who}: gt_label")
    _lib.require(pred_label, I32, tuple(gt_label.shape), name=f"{who}: pred_label")
    C = int(num_classes)
    if C < 1:
        raise ValueError(f"{who}: num_classes: expected at least 1, got {num_classes}")
    if hist is None:
        hist = torch.zeros((C, C), dtype=I64, device=gt_label.device)
    if skipped is None:
        skipped = torch.zeros((1,), dtype=I64, device=gt_label.device)
    _lib.require(hist, I64, (C, C), name=f"{who}: hist")
    _lib.require(skipped, I64, (1,), name=f"{who}: skipped")
    _same_device(who, gt_label, pred_label=pred_label, hist=hist, skipped=skipped)
    rc = _load().pcnn_confusion(_lib.ptr(gt_label), _lib.ptr(pred_label), gt_label.numel(), C, _lib.ptr(hist),
                                _lib.ptr(skipped), _lib.stream_ptr(stream))
    _lib.check(rc, who)
    return hist, skipped


def quat_poses_to_rt(poses):
    """(R, 7) [qw qx qy qz tx ty tz] (any float dtype) -> (R, 3, 4) float32
    [R | t] on the same device: the quaternion is normalised and turned into a
    matrix in float64 and rounded to float32 once, as the reference's
    RT[:3, :3] = quat2mat(...) into a float32 array does.  (A zero quaternion
    -- a padding row -- gives NaN; such a row has no class and is not read.)"""
    if not isinstance(poses, torch.Tensor) or poses.dim() != 2 or poses.shape[1] != 7:
        raise ValueError("quat_poses_to_rt: poses: expected an (R, 7) tensor")
    p = poses.to(torch.float64)
    w, x, y, z = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    n = torch.sqrt(((w * w + x * x) + y * y) + z * z)
    w, x, y, z = w / n, x / n, y / n, z / n
    rt = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), p[:, 4],
                      2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w), p[:, 5],
                      2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y), p[:, 6]], dim=1)
    return rt.to(F32).reshape(-1, 3, 4).contiguous()


def segmentation_scores(hist):
    """The figures of lov.py:645-658 from a (C, C) confusion matrix: overall
    accuracy, per-class and mean accuracy, per-class and mean IU (nanmean, as
    the reference) and the frequency-weighted IU."""
    hist = np.asarray(hist, np.float64)
    diag = np.diag(hist)
    with np.errstate(divide="ignore", invalid="ignore"):
        overall = diag.sum() / hist.sum()
        acc = diag / hist.sum(1)
        iu = diag / (hist.sum(1) + hist.sum(0) - diag)
        freq = hist.sum(1) / hist.sum()
        seen = freq > 0
        return dict(overall_accuracy=overall, class_accuracy=acc,
                    mean_accuracy=np.nanmean(acc) if np.isfinite(acc).any() else np.nan, iu=iu,
                    mean_iu=np.nanmean(iu) if np.isfinite(iu).any() else np.nan,
                    fwavacc=(freq[seen] * iu[seen]).sum() if hist.sum() > 0 else np.nan)


def pose_scores(count_all, scored, correct, first_add, first_adds):
    """The pose figures of summary() from the accumulated counts."""
    count_all = np.asarray(count_all, np.int64)
    T = first_add.shape[1] - 1
    with np.errstate(divide="ignore", invalid="ignore"):
        den = count_all.astype(np.float64)
        out = dict(count_all=count_all, count_scored=np.asarray(scored, np.int64),
                   count_correct=np.asarray(correct, np.int64), accuracy=np.asarray(correct, np.float64) / den)
        for name, first in (("add", first_add), ("adds", first_adds)):
            curve = np.cumsum(np.asarray(first, np.int64)[:, :T], axis=1) / den[:, None]
            out[f"{name}_curve"] = curve
            out[f"{name}_auc"] = curve.mean(axis=1) if T else np.full(len(den), np.nan)
    return out


class PoseEvaluator:
    """Accumulates the reference's evaluation of ONE pose set over a test set,
    on the device (make one evaluator each for poses, poses_refined and
    poses_icp).

    points (C, P, 3) float32 and num_points (C) int32, symmetry (C) float32
    (> 0: scored by ADD-S), extents (C, 3), K (3, 3) float32: device tensors
    (extents may be a host array: the thresholds 0.1 |extents[c]| are computed
    in float32 on the host, once).  curve_max, curve_bins: the accuracy
    curves' thresholds (t + 1) curve_max / curve_bins, t < curve_bins.

    All accumulators are int64 device tensors (count_all, scored, correct,
    first_add, first_adds, hist, skipped): a sharded run can all-reduce them
    before summary()."""

    def __init__(self, points, num_points, symmetry, extents, K, curve_max=0.1, curve_bins=1000):
        who = "PoseEvaluator"
        _lib.require(points, F32, (None, None, 3), name=f"{who}: points")
        C = self.C = int(points.shape[0])
        _lib.require(num_points, I32, (C,), name=f"{who}: num_points")
        _lib.require(symmetry, F32, (C,), name=f"{who}: symmetry")
        _lib.require(K, F32, (3, 3), name=f"{who}: K")
        if curve_bins < 0 or not curve_max > 0:
            raise ValueError(f"{who}: curve_max > 0 and curve_bins >= 0")
        dev = self.device = points.device
        self.points, self.num_points, self.symmetry, self.K = points, num_points, symmetry, K
        ext = extents.detach().cpu().numpy() if isinstance(extents, torch.Tensor) else np.asarray(extents)
        ext = np.asarray(ext, np.float32)
        if ext.shape != (C, 3):
            raise ValueError(f"{who}: extents: expected shape {(C, 3)}, got {ext.shape}")
        thr = np.zeros(C, np.float32)
        for c in range(C):  # lov.py:539-541
            thr[c] = 0.1 * np.linalg.norm(ext[c, :])
        T = self.T = int(curve_bins)
        curve = ((np.arange(T, dtype=np.float64) + 1.0) * float(curve_max) / max(T, 1)).astype(np.float32)
        self.thresholds = torch.from_numpy(thr).to(dev)
        self.curve_thr = torch.from_numpy(curve).to(dev)
        z = lambda *s: torch.zeros(s, dtype=I64, device=dev)  # noqa: E731
        self.count_all, self.scored, self.correct = z(C), z(C), z(C)
        self.first_add, self.first_adds = z(C, T + 1), z(C, T + 1)
        self.hist, self.skipped = z(C, C), z(1)

    def update(self, rois, poses, gt, num_rois=None, stream=None):
        """Score the poses of one batch.  rois (cap, 7) [b, cls, ...] and
        poses (cap, 7) [qw qx qy qz tx ty tz] as the Hough op emits them, gt
        (num_gt, 13) [b, cls, 0, 0, 0, 0, qw .. tz] as it takes them, num_rois
        an optional (1,) int32 device counter of the valid RoIs.  Every RoI of
        a ground truth's class in its image is scored against it
        (lov.py:582-607): row k num_gt + j of the pairing carries the class
        when RoI k and ground truth j share image and class and the class is
        > 0, else -1.  Every ground truth of a class in (0, C) counts in
        count_all.  Returns the (cap num_gt, 5) errors; nothing is read back."""
        who = "PoseEvaluator.update"
        _lib.require(rois, F32, (None, 7), name=f"{who}: rois")
        cap = rois.shape[0]
        _lib.require(poses, F32, (cap, 7), name=f"{who}: poses")
        _lib.require(gt, F32, (None, 13), name=f"{who}: gt")
        _lib.require_counter(num_rois, f"{who}: num_rois")
        G = gt.shape[0]
        if stream is not None:
            with torch.cuda.stream(stream):
                return self._update(rois, poses, gt, num_rois, cap, G, stream)
        return self._update(rois, poses, gt, num_rois, cap, G, None)

    def _update(self, rois, poses, gt, num_rois, cap, G, stream):
        gcls = gt[:, 1].to(I64)
        counted = (gcls > 0) & (gcls < self.C)
        self.count_all.index_add_(0, gcls.clamp(0, self.C - 1), counted.to(I64))
        if cap == 0 or G == 0:
            return torch.empty((0, 5), dtype=F32, device=self.device)
        rcls = rois[:, 1].to(I32)
        match = (rois[:, 0:1] == gt[None, :, 0]) & (rois[:, 1:2] == gt[None, :, 1]) & (rcls[:, None] > 0)
        if num_rois is not None:
            match &= (torch.arange(cap, device=self.device) < num_rois[0])[:, None]
        cls = torch.where(match, rcls[:, None], torch.full_like(rcls[:, None], -1)).reshape(-1).contiguous()
        rt_est = quat_poses_to_rt(poses)[:, None].expand(cap, G, 3, 4).reshape(cap * G, 3, 4)
        rt_gt = quat_poses_to_rt(gt[:, 6:13])[None].expand(cap, G, 3, 4).reshape(cap * G, 3, 4)
        errors = pose_errors(cls, rt_est, rt_gt, self.points, self.num_points, self.K, stream=stream)
        pose_tally(errors, cls, self.symmetry, self.thresholds, self.curve_thr, self.scored, self.correct,
                   self.first_add, self.first_adds, stream=stream)
        return errors

    def update_segmentation(self, gt_label, pred_label, stream=None):
        """Add two int32 label maps of the same shape to the confusion matrix."""
        confusion(gt_label, pred_label, self.C, self.hist, self.skipped, stream=stream)

    def summary(self):
        """Plain numpy (this reads the device): per class count_all (ground
        truths), count_scored (scored pairs), count_correct and accuracy =
        count_correct / count_all (lov.py:675; NaN where count_all is 0);
        add_curve, adds_curve (C, T): the fraction of count_all whose error is
        below (t + 1) curve_max / T (the cumulative first_* histograms), and
        add_auc, adds_auc (C): the mean of the curve over the T thresholds,
        the YCB-Video toolbox's area-under-curve convention -- the toolbox is
        not part of the reference, so this figure is unpinned; curve_thr; and
        hist, skipped, overall_accuracy, class_accuracy, mean_accuracy, iu,
        mean_iu and fwavacc by the expressions of lov.py:645-658."""
        h = lambda t: t.cpu().numpy()  # noqa: E731
        out = pose_scores(h(self.count_all), h(self.scored), h(self.correct), h(self.first_add), h(self.first_adds))
        out["curve_thr"] = h(self.curve_thr)
        out["thresholds"] = h(self.thresholds)
        out["hist"], out["skipped"] = h(self.hist), int(h(self.skipped)[0])
        out.update(segmentation_scores(out["hist"]))
        return out
