"""numpy restatement of the segmentation and vertex losses of
include/posecnn_hip.h (pcnn_seg_loss, pcnn_cross_entropy, pcnn_vertex_loss),
in two modes from the same float32 inputs:

  "f32"  every per-element op in float32 in the stated order, loss sums in
         float64: the arithmetic the device performs;
  "f64"  everything in float64 (the loss too is left unrounded).

max |f32 - f64| of an output is the error float32 arithmetic itself makes on
that input: the yardstick the GPU tests hold the device to.
"""
import numpy as np

EPS = 1e-10


def _T(mode):
    return {"f32": np.float32, "f64": np.float64}[mode]


def _finish(S, wsum, grad_scale, mode):
    """(loss, inv) from the double sums."""
    if mode == "f32":
        return np.float32(S / (wsum + EPS)), np.float32(grad_scale) / (np.float32(wsum) + np.float32(EPS))
    return np.float64(S / (wsum + EPS)), np.float64(grad_scale) / (np.float64(wsum) + EPS)


def seg_ref(score, gt, threshold, grad_scale=1.0, mode="f32"):
    """score (..., C) float32, gt (...) int -> dict of log_prob,
    prob_normalized, label_2d, gt_label_weight, hard, n, loss, d_score."""
    T = _T(mode)
    x = np.asarray(score, np.float32).astype(T)
    gt = np.asarray(gt)
    C = x.shape[-1]
    m = x.max(axis=-1, keepdims=True)
    d = x - m
    e = np.exp(d)
    s = e[..., 0].copy()
    for c in range(1, C):  # class order, starting from e_0
        s = s + e[..., c]
    assert d.dtype == e.dtype == s.dtype == T
    logs = np.log(s)
    log_prob = d - logs[..., None]
    prob = e / s[..., None]
    label = prob.argmax(axis=-1).astype(np.int32)  # first maximum
    valid = (gt >= 0) & (gt < C)
    hard = valid & ((gt > 0) | (prob[..., 0] < T(np.float32(threshold))))
    onehot = (np.arange(C) == gt[..., None]) & hard[..., None]
    n = int(hard.sum())
    g = np.where(valid, gt, 0)
    lp_gt = np.take_along_axis(log_prob, g[..., None], axis=-1)[..., 0]
    S = float((-lp_gt[hard]).astype(np.float64).sum())
    loss, inv = _finish(S, n, grad_scale, mode)
    d_score = np.where(hard[..., None], (prob - onehot.astype(T)) * inv, T(0))
    assert log_prob.dtype == prob.dtype == d_score.dtype == T
    return dict(log_prob=log_prob, prob_normalized=prob, label_2d=label, gt_label_weight=onehot.astype(np.float32),
                hard=hard, n=n, loss=loss, d_score=d_score)


def cross_entropy_ref(scores, labels, grad_scale=1.0, mode="f32"):
    """(loss, d_scores) of loss_cross_entropy_single_frame."""
    T = _T(mode)
    sc, lb = np.asarray(scores, np.float32).astype(T), np.asarray(labels, np.float32).astype(T)
    S = float((-(lb * sc)).astype(np.float64).sum())
    wsum = float(lb.astype(np.float64).sum())
    loss, inv = _finish(S, wsum, grad_scale, mode)
    return loss, -lb * inv


def smooth_l1_constants(sigma, mode="f32"):
    """(1/sigma^2, sigma^2/2, 0.5/sigma^2, sigma^2) from the float32 sigma, in double, then rounded."""
    T = _T(mode)
    s2 = float(np.float32(sigma)) ** 2
    return T(1.0 / s2), T(s2 / 2.0), T(0.5 / s2), T(s2)


def vertex_ref(pred, tgt, w, sigma=1.0, grad_scale=1.0, mode="f32"):
    """dict of in_loss, near, diff, loss, d_pred of smooth_l1_loss_vertex."""
    T = _T(mode)
    pred, tgt, w = (np.asarray(a, np.float32).astype(T) for a in (pred, tgt, w))
    c_inv, c_half, c_off, c_s2 = smooth_l1_constants(sigma, mode)
    diff = w * (pred - tgt)
    a = np.abs(diff)
    near = a < c_inv
    in_loss = np.where(near, (diff * diff) * c_half, a - c_off)
    S = float(in_loss.astype(np.float64).sum())
    wsum = float(w.astype(np.float64).sum())
    loss, inv = _finish(S, wsum, grad_scale, mode)
    d_pred = (w * np.where(near, diff * c_s2, np.sign(diff))) * inv
    assert in_loss.dtype == d_pred.dtype == T
    return dict(in_loss=in_loss, near=near, diff=diff, loss=loss, d_pred=d_pred)
