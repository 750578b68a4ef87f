"""The segmentation and vertex-regression terms of the training objective
(lib/fcn/train.py:489-515: loss_cls and loss_vertex), forward and backward, on
the HIP ops of csrc/seg_loss.hip.

Reference names (same argument order and meaning):
    loss_cross_entropy_single_frame(scores, labels)            train.py:455-465
    smooth_l1_loss_vertex(vertex_pred, vertex_targets, vertex_weights, sigma=1.0)   train.py:565-574
    softmax_high_dimension / log_softmax_high_dimension        network.py:475-506
Fused forms:
    seg_loss(score, gt_label_2d, threshold, want=..., grad_scale=1.0)
        log-softmax, softmax, argmax_2d, Hardlabel, the loss and d loss / d score
        in two passes over the score map.
    vertex_loss_compact(vertex_pred, label, vertex3, num_classes, w_inside, sigma=1.0)
        smooth_l1_loss_vertex on the blobs synthesize.scene.expand would write,
        without writing them.
Losses come back as 0-d device tensors; nothing here synchronises.
"""
import torch

from . import _lib

SEG_OUTPUTS = ("log_prob", "prob_normalized", "label_2d", "gt_label_weight", "d_score")


def _scalar(device):
    return torch.empty(1, dtype=torch.float32, device=device)


def _map4(x, what):
    if x.dim() != 4:
        raise ValueError(f"{what} must be 4-dimensional (B,H,W,C), got {tuple(x.shape)}")
    return x.contiguous().float()


def seg_loss(score, gt_label_2d, threshold, *, want=("label_2d",), grad_scale=1.0, stream=None):
    """score (B,H,W,C), gt_label_2d (B,H,W) -> (loss, {name: tensor for name in
    want}); names from SEG_OUTPUTS.  The pixel set of the loss is Hardlabel's:
    gt > 0, or gt == 0 with prob_normalized[0] < threshold (include/posecnn_hip.h)."""
    _lib.require_gpu(score, gt_label_2d)
    if float(threshold) <= 0:
        raise ValueError(f"Need threshold > 0, got {threshold}")
    unknown = [w for w in want if w not in SEG_OUTPUTS]
    if unknown:
        raise ValueError(f"unknown outputs {unknown}; choose from {SEG_OUTPUTS}")
    score = _map4(score, "score")
    B, H, W, C = score.shape
    if tuple(gt_label_2d.shape) != (B, H, W):
        raise ValueError(f"gt shape {tuple(gt_label_2d.shape)} does not match score {tuple(score.shape)}")
    gt = gt_label_2d.contiguous().to(torch.int32)
    dev = score.device
    out = {w: torch.empty((B, H, W) if w == "label_2d" else (B, H, W, C),
                          dtype=torch.int32 if w == "label_2d" else torch.float32, device=dev) for w in want}
    loss = _scalar(dev)
    lib = _lib.load()
    need = lib.pcnn_seg_loss_workspace_size(B, H, W, C)
    if need == 0:
        raise ValueError(f"seg_loss: unsupported shape {tuple(score.shape)}")
    ws = _lib.workspace(need, dev, "seg_loss", stream)
    rc = lib.pcnn_seg_loss(_lib.ptr(score), _lib.ptr(gt), B, H, W, C, float(threshold), float(grad_scale),
                           *[_lib.ptr(out.get(w)) for w in SEG_OUTPUTS], _lib.ptr(loss), _lib.ptr(ws), ws.numel(),
                           _lib.stream_ptr(stream))
    _lib.check(rc, "seg_loss")
    return loss.reshape(()), out


def _softmax_map(score, which):
    _lib.require_gpu(score)
    score = _map4(score, "input")
    gt = torch.full(score.shape[:3], -1, dtype=torch.int32, device=score.device)  # no pixel enters the loss
    return seg_loss(score, gt, 1.0, want=(which,))[1][which]


def softmax_high_dimension(input, num_classes=None, name=None):
    """prob_normalized = exp(d) / sum(exp(d)), d = input - max over the class axis."""
    return _softmax_map(input, "prob_normalized")


def log_softmax_high_dimension(input, num_classes=None, name=None):
    """prob = d - log(sum(exp(d)))."""
    return _softmax_map(input, "log_prob")


def loss_cross_entropy_single_frame(scores, labels, *, want_grad=False, grad_scale=1.0, stream=None):
    """sum(-labels * scores) / (sum(labels) + 1e-10); scores are log-probabilities
    and labels the Hardlabel weights, same shape (..., C).  want_grad: also
    d loss / d scores = -labels * grad_scale / (sum(labels) + 1e-10)."""
    _lib.require_gpu(scores, labels)
    if scores.dim() < 2 or scores.shape != labels.shape:
        raise ValueError(f"scores {tuple(scores.shape)} and labels {tuple(labels.shape)} must have one shape (..., C)")
    scores, labels = scores.contiguous().float(), labels.contiguous().float()
    C = scores.shape[-1]
    n_pix = scores.numel() // max(C, 1)
    dev = scores.device
    loss = _scalar(dev)
    d = torch.empty_like(scores) if want_grad else None
    lib = _lib.load()
    need = lib.pcnn_cross_entropy_workspace_size(n_pix, C)
    if need == 0:
        raise ValueError(f"loss_cross_entropy_single_frame: unsupported shape {tuple(scores.shape)}")
    ws = _lib.workspace(need, dev, "seg_loss", stream)
    rc = lib.pcnn_cross_entropy(_lib.ptr(scores), _lib.ptr(labels), n_pix, C, float(grad_scale), _lib.ptr(d),
                                _lib.ptr(loss), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(stream))
    _lib.check(rc, "loss_cross_entropy_single_frame")
    return (loss.reshape(()), d) if want_grad else loss.reshape(())


def smooth_l1_loss_vertex(vertex_pred, vertex_targets, vertex_weights, sigma=1.0, *, want_grad=False, grad_scale=1.0,
                          stream=None):
    """sum(smooth_l1(w * (pred - tgt))) / (sum(w) + 1e-10) with the branch point
    at 1 / sigma^2; the caller multiplies by VERTEX_W.  want_grad: also
    d loss / d vertex_pred."""
    _lib.require_gpu(vertex_pred, vertex_targets, vertex_weights)
    if float(sigma) <= 0:
        raise ValueError(f"Need sigma > 0, got {sigma}")
    if vertex_pred.shape != vertex_targets.shape or vertex_pred.shape != vertex_weights.shape:
        raise ValueError(f"vertex_pred {tuple(vertex_pred.shape)}, vertex_targets {tuple(vertex_targets.shape)} and "
                         f"vertex_weights {tuple(vertex_weights.shape)} must have one shape")
    pred, tgt, wt = (x.contiguous().float() for x in (vertex_pred, vertex_targets, vertex_weights))
    dev = pred.device
    loss = _scalar(dev)
    d = torch.empty_like(pred) if want_grad else None
    lib = _lib.load()
    need = lib.pcnn_vertex_loss_workspace_size(pred.numel())
    if need == 0:
        raise ValueError(f"smooth_l1_loss_vertex: unsupported shape {tuple(pred.shape)}")
    ws = _lib.workspace(need, dev, "seg_loss", stream)
    rc = lib.pcnn_vertex_loss(_lib.ptr(pred), _lib.ptr(tgt), _lib.ptr(wt), pred.numel(), float(sigma),
                              float(grad_scale), _lib.ptr(d), _lib.ptr(loss), _lib.ptr(ws), ws.numel(),
                              _lib.stream_ptr(stream))
    _lib.check(rc, "smooth_l1_loss_vertex")
    return (loss.reshape(()), d) if want_grad else loss.reshape(())


def vertex_loss_compact(vertex_pred, label, vertex3, num_classes, w_inside, sigma=1.0, *, dense_grad=False,
                        want_grad=False, grad_scale=1.0, stream=None):
    """smooth_l1_loss_vertex against the compact ground truth: label (B,H,W)
    and vertex3 (B,H,W,3) as the scene renderer writes them.  vertex_pred is
    (B,H,W,3 * num_classes), or (B,H,W,3) holding each pixel's prediction at
    its ground-truth class.  want_grad: also d loss / d vertex_pred, (B,H,W,3)
    at the label's channels, or the whole (B,H,W,3 * num_classes) map, zeros
    included, with dense_grad."""
    _lib.require_gpu(vertex_pred, label, vertex3)
    if float(sigma) <= 0:
        raise ValueError(f"Need sigma > 0, got {sigma}")
    C = int(num_classes)
    if label.dim() != 3 or tuple(vertex3.shape) != (*label.shape, 3):
        raise ValueError("vertex_loss_compact: label (B,H,W) and vertex3 (B,H,W,3)")
    B, H, W = label.shape
    if vertex_pred.dim() != 4 or tuple(vertex_pred.shape[:3]) != (B, H, W) or vertex_pred.shape[3] not in (3, 3 * C):
        raise ValueError(f"vertex_pred must be (B,H,W,3) or (B,H,W,{3 * C}), got {tuple(vertex_pred.shape)}")
    pred = vertex_pred.contiguous().float()
    label, vertex3 = label.contiguous().to(torch.int32), vertex3.contiguous().float()
    dev = pred.device
    loss = _scalar(dev)
    d_ch = 3 * C if dense_grad else 3
    d = torch.empty((B, H, W, d_ch), dtype=torch.float32, device=dev) if want_grad else None
    lib = _lib.load()
    need = lib.pcnn_vertex_loss_compact_workspace_size(B, H, W, C)
    if need == 0:
        raise ValueError(f"vertex_loss_compact: unsupported shape {(B, H, W, C)}")
    ws = _lib.workspace(need, dev, "seg_loss", stream)
    rc = lib.pcnn_vertex_loss_compact(_lib.ptr(label), _lib.ptr(vertex3), _lib.ptr(pred), pred.shape[3], B, H, W, C,
                                      float(w_inside), float(sigma), float(grad_scale), _lib.ptr(d), d_ch,
                                      _lib.ptr(loss), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(stream))
    _lib.check(rc, "vertex_loss_compact")
    return (loss.reshape(()), d) if want_grad else loss.reshape(())
