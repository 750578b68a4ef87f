"""Drop-in for lib/average_distance_loss/average_distance_loss_op.py (:4-7):
`average_distance_loss` / `average_distance_loss_grad` (REGISTER_OP
"Averagedistance" / "AveragedistanceGrad", average_distance_loss_op.cc:38-54),
backed by libposecnn_hip.so.

average_distance_loss(pred (R,4C), target, weight, points (C,P,3), symmetry (C), margin)
    -> (loss (1,), bottom_diff (R,4C))   [ADD, or ADD-S for symmetric classes]
average_distance_loss_grad(bottom_diff, grad, margin) -> grad[0] * bottom_diff
"""
import warnings

import torch

from .. import _lib


def workspace_bytes(R, num_classes, num_points):
    return _lib.load().pcnn_add_loss_workspace_size(R, num_classes, num_points)


def search_stats(workspace, R, num_classes, num_points):
    """The ADD-S search counters the last loss on `workspace` left there (a
    device read): symmetric (row, chunk) items searched by the MFMA filter,
    items searched by the exact scan (out of the filter's range, or
    PCNN_ADD_SEARCH=scan), the filter items' passing (query, 32-candidate
    block, half) triples and their exact evaluations (16 per triple)."""
    off = _lib.load().pcnn_add_loss_stats_offset(R, num_classes, num_points)
    f, s, t = workspace[off:off + 12].cpu().view(torch.int32).tolist()
    return {"filter_items": f, "scan_items": s, "triples": t, "exact_evals": 16 * t}


def _workspace(what, ws, R, C, P):
    """A caller's loss workspace: contiguous uint8 device bytes, at least workspace_bytes(R, C, P)."""
    _lib.require(ws, torch.uint8, name=f"{what}: workspace")
    need = workspace_bytes(R, C, P)
    if ws.numel() < need:
        raise ValueError(f"{what}: workspace must hold {need} bytes, got {ws.numel()}")


def _models(what, points, symmetry, C, normalise):
    """points (C, P, 3) and symmetry (C): packed fp32 (normalise: made so; else refused)."""
    if normalise:
        points, symmetry = points.contiguous().float(), symmetry.contiguous().float()
    if points.dim() != 3 or points.shape[0] != C or points.shape[2] != 3:
        raise ValueError(f"{what}: points must be ({C}, P, 3), got {tuple(points.shape)}")
    _lib.require(points, torch.float32, name=f"{what}: points")
    _lib.require(symmetry, torch.float32, name=f"{what}: symmetry")
    if symmetry.numel() != C:
        raise ValueError(f"{what}: symmetry must have {C} elements, got {symmetry.numel()}")
    return points, symmetry


def average_distance_loss_prep(bottom_weight, bottom_symmetry, num_points, workspace, num_rois=None, points=None):
    """Row classification of the loss (pcnn_add_loss_prep) into `workspace`
    (uint8, >= workspace_bytes); may run on another stream as soon as the
    weights exist.  Follow with average_distance_loss(..., prepared=True,
    workspace=workspace) ordered after it (the same bits as the unprepared
    call).  `points` is deprecated and ignored (DeprecationWarning): callers
    written for the removed pruned ADD-S search passed the model points here;
    the loss they get is the same, bit for bit."""
    if points is not None:
        warnings.warn("average_distance_loss_prep: `points` is ignored (the pruned ADD-S search is removed)",
                      DeprecationWarning, stacklevel=2)
    _lib.require_gpu(bottom_weight, bottom_symmetry, workspace)
    if bottom_weight.dim() != 2 or bottom_weight.shape[1] % 4:
        raise ValueError("average_distance_loss_prep: weight must be (R, 4C)")
    w = bottom_weight.contiguous().float()
    R, PC = w.shape
    sym = bottom_symmetry.contiguous().float()
    if sym.numel() != PC // 4:
        raise ValueError(f"average_distance_loss_prep: symmetry must have {PC // 4} elements, got {sym.numel()}")
    _workspace("average_distance_loss_prep", workspace, R, PC // 4, int(num_points))
    _lib.require_counter(num_rois, "average_distance_loss_prep: num_rois")
    rc = _lib.load().pcnn_add_loss_prep(_lib.ptr(w), _lib.ptr(sym), R,
                                        _lib.ptr(num_rois), PC // 4, int(num_points), _lib.ptr(workspace),
                                        workspace.numel(), _lib.stream_ptr())
    _lib.check(rc, "average_distance_loss_prep")


def average_distance_loss(bottom_prediction, bottom_target, bottom_weight, bottom_point, bottom_symmetry, margin,
                          name=None, num_rois=None, loss_norm_rows=0, loss_norm_rows_dev=None, out=None,
                          workspace=None, prepared=False):
    _lib.require_gpu(bottom_prediction, bottom_target, bottom_weight, bottom_point, bottom_symmetry)
    if margin < 0:
        raise ValueError(f"Need margin >= 0, got {margin}")  # average_distance_loss_op.cc:64-65
    what = "average_distance_loss"
    if bottom_prediction.dim() != 2 or bottom_prediction.shape[1] % 4:
        raise ValueError(f"{what}: prediction must be (R, 4C)")
    pred = bottom_prediction.contiguous().float()
    R, PC = pred.shape
    C = PC // 4
    for name, t in (("target", bottom_target), ("weight", bottom_weight)):
        if tuple(t.shape) != (R, PC):
            raise ValueError(f"{what}: {name} must be {(R, PC)} as the prediction, got {tuple(t.shape)}")
    points, symmetry = _models(what, bottom_point, bottom_symmetry, C, normalise=True)
    P = points.shape[1]
    _lib.require_counter(num_rois, f"{what}: num_rois")
    _lib.require_counter(loss_norm_rows_dev, f"{what}: loss_norm_rows_dev")
    if workspace is not None:
        _workspace(what, workspace, R, C, P)
    lib = _lib.load()
    if prepared and workspace is None:
        raise ValueError("prepared=True needs the workspace average_distance_loss_prep wrote")
    ws = workspace if workspace is not None else _lib.workspace(lib.pcnn_add_loss_workspace_size(R, C, P),
                                                                pred.device, "add_loss")
    if out is None:
        loss = torch.empty((1,), dtype=torch.float32, device=pred.device)
        diff = torch.empty((R, PC), dtype=torch.float32, device=pred.device)
    else:
        loss, diff = out
        _lib.require(loss, torch.float32, shape=(1,), name=f"{what}: out[0] (loss)")
        _lib.require(diff, torch.float32, shape=(R, PC), name=f"{what}: out[1] (bottom_diff)")
    fn = lib.pcnn_add_loss_fwd_prepared if prepared else lib.pcnn_add_loss_fwd
    rc = fn(_lib.ptr(pred), _lib.ptr(bottom_target.contiguous().float()), _lib.ptr(bottom_weight.contiguous().float()),
            _lib.ptr(points), _lib.ptr(symmetry), R,
            _lib.ptr(num_rois), C, P, float(margin), int(loss_norm_rows), _lib.ptr(loss_norm_rows_dev), _lib.ptr(loss),
            _lib.ptr(diff), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    _lib.check(rc, "average_distance_loss")
    return loss, diff


def average_distance_loss_head_bwd(pred, target, weight, points, symmetry, margin, tanh_out, d_pred_scale, diff, dy8,
                                   workspace, num_rois=None, loss_norm_rows_dev=None, checked=True):
    """The pose step's fused loss tail (pcnn_add_loss_fwd_head_bwd, prepared
    rows): bottom_diff into `diff` and the pose head's backward of it into
    `dy8`; the scalar loss follows with average_distance_loss_total.  A
    primitive of the step's hot path: nothing is copied or converted, every
    tensor is a packed fp32 device tensor of its shape or the call raises
    ValueError (float64 model points from numpy included)."""
    _lib.require_gpu(pred, target, weight, points, symmetry, tanh_out, diff, dy8, workspace)
    what = "average_distance_loss_head_bwd"
    if margin < 0:
        raise ValueError(f"Need margin >= 0, got {margin}")  # average_distance_loss_op.cc:64-65
    if pred.dim() != 2 or pred.shape[1] % 4:
        raise ValueError(f"{what}: pred must be (R, 4C)")
    R, PC = pred.shape
    if PC > 256:
        raise ValueError(f"{what}: at most 256 columns (4C), got {PC}")
    _models(what, points, symmetry, PC // 4, normalise=False)  # (per minibatch: checked on every call)
    if checked:  # False: the caller's fixed buffers, already passed through these once (PoseStep)
        for name, t in (("pred", pred), ("target", target), ("weight", weight), ("tanh_out", tanh_out),
                        ("diff", diff), ("dy8", dy8)):
            _lib.require(t, torch.float32, shape=(R, PC), name=f"{what}: {name}")
        if d_pred_scale is not None and _lib.require(d_pred_scale, torch.float32,
                                                     name=f"{what}: d_pred_scale").numel() < 1:
            raise ValueError(f"{what}: d_pred_scale needs one element")
        _workspace(what, workspace, R, PC // 4, points.shape[1])
        _lib.require_counter(num_rois, f"{what}: num_rois")
        _lib.require_counter(loss_norm_rows_dev, f"{what}: loss_norm_rows_dev")
    rc = _lib.load().pcnn_add_loss_fwd_head_bwd(
        _lib.ptr(pred), _lib.ptr(target), _lib.ptr(weight), _lib.ptr(points), _lib.ptr(symmetry), R,
        _lib.ptr(num_rois), PC // 4, points.shape[1], float(margin), 0, _lib.ptr(loss_norm_rows_dev), _lib.ptr(diff),
        _lib.ptr(workspace), workspace.numel(), _lib.ptr(tanh_out), _lib.ptr(d_pred_scale), _lib.ptr(dy8),
        _lib.stream_ptr())
    _lib.check(rc, "average_distance_loss_head_bwd")


def average_distance_loss_total(R, num_classes, num_points, workspace, loss, num_rois=None, checked=True):
    """The scalar loss of an average_distance_loss_head_bwd call (its row losses in `workspace`)."""
    _lib.require_gpu(workspace, loss)
    if checked:
        _workspace("average_distance_loss_total", workspace, R, num_classes, num_points)
        _lib.require(loss, torch.float32, shape=(1,), name="average_distance_loss_total: loss")
        _lib.require_counter(num_rois, "average_distance_loss_total: num_rois")
    rc = _lib.load().pcnn_add_loss_total(R, _lib.ptr(num_rois), num_classes, num_points, _lib.ptr(workspace),
                                         workspace.numel(), _lib.ptr(loss), _lib.stream_ptr())
    _lib.check(rc, "average_distance_loss_total")


def average_distance_loss_grad(bottom_diff, grad, margin=0.01, name=None, num_rois=None, out=None):
    _lib.require_gpu(bottom_diff, grad)
    bd = bottom_diff.contiguous().float()
    g = grad.contiguous().float()
    if g.numel() < 1:
        raise ValueError("average_distance_loss_grad: grad needs one element")
    o = out if out is not None else torch.empty_like(bd)
    if out is not None:
        _lib.require(out, torch.float32, shape=tuple(bd.shape), name="average_distance_loss_grad: out")
    _lib.require_counter(num_rois, "average_distance_loss_grad: num_rois")
    rc = _lib.load().pcnn_add_loss_bwd(_lib.ptr(g), _lib.ptr(bd), bd.numel(),
                                       _lib.ptr(num_rois), bd.shape[-1], _lib.ptr(o), _lib.stream_ptr())
    _lib.check(rc, "average_distance_loss_grad")
    return o


class AverageDistanceFunction(torch.autograd.Function):
    """autograd binding (average_distance_loss_op_grad.py:5-14)."""

    @staticmethod
    def forward(ctx, pred, target, weight, points, symmetry, margin):
        loss, diff = average_distance_loss(pred, target, weight, points, symmetry, margin)
        ctx.save_for_backward(diff)
        ctx.margin = margin
        return loss

    @staticmethod
    def backward(ctx, grad):
        (diff,) = ctx.saved_tensors
        return average_distance_loss_grad(diff, grad.reshape(1), ctx.margin), None, None, None, None, None
