"""Class-compact vertex wire format.

The reference's `vertex_pred` layer (lib/networks/vgg16_convs.py:152-163: a
1x1 conv 128 -> 3C plus bias_add, network.py:168-185) writes a (B,H,W,3C)
map — 264 B per pixel at C = 22 — of which the Hough vote reads only the three
channels of each voter's own class (hough_voting_gpu_op.cu.cc:276-280).
`vertex_pred_compact` evaluates the layer only at those channels, given the
label map, and writes (B,H,W,3); `hough_voting_gpu_capacity(...,
vertex_compact=True)` votes from it with outputs identical to the full map's.
`vertex_pred_compact_bwd` is the layer's backward from a (B,H,W,3) gradient
(`losses.vertex_loss_compact`'s `d_pred`): with the ground-truth label map,
the reference's gradients under the loss's own mask, the (B,H,W,3C) gradient
never formed.  `pth.VertexPredCompact` wraps the pair for autograd.
"""
import torch

from . import _lib


def vertex_pred_compact(feat, weights, biases, label, out=None, stream=None):
    """feat (B,H,W,K) NHWC, weights (K,3C) or the reference's (1,1,K,3C) kernel,
    biases (3C), label (B,H,W) int -> (B,H,W,3) float32."""
    _lib.require_gpu(feat, weights, biases, label)
    if feat.dim() != 4 or label.dim() != 3:
        raise ValueError("feat must be (B,H,W,K) and label (B,H,W)")
    B, H, W, K = feat.shape
    w = weights.reshape(K, -1).contiguous().float()
    if w.shape[1] % 3 or biases.numel() != w.shape[1]:
        raise ValueError("weights must be (K, 3C) with a 3C bias")
    C = w.shape[1] // 3
    feat = feat.contiguous().float()
    lab = label.contiguous().to(torch.int32)
    if tuple(label.shape) != (B, H, W):
        raise ValueError(f"label must be {(B, H, W)}, got {tuple(label.shape)}")
    if out is None:
        out = torch.empty((B, H, W, 3), dtype=torch.float32, device=feat.device)
    else:
        _lib.require(out, torch.float32, shape=(B, H, W, 3), name="vertex_pred_compact: out")
    rc = _lib.load().pcnn_vertex_pred_compact(_lib.ptr(feat), _lib.ptr(w), _lib.ptr(biases.contiguous().float()),
                                              _lib.ptr(lab), B, H, W, K, C, _lib.ptr(out), _lib.stream_ptr(stream))
    _lib.check(rc, "vertex_pred_compact")
    return out


BWD_OUTPUTS = ("feat", "weights", "bias")


def vertex_pred_compact_bwd(feat, weights, label, d_vertex3, *, want=BWD_OUTPUTS, stream=None):
    """The layer's backward from d_vertex3 (B,H,W,3), the gradient of
    vertex_pred_compact's output: {name: gradient for name in want}, names from
    BWD_OUTPUTS.  d_feat is (B,H,W,K), d_weights has the shape `weights` came
    in ((K,3C) or (1,1,K,3C)), d_bias is (3C).  A pixel whose label is outside
    [0, C) has a zero d_feat row and adds nothing to the sums
    (include/posecnn_hip.h)."""
    _lib.require_gpu(feat, weights, label, d_vertex3)
    unknown = [w for w in want if w not in BWD_OUTPUTS]
    if unknown or not want:
        raise ValueError(f"want must name at least one of {BWD_OUTPUTS}, got {tuple(want)}")
    if feat.dim() != 4 or label.dim() != 3:
        raise ValueError("feat must be (B,H,W,K) and label (B,H,W)")
    B, H, W, K = feat.shape
    if tuple(label.shape) != (B, H, W) or tuple(d_vertex3.shape) != (B, H, W, 3):
        raise ValueError(f"label must be {(B, H, W)} and d_vertex3 {(B, H, W, 3)}")
    w = weights.reshape(K, -1).contiguous().float()
    if w.shape[1] % 3:
        raise ValueError("weights must be (K, 3C)")
    C = w.shape[1] // 3
    feat = feat.contiguous().float()
    lab = label.contiguous().to(torch.int32)
    g = d_vertex3.contiguous().float()
    dev = feat.device
    out = {}
    if "feat" in want:
        out["feat"] = torch.empty((B, H, W, K), dtype=torch.float32, device=dev)
    if "weights" in want:
        out["weights"] = torch.empty(tuple(weights.shape), dtype=torch.float32, device=dev)
    if "bias" in want:
        out["bias"] = torch.empty((3 * C,), dtype=torch.float32, device=dev)
    lib = _lib.load()
    need = lib.pcnn_vertex_pred_compact_bwd_workspace_size(B, H, W, K, C)
    if need == 0:
        raise ValueError(f"vertex_pred_compact_bwd: unsupported shape {(B, H, W, K, C)}")
    ws = _lib.workspace(need, dev, "vertex_pred_bwd", stream)
    rc = lib.pcnn_vertex_pred_compact_bwd(_lib.ptr(feat), _lib.ptr(w), _lib.ptr(lab), _lib.ptr(g), B, H, W, K, C,
                                          _lib.ptr(out.get("feat")), _lib.ptr(out.get("weights")),
                                          _lib.ptr(out.get("bias")), _lib.ptr(ws), ws.numel(),
                                          _lib.stream_ptr(stream))
    _lib.check(rc, "vertex_pred_compact_bwd")
    return out
