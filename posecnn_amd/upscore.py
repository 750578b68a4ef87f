"""The upscore layers (include/posecnn_hip.h, csrc/upscore.hip).

The reference's fixed bilinear transposed conv (`upscore`, `upscore_vertex`:
16x16 at stride 8, lib/networks/vgg16_convs.py:138,162; `upscore_conv5(_vertex)`:
4x4 at stride 2, :122,130,154; network.py:141-157, 207-222) is `upscore` with
its backward `upscore_bwd`; an optional bias and ReLU ride in the forward's
epilogue and the backward's mask, which is what the segmentation head
`score = relu(upscore(x W) + b)` needs.

`upscore_compact` / `upscore_compact_bwd` are the layer folded behind the 1x1
conv of the vertex head: with z = x W at 1/s resolution,
vertex_pred(upscore_vertex(x)) = upscore(z) + b, evaluated only at each
pixel's own class -- the (B,H,W,128) map between the two layers is never
formed.  `pth.VertexHeadCompact`, `pth.ScoreHead` and `pth.Upscore` wrap them
for autograd.
"""
import torch

from . import _lib

STRIDES = (2, 4, 8, 16)


def _check_stride(stride):
    if stride not in STRIDES:
        raise ValueError(f"stride must be one of {STRIDES}, got {stride}")
    return int(stride)


def upscore(x, stride, bias=None, relu=False, out=None, stream=None):
    """x (B,h,w,Ch) NHWC -> (B, stride*h, stride*w, Ch) float32; bias (Ch) and
    ReLU, if asked for, are applied after the four taps."""
    _lib.require_gpu(x, bias, out)
    s = _check_stride(stride)
    if x.dim() != 4:
        raise ValueError("x must be (B,h,w,Ch)")
    B, h, w, Ch = x.shape
    if bias is not None and bias.numel() != Ch:
        raise ValueError(f"bias must have {Ch} elements")
    x = x.contiguous().float()
    b = None if bias is None else bias.contiguous().float()
    if out is None:
        out = torch.empty((B, s * h, s * w, Ch), dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (B, s * h, s * w, Ch) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float32 {(B, s * h, s * w, Ch)}")
    rc = _lib.load().pcnn_upscore_fwd(_lib.ptr(x), B, h, w, Ch, s, _lib.ptr(b), int(bool(relu)), _lib.ptr(out),
                                      _lib.stream_ptr(stream))
    _lib.check(rc, "upscore")
    return out


def upscore_bwd(d_y, stride, y=None, want_bias=False, stream=None):
    """The backward of `upscore` from d_y (B,H,W,Ch): d_x (B,H/s,W/s,Ch), or
    (d_x, d_bias) with want_bias.  y, the forward's output, is the ReLU mask
    (y > 0); None for a forward without ReLU."""
    _lib.require_gpu(d_y, y)
    s = _check_stride(stride)
    if d_y.dim() != 4 or d_y.shape[1] % s or d_y.shape[2] % s:
        raise ValueError(f"d_y must be (B,H,W,Ch) with H and W multiples of {s}")
    B, H, W, Ch = d_y.shape
    if y is not None and tuple(y.shape) != (B, H, W, Ch):
        raise ValueError(f"y must be {(B, H, W, Ch)}")
    h, w = H // s, W // s
    g = d_y.contiguous().float()
    yv = None if y is None else y.contiguous().float()
    dev = g.device
    d_x = torch.empty((B, h, w, Ch), dtype=torch.float32, device=dev)
    d_b = torch.empty((Ch,), dtype=torch.float32, device=dev) if want_bias else None
    lib = _lib.load()
    need = lib.pcnn_upscore_bwd_workspace_size(B, h, w, Ch, s)
    if need == 0:
        raise ValueError(f"upscore_bwd: unsupported shape {(B, h, w, Ch, s)}")
    ws = _lib.workspace(need, dev, "upscore_bwd", stream) if want_bias else None
    rc = lib.pcnn_upscore_bwd(_lib.ptr(g), _lib.ptr(yv), B, h, w, Ch, s, _lib.ptr(d_x), _lib.ptr(d_b), _lib.ptr(ws),
                              ws.numel() if want_bias else 0, _lib.stream_ptr(stream))
    _lib.check(rc, "upscore_bwd")
    return (d_x, d_b) if want_bias else d_x


def _compact_dims(z_shape, label, stride):
    s = _check_stride(stride)
    if len(z_shape) != 4 or z_shape[3] % 3 or label.dim() != 3:
        raise ValueError("z must be (B,h,w,3C) and label (B,H,W)")
    B, h, w, NC3 = z_shape
    if tuple(label.shape) != (B, s * h, s * w):
        raise ValueError(f"label must be {(B, s * h, s * w)}, got {tuple(label.shape)}")
    return B, h, w, NC3 // 3, s


def upscore_compact(z, bias, label, stride=8, out=None, stream=None):
    """z (B,h,w,3C), bias (3C), label (B,H,W) int -> (B,H,W,3) float32: the
    upscore of z plus bias at the three channels of each pixel's class, the
    bits `upscore(z, stride, bias)` has there; zeros where the label is
    outside [0, C)."""
    _lib.require_gpu(z, bias, label, out)
    B, h, w, C, s = _compact_dims(tuple(z.shape), label, stride)
    if bias.numel() != 3 * C:
        raise ValueError(f"bias must have {3 * C} elements")
    z = z.contiguous().float()
    lab = label.contiguous().to(torch.int32)
    if out is None:
        out = torch.empty((B, s * h, s * w, 3), dtype=torch.float32, device=z.device)
    elif tuple(out.shape) != (B, s * h, s * w, 3) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float32 {(B, s * h, s * w, 3)}")
    rc = _lib.load().pcnn_upscore_compact_fwd(_lib.ptr(z), _lib.ptr(bias.contiguous().float()), _lib.ptr(lab), B, h, w,
                                              C, s, _lib.ptr(out), _lib.stream_ptr(stream))
    _lib.check(rc, "upscore_compact")
    return out


COMPACT_BWD_OUTPUTS = ("z", "bias")


def upscore_compact_bwd(label, d_vertex3, num_classes, stride=8, *, want=COMPACT_BWD_OUTPUTS, stream=None):
    """The backward of `upscore_compact` from d_vertex3 (B,H,W,3): {name:
    gradient for name in want}, names from COMPACT_BWD_OUTPUTS; d_z is
    (B,H/s,W/s,3C), d_bias (3C)."""
    _lib.require_gpu(label, d_vertex3)
    s = _check_stride(stride)
    unknown = [n for n in want if n not in COMPACT_BWD_OUTPUTS]
    if unknown or not want:
        raise ValueError(f"want must name at least one of {COMPACT_BWD_OUTPUTS}, got {tuple(want)}")
    if label.dim() != 3 or label.shape[1] % s or label.shape[2] % s:
        raise ValueError(f"label must be (B,H,W) with H and W multiples of {s}")
    B, H, W = label.shape
    if tuple(d_vertex3.shape) != (B, H, W, 3):
        raise ValueError(f"d_vertex3 must be {(B, H, W, 3)}, got {tuple(d_vertex3.shape)}")
    C = int(num_classes)
    h, w = H // s, W // s
    lab = label.contiguous().to(torch.int32)
    g = d_vertex3.contiguous().float()
    dev = g.device
    out = {}
    if "z" in want:
        out["z"] = torch.empty((B, h, w, 3 * C), dtype=torch.float32, device=dev)
    if "bias" in want:
        out["bias"] = torch.empty((3 * C,), dtype=torch.float32, device=dev)
    lib = _lib.load()
    need = lib.pcnn_upscore_compact_bwd_workspace_size(B, h, w, C, s)
    if need == 0:
        raise ValueError(f"upscore_compact_bwd: unsupported shape {(B, h, w, C, s)}")
    ws = _lib.workspace(need, dev, "upscore_compact_bwd", stream) if "bias" in want else None
    rc = lib.pcnn_upscore_compact_bwd(_lib.ptr(lab), _lib.ptr(g), B, h, w, C, s, _lib.ptr(out.get("z")),
                                      _lib.ptr(out.get("bias")), _lib.ptr(ws), ws.numel() if ws is not None else 0,
                                      _lib.stream_ptr(stream))
    _lib.check(rc, "upscore_compact_bwd")
    return out
