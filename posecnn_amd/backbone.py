"""The VGG16 backbone's forward, backed by libposecnn_hip.so (csrc/backbone.hip,
include/posecnn_backbone.h): the thirteen 3x3 convolutions with bias and ReLU
and the four 2x2 max-pools of lib/networks/vgg16_convs.py:80-97 that turn the
(B,H,W,3) blob into conv4_3 and conv5_3.

conv3x3(x, weights, bias, relu=True, out=None)    one layer, NHWC float32, SAME
max_pool2x2(x, out=None)                          2x2, stride 2, SAME (ceil)
LAYERS                                            the reference's layer table
vgg16_convs(x, params, keep=()) -> (conv4_3, conv5_3[, {name: map}])

Weights are the reference's TF variables as they are: HWIO (3,3,Cin,Cout); bias
(Cout).  Cin % 16 == 0 runs the exact three-way split-bf16 MFMA kernel (the
numerics of pose_head.gemm at precision 2), Cin == 3 (conv1_1) a direct float32
kernel; the arithmetic of each is stated in the header and restated in numpy by
tests/backbone_ref.py.  Forward only: the backward is not built.  Nothing here
syncs with or reads back to the host.
"""
import ctypes

import torch

from . import _lib

_v, _i = ctypes.c_void_p, ctypes.c_int
# include/posecnn_backbone.h: name -> (restype, argtypes); v = device pointer or stream
SIGS = {
    "pcnn_backbone_abi_version": (_i, []),
    "pcnn_conv3x3_workspace_size": (ctypes.c_size_t, [_i, _i, _i, _i, _i, _i]),
    "pcnn_conv3x3_fwd": (_i, [_v, _v, _v, _i, _i, _i, _i, _i, _i, _i, _v, _v, ctypes.c_size_t, _v]),
    "pcnn_maxpool2x2_fwd": (_i, [_v, _i, _i, _i, _i, _v, _v]),
}
_bound = None
F32 = torch.float32
PRECISION = 2  # the only one built
MAX_BYTES = 1 << 31

# (name, Cin, Cout) of a conv, or (name,) of a pool: vgg16_convs.py:80-97
LAYERS = (
    ("conv1_1", 3, 64), ("conv1_2", 64, 64), ("pool1",),
    ("conv2_1", 64, 128), ("conv2_2", 128, 128), ("pool2",),
    ("conv3_1", 128, 256), ("conv3_2", 256, 256), ("conv3_3", 256, 256), ("pool3",),
    ("conv4_1", 256, 512), ("conv4_2", 512, 512), ("conv4_3", 512, 512), ("pool4",),
    ("conv5_1", 512, 512), ("conv5_2", 512, 512), ("conv5_3", 512, 512),
)
CONVS = tuple(layer for layer in LAYERS if len(layer) == 3)
OUTPUTS = ("conv4_3", "conv5_3")


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


def _map(who, x, name="x"):
    _lib.require(x, F32, (None, None, None, None), name=f"{who}: {name}")
    B, H, W, C = (int(s) for s in x.shape)
    if B < 1 or H < 1 or W < 1 or C < 1:
        raise ValueError(f"{who}: {name}: expected a non-empty (B,H,W,C) map, got shape {tuple(x.shape)}")
    if B * H * W * C * 4 >= MAX_BYTES:
        raise ValueError(f"{who}: {name}: {B * H * W * C * 4} bytes, expected fewer than 2^31")
    return B, H, W, C


def _out(who, out, shape, x):
    if out is None:
        return torch.empty(shape, dtype=F32, device=x.device)
    _lib.require(out, F32, shape, name=f"{who}: out")
    if out.device != x.device:
        raise ValueError(f"{who}: out: on {out.device}, expected {x.device}")
    if out.data_ptr() == x.data_ptr():
        raise ValueError(f"{who}: out: must not be the input")
    return out


def conv3x3(x, weights, bias, relu=True, out=None, stream=None):
    """relu(conv3x3(x, weights) + bias), stride 1, TF SAME: x (B,H,W,Cin) NHWC
    float32, weights (3,3,Cin,Cout) HWIO, bias (Cout) or None -> (B,H,W,Cout)
    (into `out` if given).  Cin is 3 or a multiple of 16, Cout a multiple of 4.
    relu=False leaves the pre-activation.  One or two launches, no sync."""
    who = "conv3x3"
    B, H, W, Cin = _map(who, x)
    _lib.require(weights, F32, (3, 3, Cin, None), name=f"{who}: weights")
    Cout = int(weights.shape[3])
    if Cin != 3 and Cin % 16:
        raise ValueError(f"{who}: x: expected 3 channels or a multiple of 16, got {Cin}")
    if Cout < 1 or Cout % 4:
        raise ValueError(f"{who}: weights: expected a multiple of 4 output channels, got {Cout}")
    if B * H * W * Cout * 4 >= MAX_BYTES or 9 * Cin * Cout * 4 >= MAX_BYTES:
        raise ValueError(f"{who}: expected an output map and weights of fewer than 2^31 bytes")
    _lib.require(bias, F32, (Cout,), name=f"{who}: bias", optional=True)
    for name, t in (("weights", weights), ("bias", bias)):
        if t is not None and t.device != x.device:
            raise ValueError(f"{who}: {name}: on {t.device}, expected {x.device}")
    y = _out(who, out, (B, H, W, Cout), x)
    lib = _load()
    need = lib.pcnn_conv3x3_workspace_size(B, H, W, Cin, Cout, PRECISION)
    ws = _lib.workspace(need, x.device, "conv3x3", stream) if need else None
    rc = lib.pcnn_conv3x3_fwd(_lib.ptr(x), _lib.ptr(weights), _lib.ptr(bias), B, H, W, Cin, Cout, 1 if relu else 0,
                              PRECISION, _lib.ptr(y), _lib.ptr(ws), need, _lib.stream_ptr(stream))
    _lib.check(rc, who)
    return y


def max_pool2x2(x, out=None, stream=None):
    """2x2 max-pool, stride 2, TF SAME: x (B,H,W,C) NHWC float32, C a multiple
    of 4 -> (B, ceil(H/2), ceil(W/2), C) (into `out` if given).  The last window
    of an odd axis holds one row or column.  One launch, no sync."""
    who = "max_pool2x2"
    B, H, W, C = _map(who, x)
    if C % 4:
        raise ValueError(f"{who}: x: expected a multiple of 4 channels, got {C}")
    y = _out(who, out, (B, (H + 1) // 2, (W + 1) // 2, C), x)
    rc = _load().pcnn_maxpool2x2_fwd(_lib.ptr(x), B, H, W, C, _lib.ptr(y), _lib.stream_ptr(stream))
    _lib.check(rc, who)
    return y


_pingpong = {}


def _buffers(device, B, H, W):
    """The two ping-pong buffers of the intermediate maps at a blob shape: each
    holds the largest one, (B,H,W,64).  Cached: allocated on the first call."""
    key = (str(device), B, H, W)
    bufs = _pingpong.get(key)
    if bufs is None:
        n = B * H * W * max(cout for _, _, cout in CONVS[:2])
        bufs = _pingpong[key] = (torch.empty(n, dtype=F32, device=device), torch.empty(n, dtype=F32, device=device))
    return bufs


def check_params(who, params, device=None):
    """params = {name: (weights (3,3,Cin,Cout), bias (Cout) or None)} for every conv of LAYERS."""
    for name, cin, cout in CONVS:
        if name not in params:
            raise ValueError(f"{who}: params: no entry for {name}")
        w, b = params[name]
        _lib.require(w, F32, (3, 3, cin, cout), name=f"{who}: {name} weights")
        _lib.require(b, F32, (cout,), name=f"{who}: {name} biases", optional=True)
        for t in (w, b):
            if device is not None and t is not None and t.device != device:
                raise ValueError(f"{who}: {name}: on {t.device}, expected {device}")


def vgg16_convs(x, params, keep=(), stream=None):
    """The whole stack: x (B,H,W,3) NHWC float32, any H, W >= 1; params =
    {name: (weights, biases)} with the reference's variables.  Returns
    (conv4_3 (B,ceil(H/8),ceil(W/8),512), conv5_3 (B,ceil(H/16),ceil(W/16),512)),
    and with `keep` a third value {name: map} for the layer names in it (convs
    after their ReLU, or pools).  Intermediate maps live in two ping-pong
    buffers cached per (device, B, H, W): after the first call at a shape only
    the returned maps are allocated.  Not reentrant across streams at one
    shape (the buffers are shared)."""
    who = "vgg16_convs"
    B, H, W, C = _map(who, x)
    if C != 3:
        raise ValueError(f"{who}: x: expected a (B,H,W,3) blob, got shape {tuple(x.shape)}")
    if B * H * W * 64 * 4 >= MAX_BYTES:
        raise ValueError(f"{who}: x: conv1's map would hold {B * H * W * 256} bytes, expected fewer than 2^31")
    names = [layer[0] for layer in LAYERS]
    unknown = [n for n in keep if n not in names]
    if unknown:
        raise ValueError(f"{who}: keep: unknown layer names {unknown}")
    check_params(who, params, x.device)
    bufs = _buffers(x.device, B, H, W)
    cur, held, kept, outs = x, -1, {}, {}
    for layer in LAYERS:
        name = layer[0]
        h, w, c = int(cur.shape[1]), int(cur.shape[2]), int(cur.shape[3])
        shape = (B, h, w, layer[2]) if len(layer) == 3 else (B, (h + 1) // 2, (w + 1) // 2, c)
        if name in OUTPUTS or name in keep:
            out, slot = None, -1
        else:
            slot = 1 if held == 0 else 0
            n = shape[0] * shape[1] * shape[2] * shape[3]
            out = bufs[slot][:n].view(shape)
        if len(layer) == 3:
            wts, b = params[name]
            cur = conv3x3(cur, wts, b, relu=True, out=out, stream=stream)
        else:
            cur = max_pool2x2(cur, out=out, stream=stream)
        held = slot
        if name in OUTPUTS:
            outs[name] = cur
        if name in keep:
            kept[name] = cur
    if keep:
        return outs["conv4_3"], outs["conv5_3"], kept
    return outs["conv4_3"], outs["conv5_3"]
