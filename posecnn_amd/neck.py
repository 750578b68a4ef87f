"""The embedding neck of vgg16_convs, backed by libposecnn_hip.so
(csrc/neck.hip, include/posecnn_neck.h): everything between conv4_3 / conv5_3
and the two heads (lib/networks/vgg16_convs.py:128-137 and :152-161), both
branches at once, forward and backward.

    score_conv5   = relu(conv5_3 W5s + b5s)     1x1, K -> num_units
    upscore_conv5 = deconv 4x4 stride 2 (fixed bilinear)
    score_conv4   = relu(conv4_3 W4s + b4s)     1x1, K -> num_units
    add_score     = score_conv4 + upscore_conv5
    dropout       = tf.nn.dropout(add_score, keep_prob)        -> ScoreHead
    ..._vertex    : the same with vertex_units columns, no ReLU  -> VertexHeadCompact

The two branches read the same two inputs, so their weights sit side by side:
W4, W5 (K, N) and b4, b5 (N) with N = num_units + vertex_units, the score
branch's columns first.  The 1x1 convs are two GEMMs (pose_head.gemm) over all
N columns -- conv4_3 is read once -- and everything after them is one launch.

neck_fwd(z4, z5, b4, b5, relu_cols, ...)       the fused pass behind the GEMMs
neck_bwd(d_add_score, d_add_score_vertex, ...) its backward, down to dz4, dz5, db4, db5
embedding(x4, x5, W4, b4, W5, b5, num_units, ...) -> (add_score, add_score_vertex, ctx)
embedding_bwd(ctx, d_add_score, d_add_score_vertex, want=...) -> {name: gradient}

The arithmetic (float32, every op rounded separately, fixed orders) is stated
in the header; tests/neck_ref.py restates it in numpy.  pth.EmbeddingNeck wraps
the layer for autograd.  Nothing here syncs with or reads back to the host.
"""
import ctypes

import torch

from . import _lib
from . import pose_head

_v, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
# include/posecnn_neck.h: name -> (restype, argtypes); v = device pointer or stream
SIGS = {
    "pcnn_neck_abi_version": (_i, []),
    "pcnn_neck_fwd": (_i, [_v, _v, _v, _v, _i, _i, _i, _i, _i, _f, ctypes.c_uint64, _v, _i, _i, _v, _v, _v, _v, _v]),
    "pcnn_neck_bwd_workspace_size": (ctypes.c_size_t, [_i, _i, _i, _i, _i]),
    "pcnn_neck_bwd": (_i, [_v, _v, _v, _v, _v, _v, _v, _v, _i, _i, _i, _i, _i, _f, _v, _v, _v, _v, _v,
                           ctypes.c_size_t, _v]),
}
_bound = None
F32, U8, I64 = torch.float32, torch.uint8, torch.int64
STREAM_IDS = (1, 2)  # Philox stream ids of the score and the vertex branch (the pose head's drop6 / drop7: 6, 7)
BWD_OUTPUTS = ("x4", "x5", "W4", "b4", "W5", "b5")


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


def _keep_prob(who, keep_prob):
    kp = float(keep_prob)
    if not 0.0 < kp <= 1.0:
        raise ValueError(f"{who}: keep_prob: expected a value in (0, 1], got {keep_prob}")
    return kp


def _drop_gen(who, keep_prob, drop_gen):
    """(seed, step_dev, (sid_score, sid_vertex)) of a pass; drop_gen None: seed 0, step 0, STREAM_IDS."""
    if drop_gen is None:
        return 0, None, STREAM_IDS
    seed, step_dev, sids = drop_gen
    _lib.require_counter(step_dev, f"{who}: drop_gen's step counter", I64)
    sids = STREAM_IDS if sids is None else tuple(int(s) for s in sids)
    if len(sids) != 2 or min(sids) < 0:
        raise ValueError(f"{who}: drop_gen's stream ids: expected two non-negative ints, got {sids}")
    if keep_prob == 1.0:
        return 0, None, STREAM_IDS
    return int(seed), step_dev, sids


def _maps(who, z4, z5, b4, b5, relu_cols):
    """The checks both passes share: z4 (B,h,w,N), z5 (B,h/2,w/2,N), b4, b5 (N); -> B, h, w, U, V."""
    _lib.require(z4, F32, (None, None, None, None), name=f"{who}: z4")
    B, h, w, N = (int(s) for s in z4.shape)
    U = int(relu_cols)
    V = N - U
    if B < 1 or h < 1 or w < 1 or h % 2 or w % 2:
        raise ValueError(f"{who}: z4: expected (B,h,w,N) with h and w even, got shape {tuple(z4.shape)}")
    if U < 0 or V < 0 or U % 4 or V % 4 or N == 0:
        raise ValueError(f"{who}: expected {U} score and {V} vertex columns to be multiples of 4, not both 0")
    if B * h * w * N >= 1 << 31:
        raise ValueError(f"{who}: z4: {B * h * w * N} elements, expected fewer than 2^31")
    _lib.require(z5, F32, (B, h // 2, w // 2, N), name=f"{who}: z5")
    _lib.require(b4, F32, (N,), name=f"{who}: b4")
    _lib.require(b5, F32, (N,), name=f"{who}: b5")
    _same_device(who, z4, z5=z5, b4=b4, b5=b5)
    return B, h, w, U, V


def neck_fwd(z4, z5, b4, b5, relu_cols, keep_prob=1.0, drop_gen=None, stream=None):
    """The fused pass behind the two GEMMs (pcnn_neck_fwd): z4 (B,h,w,N) and
    z5 (B,h/2,w/2,N) float32, the raw products x4 W4 and x5 W5; b4, b5 (N);
    columns [0, relu_cols) are the score branch (ReLU), the rest the vertex
    branch.  Returns (add_score (B,h,w,U), add_score_vertex (B,h,w,V),
    keep_score, keep_vertex): the keep maps are uint8 (B h w, U) and (B h w, V),
    the bits dropout_mask writes for dense masks of those shapes under
    drop_gen = (seed, step_dev, (stream_id_score, stream_id_vertex)), and None
    at keep_prob 1, where nothing is drawn.  One launch, no sync."""
    who = "neck_fwd"
    B, h, w, U, V = _maps(who, z4, z5, b4, b5, relu_cols)
    kp = _keep_prob(who, keep_prob)
    seed, step_dev, sids = _drop_gen(who, kp, drop_gen)
    _same_device(who, z4, step_dev=step_dev)
    dev, M4 = z4.device, B * h * w
    out_s = torch.empty((B, h, w, U), dtype=F32, device=dev)
    out_v = torch.empty((B, h, w, V), dtype=F32, device=dev)
    keep_s = keep_v = None
    if kp < 1.0:
        keep_s = torch.empty((M4, U), dtype=U8, device=dev)
        keep_v = torch.empty((M4, V), dtype=U8, device=dev)
    rc = _load().pcnn_neck_fwd(_lib.ptr(z4), _lib.ptr(z5), _lib.ptr(b4), _lib.ptr(b5), B, h, w, U, V, kp,
                               seed & ((1 << 64) - 1), _lib.ptr(step_dev), sids[0], sids[1], _lib.ptr(out_s),
                               _lib.ptr(out_v), _lib.ptr(keep_s), _lib.ptr(keep_v), _lib.stream_ptr(stream))
    _lib.check(rc, who)
    return out_s, out_v, keep_s, keep_v


def neck_bwd(d_add_score, d_add_score_vertex, keep_score, keep_vertex, z4, z5, b4, b5, relu_cols, keep_prob=1.0,
             stream=None):
    """The backward of neck_fwd (pcnn_neck_bwd) from the two incoming gradients
    (B,h,w,U) and (B,h,w,V), the forward's keep maps (None at keep_prob 1) and
    its inputs: (dz4 (B,h,w,N), dz5 (B,h/2,w/2,N), db4 (N), db5 (N)), the
    gradients of the GEMM outputs and of the biases.  Deterministic.  Two
    launches, no sync."""
    who = "neck_bwd"
    B, h, w, U, V = _maps(who, z4, z5, b4, b5, relu_cols)
    kp = _keep_prob(who, keep_prob)
    M4, N, dev = B * h * w, U + V, z4.device
    _lib.require(d_add_score, F32, (B, h, w, U), name=f"{who}: d_add_score")
    _lib.require(d_add_score_vertex, F32, (B, h, w, V), name=f"{who}: d_add_score_vertex")
    if kp < 1.0:
        _lib.require(keep_score, U8, (M4, U), name=f"{who}: keep_score")
        _lib.require(keep_vertex, U8, (M4, V), name=f"{who}: keep_vertex")
    else:
        keep_score = keep_vertex = None
    _same_device(who, z4, d_add_score=d_add_score, d_add_score_vertex=d_add_score_vertex, keep_score=keep_score,
                 keep_vertex=keep_vertex)
    dz4 = torch.empty((B, h, w, N), dtype=F32, device=dev)
    dz5 = torch.empty((B, h // 2, w // 2, N), dtype=F32, device=dev)
    db4 = torch.empty((N,), dtype=F32, device=dev)
    db5 = torch.empty((N,), dtype=F32, device=dev)
    lib = _load()
    need = lib.pcnn_neck_bwd_workspace_size(B, h, w, U, V)
    if need == 0:
        raise ValueError(f"{who}: unsupported shape {(B, h, w, U, V)}")
    ws = _lib.workspace(need, dev, "neck_bwd", stream)
    rc = lib.pcnn_neck_bwd(_lib.ptr(d_add_score), _lib.ptr(d_add_score_vertex), _lib.ptr(keep_score),
                           _lib.ptr(keep_vertex), _lib.ptr(z4), _lib.ptr(z5), _lib.ptr(b4), _lib.ptr(b5), B, h, w, U,
                           V, kp, _lib.ptr(dz4), _lib.ptr(dz5), _lib.ptr(db4), _lib.ptr(db5), _lib.ptr(ws), need,
                           _lib.stream_ptr(stream))
    _lib.check(rc, who)
    return dz4, dz5, db4, db5


def embedding(x4, x5, W4, b4, W5, b5, num_units, keep_prob=1.0, drop_gen=None, precision=2, stream=None):
    """The whole neck: x4 (B,h,w,K) = conv4_3 and x5 (B,h/2,w/2,K) = conv5_3,
    NHWC float32 with h and w even; W4, W5 (K,N) and b4, b5 (N), columns
    [0, num_units) the score branch.  Returns (add_score (B,h,w,num_units),
    add_score_vertex (B,h,w,N - num_units), ctx); ctx is what embedding_bwd
    needs.  Two pose_head.gemm calls at `precision` (x4 and x5 are each read
    once, for both branches), then neck_fwd.  drop_gen = (seed, step_dev,
    (stream_id_score, stream_id_vertex)); the ids default to STREAM_IDS."""
    who = "embedding"
    _lib.require(x4, F32, (None, None, None, None), name=f"{who}: x4")
    B, h, w, K = (int(s) for s in x4.shape)
    if B < 1 or h < 1 or w < 1 or h % 2 or w % 2:
        raise ValueError(f"{who}: x4: expected (B,h,w,K) with h and w even, got shape {tuple(x4.shape)}")
    if K < 1 or (precision != 0 and K % 4):
        raise ValueError(f"{who}: x4: expected a multiple of 4 channels, got {K}")
    _lib.require(x5, F32, (B, h // 2, w // 2, K), name=f"{who}: x5")
    _lib.require(W4, F32, (K, None), name=f"{who}: W4")
    N = int(W4.shape[1])
    U, V = int(num_units), N - int(num_units)
    if U < 0 or V < 0 or U % 4 or V % 4 or N == 0:
        raise ValueError(f"{who}: expected {U} score and {V} vertex columns to be multiples of 4, not both 0")
    if B * h * w * max(N, K) >= 1 << 31:
        raise ValueError(f"{who}: expected maps of fewer than 2^31 elements")
    _lib.require(W5, F32, (K, N), name=f"{who}: W5")
    _lib.require(b4, F32, (N,), name=f"{who}: b4")
    _lib.require(b5, F32, (N,), name=f"{who}: b5")
    kp = _keep_prob(who, keep_prob)
    _, step_dev, _ = _drop_gen(who, kp, drop_gen)
    _same_device(who, x4, x5=x5, W4=W4, W5=W5, b4=b4, b5=b5, step_dev=step_dev)
    M4, M5, dev = B * h * w, B * h * w // 4, x4.device
    z4 = torch.empty((B, h, w, N), dtype=F32, device=dev)
    z5 = torch.empty((B, h // 2, w // 2, N), dtype=F32, device=dev)
    pose_head.gemm(x4.view(M4, K), W4, z4.view(M4, N), precision=precision, stream=stream)
    pose_head.gemm(x5.view(M5, K), W5, z5.view(M5, N), precision=precision, stream=stream)
    out_s, out_v, keep_s, keep_v = neck_fwd(z4, z5, b4, b5, U, keep_prob=kp, drop_gen=drop_gen, stream=stream)
    ctx = dict(x4=x4, x5=x5, W4=W4, W5=W5, b4=b4, b5=b5, z4=z4, z5=z5, keep_score=keep_s, keep_vertex=keep_v,
               num_units=U, keep_prob=kp, precision=precision)
    return out_s, out_v, ctx


def embedding_bwd(ctx, d_add_score, d_add_score_vertex, want=BWD_OUTPUTS, stream=None):
    """The backward of `embedding` from the gradients of its two outputs:
    {name: gradient for name in want}, names from BWD_OUTPUTS.  neck_bwd, then
    through pose_head.gemm only what `want` names: d_x4 = dz4 W4^T,
    d_W4 = x4^T dz4, d_x5 = dz5 W5^T, d_W5 = x5^T dz5."""
    who = "embedding_bwd"
    unknown = [n for n in want if n not in BWD_OUTPUTS]
    if unknown or not want:
        raise ValueError(f"{who}: want must name at least one of {BWD_OUTPUTS}, got {tuple(want)}")
    x4, x5, W4, W5 = ctx["x4"], ctx["x5"], ctx["W4"], ctx["W5"]
    B, h, w, K = (int(s) for s in x4.shape)
    N = int(W4.shape[1])
    M4, M5, dev, prec = B * h * w, B * h * w // 4, x4.device, ctx["precision"]
    dz4, dz5, db4, db5 = neck_bwd(d_add_score, d_add_score_vertex, ctx["keep_score"], ctx["keep_vertex"], ctx["z4"],
                                  ctx["z5"], ctx["b4"], ctx["b5"], ctx["num_units"], keep_prob=ctx["keep_prob"],
                                  stream=stream)
    out = {}
    if "b4" in want:
        out["b4"] = db4
    if "b5" in want:
        out["b5"] = db5
    for tag, x, W, dz, M in (("4", x4, W4, dz4, M4), ("5", x5, W5, dz5, M5)):
        if "x" + tag in want:
            d_x = torch.empty_like(x)
            pose_head.gemm(dz.view(M, N), W, d_x.view(M, K), b_trans=1, precision=prec, stream=stream)
            out["x" + tag] = d_x
        if "W" + tag in want:
            d_W = torch.empty((K, N), dtype=F32, device=dev)
            pose_head.gemm(x.view(M, K), dz.view(M, N), d_W, a_trans=1, precision=prec, stream=stream)
            out["W" + tag] = d_W
    return out
