"""Pose head of vgg16_convs (lib/networks/vgg16_convs.py:186-200) on the HIP
MFMA GEMM: pool5 + pool4 -> fc6 (relu) -> fc7 (relu) -> fc8 -> tanh ->
* poses_weight -> l2_normalize, forward and backward, with every row count
read on the device (capacity-sized RoI buffers, no host sync).

Weights follow Network.fc (network.py:393-423): `weights` [in, out] with
truncated-normal(0, 0.001) init (network.py:415), `biases` [out] zero; the
reshape of the (R,7,7,512) pooled features is NHWC-flat ((h*7+w)*512+c).
drop6 / drop7 (vgg16_convs.py:189,191, tf.nn.dropout) are fused into the fc6 /
fc7 forward epilogues and the relu-mask epilogues of the backward (keep_prob
0.5 in training, train.py:421; 1, the identity, at test time).
"""
import torch

from . import _lib


def _operands(what, M, N, K, A, a_trans, B, b_trans, C, A2=None, bias=None, mask=None, drop=None, M_dev=None,
              K_dev=None):
    """The FC GEMM family's operand contract: fp32 device operands with unit
    inner stride that hold their rows (op(A) M x K, op(B) K x N, C / mask /
    drop M x N at their own row pitch), an N-element bias, int32 counters."""
    f32 = torch.float32
    ra = (K, M) if a_trans else (M, K)
    _lib.require(A, f32, contiguous=False, rows=ra, name=f"{what}: A")
    _lib.require(A2, f32, contiguous=False, rows=ra, name=f"{what}: A2", optional=True)
    if A2 is not None and A2.stride(0) != A.stride(0):
        raise ValueError(f"{what}: A2 must have A's row pitch {A.stride(0)}, got {A2.stride(0)}")
    _lib.require(B, f32, contiguous=False, rows=(N, K) if b_trans else (K, N), name=f"{what}: B")
    _lib.require(C, f32, contiguous=False, rows=(M, N), name=f"{what}: C")
    _lib.require(mask, f32, contiguous=False, rows=(M, N), name=f"{what}: mask", optional=True)
    _lib.require(drop, torch.uint8, contiguous=False, rows=(M, N), name=f"{what}: drop", optional=True)
    if bias is not None and _lib.require(bias, f32, name=f"{what}: bias").numel() < N:
        raise ValueError(f"{what}: bias must have {N} elements, got {bias.numel()}")
    _lib.require_counter(M_dev, f"{what}: M_dev")
    _lib.require_counter(K_dev, f"{what}: K_dev")


def _head_rows(what, R, D, num_rois, **mats):
    """Pose-head matrices: packed (R, D) fp32 device rows, an int32 row counter."""
    for name, t in mats.items():
        _lib.require(t, torch.float32, shape=(R, D), name=f"{what}: {name}")
    _lib.require_counter(num_rois, f"{what}: num_rois")


def gemm(A, B, C, a_trans=0, b_trans=0, A2=None, bias=None, act=0, mask=None, M_dev=None, K_dev=None, M=None,
         N=None, K=None, precision=2, drop=None, keep_prob=1.0, drop_gen=None, stream=None, checked=True):
    """C[M,N] = epilogue(op(A) (+ op(A2)) @ op(B)); see pcnn_gemm / pcnn_gemm_drop in
    include/posecnn_hip.h.  drop (uint8 (M, >=N) 0/1) applies tf.nn.dropout after
    the activation, (v / keep_prob) * drop; with mask, keep_prob scales the kept
    gradient (v / keep_prob: the backward of relu + dropout).  drop_gen =
    (seed, step_dev, stream_id): the reduce draws the keep bits itself (as
    dropout_mask would) and writes them into drop (pcnn_gemm_drop_gen)."""
    _lib.require_gpu(A, B, C)
    if A.dim() != 2 or B.dim() != 2:
        raise ValueError("gemm: A and B must be 2-dimensional")
    if M is None:
        M = A.shape[1] if a_trans else A.shape[0]
    if K is None:
        K = A.shape[0] if a_trans else A.shape[1]
    if N is None:
        N = B.shape[0] if b_trans else B.shape[1]
    if checked:
        _operands("gemm", M, N, K, A, a_trans, B, b_trans, C, A2=A2, bias=bias, mask=mask, drop=drop, M_dev=M_dev,
                  K_dev=K_dev)
        if drop_gen is not None:
            _lib.require_counter(drop_gen[1], "gemm: drop_gen's step counter", torch.int64)
    lib = _lib.load()
    ws = _lib.workspace(lib.pcnn_gemm_workspace_size(M, N, K, int(M_dev is not None), precision), C.device, "gemm",
                        stream)
    if drop_gen is not None:
        if drop is None or mask is not None:
            raise ValueError("gemm: drop_gen needs the drop output buffer and no mask (forward only)")
        seed, step_dev, sid = drop_gen
        rc = lib.pcnn_gemm_drop_gen(M, N, K, _lib.ptr(A), _lib.ptr(A2), A.stride(0), int(a_trans), _lib.ptr(B),
                                    B.stride(0), int(b_trans), _lib.ptr(C), C.stride(0), _lib.ptr(bias), int(act),
                                    _lib.ptr(drop), drop.stride(0), float(keep_prob), int(seed) & ((1 << 64) - 1),
                                    _lib.ptr(step_dev), int(sid), _lib.ptr(M_dev), _lib.ptr(K_dev), int(precision),
                                    _lib.ptr(ws), ws.numel(), _lib.stream_ptr(stream))
    elif drop is None and keep_prob == 1.0:
        rc = lib.pcnn_gemm(M, N, K, _lib.ptr(A), _lib.ptr(A2), A.stride(0), int(a_trans), _lib.ptr(B), B.stride(0),
                           int(b_trans), _lib.ptr(C), C.stride(0), _lib.ptr(bias), int(act), _lib.ptr(mask),
                           mask.stride(0) if mask is not None else 0, _lib.ptr(M_dev), _lib.ptr(K_dev),
                           int(precision), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(stream))
    else:
        rc = lib.pcnn_gemm_drop(M, N, K, _lib.ptr(A), _lib.ptr(A2), A.stride(0), int(a_trans), _lib.ptr(B),
                                B.stride(0), int(b_trans), _lib.ptr(C), C.stride(0), _lib.ptr(bias), int(act),
                                _lib.ptr(mask), mask.stride(0) if mask is not None else 0, _lib.ptr(drop),
                                drop.stride(0) if drop is not None else 0, float(keep_prob), _lib.ptr(M_dev),
                                _lib.ptr(K_dev), int(precision), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(stream))
    _lib.check(rc, "gemm")
    return C


def tp_bytes(rows, K):
    """Bytes of the tiled three-plane (hi / mid / lo bf16) form of a rows x K operand."""
    return int(_lib.load().pcnn_tp_bytes(int(rows), int(K)))


def split_tp(src, rows, K, out, row_stride, k_stride, rows_dev=None, K_dev=None, stream=None):
    """out (uint8, >= tp_bytes(rows, K)) <- the tiled planes of the fp32 view
    src[row * row_stride + k * k_stride] (zeros past rows_dev / K_dev); see
    pcnn_split_tp in include/posecnn_hip.h."""
    _lib.require_gpu(src, out)
    if src.dtype != torch.float32 or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError("split_tp: fp32 source, contiguous uint8 destination")
    _lib.require_counter(rows_dev, "split_tp: rows_dev")
    _lib.require_counter(K_dev, "split_tp: K_dev")
    span = (int(rows) - 1) * int(row_stride) + (int(K) - 1) * int(k_stride) + 1
    if rows > 0 and K > 0 and (min(int(row_stride), int(k_stride)) < 0 or src.numel() < span or
                               not src.is_contiguous()):
        raise ValueError(f"split_tp: src must be a contiguous buffer of at least {span} elements")
    need = tp_bytes(rows, K)
    if out.numel() < need:
        raise ValueError(f"split_tp: out must hold tp_bytes(rows, K) = {need} bytes, got {out.numel()}")
    rc = _lib.load().pcnn_split_tp(_lib.ptr(src), int(row_stride), int(k_stride), int(rows), _lib.ptr(rows_dev),
                                   int(K), _lib.ptr(K_dev), _lib.ptr(out), out.numel(), _lib.stream_ptr(stream))
    _lib.check(rc, "split_tp")
    return out


def gemm_tp(A_tp, B_tp, C, M, N, K, bias=None, act=0, mask=None, drop=None, keep_prob=1.0, M_dev=None, K_dev=None,
            stream=None):
    """C[M,N] = epilogue(A @ B) from the tiled planes of op(A) (M x K) and of
    op(B)^T (N x K) (split_tp); bit-identical to gemm(..., precision=2)."""
    _lib.require_gpu(A_tp, B_tp, C)
    u8, f32 = torch.uint8, torch.float32
    for name, t, rows in (("A_tp", A_tp, M), ("B_tp", B_tp, N)):
        need = tp_bytes(rows, K)
        if _lib.require(t, u8, name=f"gemm_tp: {name}").numel() < need:
            raise ValueError(f"gemm_tp: {name} must hold tp_bytes({rows}, {K}) = {need} bytes, got {t.numel()}")
    _lib.require(C, f32, contiguous=False, rows=(M, N), name="gemm_tp: C")
    _lib.require(mask, f32, contiguous=False, rows=(M, N), name="gemm_tp: mask", optional=True)
    _lib.require(drop, u8, contiguous=False, rows=(M, N), name="gemm_tp: drop", optional=True)
    if bias is not None and _lib.require(bias, f32, name="gemm_tp: bias").numel() < N:
        raise ValueError(f"gemm_tp: bias must have {N} elements, got {bias.numel()}")
    _lib.require_counter(M_dev, "gemm_tp: M_dev")
    _lib.require_counter(K_dev, "gemm_tp: K_dev")
    lib = _lib.load()
    ws = _lib.workspace(lib.pcnn_gemm_workspace_size(M, N, K, int(M_dev is not None), 2), C.device, "gemm", stream)
    rc = lib.pcnn_gemm_tp(int(M), int(N), int(K), _lib.ptr(A_tp), _lib.ptr(B_tp), _lib.ptr(C), C.stride(0),
                          _lib.ptr(bias), int(act), _lib.ptr(mask), mask.stride(0) if mask is not None else 0,
                          _lib.ptr(drop), drop.stride(0) if drop is not None else 0, float(keep_prob),
                          _lib.ptr(M_dev), _lib.ptr(K_dev), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(stream))
    _lib.check(rc, "gemm_tp")
    return C


def dropout_mask(mask, keep_prob, seed, step_dev=None, stream_id=0, rows_dev=None, stream=None):
    """The binary tensor of tf.nn.dropout, floor(keep_prob + U[0,1)), into the
    uint8 (rows, cols) `mask` (Philox4x32-10 keyed on seed, the device step
    counter step_dev (int64 (1,)) and stream_id; rows past *rows_dev untouched)."""
    _lib.require_gpu(mask)
    if mask.dtype != torch.uint8 or mask.dim() != 2 or mask.stride(1) != 1:
        raise ValueError("dropout_mask: uint8 (rows, cols) mask with unit inner stride")
    _lib.require_counter(step_dev, "dropout_mask: step_dev", torch.int64)
    _lib.require_counter(rows_dev, "dropout_mask: rows_dev")
    rc = _lib.load().pcnn_dropout_mask(_lib.ptr(mask), mask.shape[0], mask.shape[1], mask.stride(0),
                                       _lib.ptr(rows_dev), int(seed) & ((1 << 64) - 1), _lib.ptr(step_dev),
                                       int(stream_id), float(keep_prob), _lib.stream_ptr(stream))
    _lib.check(rc, "dropout_mask")
    return mask


def colsum(X, out, M_dev=None, stream=None, checked=True):
    """out (N) = the column sums of the first min(*M_dev, M) rows of X (M, N) (pcnn_colsum)."""
    _lib.require_gpu(X, out)
    if X is None or X.dim() != 2:
        raise ValueError("colsum: X must be a 2-dimensional (M, N) tensor")
    if checked:
        _lib.require(X, torch.float32, contiguous=False, rows=tuple(X.shape), name="colsum: X")
        _lib.require(out, torch.float32, shape=(X.shape[1],), name="colsum: out")
        _lib.require_counter(M_dev, "colsum: M_dev")
    rc = _lib.load().pcnn_colsum(_lib.ptr(X), X.shape[0], X.shape[1], X.stride(0), _lib.ptr(M_dev), _lib.ptr(out),
                                 _lib.stream_ptr(stream))
    _lib.check(rc, "colsum")
    return out


def head_fwd(y8, poses_weight, tanh_out, pred, num_rois=None, stream=None, checked=True):
    _lib.require_gpu(y8, poses_weight, tanh_out, pred)
    if y8.dim() != 2:
        raise ValueError("head_fwd: y8 must be a 2-dimensional (R, D) tensor")
    R, D = y8.shape
    if checked:
        _head_rows("head_fwd", R, D, num_rois, y8=y8, poses_weight=poses_weight, tanh_out=tanh_out, pred=pred)
    rc = _lib.load().pcnn_pose_head_fwd(_lib.ptr(y8), _lib.ptr(poses_weight), R, _lib.ptr(num_rois), D,
                                        _lib.ptr(tanh_out), _lib.ptr(pred), _lib.stream_ptr(stream))
    _lib.check(rc, "pose_head_fwd")


FC8_FUSED_MAX_D = 128  # columns the fused fc8 kernels take (one wave per 32-column block)


def fc8_fused_ok(units, D, precision=2):
    """Whether the fc8 kernels fused into the split-K reduces (fc8_fused.hip)
    take this shape; otherwise the chain runs as gemm / gemm / head_fwd."""
    return precision == 2 and 0 < D <= FC8_FUSED_MAX_D and units % 4 == 0


def gemm_partial(A, B, C, bias=None, act=0, M_dev=None, precision=2, stream=None, checked=True):
    """gemm()'s GEMM kernel without the reduce pass after it (pcnn_gemm_partial):
    the split-K partial slabs stay in the stream's GEMM workspace, which is
    returned for fc8_fwd_fused."""
    _lib.require_gpu(A, B, C)
    if A.dim() != 2 or B.dim() != 2:
        raise ValueError("gemm_partial: A (M, K) and B (K, N) must be 2-dimensional")
    M, K = A.shape
    N = B.shape[1]
    if checked:
        _operands("gemm_partial", M, N, K, A, 0, B, 0, C, bias=bias, M_dev=M_dev)
    lib = _lib.load()
    ws = _lib.workspace(lib.pcnn_gemm_workspace_size(M, N, K, int(M_dev is not None), precision), C.device, "gemm",
                        stream)
    rc = lib.pcnn_gemm_partial(M, N, K, _lib.ptr(A), None, A.stride(0), 0, _lib.ptr(B), B.stride(0), 0, _lib.ptr(C),
                               C.stride(0), _lib.ptr(bias), int(act), _lib.ptr(M_dev), None, int(precision),
                               _lib.ptr(ws), ws.numel(), _lib.stream_ptr(stream))
    _lib.check(rc, "gemm_partial")
    return ws


def _fc8_workspace(M, D, K, M_dev, device, stream):
    nbytes = max(_lib.load().pcnn_gemm_workspace_size(M, D, K, int(M_dev is not None), 2), M * D * 4)
    return _lib.workspace(nbytes, device, "fc8", stream)


def fc8_fwd_fused(fc7_ws, K7, b7, y7, W8, act=1, drop=None, keep_prob=1.0, drop_gen=None, M_dev=None, stream=None,
                  checked=True):
    """After gemm_partial (the fc7 forward, workspace fc7_ws, contraction K7):
    y7 = dropout(act(slab sum + b7)) formed while it is staged as the A operand
    of y7 @ W8; fc8's split-K partials stay in the stream's fc8 workspace for
    fc8_reduce_head_fwd (pcnn_fc8_fwd_fused).  drop / keep_prob / drop_gen as gemm()."""
    _lib.require_gpu(fc7_ws, y7, W8)
    f32 = torch.float32
    if y7.dim() != 2 or W8.dim() != 2:
        raise ValueError("fc8_fwd_fused: y7 (M, N7) and W8 (N7, D) must be 2-dimensional")
    M, N7 = y7.shape
    D = W8.shape[1]
    seed, step_dev, sid = drop_gen if drop_gen is not None else (0, None, 0)
    if checked:
        _lib.require(fc7_ws, torch.uint8, name="fc8_fwd_fused: fc7_ws")
        _lib.require(y7, f32, contiguous=False, rows=(M, N7), name="fc8_fwd_fused: y7")
        _lib.require(W8, f32, contiguous=False, rows=(N7, D), name="fc8_fwd_fused: W8")
        _lib.require(drop, torch.uint8, contiguous=False, rows=(M, N7), name="fc8_fwd_fused: drop", optional=True)
        if b7 is not None and _lib.require(b7, f32, name="fc8_fwd_fused: b7").numel() < N7:
            raise ValueError(f"fc8_fwd_fused: b7 must have {N7} elements, got {b7.numel()}")
        _lib.require_counter(M_dev, "fc8_fwd_fused: M_dev")
        _lib.require_counter(step_dev, "fc8_fwd_fused: drop_gen's step counter", torch.int64)
    ws8 = _fc8_workspace(M, D, N7, M_dev, y7.device, stream)
    rc = _lib.load().pcnn_fc8_fwd_fused(M, N7, int(K7), _lib.ptr(fc7_ws), fc7_ws.numel(), _lib.ptr(b7), int(act),
                                        _lib.ptr(y7), y7.stride(0), _lib.ptr(drop),
                                        drop.stride(0) if drop is not None else 0, float(keep_prob),
                                        int(drop_gen is not None), int(seed) & ((1 << 64) - 1), _lib.ptr(step_dev),
                                        int(sid), _lib.ptr(W8), W8.stride(0), D, _lib.ptr(M_dev), _lib.ptr(ws8),
                                        ws8.numel(), _lib.stream_ptr(stream))
    _lib.check(rc, "fc8_fwd_fused")


def fc8_reduce_head_fwd(b8, K, poses_weight, y8, tanh_out, pred, num_rois=None, stream=None, checked=True):
    """y8 = fc8's split-K partials (left by fc8_fwd_fused on this stream) in
    slice order + b8, and head_fwd on it, in one row pass (pcnn_fc8_reduce_head_fwd)."""
    _lib.require_gpu(b8, poses_weight, y8, tanh_out, pred)
    if y8.dim() != 2:
        raise ValueError("fc8_reduce_head_fwd: y8 must be a 2-dimensional (R, D) tensor")
    R, D = y8.shape
    if checked:
        _head_rows("fc8_reduce_head_fwd", R, D, num_rois, poses_weight=poses_weight, y8=y8, tanh_out=tanh_out,
                   pred=pred)
        if b8 is not None and _lib.require(b8, torch.float32, name="fc8_reduce_head_fwd: b8").numel() < D:
            raise ValueError(f"fc8_reduce_head_fwd: b8 must have {D} elements, got {b8.numel()}")
    ws8 = _fc8_workspace(R, D, K, num_rois, y8.device, stream)
    rc = _lib.load().pcnn_fc8_reduce_head_fwd(_lib.ptr(ws8), ws8.numel(), _lib.ptr(b8), R, int(K), D,
                                              _lib.ptr(num_rois), _lib.ptr(poses_weight), _lib.ptr(y8),
                                              _lib.ptr(tanh_out), _lib.ptr(pred), _lib.stream_ptr(stream))
    _lib.check(rc, "fc8_reduce_head_fwd")


def fc8_dx(dy8, W8, dy7, mask=None, keep_prob=1.0, M_dev=None, precision=2, stream=None, checked=True):
    """dy7 = (mask > 0 ? dy8 @ W8^T : 0) / keep_prob: the skinny kernel
    (pcnn_fc8_dx_skinny) where it applies, else gemm(b_trans=1); the same bits."""
    if W8.dim() != 2 or dy8.dim() != 2:
        raise ValueError("fc8_dx: dy8 (M, D) and W8 (N7, D) must be 2-dimensional")
    D = W8.shape[1]
    if not (fc8_fused_ok(W8.shape[0], D, precision) and D % 4 == 0):
        return gemm(dy8, W8, dy7, b_trans=1, mask=mask, M_dev=M_dev, precision=precision, keep_prob=keep_prob,
                    stream=stream, checked=checked)
    _lib.require_gpu(dy8, W8, dy7, mask)
    if checked:
        M, N7 = dy8.shape[0], W8.shape[0]
        _lib.require(dy8, torch.float32, contiguous=False, rows=(M, D), name="fc8_dx: dy8")
        _lib.require(W8, torch.float32, contiguous=False, rows=(N7, D), name="fc8_dx: W8")
        _lib.require(dy7, torch.float32, contiguous=False, rows=(M, N7), name="fc8_dx: dy7")
        _lib.require(mask, torch.float32, contiguous=False, rows=(M, N7), name="fc8_dx: mask", optional=True)
        _lib.require_counter(M_dev, "fc8_dx: M_dev")
    rc = _lib.load().pcnn_fc8_dx_skinny(_lib.ptr(dy8), dy8.stride(0), _lib.ptr(W8), W8.stride(0), _lib.ptr(mask),
                                        mask.stride(0) if mask is not None else 0, float(keep_prob), _lib.ptr(dy7),
                                        dy7.stride(0), dy8.shape[0], D, W8.shape[0], _lib.ptr(M_dev),
                                        _lib.stream_ptr(stream))
    _lib.check(rc, "fc8_dx_skinny")
    return dy7


def fc7_fc8_head_fwd(y6, w7, b7, y7, w8, b8, y8, poses_weight, tanh_out, pred, drop=None, keep_prob=1.0,
                     drop_gen=None, M_dev=None, precision=2, fuse=True, stream=None):
    """fc7 (relu, dropout) -> fc8 -> pose head forward.  4C <= 128 columns at
    precision 2: the fc7 GEMM, then two launches (fc8_fwd_fused,
    fc8_reduce_head_fwd); otherwise gemm, gemm, head_fwd -- the same bits."""
    # the whole chain's arguments, once, before its first launch; the primitives then run unchecked
    what = "fc7_fc8_head_fwd"
    _lib.require_gpu(y6, w7, b7, y7, w8, b8, y8, poses_weight, tanh_out, pred)
    if y6.dim() != 2 or w7.dim() != 2 or w8.dim() != 2:
        raise ValueError(f"{what}: y6 (M, K), w7 (K, N7) and w8 (N7, D) must be 2-dimensional")
    (M, K), N7, D = y6.shape, w7.shape[1], w8.shape[1]
    _operands(f"{what} (fc7)", M, N7, K, y6, 0, w7, 0, y7, bias=b7, drop=drop, M_dev=M_dev)
    _operands(f"{what} (fc8)", M, D, N7, y7, 0, w8, 0, y8, bias=b8)
    _head_rows(what, M, D, None, poses_weight=poses_weight, y8=y8, tanh_out=tanh_out, pred=pred)
    if drop_gen is not None:
        _lib.require_counter(drop_gen[1], f"{what}: drop_gen's step counter", torch.int64)
    kw = dict(M_dev=M_dev, stream=stream, checked=False)
    dk = dict(keep_prob=keep_prob) if keep_prob < 1.0 else {}
    if fuse and fc8_fused_ok(w7.shape[1], w8.shape[1], precision):
        ws7 = gemm_partial(y6, w7, y7, bias=b7, act=1, precision=precision, **kw)
        fc8_fwd_fused(ws7, w7.shape[0], b7, y7, w8, act=1, drop=drop, drop_gen=drop_gen, **kw, **dk)
        fc8_reduce_head_fwd(b8, w8.shape[0], poses_weight, y8, tanh_out, pred, num_rois=M_dev, stream=stream,
                            checked=False)
        return
    gemm(y6, w7, y7, bias=b7, act=1, drop=drop, drop_gen=drop_gen, precision=precision, **kw, **dk)
    gemm(y7, w8, y8, bias=b8, act=0, precision=precision, **kw)
    head_fwd(y8, poses_weight, tanh_out, pred, num_rois=M_dev, stream=stream, checked=False)


def head_bwd(d_pred, tanh_out, poses_weight, pred, d_y8, num_rois=None, d_pred_scale=None, stream=None,
             checked=True):
    """d_y8 from d_pred; with d_pred_scale (device scalar) d_pred is taken as
    d_pred_scale[0] * d_pred -- the ADD-loss gradient op folded into this pass."""
    _lib.require_gpu(d_pred, tanh_out, poses_weight, pred, d_y8)
    if d_pred.dim() != 2:
        raise ValueError("head_bwd: d_pred must be a 2-dimensional (R, D) tensor")
    R, D = d_pred.shape
    if checked:
        _head_rows("head_bwd", R, D, num_rois, d_pred=d_pred, tanh_out=tanh_out, poses_weight=poses_weight,
                   pred=pred, d_y8=d_y8)
        if d_pred_scale is not None and _lib.require(d_pred_scale, torch.float32,
                                                     name="head_bwd: d_pred_scale").numel() < 1:
            raise ValueError("head_bwd: d_pred_scale needs one element")
    rc = _lib.load().pcnn_pose_head_bwd(_lib.ptr(d_pred), _lib.ptr(d_pred_scale), _lib.ptr(tanh_out),
                                        _lib.ptr(poses_weight), _lib.ptr(pred), R, _lib.ptr(num_rois), D,
                                        _lib.ptr(d_y8), _lib.stream_ptr(stream))
    _lib.check(rc, "pose_head_bwd")


def truncated_normal(shape, std, generator, device):
    t = torch.empty(shape, dtype=torch.float32, device=device)
    torch.nn.init.trunc_normal_(t, 0.0, std, -2 * std, 2 * std, generator=generator)
    return t


class PoseHeadWeights:
    """fc6 / fc7 / fc8 variables of the pose head (vgg16_convs.py:186-192)."""

    def __init__(self, num_classes, device, in_dim=7 * 7 * 512, units=4096, seed=0):
        g = torch.Generator(device=device)
        g.manual_seed(seed)
        D = 4 * num_classes
        self.w6 = truncated_normal((in_dim, units), 0.001, g, device)
        self.b6 = torch.zeros(units, device=device)
        self.w7 = truncated_normal((units, units), 0.001, g, device)
        self.b7 = torch.zeros(units, device=device)
        self.w8 = truncated_normal((units, D), 0.001, g, device)
        self.b8 = torch.zeros(D, device=device)
        self.in_dim, self.units, self.D = in_dim, units, D

    def grads_like(self):
        return {k: torch.empty_like(getattr(self, k)) for k in ("w6", "b6", "w7", "b7", "w8", "b8")}
