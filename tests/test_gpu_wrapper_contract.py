"""Every public op wrapper under the ABI guard (tests/abi_guard.py).

All device work goes through ctypes with raw pointers and a few ints, so a
wrapper that forwards a mistyped or strided tensor gives no error: it gives a
wrong number, or a write past a buffer.  Here each wrapper runs with the guard
installed at the boundary, on the smallest shapes at which layout still
matters (R_cap = 5 with a device count of 3, C = 3 / D = 12, 16 x 24 x 8 maps,
P = 64 model points, 64-unit GEMMs plus a ragged 37 x 20 x 52 through padded
leading dimensions, 48 x 64 frames for the vote):

 (a) canonical inputs: the guard is silent and the case's entry points were reached;
 (b) every tensor input, one at a time, as float64 / int64, as a
     non-contiguous view, as a contiguous view at a 16-byte storage offset and
     as a CPU tensor -- device counters included: either the wrapper raises
     ValueError / TypeError before any launch, or the call completes with the
     guard silent and the outputs of (a), bit for bit;
 (c) every caller-supplied output or in-place buffer with a wrong dtype, as a
     non-contiguous view and one row short: ValueError before any launch.

The guard refuses before forwarding, so no malformed call reaches a kernel; an
AbiContractError (an AssertionError) always fails the test.  The coverage
meta-test (no GPU) keeps the case table complete over the binding.
"""
from collections import namedtuple

import numpy as np
import pytest
import torch

import abi_guard as ag
from posecnn_amd import _lib, label_2d, losses, synth, upscore as up, vertex_pred as vp
from posecnn_amd import pose_head as ph
from posecnn_amd.average_distance_loss import average_distance_loss_op as adl
from posecnn_amd.backprojecting_layer import backprojecting_op as bp
from posecnn_amd.hard_label_layer import hard_label_op as hl
from posecnn_amd.hough_voting_gpu_layer import hough_voting_gpu_op as hv
from posecnn_amd.roi_pooling_layer import roi_pooling_op as rp
from posecnn_amd.utils import nms as dn

DEV = "cuda"
R, NR, C, P = 5, 3, 3, 64          # RoI capacity, live rows (device count), classes, model points
D = 4 * C
H, W, CH = 16, 24, 8               # feature maps
U = 64                             # FC units
F32, I32, I64, U8 = torch.float32, torch.int32, torch.int64, torch.uint8

# name, build() -> {argument: value}, call(args) -> output tensors, symbols it must reach,
# outputs: the caller-supplied output / in-place buffers among the arguments,
# skip: {(argument, variant): reason} for a variant that changes what the argument means
# tier: "A" gets (a), (b) and (c); "B" (the refinement / rendering wrappers) (a) and the dtype and
# CPU-tensor variants of (b); wrapper: the public callable(s) the case is about (the coverage meta-test)
Case = namedtuple("Case", "name build call symbols outputs skip tier wrapper")
CASES = []


def case(name, symbols, outputs=(), skip=None, tier="A", wrapper=None):
    def deco(fn):
        build, call = fn()
        CASES.append(Case(name, build, call, tuple(symbols), tuple(outputs), dict(skip or {}), tier,
                          tuple([wrapper] if isinstance(wrapper, str) else wrapper or [name])))
        return fn
    return deco


# ------------------------------------------------------------------ builders' helpers
def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(1000 + seed)
    return (torch.randn(shape, generator=g) * scale).to(DEV)


def uni(*shape, seed=0, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(2000 + seed)
    return (torch.rand(shape, generator=g) * (hi - lo) + lo).to(DEV)


def zeros(*shape, dtype=F32):
    return torch.zeros(shape, dtype=dtype, device=DEV)


def count(n, dtype=I32):
    return torch.tensor([n], dtype=dtype, device=DEV)


def padded(x, pad=4):
    """x as the [:, :n] view of a buffer whose rows are `pad` elements wider."""
    buf = torch.zeros((x.shape[0], x.shape[1] + pad), dtype=x.dtype, device=x.device)
    buf[:, :x.shape[1]] = x
    return buf[:, :x.shape[1]]


def rois(n=R, scale=16.0, seed=0):
    """n rows [b, cls, x1, y1, x2, y2, score] inside the H x W map at 1/scale."""
    g = torch.Generator().manual_seed(3000 + seed)
    x1 = torch.rand(n, generator=g) * (W * scale * 0.5)
    y1 = torch.rand(n, generator=g) * (H * scale * 0.5)
    w = torch.rand(n, generator=g) * (W * scale * 0.4) + scale
    h = torch.rand(n, generator=g) * (H * scale * 0.4) + scale
    cls = torch.arange(n) % (C - 1) + 1
    score = torch.rand(n, generator=g)
    return torch.stack([torch.zeros(n), cls.float(), x1, y1, x1 + w, y1 + h, score], 1).to(DEV)


def head_weight():
    """(R, D) pose weights as the vote writes them: ones in the four columns of each row's class."""
    w = torch.zeros((R, D))
    for r in range(R):
        c = 1 + r % (C - 1)
        w[r, 4 * c:4 * c + 4] = 1.0
    return w.to(DEV)


def labels(*shape, seed=0, lo=0, hi=C):
    g = torch.Generator().manual_seed(4000 + seed)
    return torch.randint(lo, hi, shape, generator=g, dtype=torch.int32).to(DEV)


# ------------------------------------------------------------------ pose_head.py
@case("gemm", ["pcnn_gemm"], outputs=["C"])
def _():
    def build():
        return dict(A=rnd(U, U, seed=1), A2=rnd(U, U, seed=2), B=rnd(U, U, seed=3), bias=rnd(U, seed=4),
                    mask=rnd(U, U, seed=5), M_dev=count(40), C=zeros(U, U))
    return build, lambda a: ph.gemm(a["A"], a["B"], a["C"], A2=a["A2"], bias=a["bias"], act=1, mask=a["mask"],
                                    M_dev=a["M_dev"])


@case("gemm_weight_grad", ["pcnn_gemm"], outputs=["C"])
def _():
    def build():  # C = A^T B over the first *K_dev rows, exact fp32 MFMA
        return dict(A=rnd(U, U, seed=6), B=rnd(U, U, seed=7), K_dev=count(40), C=zeros(U, U))
    return build, lambda a: ph.gemm(a["A"], a["B"], a["C"], a_trans=1, K_dev=a["K_dev"], M=U, N=U, K=U, precision=0)


@case("gemm_ragged", ["pcnn_gemm"], outputs=["C"])
def _():
    M, N, K = 37, 20, 52

    def build():  # no multiple of 4 or of a tile, through padded leading dimensions
        return dict(A=padded(rnd(M, K, seed=8)), B=padded(rnd(N, K, seed=9)), bias=rnd(N, seed=10),
                    C=padded(zeros(M, N)))
    return build, lambda a: ph.gemm(a["A"], a["B"], a["C"], b_trans=1, bias=a["bias"], M=M, N=N, K=K)


@case("gemm_drop", ["pcnn_gemm_drop"], outputs=["C"])
def _():
    def build():
        return dict(A=rnd(U, U, seed=11), B=rnd(U, U, seed=12), bias=rnd(U, seed=13),
                    drop=(uni(U, U, seed=14) < 0.5).to(U8), M_dev=count(40), C=zeros(U, U))
    return build, lambda a: ph.gemm(a["A"], a["B"], a["C"], bias=a["bias"], act=1, drop=a["drop"], keep_prob=0.5,
                                    M_dev=a["M_dev"])


@case("gemm_drop_gen", ["pcnn_gemm_drop_gen"], outputs=["C", "drop"])
def _():
    def build():
        return dict(A=rnd(U, U, seed=15), B=rnd(U, U, seed=16), bias=rnd(U, seed=17), drop=zeros(U, U, dtype=U8),
                    step_dev=count(7, I64), M_dev=count(40), C=zeros(U, U))

    def call(a):
        ph.gemm(a["A"], a["B"], a["C"], bias=a["bias"], act=1, drop=a["drop"], keep_prob=0.5,
                drop_gen=(0x5EED, a["step_dev"], 6), M_dev=a["M_dev"])
        return a["C"], a["drop"]
    return build, call


@case("split_tp", ["pcnn_split_tp", "pcnn_tp_bytes"], outputs=["out"])
def _():
    def build():
        return dict(src=rnd(U, U, seed=18), rows_dev=count(40), K_dev=count(50),
                    out=zeros(ph.tp_bytes(U, U), dtype=U8))
    return build, lambda a: ph.split_tp(a["src"], U, U, a["out"], U, 1, rows_dev=a["rows_dev"], K_dev=a["K_dev"])


@case("gemm_tp", ["pcnn_gemm_tp"], outputs=["C"])
def _():
    def build():
        A, B = rnd(U, U, seed=19), rnd(U, U, seed=20)
        A_tp, B_tp = (zeros(ph.tp_bytes(U, U), dtype=U8) for _ in range(2))
        ph.split_tp(A, U, U, A_tp, U, 1)
        ph.split_tp(B, U, U, B_tp, 1, U)  # op(B)^T: row n, element k = B[k, n]
        return dict(A_tp=A_tp, B_tp=B_tp, bias=rnd(U, seed=21), mask=rnd(U, U, seed=22), M_dev=count(40),
                    K_dev=count(50), C=zeros(U, U))
    return build, lambda a: ph.gemm_tp(a["A_tp"], a["B_tp"], a["C"], U, U, U, bias=a["bias"], mask=a["mask"],
                                       M_dev=a["M_dev"], K_dev=a["K_dev"])


@case("dropout_mask", ["pcnn_dropout_mask"], outputs=["mask"])
def _():
    def build():
        return dict(mask=zeros(R, U, dtype=U8), step_dev=count(3, I64), rows_dev=count(NR))
    return build, lambda a: ph.dropout_mask(a["mask"], 0.5, 0x5EED, a["step_dev"], 6, rows_dev=a["rows_dev"])


@case("colsum", ["pcnn_colsum"], outputs=["out"])
def _():
    def build():
        return dict(X=rnd(R, U, seed=24), M_dev=count(NR), out=zeros(U))
    return build, lambda a: ph.colsum(a["X"], a["out"], M_dev=a["M_dev"])


@case("colsum_padded", ["pcnn_colsum"], outputs=["out"])
def _():
    def build():
        return dict(X=padded(rnd(R, 37, seed=25)), out=zeros(37))
    return build, lambda a: ph.colsum(a["X"], a["out"])


def _head_fwd_args():
    return dict(y8=rnd(R, D, seed=26), poses_weight=head_weight(), num_rois=count(NR), tanh_out=zeros(R, D),
                pred=zeros(R, D))


@case("head_fwd", ["pcnn_pose_head_fwd"], outputs=["tanh_out", "pred"])
def _():
    def call(a):
        ph.head_fwd(a["y8"], a["poses_weight"], a["tanh_out"], a["pred"], num_rois=a["num_rois"])
        return a["tanh_out"], a["pred"]
    return _head_fwd_args, call


def _head_state():
    """A pose head after its forward: y8, weights, tanh_out and pred of R rows."""
    a = _head_fwd_args()
    ph.head_fwd(a["y8"], a["poses_weight"], a["tanh_out"], a["pred"], num_rois=a["num_rois"])
    return a


@case("head_bwd", ["pcnn_pose_head_bwd"], outputs=["d_y8"])
def _():
    def build():
        s = _head_state()
        return dict(d_pred=rnd(R, D, seed=27), tanh_out=s["tanh_out"], poses_weight=s["poses_weight"],
                    pred=s["pred"], num_rois=s["num_rois"], d_pred_scale=count(1).float() * 0.5, d_y8=zeros(R, D))

    def call(a):
        ph.head_bwd(a["d_pred"], a["tanh_out"], a["poses_weight"], a["pred"], a["d_y8"], num_rois=a["num_rois"],
                    d_pred_scale=a["d_pred_scale"])
        return a["d_y8"]
    return build, call


@case("head_bwd_unscaled", ["pcnn_pose_head_bwd"], outputs=["d_y8"], wrapper="head_bwd")
def _():
    def build():  # d_pred as given: no d_pred_scale, every row
        s = _head_state()
        return dict(d_pred=rnd(R, D, seed=27), tanh_out=s["tanh_out"], poses_weight=s["poses_weight"],
                    pred=s["pred"], d_y8=zeros(R, D))

    def call(a):
        ph.head_bwd(a["d_pred"], a["tanh_out"], a["poses_weight"], a["pred"], a["d_y8"])
        return a["d_y8"]
    return build, call


def _fc_args():
    return dict(y6=rnd(R, U, seed=28), w7=rnd(U, U, seed=29, scale=0.1), b7=rnd(U, seed=30, scale=0.1),
                w8=rnd(U, D, seed=31, scale=0.1), b8=rnd(D, seed=32, scale=0.1), poses_weight=head_weight(),
                M_dev=count(NR), y7=zeros(R, U), y8=zeros(R, D), tanh_out=zeros(R, D), pred=zeros(R, D),
                drop=(uni(R, U, seed=33) < 0.5).to(U8))


_FC_OUT = ("y7", "y8", "tanh_out", "pred")


def _fc_chain(fuse):
    def call(a):
        ph.fc7_fc8_head_fwd(a["y6"], a["w7"], a["b7"], a["y7"], a["w8"], a["b8"], a["y8"], a["poses_weight"],
                            a["tanh_out"], a["pred"], drop=a["drop"], keep_prob=0.5, M_dev=a["M_dev"], fuse=fuse)
        return tuple(a[k] for k in _FC_OUT)
    return _fc_args, call


case("fc7_fc8_head_fwd_fused", ["pcnn_gemm_partial", "pcnn_fc8_fwd_fused", "pcnn_fc8_reduce_head_fwd",
                                "pcnn_gemm_workspace_size"], outputs=_FC_OUT)(lambda: _fc_chain(True))
case("fc7_fc8_head_fwd_generic", ["pcnn_gemm_drop", "pcnn_gemm", "pcnn_pose_head_fwd"],
     outputs=_FC_OUT)(lambda: _fc_chain(False))


@case("gemm_partial", ["pcnn_gemm_partial"], outputs=["y7"])
def _():
    def build():
        a = _fc_args()
        return {k: a[k] for k in ("y6", "w7", "b7", "M_dev", "y7")}

    def call(a):
        ws = ph.gemm_partial(a["y6"], a["w7"], a["y7"], bias=a["b7"], act=1, M_dev=a["M_dev"])
        # the slabs are the kernel's own plan; fc8_fwd_fused's y7 shows what they sum to
        ph.fc8_fwd_fused(ws, U, a["b7"], a["y7"], rnd(U, D, seed=31, scale=0.1), act=1, M_dev=a["M_dev"])
        return a["y7"]
    return build, call


@case("fc8_fwd_fused", ["pcnn_fc8_fwd_fused"], outputs=["y7", "drop"],
      skip={("y7", "short"): "M is y7's own row count: one row less is a smaller call, not a short buffer"})
def _():
    def build():
        a = _fc_args()
        a["drop"] = zeros(R, U, dtype=U8)
        a["fc7_ws"] = ph.gemm_partial(a["y6"], a["w7"], a["y7"], bias=a["b7"], act=1, M_dev=a["M_dev"])
        a["step_dev"] = count(5, I64)
        return {k: a[k] for k in ("fc7_ws", "b7", "y7", "w8", "drop", "step_dev", "M_dev")}

    def call(a):
        ph.fc8_fwd_fused(a["fc7_ws"], U, a["b7"], a["y7"], a["w8"], act=1, drop=a["drop"], keep_prob=0.5,
                         drop_gen=(0x5EED, a["step_dev"], 7), M_dev=a["M_dev"])
        return a["y7"], a["drop"]
    return build, call


@case("fc8_reduce_head_fwd", ["pcnn_fc8_reduce_head_fwd"], outputs=["y8", "tanh_out", "pred"])
def _():
    def build():
        a = _fc_args()
        ws = ph.gemm_partial(a["y6"], a["w7"], a["y7"], bias=a["b7"], act=1, M_dev=a["M_dev"])
        ph.fc8_fwd_fused(ws, U, a["b7"], a["y7"], a["w8"], act=1, M_dev=a["M_dev"])
        return {k: a[k] for k in ("b8", "poses_weight", "y8", "tanh_out", "pred", "M_dev")}

    def call(a):
        ph.fc8_reduce_head_fwd(a["b8"], U, a["poses_weight"], a["y8"], a["tanh_out"], a["pred"], num_rois=a["M_dev"])
        return a["y8"], a["tanh_out"], a["pred"]
    return build, call


@case("fc8_dx", ["pcnn_fc8_dx_skinny"], outputs=["dy7"])
def _():
    def build():
        return dict(dy8=rnd(R, D, seed=34), W8=rnd(U, D, seed=35), mask=rnd(R, U, seed=36), M_dev=count(NR),
                    dy7=zeros(R, U))
    return build, lambda a: ph.fc8_dx(a["dy8"], a["W8"], a["dy7"], mask=a["mask"], keep_prob=0.5, M_dev=a["M_dev"])


# ------------------------------------------------------------------ the ADD loss family
def _add_args(seed=40):
    pred = torch.nn.functional.normalize(rnd(R, D, seed=seed), dim=1)
    target = torch.nn.functional.normalize(rnd(R, D, seed=seed + 1), dim=1)
    sym = torch.tensor([0.0, 0.0, 1.0], device=DEV)  # class 2 is symmetric (ADD-S)
    return dict(pred=pred, target=target, weight=head_weight(), points=rnd(C, P, 3, seed=seed + 2, scale=0.1),
                symmetry=sym, num_rois=count(NR), loss_norm_rows_dev=count(NR))


@case("average_distance_loss", ["pcnn_add_loss_fwd", "pcnn_add_loss_workspace_size"],
      outputs=["loss", "diff", "workspace"])
def _():
    def build():
        a = _add_args()
        a.update(loss=zeros(1), diff=zeros(R, D), workspace=zeros(adl.workspace_bytes(R, C, P), dtype=U8))
        return a
    return build, lambda a: adl.average_distance_loss(
        a["pred"], a["target"], a["weight"], a["points"], a["symmetry"], 0.01, num_rois=a["num_rois"],
        loss_norm_rows_dev=a["loss_norm_rows_dev"], out=(a["loss"], a["diff"]), workspace=a["workspace"])


@case("average_distance_loss_alloc", ["pcnn_add_loss_fwd"])
def _():
    def call(a):  # the reference-shaped call: outputs and workspace are the wrapper's own
        loss, diff = adl.average_distance_loss(a["pred"], a["target"], a["weight"], a["points"], a["symmetry"], 0.01)
        return loss, diff
    return lambda: {k: v for k, v in _add_args().items() if k not in ("num_rois", "loss_norm_rows_dev")}, call


@case("average_distance_loss_prep", ["pcnn_add_loss_prep"], outputs=["workspace"])
def _():
    def build():
        a = _add_args()
        return dict(weight=a["weight"], symmetry=a["symmetry"], num_rois=a["num_rois"],
                    workspace=zeros(adl.workspace_bytes(R, C, P), dtype=U8))

    def call(a):
        adl.average_distance_loss_prep(a["weight"], a["symmetry"], P, a["workspace"], num_rois=a["num_rois"])
        return a["workspace"]
    return build, call


@case("average_distance_loss_prepared", ["pcnn_add_loss_fwd_prepared"], outputs=["loss", "diff", "workspace"])
def _():
    def build():
        a = _add_args()
        a.update(loss=zeros(1), diff=zeros(R, D), workspace=zeros(adl.workspace_bytes(R, C, P), dtype=U8))
        adl.average_distance_loss_prep(a["weight"], a["symmetry"], P, a["workspace"], num_rois=a["num_rois"])
        return a

    def call(a):
        return adl.average_distance_loss(
            a["pred"], a["target"], a["weight"], a["points"], a["symmetry"], 0.01, num_rois=a["num_rois"],
            loss_norm_rows_dev=a["loss_norm_rows_dev"], out=(a["loss"], a["diff"]), workspace=a["workspace"],
            prepared=True)
    return build, call


def _tail_args():
    a = _add_args()
    s = _head_state()
    a.update(pred=s["pred"], weight=s["poses_weight"], tanh_out=s["tanh_out"], d_pred_scale=count(1).float(),
             diff=zeros(R, D), dy8=zeros(R, D), workspace=zeros(adl.workspace_bytes(R, C, P), dtype=U8))
    adl.average_distance_loss_prep(a["weight"], a["symmetry"], P, a["workspace"], num_rois=a["num_rois"])
    return a


@case("average_distance_loss_head_bwd", ["pcnn_add_loss_fwd_head_bwd"], outputs=["diff", "dy8", "workspace"])
def _():
    def call(a):
        adl.average_distance_loss_head_bwd(a["pred"], a["target"], a["weight"], a["points"], a["symmetry"], 0.01,
                                           a["tanh_out"], a["d_pred_scale"], a["diff"], a["dy8"], a["workspace"],
                                           num_rois=a["num_rois"], loss_norm_rows_dev=a["loss_norm_rows_dev"])
        return a["diff"], a["dy8"]
    return _tail_args, call


@case("average_distance_loss_total", ["pcnn_add_loss_total"], outputs=["loss", "workspace"])
def _():
    def build():
        a = _tail_args()
        adl.average_distance_loss_head_bwd(a["pred"], a["target"], a["weight"], a["points"], a["symmetry"], 0.01,
                                           a["tanh_out"], a["d_pred_scale"], a["diff"], a["dy8"], a["workspace"],
                                           num_rois=a["num_rois"], loss_norm_rows_dev=a["loss_norm_rows_dev"])
        return dict(workspace=a["workspace"], loss=zeros(1), num_rois=a["num_rois"])

    def call(a):
        adl.average_distance_loss_total(R, C, P, a["workspace"], a["loss"], num_rois=a["num_rois"])
        return a["loss"]
    return build, call


@case("average_distance_loss_grad", ["pcnn_add_loss_bwd"], outputs=["out"])
def _():
    def build():
        return dict(bottom_diff=rnd(R, D, seed=45), grad=count(1).float() * 0.25, num_rois=count(NR), out=zeros(R, D))
    return build, lambda a: adl.average_distance_loss_grad(a["bottom_diff"], a["grad"], num_rois=a["num_rois"],
                                                           out=a["out"])


# ------------------------------------------------------------------ RoI pooling
def _pool_args(pool_channel=0):
    Co = 1 if pool_channel else CH
    return dict(data=rnd(1, H, W, CH, seed=50), rois=rois(), num_rois=count(NR), top=zeros(R, 2, 2, Co),
                argmax=zeros(R, 2, 2, Co, dtype=I32))


@case("roi_pool", ["pcnn_roi_pool_fwd"], outputs=["top", "argmax"])
def _():
    return _pool_args, lambda a: rp.roi_pool(a["data"], a["rois"], 2, 2, 1.0 / 16.0, num_rois=a["num_rois"],
                                             out=(a["top"], a["argmax"]))


@case("roi_pool_alloc", ["pcnn_roi_pool_fwd"])
def _():
    def build():  # the reference-shaped call: its own outputs, the channel of each row's class
        return dict(data=rnd(1, H, W, CH, seed=51), rois=rois())
    return build, lambda a: rp.roi_pool(a["data"], a["rois"], 2, 2, 1.0 / 16.0, pool_channel=1)


@case("roi_pool_pth_rows", ["pcnn_roi_pool_fwd"])
def _():
    def build():  # the pth API's 5-column rows [b, x1, y1, x2, y2]
        return dict(data=rnd(1, H, W, CH, seed=51), rois=rois()[:, [0, 2, 3, 4, 5]])
    return build, lambda a: rp.roi_pool(a["data"], a["rois"], 2, 2, 1.0 / 16.0)


@case("roi_pool_accumulate", ["pcnn_roi_pool_fwd_accumulate"], outputs=["top", "argmax"])
def _():
    def build():
        a = _pool_args()
        a["top"] = rnd(R, 2, 2, CH, seed=52)
        return a
    return build, lambda a: rp.roi_pool(a["data"], a["rois"], 2, 2, 1.0 / 16.0, num_rois=a["num_rois"],
                                        out=(a["top"], a["argmax"]), accumulate=True)


def _pair(adt):
    def build():
        return dict(data_a=rnd(1, H, W, CH, seed=53), data_b=rnd(1, 2 * H, 2 * W, CH, seed=54), rois=rois(),
                    num_rois=count(NR), top=zeros(R, 2, 2, CH), arg_a=zeros(R, 2, 2, CH, dtype=adt),
                    arg_b=zeros(R, 2, 2, CH, dtype=adt))
    return build, lambda a: rp.roi_pool_pair(a["data_a"], 1.0 / 16.0, a["data_b"], 1.0 / 8.0, a["rois"], 2, 2,
                                             num_rois=a["num_rois"], out=(a["top"], a["arg_a"], a["arg_b"]))


case("roi_pool_pair", ["pcnn_roi_pool_fwd_pair"], outputs=["top", "arg_a", "arg_b"])(lambda: _pair(I32))
case("roi_pool_pair_px", ["pcnn_roi_pool_fwd_pair_px"], outputs=["top", "arg_a", "arg_b"])(lambda: _pair(torch.int16))


def _pool_grad(px):
    def build():
        data, rs, nr = rnd(1, H, W, CH, seed=55), rois(), count(NR)
        out = (zeros(R, 2, 2, CH), zeros(R, 2, 2, CH, dtype=torch.int16 if px else I32),
               zeros(R, 2, 2, CH, dtype=torch.int16 if px else I32))
        rp.roi_pool_pair(data, 1.0 / 16.0, rnd(1, 2 * H, 2 * W, CH, seed=56), 1.0 / 8.0, rs, 2, 2, num_rois=nr,
                         out=out)
        return dict(data=data, rois=rs, argmax=out[1], grad=rnd(R, 2, 2, CH, seed=57), num_rois=nr,
                    out=zeros(1, H, W, CH))
    return build, lambda a: rp.roi_pool_grad(a["data"], a["rois"], a["argmax"], a["grad"], 2, 2, 1.0 / 16.0,
                                             num_rois=a["num_rois"], out=a["out"])


case("roi_pool_grad", ["pcnn_roi_pool_bwd", "pcnn_roi_pool_bwd_workspace_size"],
     outputs=["out"])(lambda: _pool_grad(False))
case("roi_pool_grad_px", ["pcnn_roi_pool_bwd_px"], outputs=["out"],
     skip={("argmax", "dtype"): "the argmax's dtype is its format: int16 pixel index, any other width the flat index"}
     )(lambda: _pool_grad(True))


# ------------------------------------------------------------------ the Hough op
HH, HW, CAP = 48, 64, 32
_HOUGH_OUT = ("box", "pose", "target", "weight", "domain", "num_rois")


def _hough_args():
    fr = synth.make_frames(1, H=HH, W=HW, num_classes=C, objects_per_image=2, seed=5)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)  # noqa: E731
    return dict(label=t(fr["label"]), vertex=t(fr["vertex"]), extents=t(fr["extents"]), meta=t(fr["meta"]),
                gt=t(fr["gt"]), box=zeros(CAP, 7), pose=zeros(CAP, 7), target=zeros(CAP, D), weight=zeros(CAP, D),
                domain=zeros(CAP, dtype=I32), num_rois=zeros(2, dtype=I32))


def _hough_call(a, label="label", vertex="vertex", **kw):
    out = {k: a[k] for k in _HOUGH_OUT}
    if "label_out" in a:
        out["label"] = a["label_out"]
    o = hv.hough_voting_gpu_capacity(a[label] if label else None, a[vertex], a["extents"], a["meta"], a["gt"], 1, -1.0,
                                     0.02, 1, label_threshold=20, out=out, **kw)
    assert not hv.hough_voting_diag(o)[:3].any()
    return [o[k] for k in _HOUGH_OUT] + ([o["label"]] if "label" in out else [])


@case("hough_voting", ["pcnn_hough_voting", "pcnn_hough_voting_diag", "pcnn_hough_voting_workspace_size"],
      outputs=_HOUGH_OUT, wrapper="hough_voting_gpu_capacity")
def _():
    return _hough_args, _hough_call


@case("hough_voting_prob", ["pcnn_hough_voting_prob"], outputs=_HOUGH_OUT + ("label_out",))
def _():
    def build():
        a = _hough_args()
        lab = a.pop("label")
        a["prob"] = torch.nn.functional.one_hot(lab.long(), C).float() * 0.5 + uni(1, HH, HW, C, seed=60) * 0.25
        a["label_out"] = zeros(1, HH, HW, dtype=I32)
        return a
    return build, lambda a: _hough_call(a, label=None, prob=a["prob"])


@case("hough_voting_compact", ["pcnn_hough_voting_compact"], outputs=_HOUGH_OUT)
def _():
    def build():
        a = _hough_args()
        idx = (3 * a["label"].long()).unsqueeze(-1) + torch.arange(3, device=DEV)
        a["vertex3"] = torch.gather(a.pop("vertex"), 3, idx).contiguous()
        return a
    return build, lambda a: _hough_call(a, vertex="vertex3", vertex_compact=True)


@case("hough_voting_gpu", ["pcnn_hough_voting"])
def _():
    def build():  # the reference-shaped op: exact-size outputs of its own
        return {k: v for k, v in _hough_args().items() if k not in _HOUGH_OUT}
    return build, lambda a: hv.hough_voting_gpu(a["label"], a["vertex"], a["extents"], a["meta"], a["gt"], 1, -1.0,
                                                0.02, 1, label_threshold=20)


@case("hough_voting_gpu_from_prob", ["pcnn_hough_voting_prob"])
def _():
    def build():
        a = {k: v for k, v in _hough_args().items() if k not in _HOUGH_OUT}
        lab = a.pop("label")
        a["prob"] = torch.nn.functional.one_hot(lab.long(), C).float() * 0.5 + uni(1, HH, HW, C, seed=60) * 0.25
        return a
    return build, lambda a: hv.hough_voting_gpu_from_prob(a["prob"], a["vertex"], a["extents"], a["meta"], a["gt"], 1,
                                                          -1.0, 0.02, 1, label_threshold=20)


@case("hough_voting_gpu_grad", ["pcnn_hough_voting_grad"])
def _():
    def build():
        a = _hough_args()
        return dict(label=a["label"], vertex=a["vertex"])
    return build, lambda a: hv.hough_voting_gpu_grad(a["label"], a["vertex"], None)


# ------------------------------------------------------------------ backprojection, label producers, vertex_pred
G = 6


def _bp_args():
    K = np.array([[30.0, 0, 12], [0, 30.0, 8], [0, 0, 1]])
    meta = synth.make_meta(K, 1, voxel=([0.2, 0.16, 0.2], [-0.6, -0.48, 0.5]))
    return dict(data=rnd(1, H, W, CH, seed=70), label=uni(1, H, W, C, seed=71), depth=uni(1, H, W, 1, seed=72, lo=0.5,
                                                                                          hi=1.7),
                meta=torch.from_numpy(meta).to(DEV), label_3d=uni(1, G, G, G, C, seed=73))


@case("backproject", ["pcnn_backproject_fwd"])
def _():
    return _bp_args, lambda a: bp.backproject(a["data"], a["label"], a["depth"], a["meta"], a["label_3d"], G, 1, 0.3)


@case("backproject_grad", ["pcnn_backproject_bwd"])
def _():
    def build():
        a = _bp_args()
        return dict(data=a["data"], depth=a["depth"], meta=a["meta"], grad=rnd(1, G, G, G, CH, seed=74))
    return build, lambda a: bp.backproject_grad(a["data"], a["depth"], a["meta"], a["grad"], G, 1, 0.3)


@case("hard_label", ["pcnn_hard_label_fwd"])
def _():
    def build():
        return dict(prob=torch.softmax(rnd(1, H, W, C, seed=75), 3), gt=labels(1, H, W, seed=76, lo=-1))
    return build, lambda a: hl.hard_label(a["prob"], a["gt"], 0.4)


@case("hard_label_grad", ["pcnn_hard_label_bwd"])
def _():
    def build():
        return dict(prob=rnd(1, H, W, C, seed=77), gt=labels(1, H, W, seed=78), grad=rnd(1, H, W, C, seed=79))
    return build, lambda a: hl.hard_label_grad(a["prob"], a["gt"], a["grad"], 0.4)


@case("argmax_2d", ["pcnn_argmax_2d"], outputs=["out"])
def _():
    def build():
        return dict(prob=rnd(1, H, W, C, seed=80), out=zeros(1, H, W, dtype=I32))
    return build, lambda a: label_2d.argmax_2d(a["prob"], out=a["out"])


def _vp_args():
    return dict(feat=rnd(1, H, W, CH, seed=81), weights=rnd(CH, 3 * C, seed=82), biases=rnd(3 * C, seed=83),
                label=labels(1, H, W, seed=84, lo=-1, hi=C + 1))


@case("vertex_pred_compact", ["pcnn_vertex_pred_compact"], outputs=["out"])
def _():
    def build():
        return dict(_vp_args(), out=zeros(1, H, W, 3))
    return build, lambda a: vp.vertex_pred_compact(a["feat"], a["weights"], a["biases"], a["label"], out=a["out"])


@case("vertex_pred_compact_bwd", ["pcnn_vertex_pred_compact_bwd", "pcnn_vertex_pred_compact_bwd_workspace_size"])
def _():
    def build():
        a = _vp_args()
        return dict(feat=a["feat"], weights=a["weights"], label=a["label"], d_vertex3=rnd(1, H, W, 3, seed=85))
    return build, lambda a: vp.vertex_pred_compact_bwd(a["feat"], a["weights"], a["label"], a["d_vertex3"])


# ------------------------------------------------------------------ upscore, losses
h8, w8 = 4, 6  # low-resolution maps under stride 4: full resolution 16 x 24


@case("upscore", ["pcnn_upscore_fwd"], outputs=["out"])
def _():
    def build():
        return dict(x=rnd(1, h8, w8, CH, seed=90), bias=rnd(CH, seed=91), out=zeros(1, H, W, CH))
    return build, lambda a: up.upscore(a["x"], 4, bias=a["bias"], relu=True, out=a["out"])


@case("upscore_bwd", ["pcnn_upscore_bwd", "pcnn_upscore_bwd_workspace_size"])
def _():
    def build():
        return dict(d_y=rnd(1, H, W, CH, seed=92), y=rnd(1, H, W, CH, seed=93))
    return build, lambda a: up.upscore_bwd(a["d_y"], 4, y=a["y"], want_bias=True)


@case("upscore_compact", ["pcnn_upscore_compact_fwd"], outputs=["out"])
def _():
    def build():
        return dict(z=rnd(1, h8, w8, 3 * C, seed=94), bias=rnd(3 * C, seed=95),
                    label=labels(1, H, W, seed=96, lo=-1, hi=C + 1), out=zeros(1, H, W, 3))
    return build, lambda a: up.upscore_compact(a["z"], a["bias"], a["label"], stride=4, out=a["out"])


@case("upscore_compact_bwd", ["pcnn_upscore_compact_bwd", "pcnn_upscore_compact_bwd_workspace_size"])
def _():
    def build():
        return dict(label=labels(1, H, W, seed=97, lo=-1, hi=C + 1), d_vertex3=rnd(1, H, W, 3, seed=98))
    return build, lambda a: up.upscore_compact_bwd(a["label"], a["d_vertex3"], C, stride=4)


@case("seg_loss", ["pcnn_seg_loss", "pcnn_seg_loss_workspace_size"])
def _():
    def build():
        return dict(score=rnd(1, H, W, C, seed=100), gt=labels(1, H, W, seed=101, lo=-1))

    def call(a):
        loss, out = losses.seg_loss(a["score"], a["gt"], 0.4, want=losses.SEG_OUTPUTS, grad_scale=0.5)
        return [loss] + [out[k] for k in losses.SEG_OUTPUTS]
    return build, call


@case("softmax_high_dimension", ["pcnn_seg_loss"])
def _():
    return (lambda: dict(input=rnd(1, H, W, C, seed=102))), lambda a: (losses.softmax_high_dimension(a["input"]),
                                                                       losses.log_softmax_high_dimension(a["input"]))


@case("loss_cross_entropy_single_frame", ["pcnn_cross_entropy", "pcnn_cross_entropy_workspace_size"])
def _():
    def build():
        return dict(scores=torch.log_softmax(rnd(1, H, W, C, seed=103), 3),
                    labels=torch.nn.functional.one_hot(labels(1, H, W, seed=104).long(), C).float())
    return build, lambda a: losses.loss_cross_entropy_single_frame(a["scores"], a["labels"], want_grad=True)


@case("smooth_l1_loss_vertex", ["pcnn_vertex_loss", "pcnn_vertex_loss_workspace_size"])
def _():
    def build():
        return dict(pred=rnd(1, H, W, 3 * C, seed=105), targets=rnd(1, H, W, 3 * C, seed=106),
                    weights=(uni(1, H, W, 3 * C, seed=107) < 0.3).float())
    return build, lambda a: losses.smooth_l1_loss_vertex(a["pred"], a["targets"], a["weights"], want_grad=True)


@case("vertex_loss_compact", ["pcnn_vertex_loss_compact", "pcnn_vertex_loss_compact_workspace_size"])
def _():
    def build():
        return dict(pred=rnd(1, H, W, 3 * C, seed=108), label=labels(1, H, W, seed=109),
                    vertex3=rnd(1, H, W, 3, seed=110))
    return build, lambda a: losses.vertex_loss_compact(a["pred"], a["label"], a["vertex3"], C, 10.0, want_grad=True,
                                                       dense_grad=True)


# ------------------------------------------------------------------ utils/nms.py
def _nms_args():
    g = torch.Generator().manual_seed(120)
    n = 12
    x1, y1 = torch.rand(n, generator=g) * 40, torch.rand(n, generator=g) * 30
    d = torch.stack([torch.zeros(n), (torch.arange(n) % 2 + 1).float(), x1, y1, x1 + 20, y1 + 15,
                     torch.rand(n, generator=g)], 1).to(DEV)
    return dict(dets=d, num_rois=count(9))


@case("nms_device", ["pcnn_box_nms"])
def _():
    def call(a):
        keep, n = dn.nms_device(a["dets"], 0.3, num_rois=a["num_rois"])
        return keep[:int(n.item())], n
    return _nms_args, call


@case("nms_combine", ["pcnn_box_nms"], outputs=["rois_out", "poses_out"])
def _():
    def build():
        a = _nms_args()
        a.update(poses_init=rnd(12, 7, seed=121), poses_pred=rnd(12, D, seed=122), rois_out=zeros(12, 7),
                 poses_out=zeros(12, 7))
        return a
    return build, lambda a: dn.nms_combine(a["dets"], a["poses_init"], a["poses_pred"], 0.3, num_rois=a["num_rois"],
                                           out=(a["rois_out"], a["poses_out"]))


# ------------------------------------------------------------------ tier B: synthesize/ (refinement, rendering)
# A box rendered by the mesh rasteriser at 48 x 64 (the camera of tests/refine_scene.py at 1/10) is the scene:
# its maps are the "rendered" inputs, its depth and label the live frame.
BH, BW, BCLS = 48, 64, 2
BHALF = (0.06, 0.045, 0.035)


def _cam4():
    from refine_scene import CAMERA
    return tuple(c / 10.0 for c in CAMERA)


def _meshes():
    from render_ref import box_mesh
    return {BCLS: box_mesh(BHALF), 1: box_mesh((0.04, 0.05, 0.03))}


def _pose(dz=0.0, dx=0.0):
    q = np.array([0.9, 0.3, -0.2, 0.1])
    return np.concatenate([q / np.linalg.norm(q), [0.01 + dx, -0.005, 0.7 + dz]]).astype(np.float32)


def _box_scene():
    """Device maps of the box at its true pose (the live frame) and at a perturbed one (the rendering)."""
    from posecnn_amd.synthesize import icp as R
    from posecnn_amd.synthesize.render import MeshRenderer
    r = MeshRenderer(_meshes(), BH, BW, _cam4(), device=DEV)
    poses = torch.from_numpy(np.stack([_pose(), _pose(0.004, 0.002), _pose(-0.003, -0.002)])).to(DEV)
    vm, pv, pn, depth = r.render_many([BCLS] * 3, poses, return_depth=True)
    label = (depth[0] > 0).to(I32) * BCLS
    raw = torch.round(depth[0] * 10000.0).to(torch.int32).to(torch.uint16)
    live = R.live_vertices(raw, label, [BCLS], 10000.0, _cam4())
    return dict(renderer=r, poses=poses, vm=vm, pv=pv, pn=pn, label=label, raw=raw, live=live)


def tier_b(name, symbols, wrapper=None):
    return case(name, symbols, tier="B", wrapper=wrapper or name)


@tier_b("render_many", ["pcnn_render_meshes", "pcnn_render_workspace_size"], wrapper="MeshRenderer.render_many")
def _():
    from posecnn_amd.synthesize.render import MeshRenderer

    def build():
        return dict(r=MeshRenderer(_meshes(), BH, BW, _cam4(), device=DEV),
                    poses=torch.from_numpy(np.stack([_pose(), _pose(0.1)])).to(DEV))
    return build, lambda a: a["r"].render_many([BCLS, 1], a["poses"], return_depth=True, return_tri_id=True)


@tier_b("render_indexed", ["pcnn_render_meshes"], wrapper=["MeshRenderer.render_indexed", "MeshRenderer.__call__"])
def _():
    from posecnn_amd.synthesize.render import MeshRenderer

    def build():
        r = MeshRenderer(_meshes(), BH, BW, _cam4(), device=DEV)
        return dict(r=r, mesh_index=torch.tensor([r.slot[BCLS], r.slot[1]], dtype=I32, device=DEV),
                    class_id=torch.tensor([BCLS, 1], dtype=I32, device=DEV),
                    poses=torch.from_numpy(np.stack([_pose(), _pose(0.1)])).to(DEV))
    return build, lambda a: (a["r"].render_indexed(a["mesh_index"], a["class_id"], a["poses"]),
                             a["r"](BCLS, a["poses"][0]))


def _scene_args():
    from posecnn_amd.synthesize.scene import SceneRenderer
    r = SceneRenderer(_meshes(), BH, BW, _cam4(), device=DEV)
    return dict(r=r, scene_offset=torch.tensor([0, 2, 3], dtype=I32, device=DEV),
                mesh_index=torch.tensor([r.slot[BCLS], r.slot[1], r.slot[BCLS]], dtype=I32, device=DEV),
                class_id=torch.tensor([BCLS, 1, BCLS], dtype=I32, device=DEV),
                poses=torch.from_numpy(np.stack([_pose(), _pose(0.1, 0.05), _pose(0.2)])).to(DEV))


@tier_b("scene_render", ["pcnn_render_scenes", "pcnn_render_scenes_workspace_size"], wrapper="SceneRenderer.render")
def _():
    return _scene_args, lambda a: a["r"].render(a["scene_offset"], a["mesh_index"], a["class_id"], a["poses"])


@tier_b("scene_expand", ["pcnn_vertex_targets_expand"], wrapper=["scene.expand", "SceneRenderer.expand"])
def _():
    def build():
        a = _scene_args()
        o = a["r"].render(a["scene_offset"], a["mesh_index"], a["class_id"], a["poses"])
        return dict(r=a["r"], label=o["label"], vertex3=o["vertex3"])
    return build, lambda a: a["r"].expand(a["label"], a["vertex3"], 3)


@tier_b("live_vertices", ["pcnn_icp_live_vertices"])
def _():
    from posecnn_amd.synthesize import icp as R

    def build():
        s = _box_scene()
        return dict(depth=s["raw"], label=s["label"], obj_ids=torch.tensor([BCLS, 1], dtype=I32, device=DEV))
    return build, lambda a: R.live_vertices(a["depth"], a["label"], a["obj_ids"], 10000.0, _cam4())


@tier_b("icp", ["pcnn_icp", "pcnn_icp_workspace_size"])
def _():
    from posecnn_amd.synthesize import icp as R

    def build():
        s = _box_scene()
        return dict(live=s["live"], pv=s["pv"][1:], pn=s["pn"][1:], live_index=torch.zeros(2, dtype=I32, device=DEV),
                    pose_in=s["poses"][1:].clone())
    return build, lambda a: R.icp(a["live"], a["pv"], a["pn"], _cam4(), max_error=0.05, iterations=4,
                                  live_index=a["live_index"], pose_in=a["pose_in"], return_systems=True)


@tier_b("icp_center", ["pcnn_icp_center", "pcnn_icp_reduce_workspace_size"])
def _():
    from posecnn_amd.synthesize import icp as R

    def build():
        s = _box_scene()
        return dict(live=s["live"], label=s["label"], obj_ids=torch.tensor([BCLS], dtype=I32, device=DEV),
                    vertmap=s["vm"][1:2], pv=s["pv"][1:2], pn=s["pn"][1:2], pose_in=s["poses"][1:2].clone())
    return build, lambda a: R.icp_center(a["live"], a["label"], a["obj_ids"], a["vertmap"], a["pv"], a["pn"],
                                         max_error=0.05, pose_in=a["pose_in"])


@tier_b("pose_energy", ["pcnn_pose_energy"])
def _():
    from posecnn_amd.synthesize import icp as R

    def build():
        s = _box_scene()
        return dict(live=s["live"][0], label=s["label"], pv=s["pv"][1], poses=s["poses"].clone())
    return build, lambda a: R.pose_energy(a["live"], a["label"], BCLS, a["pv"], a["poses"])


@tier_b("pose_energy_batch", ["pcnn_pose_energy_batch"])
def _():
    from posecnn_amd.synthesize import icp as R

    def build():
        s = _box_scene()
        i = lambda *v: torch.tensor(v, dtype=I32, device=DEV)  # noqa: E731
        return dict(live=s["live"], label=s["label"], pose_obj=i(BCLS, BCLS, BCLS), pose_live=i(0, 0, 0), pv=s["pv"],
                    pose_pv=i(1, 2, 0), poses=s["poses"].clone())
    return build, lambda a: R.pose_energy_batch(a["live"], a["label"], a["pose_obj"], a["pose_live"], a["pv"],
                                                a["pose_pv"], a["poses"])


def _records_args(n=2):
    from posecnn_amd.synthesize import icp as R
    s = _box_scene()
    pv = s["pv"][1:2].expand(n, -1, -1, -1).contiguous()
    obj = torch.full((n,), BCLS, dtype=I32, device=DEV)
    rec, cnt = R.energy_records(s["live"], s["label"], obj, torch.zeros(n, dtype=I32, device=DEV), pv)
    return s, pv, obj, rec, cnt


@tier_b("energy_records", ["pcnn_energy_records", "pcnn_energy_records_workspace_size"])
def _():
    from posecnn_amd.synthesize import icp as R

    def build():
        s, pv, obj, _, _ = _records_args()
        return dict(live=s["live"], label=s["label"], prob_obj=obj, prob_live=torch.zeros(2, dtype=I32, device=DEV),
                    pv=pv)

    def call(a):
        rec, cnt = R.energy_records(a["live"], a["label"], a["prob_obj"], a["prob_live"], a["pv"])
        n = int(cnt.max())
        return rec[:, :n], cnt  # (records past a problem's count are not written)
    return build, call


@tier_b("pose_energy_records", ["pcnn_energy_rec"])
def _():
    from posecnn_amd.synthesize import icp as R

    def build():
        s, _, _, rec, cnt = _records_args()
        return dict(records=rec, counts=cnt, poses=s["poses"].clone(),
                    pose_prob=torch.tensor([0, 1, 0], dtype=I32, device=DEV))
    return build, lambda a: R.pose_energy_records(a["records"], a["counts"], a["poses"], a["pose_prob"])


def _nm(n, symbols, name):
    from posecnn_amd.synthesize import icp as R

    def build():
        s, _, _, rec, cnt = _records_args(n)
        x0 = s["poses"][1:2].double().expand(n, -1).contiguous()
        span = torch.tensor([0.05] * 4 + [0.01] * 3, dtype=torch.float64, device=DEV)
        return dict(records=rec, counts=cnt, x0=x0, lb=x0 - span, ub=x0 + span)

    def call(a):
        x, f, nev = R.nelder_mead_device(a["records"], a["counts"], a["x0"], a["lb"], a["ub"], 12)
        assert int(nev.min()) > 0
        return x, f, nev
    return tier_b(name, symbols, wrapper="nelder_mead_device")(lambda: (build, call))


_nm(2, ["pcnn_nelder_mead_energy_coop_path", "pcnn_nelder_mead_energy_workspace_size"], "nelder_mead_device")
_nm(129, ["pcnn_nelder_mead_energy"], "nelder_mead_device_one_workgroup")


@tier_b("icp_score", ["pcnn_icp_score", "pcnn_icp_score_workspace_size"])
def _():
    from posecnn_amd.synthesize import icp as R

    def build():
        s = _box_scene()
        return dict(live=s["live"][0], label=s["label"], vertmap=s["vm"][0], hyps=s["poses"].clone())
    return build, lambda a: R.icp_score(a["live"], a["label"], BCLS, a["vertmap"], a["hyps"], radius=0.02)


_POSE_SCENE = {}


def _pose_scene():
    if not _POSE_SCENE:
        from pose2d_scene import make_scene
        _POSE_SCENE.update(make_scene(seed=0, n_obj=2, C=4))
    sc = _POSE_SCENE
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)  # noqa: E731
    return dict(labels=t(sc["label"]), vertmap=t(sc["vertmap"]), extents=t(sc["extents"]),
                depth=t(sc["depth"].astype(np.int32))), sc


@tier_b("estimate_poses_2d", ["pcnn_pose2d", "pcnn_pose2d_workspace_size"])
def _():
    from posecnn_amd.synthesize import pose2d

    def build():
        a, _ = _pose_scene()
        del a["depth"]
        return a

    def call(a):
        sc = _POSE_SCENE
        poses = torch.zeros((3, 4, sc["C"]), device=DEV)
        _, d = pose2d.estimate_poses_2d(a["labels"], a["vertmap"], a["extents"], poses, sc["C"], *sc["camera"],
                                        n_hyp=16, return_diag=True)
        return poses, d["final"]
    return build, call


@tier_b("estimate_poses_3d", ["pcnn_pose3d", "pcnn_pose3d_workspace_size"])
def _():
    from posecnn_amd.synthesize import pose3d

    def build():
        return _pose_scene()[0]

    def call(a):
        sc = _POSE_SCENE
        poses = torch.zeros((3, 4, sc["C"]), device=DEV)
        _, d = pose3d.estimate_poses_3d(a["labels"], a["depth"], a["vertmap"], a["extents"], poses, sc["C"],
                                        *sc["camera"], sc["depth_factor"], n_hyp=16, nm_evals=10, return_diag=True)
        return poses, d["final"], d["eye"]
    return build, call


# ------------------------------------------------------------------ coverage (no GPU work)
# entry points with device pointers that no case reaches, each with its reason
EXEMPT = {
    "pcnn_div_rn_check": "test-only self-check of the ADD loss's division; no wrapper, called by its own test",
    "pcnn_philox_check": "test-only Philox self-check; no wrapper, called by the dropout test",
}
EXEMPT["pcnn_nelder_mead_energy_coop"] = ("no wrapper calls it: icp.nelder_mead_device goes through the _path form, "
                                          "which takes the same tensors")


def _public_wrappers():
    """{name: callable} of every public callable of the op modules that hands a tensor to the library."""
    import inspect
    from posecnn_amd.synthesize import icp, pose2d, pose3d, render, scene
    found = {}
    for mod in (ph, adl, rp, hv, bp, hl, label_2d, vp, up, losses, dn, icp, pose2d, pose3d, scene, render):
        for name, obj in vars(mod).items():
            if name.startswith("_") or getattr(obj, "__module__", None) != mod.__name__:
                continue
            if inspect.isfunction(obj):
                members = {name: obj}
            elif inspect.isclass(obj) and not issubclass(obj, torch.autograd.Function):
                members = {f"{name}.{m}": f for m, f in vars(obj).items()
                           if inspect.isfunction(f) and (not m.startswith("_") or m == "__call__")}
            else:
                continue
            for full, fn in members.items():
                src = inspect.getsource(fn)
                if "_lib.ptr(" in src or "_lib.load()" in src or "hough_voting_gpu_capacity(" in src:
                    found[full] = fn
    return found


# public callables that reach the library only through another public wrapper with a case of its own
VIA = {
    "workspace_bytes": "a size query (no tensor)", "search_stats": "reads a workspace back on the host (no launch)",
    "tp_bytes": "a size query, reached by the split_tp case", "hough_voting_diag": "part of the hough_voting case",
    "nms": "nms_device plus one host read", "softmax_high_dimension": "case softmax_high_dimension",
    "log_softmax_high_dimension": "case softmax_high_dimension",
    "PackedMeshes.mesh_args": "the packed mesh set of every render case",
    "MeshRenderer.render_into": "the call under MeshRenderer.render_indexed",
    "SceneRenderer.render_into": "the call under SceneRenderer.render",
}


def test_case_table_names_every_public_wrapper():
    named = {w.split(".")[-1] if "." not in w or w.startswith("scene.") else w for c in CASES for w in c.wrapper}
    named |= {c.name for c in CASES}
    missing = [w for w in _public_wrappers() if w not in named and w not in VIA]
    assert not missing, f"public wrappers without a case: {missing}"


def test_case_table_covers_every_entry_point_with_a_device_pointer():
    protos = ag.prototypes()
    need = {name for name in _lib._SIGS
            if any(p.is_pointer and not ag.is_host_param(p) for p in protos[name])}
    reached = set().union(*(c.symbols for c in CASES))
    assert reached <= set(_lib._SIGS), sorted(reached - set(_lib._SIGS))
    missing = need - reached - set(EXEMPT)
    assert not missing, f"entry points without a case or an EXEMPT reason: {sorted(missing)}"
    stale = set(EXEMPT) & reached
    assert not stale, f"EXEMPT entries that a case reaches: {sorted(stale)}"
    assert all(isinstance(r, str) and r for r in EXEMPT.values())
    assert len({c.name for c in CASES}) == len(CASES)


# ------------------------------------------------------------------ the engine
def tensors_of(out):
    """The tensors of a wrapper's result (tensor, tuple / list, or dict by sorted key), in a fixed order."""
    if isinstance(out, torch.Tensor):
        return [out]
    if isinstance(out, dict):
        return [t for k in sorted(out) for t in tensors_of(out[k])]
    if isinstance(out, (tuple, list)):
        return [t for o in out for t in tensors_of(o)]
    return []


def same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    view = torch.int32 if a.element_size() == 4 else torch.uint8
    return torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def run(c, mutate=None):
    """(outcome, outputs or the exception, launching calls counted, calls per symbol) of one guarded call."""
    a = c.build()
    if mutate is not None:
        mutate(a)
    torch.cuda.synchronize()
    with ag.installed() as guard:
        try:
            out = [t.clone() for t in tensors_of(c.call(a))]
            torch.cuda.synchronize()
        except (ValueError, TypeError) as e:
            return "raised", e, guard.launches, dict(guard.calls)
        except (RuntimeError, _lib.PcnnError) as e:
            if "HIP" in str(e) or "illegal memory access" in str(e):
                pytest.exit(f"{c.name}: device error, nothing more is started on the GPU: {e}", returncode=3)
            raise
    return "ok", out, guard.launches, dict(guard.calls)


_CANON = {}


def canonical(c):
    if c.name not in _CANON:
        outcome, out, launches, calls = run(c)
        assert outcome == "ok", f"{c.name}: canonical inputs raised {out!r}"
        _CANON[c.name] = (out, launches, calls)
    return _CANON[c.name]


def v_dtype(x):
    if x.dtype.is_floating_point:
        return x.double()
    return x.to(torch.int32 if x.dtype == torch.int64 else torch.int64)


def v_noncontig(x):
    """The same values behind strides no packed tensor has (None: the shape has no such view)."""
    if x.numel() <= 1:
        return None
    if x.dim() == 2:
        v = x.t().contiguous().t()
    elif x.dim() == 1:
        wide = torch.zeros(2 * x.numel(), dtype=x.dtype, device=x.device)
        wide[::2] = x
        v = wide[::2]
    else:
        wide = torch.zeros((*x.shape[:-1], x.shape[-1] + 4), dtype=x.dtype, device=x.device)
        wide[..., :x.shape[-1]] = x
        v = wide[..., :x.shape[-1]]
    return None if v.is_contiguous() else v


def v_offset(x):
    """A contiguous copy at a storage offset of 16 bytes."""
    off = 16 // x.element_size()
    buf = torch.zeros(x.numel() + off, dtype=x.dtype, device=x.device)
    v = buf[off:].view(x.shape)
    v.copy_(x)
    assert v.is_contiguous() and v.data_ptr() % 16 == x.data_ptr() % 16
    return v


def v_short(x):
    """One row short (one element, for a vector)."""
    return x[:-1].contiguous() if x.dim() else None


INPUT_VARIANTS = (("dtype", v_dtype), ("noncontig", v_noncontig), ("offset", v_offset), ("cpu", lambda x: x.cpu()))


def set_key(key, fn):
    def mutate(a):
        a[key] = fn(a[key])
    return mutate


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_canonical(hip, c):
    out, launches, calls = canonical(c)
    assert out, "the case returns no output tensor"
    assert launches > 0
    for sym in c.symbols:
        assert calls.get(sym, 0) > 0, f"{sym} was not reached"
    # deterministic: a second run gives the same bits (what (b) compares against)
    outcome, again, _, _ = run(c)
    assert outcome == "ok" and len(again) == len(out)
    assert all(same_bits(x, y) for x, y in zip(out, again))
    if c.name in ("hough_voting", "hough_voting_prob", "hough_voting_compact"):
        assert int(out[_HOUGH_OUT.index("num_rois")][0]) > 0, "the vote found no object"


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_input_variants(hip, c):
    ref, _, _ = canonical(c)
    keys = [k for k, v in c.build().items() if isinstance(v, torch.Tensor) and k not in c.outputs]
    assert keys
    bad, seen = [], {"raised": 0, "ok": 0}
    variants = INPUT_VARIANTS if c.tier == "A" else [v for v in INPUT_VARIANTS if v[0] in ("dtype", "cpu")]
    for key in keys:
        for vname, fn in variants:
            if (key, vname) in c.skip or fn(c.build()[key]) is None:
                continue
            outcome, res, launches, _ = run(c, set_key(key, fn))
            seen[outcome] += 1
            if outcome == "raised":
                if launches:
                    bad.append(f"{key}/{vname}: raised {res!r} after {launches} launching calls")
            elif len(res) != len(ref) or not all(same_bits(x, y) for x, y in zip(res, ref)):
                bad.append(f"{key}/{vname}: completed with other bits than the canonical call")
    assert not bad, "\n".join(bad)
    if c.tier == "A":  # (tier B's estimators and index arguments take host data by design and stage it)
        assert seen["raised"] >= len(keys)  # at least the CPU tensor of every input is refused


@pytest.mark.gpu
@pytest.mark.parametrize("c", [c for c in CASES if c.outputs], ids=lambda c: c.name)
def test_output_buffers(hip, c):
    canonical(c)
    short_ok = any(s in ag.EXTENTS for s in c.symbols)  # one row short only where the guard checks extents
    bad = []
    for key in c.outputs:
        variants = [("dtype", v_dtype), ("noncontig", v_noncontig)] + ([("short", v_short)] if short_ok else [])
        for vname, fn in variants:
            if (key, vname) in c.skip or fn(c.build()[key]) is None:
                continue
            outcome, res, launches, _ = run(c, set_key(key, fn))
            if outcome != "raised" or not isinstance(res, ValueError):
                bad.append(f"{key}/{vname}: expected ValueError, got {outcome} {res if outcome == 'raised' else ''}")
            elif launches:
                bad.append(f"{key}/{vname}: raised after {launches} launching calls")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------ the step, end to end
def _same(a, b):
    return same_bits(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("fuse_loss_tail", [True, False])
def test_pose_step_takes_float64_strided_model_points(hip, fuse_loss_tail):
    """PoseStep at the geometry of test_pose_step_fuse_fc8_is_bitwise_neutral
    with `points` and `symmetry` as float64, non-contiguous tensors (numpy's
    loadtxt default, sliced out of a wider table): the loss, pred, the ADD
    gradient and every other gradient are those of the fp32 contiguous
    inputs, bit for bit, with the guard installed at the boundary."""
    from posecnn_amd.pipeline import PoseStep
    B, SH, SW, SC, SCH, UN = 1, 120, 160, 22, 64, 256
    fr = synth.make_frames(B, H=SH, W=SW, num_classes=SC, objects_per_image=4, seed=93)
    g = torch.Generator().manual_seed(9)
    conv4 = torch.randn((B, SH // 8, SW // 8, SCH), generator=g)
    conv5 = torch.randn((B, SH // 16, SW // 16, SCH), generator=g)
    pts, sym = synth.rescaled_points(SC)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    pts, sym = t(pts), t(sym)
    pts_wide = torch.zeros((*pts.shape[:2], 5), dtype=torch.float64, device=DEV)
    pts_wide[..., :3] = pts
    sym_wide = torch.zeros(2 * sym.numel(), dtype=torch.float64, device=DEV)
    sym_wide[::2] = sym
    pts64, sym64 = pts_wide[..., :3], sym_wide[::2]
    assert pts64.dtype == sym64.dtype == torch.float64 and not pts64.is_contiguous() and not sym64.is_contiguous()
    base = dict(label=t(fr["label"]), vertex=t(fr["vertex"]), extents=t(fr["extents"]), meta=t(fr["meta"]),
                gt=t(fr["gt"]), conv4=conv4.to(DEV), conv5=conv5.to(DEV))
    outs, weights = [], None
    for points, symmetry in ((pts, sym), (pts64, sym64)):
        step = PoseStep(B, SH, SW, SC, DEV, channels=SCH, units=UN, is_train=1, skip_pixels=3, weights=weights,
                        fuse_loss_tail=fuse_loss_tail)
        if weights is None:
            weights = step.weights
            for b in (weights.b6, weights.b7, weights.b8):
                b.copy_(torch.randn(b.shape, generator=g) * 1e-3)
        with ag.installed() as guard:
            loss = step.step(dict(base, points=points, symmetry=symmetry))
            torch.cuda.synchronize()
        tail = guard.calls["pcnn_add_loss_fwd_head_bwd"]
        assert (tail == 1) if fuse_loss_tail else (tail == 0 and guard.calls["pcnn_add_loss_fwd_prepared"] == 1)
        assert int(step.hough["num_rois"][1].item()) > 4
        res = dict(loss=loss, pred=step.pred, diff=step.diff, dy8=step.dy8, dy7=step.dy7, dx=step.dx,
                   dconv4=step.dconv4, dconv5=step.dconv5)
        res.update({"g_" + k: v for k, v in step.grads.items()})
        outs.append({k: v.clone() for k, v in res.items()})
    for k in outs[0]:
        assert _same(outs[0][k], outs[1][k]), k
    assert bool(outs[0]["diff"].any()) and bool(outs[0]["dconv4"].any()) and bool(outs[0]["g_w7"].any())
    assert float(outs[0]["loss"]) > 0


@pytest.mark.gpu
def test_pose_step_checks_its_buffers_once_and_holds_no_minibatch(hip):
    """PoseStep passes the weights and its own fixed buffers through the
    primitives' checks at construction and calls the primitives unchecked
    (DESIGN.md section 1): mistyped or strided weights are refused there, before
    any launch.  What arrives per minibatch is checked on every step, so a
    loop that feeds a fresh dict of fresh tensors each step gives the same
    bits under the guard, and the step keeps none of those tensors alive."""
    import gc
    import weakref
    from posecnn_amd.pipeline import PoseStep
    B, SH, SW, SC, SCH, UN = 1, 120, 160, 22, 64, 256
    mk = lambda **kw: PoseStep(B, SH, SW, SC, DEV, channels=SCH, units=UN, is_train=1, skip_pixels=3,  # noqa: E731
                               keep_prob=1.0, **kw)
    for name, bad in (("w7", lambda w: w.double()), ("w6", lambda w: w.t().contiguous().t()),
                      ("b8", lambda w: w[:-1].contiguous()), ("w8", lambda w: w.cpu())):
        wts = ph.PoseHeadWeights(SC, DEV, in_dim=49 * SCH, units=UN)
        setattr(wts, name, bad(getattr(wts, name)))
        with ag.installed() as guard:
            with pytest.raises(ValueError, match=name):
                mk(weights=wts)
        assert guard.launches == 0
    fr = synth.make_frames(B, H=SH, W=SW, num_classes=SC, objects_per_image=4, seed=93)
    g = torch.Generator().manual_seed(9)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    pts, sym = synth.rescaled_points(SC)
    conv4 = torch.randn((B, SH // 8, SW // 8, SCH), generator=g)
    conv5 = torch.randn((B, SH // 16, SW // 16, SCH), generator=g)

    def minibatch():
        return dict(label=t(fr["label"]), vertex=t(fr["vertex"]), extents=t(fr["extents"]), meta=t(fr["meta"]),
                    gt=t(fr["gt"]), conv4=conv4.to(DEV), conv5=conv5.to(DEV), points=t(pts), symmetry=t(sym))
    step = mk()
    outs, refs = [], []
    for _ in range(3):
        inputs = minibatch()
        refs.append([weakref.ref(inputs[k]) for k in ("vertex", "conv4", "conv5", "label")])
        with ag.installed():
            loss = step.step(inputs)
            torch.cuda.synchronize()
        outs.append([x.clone() for x in (loss, step.pred, step.diff, step.dy8, step.dconv4, step.grads["w6"])])
        del inputs, loss
    for o in outs[1:]:
        assert all(same_bits(x, y) for x, y in zip(outs[0], o))
    assert bool(outs[0][2].any())
    gc.collect()
    assert not any(r() is not None for rs in refs for r in rs), "the step keeps a minibatch's tensors alive"


@pytest.mark.gpu
def test_fused_tail_refuses_what_the_reference_shaped_loss_converts(hip):
    """average_distance_loss_head_bwd is a hot-path primitive: float64 model
    points raise, as does a negative margin, with no launch."""
    a = _tail_args()
    for key, bad in (("points", a["points"].double()), ("symmetry", a["symmetry"].double())):
        b = dict(a)
        b[key] = bad
        with ag.installed() as guard:
            with pytest.raises(ValueError, match=key):
                adl.average_distance_loss_head_bwd(b["pred"], b["target"], b["weight"], b["points"], b["symmetry"],
                                                   0.01, b["tanh_out"], b["d_pred_scale"], b["diff"], b["dy8"],
                                                   b["workspace"], num_rois=b["num_rois"])
        assert guard.launches == 0
    with ag.installed() as guard:
        with pytest.raises(ValueError, match="margin"):
            adl.average_distance_loss_head_bwd(a["pred"], a["target"], a["weight"], a["points"], a["symmetry"], -0.01,
                                               a["tanh_out"], a["d_pred_scale"], a["diff"], a["dy8"], a["workspace"],
                                               num_rois=a["num_rois"])
    assert guard.launches == 0
