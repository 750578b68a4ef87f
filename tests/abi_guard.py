"""A guard on the ctypes boundary of libposecnn_hip.so (a test helper, not a
conftest).

Everything the Python wrappers hand to the library is a raw pointer and a few
ints: nothing at that boundary knows a tensor's dtype, strides, device or
size.  `_lib.ptr` keeps the tensor on the pointer object, the header
(include/posecnn_hip.h) gives every parameter's element type and states that
"every pointer is a DEVICE pointer unless the name ends in _host", so the
contract can be checked mechanically before a launch:

    with abi_guard.installed() as guard:      # posecnn_amd._lib._lib <- proxy
        wrapper(...)                          # AbiContractError on a violation
    guard.calls, guard.launches

`GuardedLib` checks every `_TensorPtr` argument against its prototype (device,
element type, layout), checks the extents of the entry points in `EXTENTS`
against the integer arguments, and refuses -- raises `AbiContractError`
without calling the real function -- on a violation: no malformed call ever
reaches a kernel through it.
"""
import contextlib
import ctypes
import os
import re
from collections import Counter, namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "posecnn_hip.h")

Param = namedtuple("Param", "c_type name is_pointer elem_type is_const")


class AbiContractError(AssertionError):
    """A wrapper handed the library an argument that breaks the header's contract."""


def declarations(header=HEADER):
    """{name: argument text} of every pcnn_* function declared in the header."""
    src = open(header).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    return {m.group(1): m.group(2).strip() for m in re.finditer(r"\b(pcnn_\w+)\s*\(([^)]*)\)\s*;", src)}


_ARG = re.compile(r"^(const\s+)?([A-Za-z_]\w*(?:\s+[A-Za-z_]\w*)*?)\s*(\*?)\s*([A-Za-z_]\w*)$")


def prototypes(header=HEADER):
    """{symbol: [Param(c_type, name, is_pointer, elem_type, is_const)]} of the header."""
    out = {}
    for name, args in declarations(header).items():
        params = []
        if args not in ("", "void"):
            for a in args.split(","):
                m = _ARG.match(" ".join(a.split()))
                if m is None:
                    raise ValueError(f"{name}: cannot parse parameter {a!r}")
                const, base, star, pname = m.groups()
                ptr = star == "*"
                params.append(Param((("const " if const else "") + base + ("*" if ptr else "")), pname, ptr,
                                    base if ptr else None, bool(const)))
        out[name] = params
    return out


# element type -> (kind, bytes): "f" floating point, "i" integer; void: any dtype
ELEM = {"float": ("f", 4), "double": ("f", 8), "int32_t": ("i", 4), "uint32_t": ("i", 4), "uint16_t": ("i", 2),
        "uint8_t": ("i", 1), "int64_t": ("i", 8), "uint64_t": ("i", 8), "void": None}


def dtype_matches(dtype, elem_type):
    want = ELEM[elem_type]
    if want is None:
        return True
    kind, size = want
    if dtype.is_complex or str(dtype) == "torch.bool":
        return False
    return ("f" if dtype.is_floating_point else "i") == kind and dtype.itemsize == size


_HOST_NAME = re.compile(r"_host\d*$")  # `..._host`, or `..._host<n>` (a host array of n elements)
_BYREF = type(ctypes.byref(ctypes.c_int()))


def is_host_param(p):
    """Host-side pointer parameters, never tensors: `*_host`, the stream and event handles."""
    return p.is_pointer and (p.name in ("stream", "event") or bool(_HOST_NAME.search(p.name)))


def launches(params):
    """A launching entry point is one whose prototype has a `stream` parameter."""
    return any(p.name == "stream" for p in params)


# Operands passed with a leading dimension: {symbol: {pointer parameter: ld parameter}}.  These need
# unit inner stride and ld == stride(0); every other tensor must be contiguous.  None: the entry point
# takes explicit element strides for the operand (pcnn_split_tp's source), whose layout is the caller's.
_GEMM_LD = {"A": "lda", "A2": "lda", "B": "ldb", "Cm": "ldc", "mask": "ldm"}
LEADING_DIM = {
    "pcnn_gemm": _GEMM_LD,
    "pcnn_gemm_drop": dict(_GEMM_LD, drop="ldd"),
    "pcnn_gemm_drop_gen": {"A": "lda", "A2": "lda", "B": "ldb", "Cm": "ldc", "drop_out": "ldd"},
    "pcnn_gemm_partial": {"A": "lda", "A2": "lda", "B": "ldb", "Cm": "ldc"},
    "pcnn_gemm_tp": {"Cm": "ldc", "mask": "ldm", "drop": "ldd"},
    "pcnn_colsum": {"X": "ldx"},
    "pcnn_dropout_mask": {"mask": "ld"},
    "pcnn_fc8_fwd_fused": {"y7": "ld7", "drop": "ldd", "W8": "ldb"},
    "pcnn_fc8_dx_skinny": {"dy8": "lda", "W8": "ldb", "mask": "ldm", "dy7": "ldc"},
    "pcnn_split_tp": {"src": None},
}


# ---- extents: elements each pointer must hold, from the integer arguments (the header's comments) ----
def _mat(rows, cols, ld):
    """Elements spanned by `rows` rows of `cols` at pitch `ld`."""
    return (rows - 1) * ld + cols if rows > 0 and cols > 0 else 0


def _ext_pose_head(a):
    n = a["R_cap"] * a["D"]
    need = {k: n for k in ("y8", "poses_weight", "tanh_out", "pred", "d_pred", "d_y8")}
    need.update(num_rois_dev=1, d_pred_scale=1)
    return need


def _ext_colsum(a):
    return {"X": _mat(a["M"], a["N"], a["ldx"]), "out": a["N"], "M_dev": 1}


def _ext_gemm(a):
    M, N, K = a["M"], a["N"], a["K"]
    ra = (K, M) if a["a_trans"] else (M, K)
    rb = (N, K) if a["b_trans"] else (K, N)
    need = {"A": _mat(*ra, a["lda"]), "A2": _mat(*ra, a["lda"]), "B": _mat(*rb, a["ldb"]),
            "Cm": _mat(M, N, a["ldc"]), "bias": N, "M_dev": 1, "K_dev": 1, "step_dev": 1}
    if "ldm" in a:
        need["mask"] = _mat(M, N, a["ldm"])
    if "ldd" in a:
        need["drop"] = need["drop_out"] = _mat(M, N, a["ldd"])
    return need


def _ext_fc8_fwd_fused(a):
    M, N7, D = a["M"], a["N7"], a["D"]
    return {"b7": N7, "y7": _mat(M, N7, a["ld7"]), "drop": _mat(M, N7, a["ldd"]), "W8": _mat(N7, D, a["ldb"]),
            "step_dev": 1, "M_dev": 1}


def _ext_fc8_reduce_head_fwd(a):
    n = a["R_cap"] * a["D"]
    return {"b8": a["D"], "poses_weight": n, "y8": n, "tanh_out": n, "pred": n, "num_rois_dev": 1}


def _ext_fc8_dx_skinny(a):
    M, D, N7 = a["M"], a["D"], a["N7"]
    return {"dy8": _mat(M, D, a["lda"]), "W8": _mat(N7, D, a["ldb"]), "mask": _mat(M, N7, a["ldm"]),
            "dy7": _mat(M, N7, a["ldc"]), "M_dev": 1}


def _ext_add_loss(a):
    R, C, P = a["R_cap"], a["C"], a["P"]
    need = {k: R * 4 * C for k in ("pred", "target", "weight", "bottom_diff", "tanh_out", "d_y8")}
    need.update(points=C * P * 3, symmetry=C, loss=1, num_rois_dev=1, loss_norm_rows_dev=1, d_pred_scale=1)
    return need


def _ext_add_loss_bwd(a):
    return {"top_diff": 1, "bottom_diff": a["n"], "out": a["n"], "num_rois_dev": 1}


def _ext_roi_pool(a):
    B, C, R = a["B"], a["C"], a["R_cap"]
    Co = 1 if a.get("pool_channel") else C
    n_top = R * a["pooled_h"] * a["pooled_w"] * Co
    need = {"rois": R * a["roi_stride"], "num_rois_dev": 1}
    if "Ha" in a:  # the pair: two maps, all channels
        need.update(data_a=B * a["Ha"] * a["Wa"] * C, data_b=B * a["Hb"] * a["Wb"] * C)
        need.update({k: n_top for k in ("top_sum", "argmax_a", "argmax_b")})
    else:
        n_map = B * a["H"] * a["W"] * C
        need.update(data=n_map, bottom_diff=n_map)
        need.update({k: n_top for k in ("top", "argmax", "top_diff", "argmax_px")})
    return need


def _ext_hough(a):
    B, H, W, C, cap = a["B"], a["H"], a["W"], a["C"], a["cap"]
    px = B * H * W
    return {"label": px, "label_out": px, "prob": px * C, "vertex": px * 3 * C, "vertex3": px * 3,
            "extents": C * 3, "meta": B * a["num_meta"], "gt": a["num_gt"] * 13, "top_box": cap * 7,
            "top_pose": cap * 7, "top_target": cap * 4 * C, "top_weight": cap * 4 * C, "top_domain": cap,
            "num_rois": 2}


EXTENTS = {
    "pcnn_pose_head_fwd": _ext_pose_head, "pcnn_pose_head_bwd": _ext_pose_head,
    "pcnn_colsum": _ext_colsum,
    "pcnn_gemm": _ext_gemm, "pcnn_gemm_drop": _ext_gemm, "pcnn_gemm_drop_gen": _ext_gemm,
    "pcnn_gemm_partial": _ext_gemm,
    "pcnn_fc8_fwd_fused": _ext_fc8_fwd_fused, "pcnn_fc8_reduce_head_fwd": _ext_fc8_reduce_head_fwd,
    "pcnn_fc8_dx_skinny": _ext_fc8_dx_skinny,
    "pcnn_add_loss_fwd": _ext_add_loss, "pcnn_add_loss_fwd_prepared": _ext_add_loss,
    "pcnn_add_loss_prep": _ext_add_loss, "pcnn_add_loss_fwd_head_bwd": _ext_add_loss,
    "pcnn_add_loss_total": _ext_add_loss, "pcnn_add_loss_bwd": _ext_add_loss_bwd,
    "pcnn_roi_pool_fwd": _ext_roi_pool, "pcnn_roi_pool_fwd_accumulate": _ext_roi_pool,
    "pcnn_roi_pool_fwd_pair": _ext_roi_pool, "pcnn_roi_pool_fwd_pair_px": _ext_roi_pool,
    "pcnn_roi_pool_bwd": _ext_roi_pool, "pcnn_roi_pool_bwd_px": _ext_roi_pool,
    "pcnn_hough_voting": _ext_hough, "pcnn_hough_voting_prob": _ext_hough, "pcnn_hough_voting_compact": _ext_hough,
}


def span(t):
    """Elements from the tensor's first to its last, inclusive: numel for a packed tensor."""
    if t.numel() == 0:
        return 0
    return 1 + sum((n - 1) * s for n, s in zip(t.shape, t.stride()))


def _value(x):
    return x.value if isinstance(x, ctypes._SimpleCData) else x


class GuardedLib:
    """A proxy of the loaded library: every declared entry point is wrapped in
    the contract check.  `calls[symbol]` counts the calls forwarded,
    `launches` those to an entry point with a `stream` parameter.
    require_device=False switches the device rule off (the guard's own CPU
    test, around a fake library)."""

    def __init__(self, real, require_device=True, header=HEADER):
        from posecnn_amd import _lib
        self._real = real
        self._ptr_type = _lib._TensorPtr
        self._protos = prototypes(header)
        self.require_device = require_device
        self.calls = Counter()
        self.launches = 0

    def reset(self):
        self.calls.clear()
        self.launches = 0

    def __getattr__(self, name):
        real = getattr(self._real, name)
        params = self.__dict__["_protos"].get(name)
        if params is None:
            return real

        def guarded(*args):
            self.check(name, args)
            self.calls[name] += 1
            if launches(params):
                self.launches += 1
            return real(*args)
        guarded.__name__ = name
        return guarded

    def _fail(self, symbol, param, rule):
        raise AbiContractError(f"{symbol}: parameter `{param}`: {rule}")

    def check(self, symbol, args):
        params = self._protos[symbol]
        if len(args) != len(params):
            self._fail(symbol, "*", f"{len(args)} arguments for {len(params)} parameters")
        named = {p.name: _value(a) for p, a in zip(params, args) if not p.is_pointer}
        lds = LEADING_DIM.get(symbol, {})
        tensors = {}
        for p, a in zip(params, args):
            if not p.is_pointer or is_host_param(p):
                if isinstance(a, self._ptr_type):
                    self._fail(symbol, p.name, "a tensor where a host-side value belongs")
                continue
            if a is None or isinstance(a, _BYREF):  # (byref: a host out-parameter such as path_out, never a tensor)
                continue
            if not isinstance(a, self._ptr_type):
                self._fail(symbol, p.name, f"a bare {type(a).__name__} where a tensor (through _lib.ptr) belongs")
            t = a.tensor
            tensors[p.name] = t
            if a.value != (t.data_ptr() or None):
                self._fail(symbol, p.name, "the pointer is not its tensor's data_ptr()")
            if self.require_device and not t.is_cuda:
                self._fail(symbol, p.name, "a CPU tensor where a device pointer belongs")
            if not dtype_matches(t.dtype, p.elem_type):
                self._fail(symbol, p.name, f"dtype {t.dtype} where the prototype has {p.c_type}")
            if p.name in lds:
                ld = lds[p.name]
                if ld is None:
                    continue
                if t.dim() < 1 or t.stride(-1) != 1:
                    self._fail(symbol, p.name, f"strides {tuple(t.stride())}: unit inner stride needed")
                if t.dim() > 2:
                    self._fail(symbol, p.name, f"a {t.dim()}-dimensional view where `{ld}` gives one row pitch")
                if t.dim() == 2 and t.shape[0] > 1 and named[ld] != t.stride(0):
                    self._fail(symbol, p.name, f"`{ld}` = {named[ld]} but the tensor's row stride is {t.stride(0)}")
            elif not t.is_contiguous():
                self._fail(symbol, p.name, f"a non-contiguous tensor (strides {tuple(t.stride())}) and no "
                                           "leading dimension for it")
        # byte-counted buffers: `void* x, size_t x_bytes`
        for name, t in tensors.items():
            nbytes = named.get(name + "_bytes")
            if nbytes is not None and span(t) * t.element_size() < nbytes:
                self._fail(symbol, name, f"{span(t) * t.element_size()} bytes where the integer arguments imply "
                                         f"{nbytes} (`{name}_bytes`)")
        ext = EXTENTS.get(symbol)
        if ext is not None:
            for name, need in ext(named).items():
                t = tensors.get(name)
                if t is not None and span(t) < need:
                    self._fail(symbol, name, f"{span(t)} elements where the integer arguments imply {need}")


@contextlib.contextmanager
def installed(require_device=True):
    """Route every wrapper through a GuardedLib: the wrappers fetch
    `_lib.load()` per call, which returns the cached handle set here."""
    from posecnn_amd import _lib
    real = _lib.load()
    guard = GuardedLib(real, require_device=require_device)
    _lib._lib = guard
    try:
        yield guard
    finally:
        _lib._lib = real
