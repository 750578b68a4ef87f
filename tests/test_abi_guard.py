"""The ABI guard (tests/abi_guard.py) tested without a GPU: its prototype table
against the ctypes binding, and every rule shown firing and passing around a
fake library (plain callables that record their arguments; the device rule is
switched off here, and on for its own case).  A fired rule never reaches the
fake: its call log stays empty."""
import ctypes

import pytest
import torch

import abi_guard as ag
from posecnn_amd import _lib

PROTOS = ag.prototypes()


class FakeLib:
    """Every entry point of the binding as a callable that logs (name, args) and returns 0."""

    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        if name not in _lib._SIGS:
            raise AttributeError(name)
        return lambda *args: (self.log.append((name, args)), 0)[1]


@pytest.fixture
def guard():
    return ag.GuardedLib(FakeLib(), require_device=False)


def P(t):
    return _lib.ptr(t)


def f32(*shape):
    return torch.zeros(shape, dtype=torch.float32)


def i32(*shape):
    return torch.zeros(shape, dtype=torch.int32)


STREAM = ctypes.c_void_p(0)


def passes(guard, name, *args):
    n = len(guard._real.log)
    launches = guard.launches
    assert getattr(guard, name)(*args) == 0
    assert [c[0] for c in guard._real.log[n:]] == [name]
    assert guard.calls[name] >= 1
    assert guard.launches == launches + int(ag.launches(PROTOS[name]))


def fires(guard, name, *args, param, rule=None):
    with pytest.raises(ag.AbiContractError) as e:
        getattr(guard, name)(*args)
    msg = str(e.value)
    assert name in msg and f"`{param}`" in msg, msg
    if rule is not None:
        assert rule in msg, msg
    assert guard._real.log == []  # refused before forwarding
    assert guard.calls[name] == 0 and guard.launches == 0


# ------------------------------------------------------------------ the prototype table
def test_table_has_the_bindings_symbols_and_pointers():
    assert set(PROTOS) == set(_lib._SIGS)
    for name, (_res, argtypes) in _lib._SIGS.items():
        params = PROTOS[name]
        assert len(params) == len(argtypes), name
        for p, a in zip(params, argtypes):
            assert p.is_pointer == (a is ctypes.c_void_p), (name, p.name)
            assert (p.elem_type is not None) == p.is_pointer, (name, p.name)
            if p.is_pointer:
                assert p.elem_type in ag.ELEM, (name, p)


def test_table_spot_checks():
    def param(sym, name):
        return next(p for p in PROTOS[sym] if p.name == name)
    assert param("pcnn_pose_head_fwd", "y8") == ag.Param("const float*", "y8", True, "float", True)
    assert param("pcnn_pose_head_fwd", "pred") == ag.Param("float*", "pred", True, "float", False)
    assert param("pcnn_hough_voting", "label").elem_type == "int32_t"
    assert param("pcnn_roi_pool_fwd_pair_px", "argmax_a") == ag.Param("uint16_t*", "argmax_a", True, "uint16_t", False)
    assert param("pcnn_nelder_mead_energy", "x0").elem_type == "double"
    assert param("pcnn_gemm", "workspace") == ag.Param("void*", "workspace", True, "void", False)
    assert param("pcnn_gemm_drop_gen", "step_dev").elem_type == "int64_t"
    assert param("pcnn_gemm_drop", "drop").elem_type == "uint8_t"
    assert param("pcnn_gemm", "lda") == ag.Param("int", "lda", False, None, False)
    assert param("pcnn_split_tp", "row_stride").c_type == "long"
    # host-side pointers
    assert ag.is_host_param(param("pcnn_gemm", "stream"))
    assert ag.is_host_param(param("pcnn_set_completion_event", "event"))
    assert ag.is_host_param(param("pcnn_hough_voting_diag", "diag_host4"))
    assert not ag.is_host_param(param("pcnn_hough_voting_diag", "workspace"))
    assert ag.launches(PROTOS["pcnn_colsum"]) and not ag.launches(PROTOS["pcnn_tp_bytes"])


def test_dtype_kinds_and_sizes():
    ok = {"float": [torch.float32], "double": [torch.float64], "int32_t": [torch.int32], "uint32_t": [torch.int32],
          "uint16_t": [torch.int16], "uint8_t": [torch.uint8, torch.int8], "int64_t": [torch.int64],
          "uint64_t": [torch.int64]}
    every = [torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.int8, torch.uint8, torch.int16,
             torch.int32, torch.int64, torch.bool]
    for elem, good in ok.items():
        for dt in every:
            assert ag.dtype_matches(dt, elem) == (dt in good), (elem, dt)
    assert all(ag.dtype_matches(dt, "void") for dt in every)


def test_every_leading_dimension_and_extent_names_a_parameter():
    for sym, table in ag.LEADING_DIM.items():
        names = {p.name: p for p in PROTOS[sym]}
        for ptr, ld in table.items():
            assert names[ptr].is_pointer, (sym, ptr)
            assert ld is None or not names[ld].is_pointer, (sym, ld)
    for sym, fn in ag.EXTENTS.items():
        ints = {p.name: 3 for p in PROTOS[sym] if not p.is_pointer}
        ptrs = {p.name for p in PROTOS[sym] if p.is_pointer}
        need = fn(ints)
        assert need and all(v >= 0 for v in need.values()), sym
        assert set(need) & ptrs, sym  # (a family's formula may name parameters of its other members)


# ------------------------------------------------------------------ type, layout, device and pointer rules
R, D = 5, 12


def head_fwd_args(**over):
    a = dict(y8=f32(R, D), poses_weight=f32(R, D), tanh_out=f32(R, D), pred=f32(R, D), num=i32(1))
    a.update(over)
    return (P(a["y8"]), P(a["poses_weight"]), R, P(a["num"]), D, P(a["tanh_out"]), P(a["pred"]), STREAM)


def test_canonical_call_passes_and_is_counted(guard):
    passes(guard, "pcnn_pose_head_fwd", *head_fwd_args())
    passes(guard, "pcnn_pose_head_fwd", *head_fwd_args(num=None))  # optional pointers may be NULL
    assert guard.calls["pcnn_pose_head_fwd"] == 2 and guard.launches == 2
    # a non-launching query goes through uncounted as a launch
    passes(guard, "pcnn_tp_bytes", 4, 4)
    assert guard.launches == 2
    guard.reset()
    assert not guard.calls and guard.launches == 0


def test_float64_for_float_fires(guard):
    fires(guard, "pcnn_pose_head_fwd", *head_fwd_args(y8=f32(R, D).double()), param="y8", rule="dtype")


def test_int64_for_int32_fires(guard):
    fires(guard, "pcnn_pose_head_fwd", *head_fwd_args(num=torch.zeros(1, dtype=torch.int64)), param="num_rois_dev",
          rule="dtype")


def test_double_prototype_wants_float64(guard):
    def args(x0):
        d = torch.zeros((2, 7), dtype=torch.float64)
        return (P(f32(2, 16, 6)), P(i32(2)), 16, 2, P(x0), P(d), P(d), 10, 0.1, 5.0, P(d.clone()),
                P(torch.zeros(2, dtype=torch.float64)), P(i32(2)), STREAM)
    passes(guard, "pcnn_nelder_mead_energy", *args(torch.zeros((2, 7), dtype=torch.float64)))
    guard.reset(), guard._real.log.clear()
    fires(guard, "pcnn_nelder_mead_energy", *args(f32(2, 7)), param="x0", rule="dtype")


def test_uint16_prototype_wants_a_two_byte_integer(guard):
    def args(arg):
        a = torch.zeros((R, 2, 2, 4), dtype=arg)
        return (P(f32(1, 4, 4, 4)), 4, 4, 0.5, P(f32(1, 8, 8, 4)), 8, 8, 0.25, 1, 4, P(f32(R, 7)), R, 7, 0, P(i32(1)),
                2, 2, P(f32(R, 2, 2, 4)), P(a), P(a.clone()), STREAM)
    passes(guard, "pcnn_roi_pool_fwd_pair_px", *args(torch.int16))
    guard.reset(), guard._real.log.clear()
    fires(guard, "pcnn_roi_pool_fwd_pair_px", *args(torch.int32), param="argmax_a", rule="dtype")


def test_transposed_view_fires(guard):
    t = f32(D, R).t()  # (R, D), strides (1, R)
    fires(guard, "pcnn_pose_head_fwd", *head_fwd_args(y8=t), param="y8", rule="non-contiguous")


def test_slice_of_a_wider_buffer_fires_on_a_contiguous_only_parameter(guard):
    wide = f32(R, D + 4)
    fires(guard, "pcnn_pose_head_fwd", *head_fwd_args(pred=wide[:, :D]), param="pred", rule="non-contiguous")
    passes(guard, "pcnn_pose_head_fwd", *head_fwd_args(pred=wide[:, :D].contiguous()))


def colsum_args(X, ld, out=None):
    return (P(X), X.shape[0], X.shape[1], ld, None, P(out if out is not None else f32(X.shape[1])), STREAM)


def test_slice_on_a_leading_dimension_parameter(guard):
    wide = f32(R, D + 4)
    X = wide[:, :D]
    fires(guard, "pcnn_colsum", *colsum_args(X, D), param="X", rule="`ldx` = 12")  # the wrong ld
    passes(guard, "pcnn_colsum", *colsum_args(X, D + 4))                             # its own row stride
    guard.reset(), guard._real.log.clear()
    fires(guard, "pcnn_colsum", *colsum_args(f32(D, R).t(), R), param="X", rule="unit inner stride")


def test_cpu_tensor_fires_with_the_device_rule_on():
    g = ag.GuardedLib(FakeLib(), require_device=True)
    fires(g, "pcnn_pose_head_fwd", *head_fwd_args(), param="y8", rule="CPU tensor")


def test_bare_pointer_where_a_tensor_belongs_fires(guard):
    a = list(head_fwd_args())
    a[0] = ctypes.c_void_p(f32(R, D).data_ptr())
    fires(guard, "pcnn_pose_head_fwd", *a, param="y8", rule="bare c_void_p")
    a[0] = 4096  # an integer address
    fires(guard, "pcnn_pose_head_fwd", *a, param="y8", rule="bare int")


def test_byref_out_parameters_are_host_side(guard):
    d = torch.zeros((2, 7), dtype=torch.float64)
    u8 = torch.zeros(64, dtype=torch.uint8)
    passes(guard, "pcnn_nelder_mead_energy_coop_path", P(f32(2, 16, 6)), P(i32(2)), 16, 2, P(d), P(d), P(d), 10, 0.1,
           5.0, P(d.clone()), P(torch.zeros(2, dtype=torch.float64)), P(i32(2)), P(u8), 64, 0,
           ctypes.byref(ctypes.c_int32(0)), STREAM)


def test_host_parameters_take_host_values_and_no_tensor(guard):
    ws = torch.zeros(64, dtype=torch.uint8)
    host = (ctypes.c_int32 * 4)()
    passes(guard, "pcnn_hough_voting_diag", P(ws), 1, 8, 8, 3, 1, -1.0, ctypes.cast(host, ctypes.c_void_p), STREAM)
    passes(guard, "pcnn_set_completion_event", 12345)
    guard.reset(), guard._real.log.clear()
    fires(guard, "pcnn_hough_voting_diag", P(ws), 1, 8, 8, 3, 1, -1.0, P(i32(4)), STREAM, param="diag_host4",
          rule="host-side")


def test_wrong_arity_fires(guard):
    fires(guard, "pcnn_pose_head_fwd", *head_fwd_args()[:-1], param="*")


# ------------------------------------------------------------------ extents: one short fires, exactly enough passes
def short(t):
    """A packed tensor one element short of `t`'s count (the same dtype)."""
    return torch.zeros(t.numel() - 1, dtype=t.dtype)


ONE_SHORT = set()  # entry points some test has shown refusing a buffer one element short


def each_one_short(guard, name, build, params):
    """build(**over) -> args; for every named tensor parameter the exact call
    passes and the call with that tensor one element short fires."""
    ONE_SHORT.add(name)
    passes(guard, name, *build())
    for p, (key, t) in params.items():
        guard.reset(), guard._real.log.clear()
        fires(guard, name, *build(**{key: short(t)}), param=p, rule="imply")


def test_extents_pose_head(guard):
    m = f32(R, D)
    each_one_short(guard, "pcnn_pose_head_fwd", head_fwd_args,
                   {"y8": ("y8", m), "poses_weight": ("poses_weight", m), "tanh_out": ("tanh_out", m),
                    "pred": ("pred", m), "num_rois_dev": ("num", i32(1))})

    def bwd(**o):
        a = dict(d_pred=f32(R, D), scale=f32(1), tanh_out=f32(R, D), w=f32(R, D), pred=f32(R, D), num=i32(1),
                 d_y8=f32(R, D))
        a.update(o)
        return (P(a["d_pred"]), P(a["scale"]), P(a["tanh_out"]), P(a["w"]), P(a["pred"]), R, P(a["num"]), D,
                P(a["d_y8"]), STREAM)
    guard.reset(), guard._real.log.clear()
    each_one_short(guard, "pcnn_pose_head_bwd", bwd,
                   {"d_pred": ("d_pred", m), "d_pred_scale": ("scale", f32(1)), "tanh_out": ("tanh_out", m),
                    "poses_weight": ("w", m), "pred": ("pred", m), "num_rois_dev": ("num", i32(1)),
                    "d_y8": ("d_y8", m)})


def test_extents_colsum(guard):
    M, N, ld = 4, 6, 8
    buf = f32((M - 1) * ld + N)  # exactly (M-1)*ldx + N elements

    def args(n_x=buf.numel(), n_out=N, mdev=i32(1)):
        X = torch.as_strided(f32(n_x), (M, N), (ld, 1)) if n_x >= buf.numel() else f32(n_x)
        return (P(X), M, N, ld, P(mdev), P(f32(n_out)), STREAM)
    passes(guard, "pcnn_colsum", *args())
    guard.reset(), guard._real.log.clear()
    fires(guard, "pcnn_colsum", *args(n_x=buf.numel() - 1), param="X", rule="imply 30")
    fires(guard, "pcnn_colsum", *args(n_out=N - 1), param="out", rule="imply 6")
    fires(guard, "pcnn_colsum", *args(mdev=i32(0)), param="M_dev", rule="imply 1")
    ONE_SHORT.add("pcnn_colsum")


def gemm_args(name, M=4, N=6, K=5, at=0, bt=0, **o):
    ra = (K, M) if at else (M, K)
    rb = (N, K) if bt else (K, N)
    a = dict(A=f32(*ra), A2=f32(*ra), B=f32(*rb), C=f32(M, N), bias=f32(N), mask=f32(M, N),
             drop=torch.zeros((M, N), dtype=torch.uint8), M_dev=i32(1), K_dev=i32(1),
             step=torch.zeros(1, dtype=torch.int64), ws=torch.zeros(256, dtype=torch.uint8))
    a.update(o)
    head = (M, N, K, P(a["A"]), P(a["A2"]), ra[1], at, P(a["B"]), rb[1], bt, P(a["C"]), N, P(a["bias"]), 1)
    tail = (P(a["M_dev"]), P(a["K_dev"]), 2, P(a["ws"]), 256, STREAM)
    if name == "pcnn_gemm":
        return head + (P(a["mask"]), N) + tail
    if name == "pcnn_gemm_drop":
        return head + (P(a["mask"]), N, P(a["drop"]), N, 0.5) + tail
    if name == "pcnn_gemm_drop_gen":
        return head + (P(a["drop"]), N, 0.5, 7, P(a["step"]), 6) + tail
    return head + tail  # pcnn_gemm_partial


GEMM_PARAMS = {
    "pcnn_gemm": ("A", "A2", "B", "Cm", "bias", "mask", "M_dev", "K_dev", "workspace"),
    "pcnn_gemm_drop": ("A", "A2", "B", "Cm", "bias", "mask", "drop", "M_dev", "K_dev", "workspace"),
    "pcnn_gemm_drop_gen": ("A", "A2", "B", "Cm", "bias", "drop_out", "step_dev", "M_dev", "K_dev", "workspace"),
    "pcnn_gemm_partial": ("A", "A2", "B", "Cm", "bias", "M_dev", "K_dev", "workspace"),
}
_GEMM_KEY = {"Cm": "C", "drop_out": "drop", "step_dev": "step", "workspace": "ws"}


@pytest.mark.parametrize("name", sorted(GEMM_PARAMS))
@pytest.mark.parametrize("at,bt", [(0, 0), (1, 0), (0, 1)])
def test_extents_gemm_family(guard, name, at, bt):
    passes(guard, name, *gemm_args(name, at=at, bt=bt))
    base = dict(zip(("A", "A2", "B", "C", "bias", "mask", "drop", "M_dev", "K_dev", "step", "ws"), [None] * 11))
    for p in GEMM_PARAMS[name]:
        key = _GEMM_KEY.get(p, p)
        guard.reset(), guard._real.log.clear()
        # one element short: a packed 1-D buffer (any ld goes with a single row) of numel - 1
        M, N, K = 4, 6, 5
        full = {"A": M * K, "A2": M * K, "B": K * N, "C": M * N, "bias": N, "mask": M * N, "drop": M * N, "M_dev": 1,
                "K_dev": 1, "step": 1, "ws": 256}[key]
        dt = {"drop": torch.uint8, "ws": torch.uint8, "M_dev": torch.int32, "K_dev": torch.int32,
              "step": torch.int64}.get(key, torch.float32)
        assert key in base
        fires(guard, name, *gemm_args(name, at=at, bt=bt, **{key: torch.zeros(full - 1, dtype=dt)}), param=p,
              rule="imply")
    ONE_SHORT.add(name)


def test_gemm_padded_leading_dimensions(guard):
    """The ragged 37 x 20 x 52 product through padded rows: ld = the view's own row stride."""
    M, N, K = 37, 20, 52
    A, B, C = f32(M, K + 4)[:, :K], f32(K, N + 12)[:, :N], f32(M, N + 4)[:, :N]
    ws = torch.zeros(256, dtype=torch.uint8)

    def args(lda=K + 4, ldb=N + 12, ldc=N + 4):
        return (M, N, K, P(A), None, lda, 0, P(B), ldb, 0, P(C), ldc, None, 0, None, 0, None, None, 2, P(ws), 256,
                STREAM)
    passes(guard, "pcnn_gemm", *args())
    guard.reset(), guard._real.log.clear()
    fires(guard, "pcnn_gemm", *args(lda=K), param="A", rule="`lda`")
    fires(guard, "pcnn_gemm", *args(ldb=N), param="B", rule="`ldb`")
    fires(guard, "pcnn_gemm", *args(ldc=N), param="Cm", rule="`ldc`")


def test_extents_fc8(guard):
    M, N7, D8, K7 = 5, 8, 12, 8
    u8 = torch.uint8

    def fused(**o):
        a = dict(ws7=torch.zeros(512, dtype=u8), b7=f32(N7), y7=f32(M, N7), drop=torch.zeros((M, N7), dtype=u8),
                 step=torch.zeros(1, dtype=torch.int64), W8=f32(N7, D8), M_dev=i32(1), ws8=torch.zeros(512, dtype=u8))
        a.update(o)
        return (M, N7, K7, P(a["ws7"]), 512, P(a["b7"]), 1, P(a["y7"]), N7, P(a["drop"]), N7, 0.5, 1, 7, P(a["step"]),
                7, P(a["W8"]), D8, D8, P(a["M_dev"]), P(a["ws8"]), 512, STREAM)
    each_one_short(guard, "pcnn_fc8_fwd_fused", fused,
                   {"fc7_workspace": ("ws7", torch.zeros(512, dtype=u8)), "b7": ("b7", f32(N7)),
                    "y7": ("y7", f32(M, N7)), "drop": ("drop", torch.zeros((M, N7), dtype=u8)),
                    "step_dev": ("step", torch.zeros(1, dtype=torch.int64)), "W8": ("W8", f32(N7, D8)),
                    "M_dev": ("M_dev", i32(1)), "fc8_workspace": ("ws8", torch.zeros(512, dtype=u8))})

    def reduce(**o):
        a = dict(ws8=torch.zeros(512, dtype=u8), b8=f32(D8), num=i32(1), w=f32(M, D8), y8=f32(M, D8), t8=f32(M, D8),
                 pred=f32(M, D8))
        a.update(o)
        return (P(a["ws8"]), 512, P(a["b8"]), M, N7, D8, P(a["num"]), P(a["w"]), P(a["y8"]), P(a["t8"]),
                P(a["pred"]), STREAM)
    guard.reset(), guard._real.log.clear()
    m = f32(M, D8)
    each_one_short(guard, "pcnn_fc8_reduce_head_fwd", reduce,
                   {"fc8_workspace": ("ws8", torch.zeros(512, dtype=u8)), "b8": ("b8", f32(D8)),
                    "num_rois_dev": ("num", i32(1)), "poses_weight": ("w", m), "y8": ("y8", m),
                    "tanh_out": ("t8", m), "pred": ("pred", m)})

    def dx(**o):
        a = dict(dy8=f32(M, D8), W8=f32(N7, D8), mask=f32(M, N7), dy7=f32(M, N7), M_dev=i32(1))
        a.update(o)
        return (P(a["dy8"]), D8, P(a["W8"]), D8, P(a["mask"]), N7, 0.5, P(a["dy7"]), N7, M, D8, N7, P(a["M_dev"]),
                STREAM)
    guard.reset(), guard._real.log.clear()
    each_one_short(guard, "pcnn_fc8_dx_skinny", dx,
                   {"dy8": ("dy8", m), "W8": ("W8", f32(N7, D8)), "mask": ("mask", f32(M, N7)),
                    "dy7": ("dy7", f32(M, N7)), "M_dev": ("M_dev", i32(1))})


def test_extents_add_loss(guard):
    C, Pn = 3, 64
    PC = 4 * C
    m = f32(R, PC)
    u8 = torch.uint8

    def base(**o):
        a = dict(pred=f32(R, PC), target=f32(R, PC), weight=f32(R, PC), points=f32(C, Pn, 3), sym=f32(C), num=i32(1),
                 norm=i32(1), loss=f32(1), diff=f32(R, PC), ws=torch.zeros(1024, dtype=u8), t8=f32(R, PC),
                 scale=f32(1), dy8=f32(R, PC))
        a.update(o)
        return a

    def fwd(**o):
        a = base(**o)
        return (P(a["pred"]), P(a["target"]), P(a["weight"]), P(a["points"]), P(a["sym"]), R, P(a["num"]), C, Pn, 0.01,
                0, P(a["norm"]), P(a["loss"]), P(a["diff"]), P(a["ws"]), 1024, STREAM)
    common = {"pred": ("pred", m), "target": ("target", m), "weight": ("weight", m),
              "points": ("points", f32(C, Pn, 3)), "symmetry": ("sym", f32(C)), "num_rois_dev": ("num", i32(1)),
              "loss_norm_rows_dev": ("norm", i32(1)), "bottom_diff": ("diff", m),
              "workspace": ("ws", torch.zeros(1024, dtype=u8))}
    for name in ("pcnn_add_loss_fwd", "pcnn_add_loss_fwd_prepared"):
        guard.reset(), guard._real.log.clear()
        each_one_short(guard, name, fwd, dict(common, loss=("loss", f32(1))))

    def tail(**o):
        a = base(**o)
        return (P(a["pred"]), P(a["target"]), P(a["weight"]), P(a["points"]), P(a["sym"]), R, P(a["num"]), C, Pn, 0.01,
                0, P(a["norm"]), P(a["diff"]), P(a["ws"]), 1024, P(a["t8"]), P(a["scale"]), P(a["dy8"]), STREAM)
    guard.reset(), guard._real.log.clear()
    each_one_short(guard, "pcnn_add_loss_fwd_head_bwd", tail,
                   dict(common, tanh_out=("t8", m), d_pred_scale=("scale", f32(1)), d_y8=("dy8", m)))

    def prep(**o):
        a = base(**o)
        return (P(a["weight"]), P(a["sym"]), R, P(a["num"]), C, Pn, P(a["ws"]), 1024, STREAM)
    guard.reset(), guard._real.log.clear()
    each_one_short(guard, "pcnn_add_loss_prep", prep,
                   {"weight": ("weight", m), "symmetry": ("sym", f32(C)), "num_rois_dev": ("num", i32(1)),
                    "workspace": ("ws", torch.zeros(1024, dtype=u8))})

    def total(**o):
        a = base(**o)
        return (R, P(a["num"]), C, Pn, P(a["ws"]), 1024, P(a["loss"]), STREAM)
    guard.reset(), guard._real.log.clear()
    each_one_short(guard, "pcnn_add_loss_total", total,
                   {"num_rois_dev": ("num", i32(1)), "workspace": ("ws", torch.zeros(1024, dtype=u8)),
                    "loss": ("loss", f32(1))})

    def bwd(**o):
        a = dict(top=f32(1), diff=f32(R, PC), num=i32(1), out=f32(R, PC))
        a.update(o)
        return (P(a["top"]), P(a["diff"]), R * PC, P(a["num"]), PC, P(a["out"]), STREAM)
    guard.reset(), guard._real.log.clear()
    each_one_short(guard, "pcnn_add_loss_bwd", bwd,
                   {"top_diff": ("top", f32(1)), "bottom_diff": ("diff", m), "num_rois_dev": ("num", i32(1)),
                    "out": ("out", m)})


def test_extents_roi_pool(guard):
    B, H, W, C, ph, pw, stride = 1, 4, 6, 8, 2, 2, 7
    i16 = torch.int16
    data, rois, top = f32(B, H, W, C), f32(R, stride), f32(R, ph, pw, C)

    def fwd(**o):
        a = dict(data=data, rois=rois, num=i32(1), top=top, arg=i32(R, ph, pw, C))
        a.update(o)
        return (P(a["data"]), B, H, W, C, 0, P(a["rois"]), R, stride, 0, P(a["num"]), 0.5, ph, pw, 0, P(a["top"]),
                P(a["arg"]), STREAM)
    params = {"data": ("data", data), "rois": ("rois", rois), "num_rois_dev": ("num", i32(1)), "top": ("top", top),
              "argmax": ("arg", i32(R, ph, pw, C))}
    for name in ("pcnn_roi_pool_fwd", "pcnn_roi_pool_fwd_accumulate"):
        guard.reset(), guard._real.log.clear()
        each_one_short(guard, name, fwd, params)
    # pool_channel: one output channel
    guard.reset(), guard._real.log.clear()
    a = list(fwd(top=f32(R, ph, pw, 1), arg=i32(R, ph, pw, 1)))
    a[14] = 1
    passes(guard, "pcnn_roi_pool_fwd", *a)

    def pair(adt):
        def build(**o):
            a = dict(da=f32(B, H, W, C), db=f32(B, 2 * H, 2 * W, C), rois=rois, num=i32(1), top=top,
                     aa=torch.zeros((R, ph, pw, C), dtype=adt), ab=torch.zeros((R, ph, pw, C), dtype=adt))
            a.update(o)
            return (P(a["da"]), H, W, 0.0625, P(a["db"]), 2 * H, 2 * W, 0.125, B, C, P(a["rois"]), R, stride, 0,
                    P(a["num"]), ph, pw, P(a["top"]), P(a["aa"]), P(a["ab"]), STREAM)
        return build
    for name, adt in (("pcnn_roi_pool_fwd_pair", torch.int32), ("pcnn_roi_pool_fwd_pair_px", i16)):
        guard.reset(), guard._real.log.clear()
        arg = torch.zeros((R, ph, pw, C), dtype=adt)
        each_one_short(guard, name, pair(adt),
                       {"data_a": ("da", data), "data_b": ("db", f32(B, 2 * H, 2 * W, C)), "rois": ("rois", rois),
                        "num_rois_dev": ("num", i32(1)), "top_sum": ("top", top), "argmax_a": ("aa", arg),
                        "argmax_b": ("ab", arg)})

    ws = torch.zeros(512, dtype=torch.uint8)

    def bwd(**o):
        a = dict(td=top, arg=i32(R, ph, pw, C), rois=rois, num=i32(1), dd=data, ws=ws)
        a.update(o)
        return (P(a["td"]), P(a["arg"]), B, H, W, C, 0, P(a["rois"]), R, stride, 0, P(a["num"]), 0.5, ph, pw, 0,
                P(a["dd"]), P(a["ws"]), 512, STREAM)
    guard.reset(), guard._real.log.clear()
    each_one_short(guard, "pcnn_roi_pool_bwd", bwd,
                   {"top_diff": ("td", top), "argmax": ("arg", i32(R, ph, pw, C)), "rois": ("rois", rois),
                    "num_rois_dev": ("num", i32(1)), "bottom_diff": ("dd", data), "workspace": ("ws", ws)})

    def bwd_px(**o):
        a = dict(td=top, arg=torch.zeros((R, ph, pw, C), dtype=i16), rois=rois, num=i32(1), dd=data, ws=ws)
        a.update(o)
        return (P(a["td"]), P(a["arg"]), B, H, W, C, P(a["rois"]), R, stride, 0, P(a["num"]), 0.5, ph, pw,
                P(a["dd"]), P(a["ws"]), 512, STREAM)
    guard.reset(), guard._real.log.clear()
    each_one_short(guard, "pcnn_roi_pool_bwd_px", bwd_px,
                   {"top_diff": ("td", top), "argmax_px": ("arg", torch.zeros((R, ph, pw, C), dtype=i16)),
                    "rois": ("rois", rois), "num_rois_dev": ("num", i32(1)), "bottom_diff": ("dd", data),
                    "workspace": ("ws", ws)})


def test_extents_hough(guard):
    B, H, W, C, cap, nm, ng = 1, 4, 6, 3, 9, 48, 2
    ws = torch.zeros(512, dtype=torch.uint8)

    def outs(a):
        return (P(a["box"]), P(a["pose"]), P(a["target"]), P(a["weight"]), P(a["domain"]), P(a["num"]), cap, None,
                P(a["ws"]), 512, STREAM)

    def base(**o):
        a = dict(label=i32(B, H, W), prob=f32(B, H, W, C), vertex=f32(B, H, W, 3 * C), vertex3=f32(B, H, W, 3),
                 extents=f32(C, 3), meta=f32(B, nm), gt=f32(ng, 13), box=f32(cap, 7), pose=f32(cap, 7),
                 target=f32(cap, 4 * C), weight=f32(cap, 4 * C), domain=i32(cap), num=i32(2), ws=ws)
        a.update(o)
        return a
    mid = (B, H, W, C, 0, 1, 1, 0.9, 500, -1.0, 0.02, 1)

    def vote(**o):
        a = base(**o)
        return (P(a["label"]), P(a["vertex"]), P(a["extents"]), P(a["meta"]), nm, P(a["gt"]), ng) + mid + outs(a)

    def vote_prob(**o):
        a = base(**o)
        return (P(a["prob"]), P(a["label"]), P(a["vertex"]), P(a["extents"]), P(a["meta"]), nm, P(a["gt"]),
                ng) + mid + outs(a)

    def vote_compact(**o):
        a = base(**o)
        return (P(a["label"]), P(a["vertex3"]), P(a["extents"]), P(a["meta"]), nm, P(a["gt"]), ng) + mid + outs(a)
    b = base()
    out_params = {"top_box": ("box", b["box"]), "top_pose": ("pose", b["pose"]), "top_target": ("target", b["target"]),
                  "top_weight": ("weight", b["weight"]), "top_domain": ("domain", b["domain"]),
                  "num_rois": ("num", b["num"]), "workspace": ("ws", ws), "extents": ("extents", b["extents"]),
                  "meta": ("meta", b["meta"]), "gt": ("gt", b["gt"])}
    each_one_short(guard, "pcnn_hough_voting", vote,
                   dict(out_params, label=("label", b["label"]), vertex=("vertex", b["vertex"])))
    guard.reset(), guard._real.log.clear()
    each_one_short(guard, "pcnn_hough_voting_prob", vote_prob,
                   dict(out_params, prob=("prob", b["prob"]), label_out=("label", b["label"]),
                        vertex=("vertex", b["vertex"])))
    guard.reset(), guard._real.log.clear()
    each_one_short(guard, "pcnn_hough_voting_compact", vote_compact,
                   dict(out_params, label=("label", b["label"]), vertex3=("vertex3", b["vertex3"])))


def test_every_extents_entry_point_has_a_one_short_case():
    """Runs after the cases above (file order): they recorded every entry point they took one element short."""
    assert ONE_SHORT == set(ag.EXTENTS), sorted(set(ag.EXTENTS) ^ ONE_SHORT)


# ------------------------------------------------------------------ installing it
def test_installed_swaps_and_restores_the_cached_handle(monkeypatch):
    fake = FakeLib()
    monkeypatch.setattr(_lib, "_lib", fake)
    with ag.installed(require_device=False) as g:
        assert _lib.load() is g
        assert _lib.load().pcnn_tp_bytes(4, 4) == 0 and fake.log[-1][0] == "pcnn_tp_bytes"
    assert _lib.load() is fake
    with pytest.raises(RuntimeError):
        with ag.installed(require_device=False):
            raise RuntimeError("inside")
    assert _lib.load() is fake


# ------------------------------------------------------------------ the wrappers' shared check
def test_require_names_the_argument():
    t = torch.zeros(3)
    with pytest.raises(ValueError, match="my_arg: expected a device tensor"):
        _lib.require(t, torch.float32, name="my_arg")
    with pytest.raises(TypeError, match="my_arg"):
        _lib.require([1.0], torch.float32, name="my_arg")
    with pytest.raises(ValueError, match="my_arg: a tensor is required"):
        _lib.require(None, torch.float32, name="my_arg")
    assert _lib.require(None, torch.float32, name="my_arg", optional=True) is None
    assert _lib.require_counter(None, "n") is None
    with pytest.raises(ValueError, match="n: expected a device tensor"):
        _lib.require_counter(torch.zeros(1, dtype=torch.int32), "n")
