"""Every split-bf16 GEMM instantiation, bit-exactly, on integer operands.

On the operand classes of tests/gemm_exact_cases.py every kept plane product
and every partial sum is an exact fp32 integer, so pcnn_gemm must equal an
fp64 matmul bit for bit -- whatever the tile plan, the split-K slicing or the
accumulation order.  No tolerance anywhere in this file, except the last
section, which applies test_gpu_gemm_fc6.py's fp32-faithfulness criterion to
full-mantissa operands at one small shape per kernel form.

Every call writes into a NaN-poisoned C whose row pitch is wider than N, with
the stream's GEMM workspace NaN-poisoned too: live rows must equal the
reference, pad columns and rows past M_dev must still be poison, and a slab
or an output element nobody wrote shows up as NaN.  The case table is checked
on the CPU against the planner (tests/test_gemm_exact_cases.py), so each id
below runs the kernel instantiation or the plan edge it is named for.
"""
import functools

import numpy as np
import pytest
import torch

import gemm_exact_cases as gx
from posecnn_amd import _lib
from posecnn_amd import pose_head as ph

pytestmark = pytest.mark.gpu
D = torch.device("cuda")


@functools.lru_cache(maxsize=64)
def _ops(cls, M, N, K, a2):
    return gx.operands(cls, M, N, K, seed=1, a2=a2)


def _pitched(X, extra=4):
    """A device copy of the 2-D array X as a view of a poisoned buffer with a
    row pitch that is a multiple of 4 and wider than the row."""
    pitch = (X.shape[1] + 3 + extra) // 4 * 4
    buf = gx.poison(torch.empty((X.shape[0], pitch), dtype=torch.float32, device=D))
    buf[:, :X.shape[1]] = torch.from_numpy(np.ascontiguousarray(X)).to(D)
    return buf[:, :X.shape[1]]


def _dev(X, trans):
    return None if X is None else _pitched(X.T if trans else X)


def _counter(v):
    return None if v is None else torch.tensor([v], dtype=torch.int32, device=D)


def _poisoned_c(M, N, pad=8):
    buf = gx.poison(torch.empty((M, N + pad), dtype=torch.float32, device=D))
    return buf, buf[:, :N]


def _is_poison(t):
    return bool((t.contiguous().view(torch.int32) == -1).all())


def _poison_workspace(M, N, K, m_dynamic, prec):
    size = _lib.load().pcnn_gemm_workspace_size(M, N, K, int(m_dynamic), prec)
    gx.poison(_lib.workspace(size, D, "gemm"))


def _assert_result(buf, N, rows, ref, what):
    """Live rows bit-equal to the reference, nothing else written."""
    live = buf[:rows, :N]
    assert not bool(torch.isnan(live).any()), f"{what}: NaN in the live region"
    want = ref if isinstance(ref, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ref)).to(D)
    want = want.to(torch.float32)
    if not torch.equal(live, want):
        bad = (live != want).nonzero()
        r, c = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {live.numel()} elements differ; rows {int(bad[:, 0].min())}.."
                             f"{int(bad[:, 0].max())}, columns {int(bad[:, 1].min())}..{int(bad[:, 1].max())}; first "
                             f"({r}, {c}): got {float(live[r, c])!r}, want {float(want[r, c])!r}")
    assert _is_poison(buf[:, N:]), f"{what}: pad columns written"
    assert _is_poison(buf[rows:]), f"{what}: rows past the live {rows} written"


def run(c, cls, epi="bare", pad=8, what=""):
    """One pcnn_gemm call of case c on class cls.  epi: "bare", "full" (bias +
    relu + mask), "drop" (bias + relu, drop mask, keep 0.5: the forward),
    "bwd" (mask, keep 0.5: the backward's 1 / keep), "relu_bias"."""
    A, A2, B = _ops(cls, c.M, c.N, c.K, bool(c.a2))
    bias, mask, drop = gx.epilogue_operands(c.M, c.N)
    kw, rk = {}, {}
    if epi in ("full", "drop", "relu_bias"):
        kw.update(bias=torch.from_numpy(bias).to(D), act=1)
        rk.update(bias=bias, act=1)
    if epi in ("full", "bwd"):
        kw.update(mask=_pitched(mask))
        rk.update(mask=mask)
    if epi == "drop":
        dbuf = torch.zeros((c.M, c.N + 12), dtype=torch.uint8, device=D)
        dbuf[:, :c.N] = torch.from_numpy(drop).to(D)
        kw.update(drop=dbuf[:, :c.N])
        rk.update(drop=drop)
    if epi in ("drop", "bwd"):
        kw.update(keep_prob=0.5)
        rk.update(keep_prob=0.5)
    rows = c.M if c.m_dev is None else c.m_dev
    ref = gx.reference(A, A2, B, rows=rows, k=c.k_dev, **rk)
    buf, C = _poisoned_c(c.M, c.N, pad)
    _poison_workspace(c.M, c.N, c.K, c.m_dev is not None, c.prec)
    ph.gemm(_dev(A, c.at), _dev(B, c.bt), C, a_trans=c.at, b_trans=c.bt, A2=_dev(A2, c.at), M_dev=_counter(c.m_dev),
            K_dev=_counter(c.k_dev), M=c.M, N=c.N, K=c.K, precision=c.prec, **kw)
    _assert_result(buf, c.N, rows, ref, f"{what or c.group} {gx.FAMILY[c.prec]} {c.M}x{c.N}x{c.K} ({c.at},{c.bt}) a2={c.a2} "
                   f"m_dev={c.m_dev} k_dev={c.k_dev} {cls} {epi}")


def _classes(prec):
    return gx.FAMILY_CLASSES[gx.FAMILY[prec]]


def _by_layout(group, prec, at, bt):
    return [c for c in gx.cases(group, prec) if (c.at, c.bt) == (at, bt)]


# ---------------------------------------------------------------------------
# The variant matrix: layout x ragged x A + A2 x form, 48 ids per family

MATRIX = [(form, at, bt, rg, a2) for form in gx.FORMS for at, bt in gx.LAYOUTS for rg in (0, 1) for a2 in (0, 1)]
_mid = lambda v: f"{v[0]}-{'t' if v[1] else 'n'}{'t' if v[2] else 'n'}-{'ragged' if v[3] else 'whole'}-{'a2' if v[4] else 'a'}"  # noqa: E731


@pytest.mark.parametrize("variant", MATRIX, ids=_mid)
def test_x6_variant(hip, variant):
    c = gx.matrix_case(2, *variant)
    for i, cls in enumerate(_classes(2)):
        run(c, cls, "full" if i == 0 else "bare")


@pytest.mark.parametrize("variant", MATRIX, ids=_mid)
def test_x3_variant(hip, variant):
    c = gx.matrix_case(1, *variant)
    for i, cls in enumerate(_classes(1)):
        run(c, cls, "full" if i == 0 else "bare")


@pytest.mark.parametrize("at,bt", gx.LAYOUTS)
def test_fp32_layouts(hip, at, bt):
    """The fp32 MFMA kernel multiplies fp32 by fp32: exact on dense4 and a19."""
    for c in _by_layout("f32", 0, at, bt):
        run(c, "dense4", "full")
        run(c, "a19", "bare")


# ---------------------------------------------------------------------------
# The edges inside one variant

EDGE = [(prec, at, bt) for prec in (2, 1) for at, bt in gx.EDGE_LAYOUTS]
_eid = lambda v: f"{gx.FAMILY[v[0]]}-{'t' if v[1] else 'n'}{'t' if v[2] else 'n'}"  # noqa: E731


def _plane_class(prec):
    return "a19" if prec == 2 else "a15"


@pytest.mark.parametrize("group", ["live256", "live128"])
@pytest.mark.parametrize("edge", EDGE, ids=_eid)
def test_live_accumulator_blocks(hip, edge, group):
    """Device-side M over every count of live 32-row accumulator blocks of a
    wave (the K loop's amw specialisations) and both wm halves; M_dev = 0
    leaves C untouched."""
    for c in _by_layout(group, *edge):
        for i, cls in enumerate(_classes(c.prec)):
            run(c, cls, "full" if i == 0 else "bare")


@pytest.mark.parametrize("edge", EDGE, ids=_eid)
def test_k_steps(hip, edge):
    """One K step, two, odd and even counts (the look-ahead load clamped to the
    last step), K tails of 1 .. BK - 1."""
    for c in _by_layout("ksteps", *edge):
        for i, cls in enumerate(_classes(c.prec)):
            run(c, cls, "full" if i == 0 else "bare")


@pytest.mark.parametrize("prec", [2, 1])
def test_device_k(hip, prec):
    """K on the device in the dW layout; K_dev = 0 gives epilogue(0) = relu(bias)."""
    for c in gx.cases("kdev", prec):
        for i, cls in enumerate(_classes(prec)):
            run(c, cls, "relu_bias" if i == 0 else "bare")
        if c.k_dev == 0:
            bias = gx.epilogue_operands(c.M, c.N)[0]
            ref = gx.reference(*_ops("dense4", c.M, c.N, c.K, False), bias=bias, act=1, k=0)
            assert np.array_equal(ref, np.broadcast_to(np.maximum(bias, 0), (c.M, c.N)))


@pytest.mark.parametrize("how", ["vector", "odd_pitch", "drop", "device_m"])
@pytest.mark.parametrize("edge", EDGE, ids=_eid)
def test_split_k_with_empty_slices(hip, edge, how):
    """S = 32 slices of which the last ones get no K step: with the workspace
    poisoned, an empty slice that did not write zeros is a NaN.  Through the
    reduce's float4 path, its scalar path (odd C pitch), with dropout, and with
    a device-side M (the device re-plans; the host sized the slabs for M = 1)."""
    if how == "device_m":
        for c in _by_layout("splitk_mdev", *edge):
            for i, cls in enumerate(_classes(c.prec)):
                run(c, cls, "full" if i == 0 else "bare")
        return
    c, = _by_layout("splitk", *edge)
    pad = 9 if how == "odd_pitch" else 8
    for i, cls in enumerate(_classes(c.prec)):
        run(c, cls, "drop" if how == "drop" else ("full" if i == 0 else "bare"), pad=pad, what=f"splitk {how}")


@pytest.mark.parametrize("form", ["t128", "t256lean"])
@pytest.mark.parametrize("edge", EDGE, ids=_eid)
def test_more_than_one_item_per_workgroup(hip, edge, form):
    """The persistent loop's second round (576 tiles on 288 workgroups, 289 on
    152): the second item reuses the LDS stages and the accumulators of the
    first.  The reference is a device fp64 matmul (exact on these operands)."""
    prec, at, bt = edge
    c, = [c for c in _by_layout("multi", *edge) if (c.M, c.N, c.K) == gx.MULTI[form]]
    for cls in ("dense4", _plane_class(prec)):
        A, _, B = _ops(cls, c.M, c.N, c.K, False)
        ref = torch.from_numpy(A).to(D).double() @ torch.from_numpy(B).to(D).double()
        buf, C = _poisoned_c(c.M, c.N)
        _poison_workspace(c.M, c.N, c.K, False, prec)
        ph.gemm(_dev(A, at), _dev(B, bt), C, a_trans=at, b_trans=bt, M=c.M, N=c.N, K=c.K, precision=prec)
        _assert_result(buf, c.N, c.M, ref, f"multi {form} {gx.FAMILY[prec]} ({at},{bt}) {cls}")


@pytest.mark.parametrize("edge", EDGE, ids=_eid)
def test_keep_in_epilogue(hip, edge):
    """Tile 128: keep_prob = 0.5 with a mask and no drop mask is scaled inside
    the GEMM's epilogue; with a drop mask the reduce scales.  Both exact."""
    c, = _by_layout("keep", *edge)
    for cls in _classes(c.prec):
        run(c, cls, "bwd")
        run(c, cls, "drop")


# ---------------------------------------------------------------------------
# gemm_tp against the integer reference (not only against the staged kernel)


def _tp(src, rows, K, rs, ks, rows_dev=None, K_dev=None):
    out = torch.full((ph.tp_bytes(rows, K),), 0xAB, dtype=torch.uint8, device=D)
    return ph.split_tp(src, rows, K, out, rs, ks, rows_dev=rows_dev, K_dev=K_dev)


@pytest.mark.parametrize("shape,m_dev,k_dev", gx.TP_SHAPES, ids=["static", "device_m", "device_k"])
def test_gemm_tp_exact(hip, shape, m_dev, k_dev):
    M, N, K = shape
    bias, mask, _ = gx.epilogue_operands(M, N)
    Md, Kd = _counter(m_dev), _counter(k_dev)
    rows = M if m_dev is None else m_dev
    for i, cls in enumerate(_classes(2)):
        A, _, B = _ops(cls, M, N, K, False)
        if k_dev is None:  # forward form: A (M, K) rows, B (K, N)
            At = _tp(torch.from_numpy(A).to(D), M, K, K, 1, rows_dev=Md)
            Bt = _tp(torch.from_numpy(B).to(D), N, K, 1, N)
        else:  # dW form: A stored (K, M), B (K, N), K rows live on the device
            At = _tp(torch.from_numpy(np.ascontiguousarray(A.T)).to(D), M, K, 1, M, K_dev=Kd)
            Bt = _tp(torch.from_numpy(B).to(D), N, K, 1, N, K_dev=Kd)
        kw, rk = {}, {}
        if i == 0:
            kw = dict(bias=torch.from_numpy(bias).to(D), act=1, mask=_pitched(mask))
            rk = dict(bias=bias, act=1, mask=mask)
        buf, C = _poisoned_c(M, N)
        _poison_workspace(M, N, K, m_dev is not None, 2)
        ph.gemm_tp(At, Bt, C, M, N, K, M_dev=Md, K_dev=Kd, **kw)
        _assert_result(buf, N, rows, gx.reference(A, None, B, rows=rows, k=k_dev, **rk), f"gemm_tp {shape} {cls}")


# ---------------------------------------------------------------------------
# fp32-faithfulness on full-mantissa operands, one small shape per form

FAITHFUL = {"t128": (160, 96, 2048), "t256gen": (300, 320, 2048), "t256lean": (300, 320, 200)}


def _errs(C, ref):
    e = (C.double() - ref).abs()
    return float(e.max()), float(e.mean())


@pytest.mark.parametrize("at,bt", gx.LAYOUTS)
@pytest.mark.parametrize("form", gx.FORMS)
def test_fp32_faithful_small(hip, form, at, bt):
    """test_gpu_gemm_fc6.py's criterion at a small shape of each kernel form:
    on randn operands at the step's scales (features ~N(0, 1), weights
    N(0, 0.001^2)) x6's max and mean absolute error against an fp64 product
    are at most 2x those of torch's fp32 matmul, and x3 fails the same
    criterion (the contrast that shows the check discriminates).

    Measured on an MI355X, error relative to torch's fp32 matmul, over the four
    layouts: tile 128 (160 x 96 x 2048, splits K) x6 max 0.36-0.45, mean
    0.46-0.47, x3 max 7.5-8.7, mean 11.2-11.4; tile 256 split (300 x 320 x
    2048) x6 max 0.32-0.39, mean 0.46-0.47, x3 max 6.4-7.9, mean 11.3-11.4;
    tile 256 lean (300 x 320 x 200) x6 max 0.62-0.89, mean 0.81-0.82, x3 max
    6.8-8.8, mean 19.8-19.9.  The 2x factor is test_gpu_gemm_fc6.py's; at
    these K x6 meets it with room and x3 misses it by 3x or more."""
    M, N, K = FAITHFUL[form]
    g = torch.Generator(device=D).manual_seed(31 + 2 * at + bt)
    torch.backends.cuda.matmul.allow_tf32 = False
    A = torch.randn((M, K), generator=g, device=D)
    B = torch.randn((K, N), generator=g, device=D) * 1e-3
    ref = A.double() @ B.double()
    fmax, fmean = _errs(A @ B, ref)
    As, Bs = (A.T.contiguous() if at else A), (B.T.contiguous() if bt else B)
    out = {}
    for prec in (2, 1):
        C = torch.empty((M, N), device=D)
        ph.gemm(As, Bs, C, a_trans=at, b_trans=bt, M=M, N=N, K=K, precision=prec)
        out[prec] = _errs(C, ref)
    (emax, emean), (xmax, xmean) = out[2], out[1]
    print(f"faithful {form} ({at},{bt}) {M}x{N}x{K}: x6/fp32 max {emax / fmax:.2f} mean {emean / fmean:.2f}; "
          f"x3/fp32 max {xmax / fmax:.1f} mean {xmean / fmean:.1f}; fp32 max/mean {fmax:.3e}/{fmean:.3e}")
    assert emax <= 2 * fmax and emean <= 2 * fmean
    assert not (xmax <= 2 * fmax and xmean <= 2 * fmean)
