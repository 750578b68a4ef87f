"""The ADD-S filtered search (bf16 MFMA filter + exact fp32 re-check of the
candidates inside the window) against the exact scan it replaces
(PCNN_ADD_SEARCH=scan): the same picks, so the same bits, at the MFMA block
edges (multiples of 32 +- 1), the padding and the chunk edges at 256; on
near-ties the filter cannot separate; per-item fallback on non-finite inputs;
and the search counters, which show that the filter, not the scan, ran."""
import os

import numpy as np
import pytest
import torch

from posecnn_amd.average_distance_loss import average_distance_loss_op as adl

import add_filter_ref as ref
from test_gpu_ops import _add_s_f64

pytestmark = pytest.mark.gpu
D = torch.device("cuda")
KPTS = 256  # query points per (row, chunk) item


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(D)


def _run(pred, target, weight, pts, sym, search=None):
    """(loss, bottom_diff, counters) of one loss call; search='scan' forces the exact scan."""
    R, P = pred.shape[0], pts.shape[1]
    ws = torch.zeros(adl.workspace_bytes(R, pts.shape[0], P), dtype=torch.uint8, device=D)
    old = os.environ.pop("PCNN_ADD_SEARCH", None)
    try:
        if search is not None:
            os.environ["PCNN_ADD_SEARCH"] = search
        loss, diff = adl.average_distance_loss(T(pred), T(target), T(weight), T(pts), T(sym), 0.01, workspace=ws)
        torch.cuda.synchronize()
    finally:
        os.environ.pop("PCNN_ADD_SEARCH", None)
        if old is not None:
            os.environ["PCNN_ADD_SEARCH"] = old
    return loss.cpu().numpy(), diff.cpu().numpy(), adl.search_stats(ws, R, pts.shape[0], P)


def _rows(rng, R, C, kind):
    """R rows on the symmetric classes 1, 2 (of C = 3) in turn."""
    pred = np.zeros((R, 4 * C), np.float32)
    target = np.zeros((R, 4 * C), np.float32)
    weight = np.zeros((R, 4 * C), np.float32)
    for r in range(R):
        c = 1 + r % 2
        qt = rng.normal(size=4)
        qt /= np.linalg.norm(qt)
        qp = rng.normal(size=4)
        if kind == "near":
            qp = qt + 0.02 * rng.normal(size=4)
        qp /= np.linalg.norm(qp)
        if kind == "scale1e-3":
            qp = rng.normal(size=4) * 1e-3
        if kind == "scale3":
            qp = rng.normal(size=4) * 3.0
        pred[r, 4 * c:4 * c + 4] = qp
        target[r, 4 * c:4 * c + 4] = qt
        weight[r, 4 * c:4 * c + 4] = 1
    return pred, target, weight


def _check_fast_path(st, sym_rows, P):
    nchunk = (P + KPTS - 1) // KPTS
    assert st["scan_items"] == 0, st
    assert st["filter_items"] == sym_rows * nchunk, st
    assert st["exact_evals"] >= sym_rows * P, st  # at least one per query point


@pytest.mark.parametrize("kind", ["random", "near", "scale1e-3", "scale3"])
@pytest.mark.parametrize("P", [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 641, 2620])
def test_filter_bitwise_against_scan(hip, P, kind):
    rng = np.random.default_rng(1000 * P + len(kind))
    C, R = 3, 6
    pts = rng.normal(size=(C, P, 3)).astype(np.float32)
    sym = np.array([0, 1, 1], np.float32)
    pred, target, weight = _rows(rng, R, C, kind)
    assert ref.rows_in_range(pred, target, weight, pts, sym)
    lf, df, st = _run(pred, target, weight, pts, sym)
    ls, ds, ss = _run(pred, target, weight, pts, sym, search="scan")
    np.testing.assert_array_equal(lf, ls)
    np.testing.assert_array_equal(df, ds)
    assert np.isfinite(lf).all() and np.isfinite(df).all()
    _check_fast_path(st, R, P)
    assert ss["filter_items"] == 0 and ss["exact_evals"] == 0 and ss["scan_items"] == R * ((P + KPTS - 1) // KPTS)


def test_filter_near_ties(hip):
    """Candidates the filter cannot tell apart: 40 duplicated model points, each
    copy one ulp off in one coordinate, and lattice coordinates (exact ties
    across 32-candidate blocks and across the waves' candidate ranges), with
    pred = identity and target (1, 0, 0, 1) = 2 x Rot90z.  The exact stage must
    decide them as the scan does (bitwise), which is numpy's fp32 argmin of the
    reference expression (_add_s_f64 at its tolerances)."""
    rng = np.random.default_rng(12)
    C, P, R = 3, 1500, 6
    pts = np.zeros((C, P, 3), np.float32)
    pts[1] = rng.normal(size=(P, 3)).astype(np.float32)
    for k in range(40):
        cp = pts[1, 10 + k].copy()
        a = k % 3
        cp[a] = np.nextafter(cp[a], np.float32(np.inf if k % 2 else -np.inf), dtype=np.float32)
        pts[1, P // 2 + 7 * k] = cp  # spread over blocks and wave ranges
    pts[2] = rng.integers(-3, 4, size=(P, 3)).astype(np.float32)
    sym = np.array([0, 1, 1], np.float32)
    pred = np.zeros((R, 4 * C), np.float32)
    target = np.zeros((R, 4 * C), np.float32)
    weight = np.zeros((R, 4 * C), np.float32)
    for r in range(R):
        c = 1 + r % 2
        pred[r, 4 * c:4 * c + 4] = [1, 0, 0, 0]
        target[r, 4 * c:4 * c + 4] = [1, 0, 0, 1]
        weight[r, 4 * c:4 * c + 4] = 1
    assert ref.rows_in_range(pred, target, weight, pts, sym)
    for c in (1, 2):  # the emulated filter keeps every pick inside its window on these clouds
        q, cand = ref.clouds(pred[c - 1, 4 * c:4 * c + 4], target[c - 1, 4 * c:4 * c + 4], pts[c])
        ok, inside, _, _ = ref.filter_verdict(q, cand)
        assert ok and inside
    lf, df, st = _run(pred, target, weight, pts, sym)
    ls, ds, _ = _run(pred, target, weight, pts, sym, search="scan")
    np.testing.assert_array_equal(lf, ls)
    np.testing.assert_array_equal(df, ds)
    _check_fast_path(st, R, P)
    l64, d64 = _add_s_f64(pred, target, weight, pts, 0.01)
    np.testing.assert_allclose(lf[0], l64, rtol=2e-6)
    np.testing.assert_allclose(df, d64, rtol=2e-5, atol=1e-6 * np.abs(d64).max())


@pytest.mark.parametrize("where", ["pred", "points"])
def test_filter_fallback_is_per_item(hip, where):
    """Non-finite predictions send only their own rows' items to the scan; a
    non-finite model point the items of every row of its class."""
    rng = np.random.default_rng(7)
    C, R, P = 3, 8, 641
    nchunk = 3
    pts = (rng.normal(size=(C, P, 3)) * np.array([1.0, 2.0, 0.5])).astype(np.float32)
    sym = np.array([0, 1, 1], np.float32)
    pred, target, weight = _rows(rng, R, C, "random")
    if where == "pred":
        pred[2, 4 * 1] = np.nan      # row 2 is on class 1, row 5 on class 2
        pred[5, 4 * 2 + 2] = np.inf
        scan_rows = 2
    else:
        pts[1, 17] = np.nan          # class 1: rows 0, 2, 4, 6
        scan_rows = 4
    lf, df, st = _run(pred, target, weight, pts, sym)
    ls, ds, _ = _run(pred, target, weight, pts, sym, search="scan")
    np.testing.assert_array_equal(lf, ls)  # NaN in the same places
    np.testing.assert_array_equal(df, ds)
    assert not np.isfinite(df).all() and np.isfinite(df).any()
    assert st["scan_items"] == scan_rows * nchunk, st
    assert st["filter_items"] == (R - scan_rows) * nchunk, st


def test_filter_fragment_layout_asymmetric(hip):
    """Query points and candidates that are different, non-symmetric clouds (an
    off-centre anisotropic model, unrelated rotations, the target scaled): a
    transposed fragment map -- candidates taken for queries -- gives other
    picks, which the float64 evaluation of numpy's fp32 picks exposes."""
    rng = np.random.default_rng(31)
    C, R, P = 3, 4, 333
    pts = (rng.normal(size=(C, P, 3)) * np.array([1.0, 2.5, 0.4]) + np.array([0.7, -0.3, 0.2])).astype(np.float32)
    sym = np.array([0, 1, 1], np.float32)
    pred, target, weight = _rows(rng, R, C, "random")
    target *= np.float32(0.8)
    assert ref.rows_in_range(pred, target, weight, pts, sym)
    lf, df, st = _run(pred, target, weight, pts, sym)
    _check_fast_path(st, R, P)
    l64, d64 = _add_s_f64(pred, target, weight, pts, 0.01)
    np.testing.assert_allclose(lf[0], l64, rtol=2e-6)
    np.testing.assert_allclose(df, d64, rtol=2e-5, atol=1e-6 * np.abs(d64).max())
