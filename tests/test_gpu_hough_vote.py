"""GPU parity of the Hough vote on the hand-built voters of
tests/hough_cases.py: the whole count map of every present class and every op
output against the oracle's brute-force per-cell loop, over inlier thresholds
on both sides of the fast window of voter_cone (csrc/hough_compact.hip).

Every comparison is of integers or of bit patterns; there is no tolerance.
(The one thing not compared is the sign / payload of a NaN: which quiet NaN an
invalid operation produces is the hardware's choice, not the op's.)
tests/test_hough_cases.py shows on the oracle alone that these inputs reach
the conditions they are aimed at."""
import numpy as np
import pytest
import torch

import hough_cases as hc
from posecnn_amd.hough_voting_gpu_layer import hough_voting_gpu_op as hv

pytestmark = pytest.mark.gpu
D = torch.device("cuda")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(D)


def _bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype != np.float32:
        return a
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


def _run(fr, gt, is_train, thr, skip, vote_thr=-1.0, label_threshold=0, counts=False, vertex=None, **kw):
    """One call of the op; returns (outputs, row count, diag, count maps)."""
    B, H, W = fr["label"].shape
    C = fr["extents"].shape[0]
    dbg = torch.zeros((B, C - 1, H, W), dtype=torch.int32, device=D) if counts else None
    label = None if "prob" in kw else T(fr["label"])
    o = hv.hough_voting_gpu_capacity(label, T(fr["vertex"] if vertex is None else vertex), T(fr["extents"]),
                                     T(fr["meta"]), T(gt), is_train, vote_thr, 0.02, skip, inlier_threshold=thr,
                                     label_threshold=label_threshold, debug_counts=dbg, **kw)
    torch.cuda.synchronize()
    n = int(o["num_rois"][1].item())
    res = [o[k][:n].cpu().numpy() for k in ("box", "pose", "target", "weight", "domain")]
    return res, int(o["num_rois"][0].item()), hv.hough_voting_diag(o), (dbg.cpu().numpy() if counts else None)


def _check_counts(orc, fr, thr, skip, vote_thr=-1.0, label_threshold=0):
    """(a) dbg[b, slot] == the oracle's count map of the slot's class, slots in
    ascending class order; the slots past the present classes stay zero."""
    _, _, diag, dbg = _run(fr, fr["gt"], 0, thr, skip, vote_thr, label_threshold, counts=True)
    B = fr["label"].shape[0]
    C = fr["extents"].shape[0]
    for b in range(B):
        present = hc.present_classes(fr["label"][b], C, label_threshold)
        for s, c in enumerate(present):
            oc, _, _ = orc.hough_class_counts(fr["label"][b], fr["vertex"][b], fr["extents"], fr["meta"][b], c, skip,
                                              inlier_threshold=thr)
            np.testing.assert_array_equal(dbg[b, s], oc.astype(np.int32), err_msg=f"image {b} class {c}")
        assert not dbg[b, len(present):].any()
    assert diag[0] == 0
    return dbg


def _check_outputs(orc, fr, thr, skip, vote_thr=-1.0, label_threshold=0):
    """(b) every op output bit-equal to the oracle's, without debug_counts (so
    the vote takes its empty-band exit), is_train 0 / 1, no GT / one GT row per
    class."""
    rows = []
    for gt in (fr["gt"], hc.gt_rows(fr)):
        for is_train in (0, 1):
            got, n, diag, _ = _run(fr, gt, is_train, thr, skip, vote_thr, label_threshold)
            want = orc.hough_voting(fr["label"], fr["vertex"], fr["extents"], fr["meta"], gt, is_train, vote_thr,
                                    0.02, skip, inlier_threshold=thr, label_threshold=label_threshold)
            assert n == want[5]
            for name, g, w in zip(("box", "pose", "target", "weight", "domain"), got, want):
                np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=name)
            assert diag[0] == 0, "interval vote count != exact re-count"
            if vote_thr > 0:
                assert diag[1] == 0, "NMS candidate overflow"
            rows.append(n)
    return rows


@pytest.mark.parametrize("family,thr,B,skip", hc.VOTE_CASES)
def test_count_maps(hip, orc, family, thr, B, skip):
    fr, _ = hc.frames_for(family, thr, B, skip)
    _check_counts(orc, fr, thr, skip)


@pytest.mark.parametrize("family,thr,B,skip", hc.VOTE_CASES)
def test_op_outputs(hip, orc, family, thr, B, skip):
    fr, _ = hc.frames_for(family, thr, B, skip)
    rows = _check_outputs(orc, fr, thr, skip)
    assert min(rows) > 0  # every present class emits its maximum, voted for or not


@pytest.mark.parametrize("family,thr,B,vote_thr", hc.NMS_CASES)
def test_nms_path(hip, orc, family, thr, B, vote_thr):
    """(c) the same vote kernel writing ws.counts for the multi-instance path."""
    fr, _ = hc.frames_for(family, thr, B, 1)
    _check_counts(orc, fr, thr, 1, vote_thr=vote_thr)
    rows = _check_outputs(orc, fr, thr, 1, vote_thr=vote_thr)
    assert min(rows) >= 2


@pytest.mark.parametrize("thr", [0.9, 0.05, 0.999, 1.0])
def test_specials_compact_vertex(hip, thr):
    """magnitude_sweep + depth_specials through the class-compact (B,H,W,3)
    vertex map, gathered from the full one: equal to the label path bit for bit."""
    fr, _ = hc.specials_batch()
    lab = fr["label"]
    b, y, x = np.indices(lab.shape)
    v3 = np.stack([fr["vertex"][b, y, x, 3 * lab + j] for j in range(3)], axis=-1).astype(np.float32)
    gt = hc.gt_rows(fr)
    a, na, _, ca = _run(fr, gt, 1, thr, 1, counts=True)
    c, nc, diag, cc = _run(fr, gt, 1, thr, 1, counts=True, vertex=v3, vertex_compact=True)
    assert na == nc > 0 and diag[0] == 0
    for g, w in zip(c, a):
        np.testing.assert_array_equal(_bits(g), _bits(w))
    np.testing.assert_array_equal(cc, ca)


@pytest.mark.parametrize("thr", [0.9, 0.05, 0.999, 1.0])
def test_specials_from_prob(hip, thr):
    """The same frames with the label produced inside the op from a one-hot
    prob map: equal to the label path bit for bit."""
    fr, _ = hc.specials_batch()
    C = fr["extents"].shape[0]
    prob = np.eye(C, dtype=np.float32)[fr["label"]]
    gt = hc.gt_rows(fr)
    a, na, _, ca = _run(fr, gt, 1, thr, 1, counts=True)
    p, npb, diag, cp = _run(fr, gt, 1, thr, 1, counts=True, prob=T(prob))
    assert na == npb > 0 and diag[0] == 0
    for g, w in zip(p, a):
        np.testing.assert_array_equal(_bits(g), _bits(w))
    np.testing.assert_array_equal(cp, ca)


def test_label_threshold_edge(hip, orc):
    """A class of exactly n pixels is absent at label_threshold = n and
    present at n - 1 (cu.cc:654-664: size > labelThreshold)."""
    case = hc.label_threshold_edge()
    fr = hc.case_frame(case)
    n = case.info["n"]
    for lt, classes in ((n, [2]), (n - 1, [1, 2])):
        assert hc.present_classes(fr["label"][0], case.C, lt) == classes
        _check_counts(orc, fr, 0.9, 1, label_threshold=lt)
        assert _check_outputs(orc, fr, 0.9, 1, label_threshold=lt) == [len(classes), 9 * len(classes)] * 2
