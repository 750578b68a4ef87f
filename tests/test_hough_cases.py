"""The hand-built Hough voters of tests/hough_cases.py do what they are meant
to: checked on the oracle alone (no GPU), for every family and every threshold
tests/test_gpu_hough_vote.py runs them at, so that the GPU comparison cannot
pass vacuously."""
import numpy as np
import pytest

import hough_cases as hc

f32 = np.float32


def _counts(orc, fr, b, cls, skip, thr):
    oc, _, _ = orc.hough_class_counts(fr["label"][b], fr["vertex"][b], fr["extents"], fr["meta"][b], cls, skip,
                                      inlier_threshold=thr)
    return oc.astype(np.int32)


def _single(orc, case, fr, i, thr, direction=None):
    """Oracle count map of voter i alone (optionally with another direction)."""
    x, y, cls, u, v, z = case.voters[i]
    label = np.zeros((case.H, case.W), np.int32)
    label[y, x] = cls
    vertex = fr["vertex"][0]
    if direction is not None:
        vertex = vertex.copy()
        vertex[y, x, 3 * cls:3 * cls + 2] = direction
    oc, _, _ = orc.hough_class_counts(label, vertex, fr["extents"], fr["meta"][0], cls, 1, inlier_threshold=thr)
    return oc.astype(np.int32)


def _intended_nonzero(family, cls, thr):
    """Whether class `cls` of the family is meant to collect votes at thr
    (None: no claim).  At thr = 1.5 no rounded cosine passes; only n1 == 0
    voters (the reference's dot / 0 = +inf) vote, and only magnitude_sweep has
    them.  At thr = 1.0 the fp32 quotient of an exactly aligned cell can round
    to 1 + ulp, so finite directions may or may not vote."""
    if family == "window" and cls == 2:
        return False
    if thr >= 1.0:
        if family == "magnitude_sweep":
            return True
        return False if thr > 1.0 else None
    return True


@pytest.mark.parametrize("family,thr,B,skip", hc.VOTE_CASES)
def test_count_maps_nonzero_where_intended(orc, family, thr, B, skip):
    fr, cases = hc.frames_for(family, thr, B, skip)
    for b, case in enumerate(cases):
        present = hc.present_classes(fr["label"][b], case.C)
        assert present == sorted({vt[2] for vt in case.voters})
        for cls in present:
            oc = _counts(orc, fr, b, cls, skip, thr)
            want = _intended_nonzero(case.name, cls, thr)
            assert want is None or bool(oc.any()) == want, (case.name, cls, thr)


@pytest.mark.parametrize("family", ["magnitude_sweep", "depth_specials", "plateaus", "window"])
def test_box_bookkeeping_matches_oracle(orc, family):
    """project_T's box equals the oracle's: at inlier_threshold = -2 a voter
    with a finite direction votes for its whole box minus its own cell."""
    case = hc.make_case(family)
    fr = hc.case_frame(case)
    idx = range(len(case.voters)) if family != "window" else range(0, len(case.voters), 37)
    radii = set()
    for i in idx:
        x, y, cls, u, v, z = case.voters[i]
        T = hc.project_T(case.extents, case.K, cls, z)
        oc = _single(orc, case, fr, i, -2.0, direction=(1.0, 0.0))
        np.testing.assert_array_equal(oc != 0, hc.box_mask(case.H, case.W, x, y, T))
        radii.add("inf" if np.isinf(T) else ("dead" if not T > 0 else "finite"))
    if family == "depth_specials":
        assert radii == {"inf", "dead", "finite"}
        inf_cls = {case.voters[i][2] for i in idx
                   if np.isinf(hc.project_T(case.extents, case.K, case.voters[i][2], case.voters[i][5]))}
        assert inf_cls == {2, 3}  # d == zHalf through extent z = 2 and through extent z = 0
        for cls in (2, 3):  # kmax is the capped radius while most voters have a few pixels
            Ts = [hc.project_T(case.extents, case.K, c, z) for (_, _, c, _, _, z) in case.voters if c == cls]
            assert sum(1 for T in Ts if 0 < T < 16) > len(Ts) // 2


@pytest.mark.parametrize("thr", hc.THRESHOLDS)
def test_direction_sweep_covers_quadrants_and_axes(thr):
    for seed in range(3):
        case = hc.direction_sweep(seed, thr)
        for cls in (1, 2):
            uv = np.array([(u, v) for (_, _, c, u, v, _) in case.voters if c == cls], np.float64)
            u, v = uv[:, 0], uv[:, 1]
            for su in (1, -1):
                for sv in (1, -1):
                    assert np.sum((su * u > 0) & (sv * v > 0)) >= 80
            for (au, av) in ((1, 0), (-1, 0), (0, 1), (0, -1)):
                assert np.any((np.sign(u) == au) & (np.sign(v) == av) & ((u == 0) | (v == 0)))
            assert np.sum((np.abs(u) == np.abs(v)) & (u != 0)) >= 4  # exact diagonals
        pos = {(x, y) for (x, y, c, _, _, _) in case.voters if c == 1}
        H, W = case.H, case.W
        assert {(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (W // 2, H - 1), (0, H // 2),
                (W - 1, H // 2)} <= pos
        assert case.info["ndirs"] >= 360 + 8 + 24


def test_direction_sweep_near_axis_boundaries():
    """At a fast threshold the +-acos(c -+ 2e-6) voters put one cone boundary
    within 1e-4 rad of a row or a column (2e-6 / sin(acos 0.998) = 3.2e-5)."""
    for thr in (0.9, 0.5, 0.0501, 0.998, 0.05):
        case = hc.direction_sweep(0, thr)
        c = float(f32(thr))
        near = 0
        for (_, _, cls, u, v, _) in case.voters:
            if cls != 1:
                continue
            a = np.arctan2(float(v), float(u))
            for s in (1, -1):
                b = (a + s * np.arccos(c)) % (np.pi / 2)
                near += min(b, np.pi / 2 - b) < 1e-4
        assert near >= 24


def _at_window_ends(case, kinds):
    """Fast and slow voters within 10 % of both ends of 1e-18 <= n1 <= 1e18."""
    n1 = lambda vt: float(np.hypot(np.float64(vt[3]), np.float64(vt[4])))
    slow = [n1(vt) for vt, k in zip(case.voters, kinds) if k == "slow" and np.isfinite(n1(vt))]
    fast = [n1(vt) for vt, k in zip(case.voters, kinds) if k == "fast"]
    return (any(0.9e-18 < n < 1e-18 for n in slow) and any(1e-18 < n < 1.1e-18 for n in fast)
            and any(1e18 < n < 1.1e18 for n in slow) and any(0.9e18 < n < 1e18 for n in fast))


@pytest.mark.parametrize("thr", hc.THRESHOLDS)
def test_magnitude_sweep_has_every_kind(orc, thr):
    case = hc.magnitude_sweep(0)
    fr = hc.case_frame(case)
    kinds = hc.classify_case(case, thr)
    assert kinds.count("dead") >= 1
    assert kinds.count("slow") >= 1
    if hc.fast_ok(thr):  # outside the window every live voter is slow
        assert kinds.count("fast") >= 10
        assert _at_window_ends(case, kinds)
    else:
        assert kinds.count("fast") == 0
    # a slow voter with n1 == 0 that does vote: dot / 0 = +inf > thr
    voting = [i for i, (vt, k) in enumerate(zip(case.voters, kinds))
              if k == "slow" and hc.n1_is_zero(vt[3], vt[4]) and _single(orc, case, fr, i, thr).any()]
    assert voting


def test_magnitude_sweep_scales_matter():
    """The bookkeeping tells a benign family apart: with every scale set to
    1.0 no voter sits at the n1 window's ends."""
    case = hc.magnitude_sweep(0, scales=(1.0,) * len(hc.MAGNITUDES))
    kinds = hc.classify_case(case, 0.9)
    assert kinds.count("fast") >= 10
    assert not _at_window_ends(case, kinds)


@pytest.mark.parametrize("thr", hc.THRESHOLDS)
def test_boundary_aimed_discriminates(orc, thr):
    for seed in range(3):
        case = hc.boundary_aimed(seed, thr)
        fr = hc.case_frame(case, seed)
        on = 0
        for i, (tx, ty) in enumerate(case.info["targets"]):
            x, y = case.voters[i][:2]
            box = _single(orc, case, fr, i, -2.0)
            assert box[ty, tx] == 1, "target outside the voter's box"
            assert box.sum() == box.astype(bool).sum() and box[y, x] == 0
            on += int(_single(orc, case, fr, i, thr)[ty, tx])
        n = len(case.voters)
        if -1.0 < thr < 1.0:
            assert 0.25 * n <= on <= 0.75 * n, (thr, on)
        elif thr > 1.0:  # no rounded cosine of a finite direction reaches 1.5
            assert on == 0
        # at thr = 1.0 the direction points exactly at the target and the fp32
        # quotient may round to 1 + ulp: no claim either way


def _reach(case, skip):
    """Sampled class-1 voters of `window` as (row, box radius), raster order."""
    vs = sorted((vt for vt in case.voters if vt[2] == 1), key=lambda vt: (vt[1], vt[0]))[::skip]
    out = []
    for (x, y, cls, u, v, z) in vs:
        T = hc.project_T(case.extents, case.K, cls, z)
        assert 2.0 <= T < 6.0
        out.append((y, int(np.ceil(T)) - 1))
    return out


@pytest.mark.parametrize("skip", [1, 3])
def test_window_bands(orc, skip):
    for seed in range(3):
        case = hc.window(seed, skip)
        fr = hc.case_frame(case, seed)
        reach = _reach(case, skip)
        assert len(reach) * skip >= 1500 and (skip > 1 or len(reach) > 3 * 512)
        kmax = max(k for _, k in reach)
        assert kmax == 5
        box_counts = _counts(orc, fr, 0, 1, skip, -2.0)  # every box cell but the voter's own
        for band in (2, 4):
            empty, partial = 0, 0
            for y0 in range(0, case.H, band):
                y1 = min(y0 + band, case.H)
                boxes = sum(1 for (y, k) in reach if y - k < y1 and y + k >= y0)
                seen = sum(1 for (y, _) in reach if y0 - kmax <= y <= y1 - 1 + kmax)  # the kernel's [ibeg, iend)
                assert boxes <= seen
                if boxes == 0:
                    assert not box_counts[y0:y1].any()
                empty += seen == 0
                partial += 0 < seen < len(reach)
            assert empty >= 1 and partial >= 1, (band, empty, partial)
        # the second class votes for nothing at any threshold
        for thr in hc.THRESHOLDS:
            assert not _counts(orc, fr, 0, 2, skip, thr).any()


@pytest.mark.parametrize("thr", hc.NMS_THRESHOLDS)
def test_plateaus_tie(orc, thr):
    for seed in range(3):
        case = hc.plateaus(seed)
        fr = hc.case_frame(case, seed)
        per = (case.W + 63) // 64  # columns per lane in the vote kernel's row scan
        for cls in (1, 2):
            oc = _counts(orc, fr, 0, cls, 1, thr)
            ys, xs = np.nonzero(oc == oc.max())
            assert oc.max() >= 4 and len(ys) >= 3
            assert len(set(ys // 4)) > 1 and len(set(ys // 2)) > 1
            assert len(set(xs // per)) > 1


def _candidates(oc, vote_thr):
    """NMS candidates of one count map (k_hough_nms_cand / cu.cc:351-365):
    above the threshold and no strictly larger count in the 7x7 window."""
    H, W = oc.shape
    pad = np.full((H + 6, W + 6), -1, np.int64)
    pad[3:-3, 3:-3] = oc
    mx = np.max([pad[dy:dy + H, dx:dx + W] for dy in range(7) for dx in range(7)], axis=0)
    return int(np.sum((oc.astype(np.float32) > np.float32(vote_thr)) & (oc >= mx)))


@pytest.mark.parametrize("family,thr,B,vote_thr", hc.NMS_CASES)
def test_nms_frames_are_in_range(orc, family, thr, B, vote_thr):
    """Every NMS-mode frame of the GPU test gives 2..128 rows and stays below
    the candidate capacity (so diag[1] == 0 is a condition the inputs meet)."""
    fr, cases = hc.frames_for(family, thr, B, 1)
    *_, n = orc.hough_voting(fr["label"], fr["vertex"], fr["extents"], fr["meta"], fr["gt"], 0, vote_thr, 0.02, 1,
                             inlier_threshold=thr, label_threshold=0)
    assert 2 <= n <= 128
    for b, case in enumerate(cases):
        ncand = sum(_candidates(_counts(orc, fr, b, cls, 1, thr), vote_thr)
                    for cls in hc.present_classes(fr["label"][b], case.C))
        assert 0 < ncand <= hc.KCAND_CAP


def test_label_threshold_edge(orc):
    case = hc.label_threshold_edge()
    fr = hc.case_frame(case)
    n = case.info["n"]
    assert np.sum(fr["label"] == 1) == n < np.sum(fr["label"] == 2)
    rows = {}
    for lt in (n, n - 1):
        box, *_, cnt = orc.hough_voting(fr["label"], fr["vertex"], fr["extents"], fr["meta"], fr["gt"], 0, -1.0, 0.02,
                                        1, label_threshold=lt)
        rows[lt] = [int(c) for c in box[:cnt, 1]]
    assert rows[n] == [2] and rows[n - 1] == [1, 2]
