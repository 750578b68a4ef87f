"""CPU checks of the numpy restatement of the evaluation ops
(tests/pose_eval_ref.py): the float32 order against a float64 form with a
kd-tree, hand-computed answers, the padding rule, the tally and the confusion
matrix against brute-force loops; and of include/posecnn_eval.h against
posecnn_amd/evaluate.py's signature table, the built library's exports and
the entry points' host-side refusals."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import abi_guard
import pose_eval_ref as per

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVAL_HEADER = os.path.join(ROOT, "include", "posecnn_eval.h")
F = np.float32
EPS = 2.0 ** -24  # the unit roundoff of float32


def rot(axis, angle):
    """Rodrigues' formula, float64."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    S = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * S + (1 - np.cos(angle)) * (S @ S)


def rt_of(R, t):
    return np.concatenate([np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3, 1)], axis=1).astype(F)


def random_pair(rng, dt, dr):
    """A ground-truth pose at 0.5-2 m and an estimate dt metres and dr radians off it."""
    Rg = rot(rng.standard_normal(3), rng.uniform(0, np.pi))
    z = rng.uniform(0.5, 2.0)
    tg = np.array([rng.uniform(-0.3, 0.3) * z, rng.uniform(-0.2, 0.2) * z, z])
    d = rng.standard_normal(3)
    Re = rot(rng.standard_normal(3), dr) @ Rg
    return rt_of(Re, tg + dt * d / np.linalg.norm(d)), rt_of(Rg, tg)


def test_float32_order_against_float64_kdtree():
    """12 poses of the dataset's models, perturbed by 1e-4 m .. 5 cm and
    1e-3 .. 1 rad.  A camera-frame coordinate is three products and three
    sums of terms no larger than m = the largest |coordinate| of either point
    set, a distance three differences, three squares, two sums and a root of
    such coordinates, each rounding at most 2^-24 of its operand: the bound on
    ADD, ADD-S and te is 16 2^-24 m (2.4e-6 m at 2.5 m; the float64 means add
    nothing visible).  re is float64 throughout and differs by its one
    rounding to float32.  A pixel coordinate u = (fx X + px Z) / Z moves by at
    most (fx / Z) (dX + |X / Z| dZ) under coordinate errors dX, dZ <= 6 2^-24
    m (the six roundings above) plus its own five roundings of magnitude
    |u|: the bound on reproj is 16 2^-24 (m g + umax), g = the largest
    (f / Z)(1 + |X| / Z) over the points."""
    from posecnn_amd import synth
    mdl = synth.models()
    pts_all, K = mdl["lov_points"], mdl["K"].astype(F)
    rng = np.random.default_rng(5)
    dts = np.geomspace(1e-4, 5e-2, 12)
    drs = np.geomspace(1e-3, 1.0, 12)
    worst = np.zeros(5)
    for i in range(12):
        c = 1 + i % (len(pts_all) - 1)
        pts = pts_all[c].astype(F)
        rt_e, rt_g = random_pair(rng, dts[i], drs[i])
        got = per.pose_errors_row(rt_e, rt_g, pts, K).astype(np.float64)
        want = per.pose_errors64(rt_e, rt_g, pts, K)
        assert got.dtype == np.float64 and per.pose_errors_row(rt_e, rt_g, pts, K).dtype == F
        cam = [pts.astype(np.float64) @ r[:, :3].astype(np.float64).T + r[:, 3] for r in (rt_e, rt_g)]
        m = max(np.abs(p).max() for p in cam)
        f = float(max(K[0, 0], K[1, 1]))
        g = max((f / p[:, 2] * (1 + np.abs(p[:, :2]).max(axis=1) / p[:, 2])).max() for p in cam)
        umax = max(np.abs((p @ K.astype(np.float64).T)[:, :2] / p[:, 2:]).max() for p in cam)
        bar = 16 * EPS * m
        err = np.abs(got - want)
        worst = np.maximum(worst, err)
        assert err[0] <= bar and err[1] <= bar and err[3] <= bar, (i, err, bar)
        assert err[2] <= 2 * EPS * want[2] + 1e-9, (i, err[2], want[2])
        assert err[4] <= 16 * EPS * (m * g + umax), (i, err[4])
        assert abs(want[0] - dts[i]) < 0.2 * dts[i] + drs[i] * 0.2  # the perturbation is what is measured
    print("worst |float32 form - float64 form|: ADD %.3g m, ADD-S %.3g m, re %.3g deg, te %.3g m, reproj %.3g px"
          % tuple(worst))


def test_pure_translation_and_known_rotation():
    from posecnn_amd import synth
    mdl = synth.models()
    pts, K = mdl["lov_points"][3].astype(F), mdl["K"].astype(F)
    Rg = rot([1, 2, 3], 0.7)
    # d with exactly representable components and norm: (0.03125, 0, 0.0625) * ... -> use a 3-4-5 triple
    d = np.array([3, 0, 4]) * 2.0 ** -8  # |d| = 5 / 256
    rt_g, rt_e = rt_of(Rg, [0.1, -0.05, 1.0]), rt_of(Rg, np.array([0.1, -0.05, 1.0]) + d)
    e = per.pose_errors_row(rt_e, rt_g, pts, K)
    tnorm = np.linalg.norm(rt_e[:, 3].astype(np.float64) - rt_g[:, 3].astype(np.float64))
    assert e[3] == F(tnorm) and abs(tnorm - 5 / 256) < 4 * EPS
    assert abs(float(e[0]) - tnorm) <= 16 * EPS * 1.3  # ADD = |d| (coordinates up to ~1.3 m)
    # re: the float32 entries leave trace(R R^T) within 6 2^-24 of 3, and acos(1 - x) = sqrt(2 x)
    assert 0 <= e[2] <= np.degrees(np.sqrt(6 * EPS)) and 0 < e[1] <= e[0] and e[4] > 0
    # a rotation by a known angle about an axis through the origin (t = 0 for both): re = the angle
    for deg in (0.5, 30.0, 90.0, 179.0):
        Re = rot([0, 0, 1], np.radians(deg)) @ Rg
        e = per.pose_errors_row(rt_of(Re, [0, 0, 0]), rt_of(Rg, [0, 0, 0]), pts, K)
        # the float32 entries of both matrices move the trace by <= 9 * 2 * 2^-24: d(angle) = d(tr) / (2 sin)
        tol = np.degrees(18 * EPS / (2 * np.sin(np.radians(deg)))) + 2 * EPS * deg
        assert abs(float(e[2]) - deg) <= tol, (deg, e[2])
        assert e[3] == 0
    # identical poses: the four distances are exactly 0
    assert (per.pose_errors_row(rt_g, rt_g, pts, K)[[0, 1, 3, 4]] == 0).all()


def mirrored_box(P=400):
    """Points on a box surface, the second half the first turned by half a turn about z: exactly symmetric."""
    from posecnn_amd import synth
    half = synth.box_points(np.array([[0, 0, 0], [0.1, 0.16, 0.06]]), P=P // 2, seed=4)[1]
    return np.concatenate([half, half * np.array([-1, -1, 1], F)]).astype(F)


def test_half_turn_about_a_symmetry_axis():
    pts = mirrored_box()
    from posecnn_amd import synth
    K = synth.models()["K"].astype(F)
    Rg = rt_of(rot([2, -1, 0.5], 1.1), [0.2, 0.1, 0.9])
    Re = Rg.copy()
    Re[:, :2] = -Re[:, :2]  # R_gt diag(-1, -1, 1): exact in float32
    e = per.pose_errors_row(Re, Rg, pts, K)
    assert e[1] == 0 and e[0] > 0.02 and e[3] == 0
    assert abs(float(e[2]) - 180.0) < 0.1
    assert abs(per.pose_errors64(Re, Rg, pts, K)[1]) < 1e-12


def padded_problem():
    """Class 1: 40 points near (0.1, 0, 0) in a (2, 64, 3) array whose padding is zeros; the estimate is
    the ground truth moved by +0.08 in x, so the estimate-transformed ORIGIN (a padding point) would be
    0.02 from the ground-truth points, far nearer than any real candidate (~0.08)."""
    rng = np.random.default_rng(2)
    n, P = 40, 64
    points = np.zeros((2, P, 3), F)
    points[1, :n] = (np.array([0.1, 0, 0]) + rng.uniform(-0.005, 0.005, (n, 3))).astype(F)
    rt_g = rt_of(np.eye(3), [0, 0, 1.0])[None]
    rt_e = rt_of(np.eye(3), [0.08, 0, 1.0])[None]
    return points, np.array([0, n], np.int32), rt_e, rt_g


def test_padding_is_never_a_candidate_or_a_query():
    from posecnn_amd import synth
    K = synth.models()["K"].astype(F)
    points, num, rt_e, rt_g = padded_problem()
    n = int(num[1])
    got = per.pose_errors([1], rt_e, rt_g, points, num, K)
    tight = per.pose_errors([1], rt_e, rt_g, points[:, :n].copy(), num, K)
    np.testing.assert_array_equal(got.view(np.int32), tight.view(np.int32))
    assert 0.07 < got[0, 1] <= got[0, 0] and abs(got[0, 0] - 0.08) < 1e-6
    read = per.pose_errors([1], rt_e, rt_g, points, np.array([0, points.shape[1]], np.int32), K)
    assert read[0, 1] < 0.06  # with the padding read, the origin wins
    # garbage in the padding changes nothing
    points[1, n:] = 1e30
    np.testing.assert_array_equal(per.pose_errors([1], rt_e, rt_g, points, num, K).view(np.int32), got.view(np.int32))


def test_rows_that_are_not_scored_hold_minus_one():
    from posecnn_amd import synth
    K = synth.models()["K"].astype(F)
    points, num, rt_e, rt_g = padded_problem()
    points = np.concatenate([points, points[1:]])  # class 2: the same points, none valid
    num = np.array([5, 40, 0], np.int32)
    cls = np.array([1, 0, -1, 3, 2, 1], np.int32)
    e = per.pose_errors(cls, np.repeat(rt_e, 6, 0), np.repeat(rt_g, 6, 0), points, num, K, num_rows=5)
    assert (e[0] >= 0).all() and (e[1:] == -1).all()


def test_mean64_is_the_stated_order():
    v = np.arange(1, 601, dtype=F)
    assert per.mean64(v) == F(300.5)
    assert per.mean64(np.array([3.0], F)) == F(3.0)
    # float64 sums: 2^30 + 1 survives where a float32 sum would lose the 1
    assert per.mean64(np.array([2.0 ** 30, 1.0], F)) == F((2.0 ** 30 + 1) / 2)


def brute_tally(errors, cls, sym, thr, curve, rows):
    C, T = len(sym), len(curve)
    scored, correct = np.zeros(C, np.int64), np.zeros(C, np.int64)
    fa, fs = np.zeros((C, T + 1), np.int64), np.zeros((C, T + 1), np.int64)
    for i in range(rows):
        c = cls[i]
        if c <= 0 or c >= C or errors[i, 0] < 0:
            continue
        scored[c] += 1
        if (errors[i, 1] if sym[c] > 0 else errors[i, 0]) < thr[c]:
            correct[c] += 1
        for col, table in ((0, fa), (1, fs)):
            first = T
            for t in range(T):
                if errors[i, col] < curve[t]:
                    first = t
                    break
            table[c, first] += 1
    return scored, correct, fa, fs


def tally_problem(seed=0, N=200, C=5, T=20):
    rng = np.random.default_rng(seed)
    curve = ((np.arange(T) + 1.0) * 0.1 / T).astype(F)
    thr = rng.uniform(0.02, 0.06, C).astype(F)
    sym = np.array([0, 0, 1, 0, 1], F)[:C]
    cls = rng.integers(-1, C + 1, N).astype(np.int32)
    errors = rng.uniform(0, 0.12, (N, 5)).astype(F)
    errors[:, 1] = errors[:, 0] * rng.uniform(0.2, 1.0, N).astype(F)
    errors[rng.uniform(size=N) < 0.1] = -1          # rows pose_errors did not score
    errors[0], cls[0] = thr[1], 1                   # exactly the class threshold: not correct
    errors[1], cls[1] = np.nextafter(thr[1], F(0)), 1
    errors[2], cls[2] = curve[3], 3                 # exactly a curve threshold: the next slot
    errors[3], cls[3] = 0.0, 2
    errors[4], cls[4] = 0.5, 4                      # past every threshold: slot T
    return errors, cls, sym, thr, curve


def test_tally_against_brute_force():
    errors, cls, sym, thr, curve = tally_problem()
    for rows in (len(cls), 57, 0):
        got = per.tally(errors, cls, sym, thr, curve, num_rows=rows)
        for a, b in zip(got, brute_tally(errors, cls, sym, thr, curve, rows)):
            np.testing.assert_array_equal(a, b)
    s, c, fa, fs = per.tally(errors[:3], cls[:3], sym, thr, curve)
    assert s[1] == 2 and c[1] == 1                  # the strict <
    assert fa[3, 4] == 1 and fa[3, 3] == 0
    assert per.tally(errors[4:5], cls[4:5], sym, thr, curve)[2][4, len(curve)] == 1
    again = per.tally(errors, cls, sym, thr, curve, into=per.tally(errors, cls, sym, thr, curve))
    np.testing.assert_array_equal(again[0], 2 * per.tally(errors, cls, sym, thr, curve)[0])
    assert all(a.sum() == again[0].sum() for a in again[2:])


def test_confusion_against_brute_force():
    rng = np.random.default_rng(1)
    C = 6
    gt = rng.integers(-1, C + 1, 5000).astype(np.int32)       # includes -1 and C
    pred = rng.integers(-2, C + 2, 5000).astype(np.int32)     # includes out-of-range predictions
    hist, skipped = per.confusion(gt, pred, C)
    want, ws = np.zeros((C, C), np.int64), 0
    for g, p in zip(gt, pred):
        if 0 <= g < C:
            if 0 <= p < C:
                want[g, p] += 1
            else:
                ws += 1
    np.testing.assert_array_equal(hist, want)
    assert skipped == ws > 0 and hist.sum() + skipped == ((gt >= 0) & (gt < C)).sum()
    # with every prediction in range it is the reference's fast_hist verbatim
    pred = np.clip(pred, 0, C - 1)
    k = (gt >= 0) & (gt < C)
    np.testing.assert_array_equal(per.confusion(gt, pred, C)[0],
                                  np.bincount(C * gt[k].astype(int) + pred[k], minlength=C ** 2).reshape(C, C))


def test_evaluator_summary_on_the_host():
    """Two ground truths of class 1 and 2, three RoIs: both class-1 RoIs of image 0 are scored."""
    pts = np.stack([np.zeros((50, 3), F)] + [mirrored_box(50)] * 2)
    num = np.array([0, 50, 50], np.int32)
    ext = np.array([[0, 0, 0], [0.1, 0.16, 0.06], [0.1, 0.16, 0.06]], F)
    K = np.array([[500, 0, 320], [0, 500, 240], [0, 0, 1]], F)
    ev = per.Evaluator(pts, num, np.array([0, 0, 1], F), ext, K, curve_bins=10)
    q = [1, 0, 0, 0]
    gt = np.array([[0, 1, 0, 0, 0, 0] + q + [0, 0, 1], [1, 2, 0, 0, 0, 0] + q + [0, 0, 1]], F)
    rois = np.array([[0, 1, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0, 0], [0, 2, 0, 0, 0, 0, 0]], F)  # the last: wrong image
    poses = np.array([q + [0, 0, 1.001], q + [0, 0, 1.5], q + [0, 0, 1]], F)
    ev.update(rois, poses, gt)
    s = ev.summary()
    np.testing.assert_array_equal(s["count_all"], [0, 1, 1])
    np.testing.assert_array_equal(s["count_scored"], [0, 2, 0])
    np.testing.assert_array_equal(s["count_correct"], [0, 1, 0])
    assert np.isnan(s["accuracy"][0]) and s["accuracy"][1] == 1 and s["accuracy"][2] == 0
    assert s["add_curve"][1, 0] == 1 and s["add_curve"][1, -1] == 1 and s["add_auc"][1] == 1 and s["add_auc"][2] == 0
    ev.update_segmentation(np.array([0, 0, 1, 2, 255], np.int32), np.array([0, 1, 1, 1, 0], np.int32))
    s = ev.summary()
    assert s["overall_accuracy"] == 0.5 and s["hist"].sum() == 4 and s["skipped"] == 0
    np.testing.assert_allclose(s["iu"], [0.5, 1 / 3, 0])
    assert s["mean_iu"] == pytest.approx((0.5 + 1 / 3) / 3) and s["fwavacc"] == pytest.approx(0.5 * 0.5 + 0.25 / 3)


# ---- the header, the build and the library ----
def test_new_source_and_header_are_built():
    from posecnn_amd import build
    assert "pose_eval.hip" in build.SOURCES and "pose_eval.hip" not in build.NO_SLP
    assert os.path.abspath(EVAL_HEADER) in [os.path.abspath(h) for h in build.HEADERS]


def test_header_parses_and_matches_the_signature_table():
    from posecnn_amd import _lib, evaluate, optim
    protos = abi_guard.prototypes(header=EVAL_HEADER)
    assert set(protos) == set(evaluate.SIGS)
    assert not set(evaluate.SIGS) & set(_lib._SIGS) and not set(evaluate.SIGS) & set(optim.SIGS)
    ints = {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t, "long": ctypes.c_long}
    for name, params in protos.items():
        res, args = evaluate.SIGS[name]
        assert len(args) == len(params), name
        for p, a in zip(params, args):
            assert a is (ctypes.c_void_p if p.is_pointer else ints[p.c_type]), (name, p.name)
            assert not p.is_pointer or p.elem_type in abi_guard.ELEM, (name, p.name)
    decl = open(EVAL_HEADER).read()
    assert "size_t pcnn_pose_errors_workspace_size" in decl and "int pcnn_confusion" in decl
    assert '#include "posecnn_hip.h"' in decl


def test_library_exports_every_declared_function():
    from posecnn_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in out.stdout.splitlines() if line.strip()}
    missing = set(abi_guard.declarations(EVAL_HEADER)) - exported
    assert not missing, missing


@pytest.fixture(scope="module")
def lib():
    from posecnn_amd import evaluate
    return evaluate._load()


def test_versions_and_queries(lib):
    assert lib.pcnn_eval_abi_version() == 1
    assert lib.pcnn_abi_version() == 8 and lib.pcnn_train_abi_version() == 1
    assert lib.pcnn_pose_errors_chunk() == per.CHUNK
    assert lib.pcnn_pose_errors_workspace_size(0, 1) >= 24
    assert lib.pcnn_pose_errors_workspace_size(64, 2620) >= 64 * 11 * 3 * 8
    assert lib.pcnn_pose_errors_workspace_size(64, 2620) % 256 == 0
    assert lib.pcnn_pose_errors_workspace_size(1, 257) >= 2 * 3 * 8


def test_host_side_refusals_need_no_gpu(lib):
    """Each of these is refused by the argument check, before any HIP call; the
    pointers are never dereferenced."""
    fake = ctypes.c_void_p(0x1000)
    need = lib.pcnn_pose_errors_workspace_size(4, 100)
    ok = dict(cls=fake, rt_est=fake, rt_gt=fake, num_rows_dev=None, N_cap=4, points=fake, num_points=fake, C=3,
              P=100, K=fake, errors=fake, workspace=fake, workspace_bytes=need, stream=None)

    def errors(**kw):
        return lib.pcnn_pose_errors(*dict(ok, **kw).values())

    for name in ("cls", "rt_est", "rt_gt", "points", "num_points", "K", "errors", "workspace"):
        assert errors(**{name: None}) == 1, name
    assert errors(N_cap=-1) == 1 and errors(C=0) == 1 and errors(P=0) == 1
    assert errors(workspace_bytes=need - 1) == 1
    assert errors(workspace=ctypes.c_void_p(0x1004)) == 1
    assert errors(N_cap=(1 << 31) - 1, P=257, workspace_bytes=1 << 60) == 1
    assert errors(N_cap=0, cls=None, workspace=None, workspace_bytes=0) == 0  # nothing to do, nothing launched

    ok_t = dict(errors=fake, cls=fake, num_rows_dev=None, N_cap=4, symmetry=fake, thresholds=fake, C=3, curve_thr=fake,
                T=10, scored=fake, correct=fake, first_add=fake, first_adds=fake, stream=None)

    def tally(**kw):
        return lib.pcnn_pose_tally(*dict(ok_t, **kw).values())

    for name in ("errors", "cls", "symmetry", "thresholds", "curve_thr", "scored", "correct", "first_add",
                 "first_adds"):
        assert tally(**{name: None}) == 1, name
    assert tally(N_cap=-1) == 1 and tally(C=0) == 1 and tally(T=-1) == 1
    assert tally(N_cap=0) == 0

    ok_c = dict(gt=fake, pred=fake, n=10, C=22, hist=fake, skipped=fake, stream=None)

    def conf(**kw):
        return lib.pcnn_confusion(*dict(ok_c, **kw).values())

    for name in ("gt", "pred", "hist", "skipped"):
        assert conf(**{name: None}) == 1, name
    assert conf(n=-1) == 1 and conf(n=1 << 31) == 1 and conf(C=0) == 1 and conf(C=32769) == 1
    assert conf(gt=ctypes.c_void_p(0x1002)) == 1
    assert conf(n=0) == 0
    assert lib.pcnn_strerror(1) == b"invalid argument"


def test_quat_poses_to_rt():
    rng = np.random.default_rng(3)
    poses = rng.standard_normal((5, 7))
    poses[:, :4] *= 3.0  # not normalised
    rt = per.quat_poses_to_rt(poses)
    assert rt.dtype == F and rt.shape == (5, 3, 4)
    from posecnn_amd import synth
    for i in range(5):
        q = poses[i, :4] / np.linalg.norm(poses[i, :4])
        np.testing.assert_allclose(rt[i, :, :3], synth.quat2mat(q), atol=2 * EPS)
        np.testing.assert_array_equal(rt[i, :, 3], poses[i, 4:].astype(F))
        np.testing.assert_allclose(rt[i, :, :3].astype(np.float64) @ rt[i, :, :3].T, np.eye(3), atol=8 * EPS)
