"""The evaluation ops on the GPU (csrc/pose_eval.hip, posecnn_amd/evaluate.py)
against their numpy restatement tests/pose_eval_ref.py: pcnn_pose_errors bit
for bit in ADD, ADD-S, te and reproj and within one ulp in re, on every row;
pcnn_pose_tally and pcnn_confusion exactly; PoseEvaluator.summary() field by
field; and the header's contract at the ctypes boundary."""
import numpy as np
import pytest
import torch

import abi_guard
import pose_eval_ref as per
from test_pose_eval_ref import EVAL_HEADER, mirrored_box, padded_problem, random_pair, tally_problem

pytestmark = pytest.mark.gpu
D = torch.device("cuda")
F = np.float32
SENTINEL = -777.25


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(D)


def carve(shape, dtype=torch.float32, pad=64):
    """A contiguous tensor inside a sentinel-filled buffer, and a check that the buffer around it is intact."""
    n = int(np.prod(shape))
    mark = SENTINEL if dtype.is_floating_point else int(SENTINEL)
    buf = torch.full((n + 2 * pad,), mark, dtype=dtype, device=D)
    view = buf[pad:pad + n].view(*shape)

    def intact():
        b = buf.cpu().numpy()
        return bool((b[:pad] == mark).all() and (b[pad + n:] == mark).all())
    return view, intact


def camera():
    from posecnn_amd import synth
    return synth.models()["K"].astype(F)


def same_errors(got, want, what=""):
    """Every row: ADD, ADD-S, te, reproj the same bits; re within one ulp."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == F
    for col, name in ((0, "ADD"), (1, "ADD-S"), (3, "te"), (4, "reproj")):
        np.testing.assert_array_equal(got[:, col].view(np.int32), want[:, col].view(np.int32),
                                      err_msg=f"{what}: {name}")
    a, b = got[:, 2].astype(F), want[:, 2].astype(F)
    assert ((a >= 0) == (b >= 0)).all(), what
    ulp = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
    assert ulp.max(initial=0) <= 1, (what, "re", a, b)


def problem(P, N, C=3, seed=0, real=False):
    """Random pairs over C classes of P points; class c has P - (c - 1) valid points (at least 1)."""
    from posecnn_amd import synth
    rng = np.random.default_rng(seed)
    if real:
        points = synth.models()["lov_points"][:C, :P].astype(F).copy()
    else:
        points = (rng.standard_normal((C, P, 3)) * 0.06).astype(F)
    num = np.array([P] + [max(1, P - (c - 1)) for c in range(1, C)], np.int32)
    for c in range(1, C):
        points[c, num[c]:] = 0
    cls = (1 + np.arange(N) % (C - 1)).astype(np.int32)
    dts, drs = np.geomspace(1e-4, 5e-2, max(N, 1)), np.geomspace(1e-3, 1.0, max(N, 1))
    pairs = [random_pair(rng, dts[i], drs[i]) for i in range(N)]
    rt_e = np.stack([p[0] for p in pairs]) if N else np.zeros((0, 3, 4), F)
    rt_g = np.stack([p[1] for p in pairs]) if N else np.zeros((0, 3, 4), F)
    return cls, rt_e, rt_g, points, num


@pytest.mark.parametrize("P", [1, 63, 64, 65, 257, 2620])
def test_pose_errors_equal_the_restatement(hip, P):
    from posecnn_amd import evaluate
    K = camera()
    cls, rt_e, rt_g, points, num = problem(P, 4, real=P == 2620, seed=P)
    want = per.pose_errors(cls, rt_e, rt_g, points, num, K)
    got = evaluate.pose_errors(dev(cls), dev(rt_e), dev(rt_g), dev(points), dev(num), dev(K))
    torch.cuda.synchronize()
    assert (want >= 0).all()
    same_errors(got, want, f"P = {P}")


def test_pose_errors_tiled_candidates(hip):
    """P = 8200 > 8192: the candidates pass through LDS in two tiles with a running minimum."""
    from posecnn_amd import evaluate
    K = camera()
    cls, rt_e, rt_g, points, num = problem(8200, 2, seed=11)
    assert num[1] == 8200 and num[2] == 8199
    want = per.pose_errors(cls, rt_e, rt_g, points, num, K)
    got = evaluate.pose_errors(dev(cls), dev(rt_e), dev(rt_g), dev(points), dev(num), dev(K))
    torch.cuda.synchronize()
    same_errors(got, want, "P = 8200")
    # the points past the first tile count: without them the figures are others
    first_tile_only = per.pose_errors(cls, rt_e, rt_g, points, np.minimum(num, 8192), K)
    assert (first_tile_only[:, 1] != want[:, 1]).all()


def test_pose_errors_no_rows(hip):
    from posecnn_amd import evaluate
    K = camera()
    cls, rt_e, rt_g, points, num = problem(65, 0)
    got = evaluate.pose_errors(dev(cls), dev(rt_e), dev(rt_g), dev(points), dev(num), dev(K))
    torch.cuda.synchronize()
    assert tuple(got.shape) == (0, 5)


def mixed_problem():
    """N = 37 rows over C = 5 classes of P = 300: class 1 full, class 2 without points, class 3 the padded
    class of the CPU test (40 points, zeros behind them, a pose that makes the origin the nearest
    candidate), class 4 with 257 points; rows of class 0, -1 and C in between."""
    rng = np.random.default_rng(7)
    C, P, N = 5, 300, 37
    points = (rng.standard_normal((C, P, 3)) * 0.06).astype(F)
    pad_pts, pad_num, pad_e, pad_g = padded_problem()
    points[3] = 0
    points[3, :pad_pts.shape[1]] = pad_pts[1]
    num = np.array([P, P, 0, pad_num[1], 257], np.int32)
    points[4, 257:] = 0
    cls = np.array([1, 2, 3, 4, 0, -1, C, 1, 3, 4] * 4, np.int32)[:N]
    dts, drs = np.geomspace(1e-4, 5e-2, N), np.geomspace(1e-3, 1.0, N)
    pairs = [random_pair(rng, dts[i], drs[i]) for i in range(N)]
    rt_e, rt_g = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    rt_e[cls == 3], rt_g[cls == 3] = pad_e[0], pad_g[0]
    return cls, rt_e, rt_g, points, num


def test_pose_errors_mixed_rows_device_count_and_sentinels(hip):
    from posecnn_amd import evaluate
    K = camera()
    cls, rt_e, rt_g, points, num = mixed_problem()
    N, rows = len(cls), 30
    want = per.pose_errors(cls, rt_e, rt_g, points, num, K, num_rows=rows)
    assert (want[rows:] == -1).all() and (want[:rows][np.isin(cls[:rows], (0, -1, 5, 2))] == -1).all()
    assert (want[:rows][np.isin(cls[:rows], (1, 3, 4))] >= 0).all()
    trap = per.pose_errors(cls, rt_e, rt_g, points, np.where(np.arange(5) == 3, 64, num).astype(np.int32), K,
                           num_rows=rows)
    assert (trap[cls == 3][:2, 1] < 0.06).all() and (want[cls == 3][:2, 1] > 0.07).all()  # the padding is a trap
    out, intact = carve((N, 5))
    count = torch.tensor([rows], dtype=torch.int32, device=D)
    got = evaluate.pose_errors(dev(cls), dev(rt_e), dev(rt_g), dev(points), dev(num), dev(K), num_rows=count, out=out)
    torch.cuda.synchronize()
    assert got is out and intact()
    same_errors(got, want, "mixed rows")
    # without the device count every row below N_cap is considered; a count past N_cap is clamped
    want_all = per.pose_errors(cls, rt_e, rt_g, points, num, K)
    for nr in (None, torch.tensor([1000], dtype=torch.int32, device=D)):
        got = evaluate.pose_errors(dev(cls), dev(rt_e), dev(rt_g), dev(points), dev(num), dev(K), num_rows=nr, out=out)
        torch.cuda.synchronize()
        same_errors(got, want_all, "all rows")
        assert intact()


def test_pose_errors_same_bits_again_on_a_stream_and_from_a_graph(hip):
    from posecnn_amd import evaluate
    K = camera()
    cls, rt_e, rt_g, points, num = problem(257, 6, seed=3)
    args = [dev(a) for a in (cls, rt_e, rt_g, points, num, K)]
    first = evaluate.pose_errors(*args).clone()
    second = evaluate.pose_errors(*args).clone()
    torch.cuda.synchronize()
    same_errors(first, per.pose_errors(cls, rt_e, rt_g, points, num, K), "first run")
    assert torch.equal(first.view(torch.int32), second.view(torch.int32))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    out = torch.full((6, 5), SENTINEL, device=D)
    with torch.cuda.stream(s):
        evaluate.pose_errors(*args, out=out, stream=s)  # (also the warm-up of the capture below)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.int32), out.view(torch.int32))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        evaluate.pose_errors(*args, out=out)
    torch.cuda.synchronize()
    out.fill_(SENTINEL)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.int32), out.view(torch.int32))


def _tally_tensors(C, T):
    z = lambda *s: torch.zeros(s, dtype=torch.int64, device=D)  # noqa: E731
    return z(C), z(C), z(C, T + 1), z(C, T + 1)


def test_pose_tally_is_exact_and_accumulates(hip):
    from posecnn_amd import evaluate
    errors, cls, sym, thr, curve = tally_problem(N=1000)
    C, T = len(sym), len(curve)
    outs = _tally_tensors(C, T)
    fixed = [dev(a) for a in (sym, thr, curve)]
    evaluate.pose_tally(dev(errors), dev(cls), *fixed, *outs)
    torch.cuda.synchronize()
    want = per.tally(errors, cls, sym, thr, curve)
    for a, b in zip(outs, want):
        np.testing.assert_array_equal(a.cpu().numpy(), b)
    assert want[0].sum() > 500 and 0 < want[1].sum() < want[0].sum()
    # a second block with a device row count: the counts add up
    e2, c2, _, _, _ = tally_problem(seed=1, N=300)
    evaluate.pose_tally(dev(e2), dev(c2), *fixed, *outs, num_rows=torch.tensor([211], dtype=torch.int32, device=D))
    torch.cuda.synchronize()
    want = per.tally(e2, c2, sym, thr, curve, num_rows=211, into=want)
    for a, b in zip(outs, want):
        np.testing.assert_array_equal(a.cpu().numpy(), b)
    # an error exactly equal to the class threshold is not correct; one float below it is
    outs = _tally_tensors(C, T)
    evaluate.pose_tally(dev(errors[:2]), dev(cls[:2]), *fixed, *outs)
    torch.cuda.synchronize()
    assert errors[0, 0] == thr[1] and int(outs[0][1]) == 2 and int(outs[1][1]) == 1
    # T = 0: only slot 0 exists
    outs = _tally_tensors(C, 0)
    evaluate.pose_tally(dev(errors), dev(cls), fixed[0], fixed[1], torch.zeros((0,), device=D), *outs)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(outs[2].cpu().numpy()[:, 0], per.tally(errors, cls, sym, thr, curve)[0])


def label_pair(shape, C, seed, background=False):
    """A ground-truth map with objects on background and a prediction that is mostly right; both hold
    labels outside [0, C): gt = -1 and gt = C (not counted), pred = -3 and pred = C + 2 (skipped)."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    if background:
        return np.zeros(shape, np.int32), np.zeros(shape, np.int32)
    gt = np.where(rng.uniform(size=n) < 0.7, 0, rng.integers(0, C, n)).astype(np.int32)
    pred = np.where(rng.uniform(size=n) < 0.8, gt, rng.integers(0, C, n)).astype(np.int32)
    edit = rng.uniform(size=n)
    gt[edit < 0.02] = -1
    gt[(edit >= 0.02) & (edit < 0.04)] = C
    pred[(edit >= 0.03) & (edit < 0.05)] = -3
    pred[(edit >= 0.05) & (edit < 0.06)] = C + 2
    return gt.reshape(shape), pred.reshape(shape)


@pytest.mark.parametrize("shape,C", [((1, 1, 1), 2), ((1, 1, 1), 22), ((1, 7, 13), 2), ((1, 7, 13), 22),
                                     ((2, 120, 160), 2), ((2, 120, 160), 22), ((1, 7, 13), 130),
                                     ((2, 120, 160), 130)])
def test_confusion_equals_bincount(hip, shape, C):
    from posecnn_amd import evaluate
    gt, pred = label_pair(shape, C, seed=C + shape[1])
    hist, skipped = evaluate.confusion(dev(gt), dev(pred), C)
    torch.cuda.synchronize()
    want, ws = per.confusion(gt, pred, C)
    np.testing.assert_array_equal(hist.cpu().numpy(), want)
    assert int(skipped) == ws
    if C <= 22 and np.prod(shape) > 1:
        k = (gt >= 0) & (gt < C) & (pred >= 0) & (pred < C)
        np.testing.assert_array_equal(want, np.bincount(C * gt[k] + pred[k], minlength=C * C).reshape(C, C))
    # a second call accumulates
    evaluate.confusion(dev(gt), dev(pred), C, hist, skipped)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(hist.cpu().numpy(), 2 * want)
    assert int(skipped) == 2 * ws


def test_confusion_all_background_from_frames_and_misaligned(hip):
    from posecnn_amd import evaluate, synth
    C = 22
    gt, pred = label_pair((2, 120, 160), C, seed=0, background=True)  # every lane on one counter
    hist, skipped = evaluate.confusion(dev(gt), dev(pred), C)
    torch.cuda.synchronize()
    assert int(hist[0, 0]) == gt.size and int(hist.sum()) == gt.size and int(skipped) == 0
    # a rendered label map against a shifted copy of itself
    fr = synth.make_frames(2, H=120, W=160, num_classes=C, objects_per_image=4, seed=5)
    gt = fr["label"].astype(np.int32)
    pred = np.roll(gt, 3, axis=2)
    hist, skipped = evaluate.confusion(dev(gt), dev(pred), C)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(hist.cpu().numpy(), per.confusion(gt, pred, C)[0])
    assert int(hist.sum()) == gt.size and int(hist[0, 0]) < gt.size
    # bases one element past 16-byte alignment: both (a scalar head, then int4 loads), one alone (scalar)
    gt, pred = label_pair((1, 1, 4999), C, seed=9)
    g1, p1 = dev(np.concatenate([[7], gt.ravel()]).astype(np.int32)), dev(np.concatenate([[7], pred.ravel()]).astype(np.int32))
    want, ws = per.confusion(gt, pred, C)
    canvas, intact = carve((C, C), torch.int64)
    for a, b in ((g1[1:], p1[1:]), (g1[1:], dev(pred.ravel())), (dev(gt.ravel()), p1[1:])):
        assert a.data_ptr() % 16 == 4 or b.data_ptr() % 16 == 4
        canvas.zero_()
        hist, skipped = evaluate.confusion(a, b, C, hist=canvas)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(hist.cpu().numpy(), want)
        assert int(skipped) == ws and intact()
    # the global path, misaligned
    want, ws = per.confusion(gt, pred, 130)
    hist, skipped = evaluate.confusion(g1[1:], p1[1:], 130)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(hist.cpu().numpy(), want)
    assert int(skipped) == ws


def evaluator_problem():
    """2 images, 5 ground truths, 9 RoIs (12 slots): two RoIs of class 1 in image 0, one RoI of class 4,
    which no ground truth has, one RoI whose class is in the other image only; class 5 has no ground
    truth at all (NaN accuracy); class 2 is symmetric."""
    from posecnn_amd import synth
    rng = np.random.default_rng(21)
    mdl = synth.models()
    C = 6
    points = mdl["lov_points"][:C].astype(F).copy()
    points[2, :400] = mirrored_box(400)
    num = np.array([0, 2620, 400, 2620, 2620, 2620], np.int32)
    sym = np.array([0, 0, 1, 0, 0, 0], F)
    ext = mdl["lov_extents"][:C].astype(F)

    def quat_pose(rt):
        R = rt[:, :3].astype(np.float64)
        w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
        q = np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])
        return np.concatenate([q, rt[:, 3]])

    gts, rois, poses = [], [], []
    for b, c, dt, dr, copies in ((0, 1, 0.004, 0.02, 2), (0, 2, 0.002, 0.01, 1), (0, 3, 0.08, 0.5, 1),
                                 (1, 1, 0.001, 0.005, 1), (1, 3, 0.01, 0.05, 1)):
        est, ref = random_pair(rng, dt, dr)
        while 1 + np.trace(ref[:, :3]) < 0.5 or 1 + np.trace(est[:, :3]) < 0.5:  # keep the quaternion's w well away from 0
            est, ref = random_pair(rng, dt, dr)
        gts.append(np.concatenate([[b, c, 0, 0, 0, 0], quat_pose(ref)]))
        for k in range(copies):
            rois.append([b, c, 10, 10, 50, 50, 0.9])
            p = quat_pose(est)
            p[4:] += 0.03 * k  # the second RoI of the class is further off
            poses.append(p)
    rois += [[1, 4, 0, 0, 9, 9, 0.5], [1, 2, 0, 0, 9, 9, 0.5], [0, 1, 0, 0, 9, 9, 0.1]]
    poses += [poses[0], poses[1], poses[0] * 3.0]  # (the last: an unnormalised quaternion, a far translation)
    assert len(gts) == 5 and len(rois) == 9
    rois = np.array(rois + [[0, 1, 0, 0, 0, 0, 0]] * 3, F)   # three slots past num_rois, with a class that would match
    poses = np.array(poses + [[0] * 7] * 3, F)
    return points, num, sym, ext, np.array(gts, F), rois, poses


def test_pose_evaluator_summary_equals_the_restatement(hip):
    from posecnn_amd import evaluate
    K = camera()
    points, num, sym, ext, gt, rois, poses = evaluator_problem()
    ev = evaluate.PoseEvaluator(dev(points), dev(num), dev(sym), ext, dev(K), curve_bins=100)
    ref = per.Evaluator(points, num, sym, ext, K, curve_bins=100)
    count = torch.tensor([9], dtype=torch.int32, device=D)
    errors = ev.update(dev(rois), dev(poses), dev(gt), num_rois=count)
    ref.update(rois, poses, gt, num_rois=9)
    assert tuple(errors.shape) == (12 * 5, 5)
    labels = [label_pair((2, 60, 80), 6, seed=s) for s in (1, 2)]
    for g, p in labels:
        ev.update_segmentation(dev(g), dev(p))
        ref.update_segmentation(g, p)
    got, want = ev.summary(), ref.summary()
    assert set(got) == set(want)
    for key in want:
        np.testing.assert_array_equal(np.asarray(got[key]), np.asarray(want[key]), err_msg=key)
    np.testing.assert_array_equal(got["count_all"], [0, 2, 1, 2, 0, 0])
    np.testing.assert_array_equal(got["count_scored"], [0, 4, 1, 2, 0, 0])  # both class-1 RoIs of image 0, and RoI 8
    assert got["count_correct"].sum() >= 3 and got["count_correct"][3] == 1
    assert np.isnan(got["accuracy"][[0, 4, 5]]).all() and np.isfinite(got["accuracy"][[1, 2, 3]]).all()
    assert np.isnan(got["add_auc"][5]) and 0 < got["add_auc"][1] and got["adds_auc"][2] >= got["add_auc"][2]
    assert got["hist"].sum() + got["skipped"] > 0 and 0 < got["mean_iu"] < 1
    # a second batch accumulates
    ev.update(dev(rois), dev(poses), dev(gt), num_rois=count)
    again = ev.summary()
    np.testing.assert_array_equal(again["count_all"], 2 * got["count_all"])
    np.testing.assert_array_equal(again["count_correct"], 2 * got["count_correct"])
    np.testing.assert_array_equal(again["accuracy"], got["accuracy"])


def test_quat_poses_to_rt_equals_the_restatement(hip):
    from posecnn_amd import evaluate
    rng = np.random.default_rng(3)
    poses = rng.standard_normal((64, 7)).astype(F)
    got = evaluate.quat_poses_to_rt(dev(poses))
    assert got.dtype == torch.float32 and got.is_contiguous()
    np.testing.assert_array_equal(got.cpu().numpy().view(np.int32), per.quat_poses_to_rt(poses).view(np.int32))


def _variants(t):
    """A wrong-dtype, a strided and a CPU form of `t`."""
    strided = torch.zeros(tuple(t.shape) + (2,), dtype=t.dtype, device=t.device)[..., 0]
    strided.copy_(t)
    assert not strided.is_contiguous() or t.numel() <= 1
    other = t.double() if t.dtype == torch.float32 else (t.long() if t.dtype == torch.int32 else t.int())
    return {"dtype": other, "strided": strided, "cpu": t.cpu()}


def test_wrappers_keep_the_header_contract(hip):
    from posecnn_amd import _lib, evaluate
    real = evaluate._load()
    assert isinstance(real, type(_lib.load())) and real.pcnn_pose_errors.argtypes is not None
    guard = abi_guard.GuardedLib(real, header=EVAL_HEADER)
    K = camera()
    cls, rt_e, rt_g, points, num = problem(65, 5, seed=2)
    pe = dict(cls=dev(cls), rt_est=dev(rt_e), rt_gt=dev(rt_g), points=dev(points), num_points=dev(num), K=dev(K))
    errors_h, cls_h, sym, thr, curve = tally_problem(N=64)
    C, T = len(sym), len(curve)
    s, c, fa, fs = _tally_tensors(C, T)
    pt = dict(errors=dev(errors_h), cls=dev(cls_h), symmetry=dev(sym), thresholds=dev(thr), curve_thr=dev(curve),
              scored=s, correct=c, first_add=fa, first_adds=fs)
    g, p = label_pair((1, 7, 13), 22, seed=1)
    cf = dict(gt_label=dev(g), pred_label=dev(p), num_classes=22, hist=torch.zeros((22, 22), dtype=torch.int64, device=D),
              skipped=torch.zeros((1,), dtype=torch.int64, device=D))
    _lib._lib = guard
    try:
        guard.reset()
        evaluate.pose_errors(**pe)
        evaluate.pose_tally(**pt)
        evaluate.confusion(**cf)
        torch.cuda.synchronize()
        assert guard.calls["pcnn_pose_errors"] == 1 and guard.calls["pcnn_pose_tally"] == 1
        assert guard.calls["pcnn_confusion"] == 1 and guard.launches == 3
        guard.reset()
        for fn, kw in ((evaluate.pose_errors, pe), (evaluate.pose_tally, pt), (evaluate.confusion, cf)):
            for name, t in kw.items():
                if not isinstance(t, torch.Tensor):
                    continue
                for what, bad in _variants(t).items():
                    if what == "strided" and t.numel() <= 1:
                        continue
                    with pytest.raises(ValueError, match=name):
                        fn(**dict(kw, **{name: bad}))
                    assert sum(guard.calls.values()) == 0, (fn.__name__, name, what)
        with pytest.raises(ValueError, match="rt_gt"):
            evaluate.pose_errors(**dict(pe, rt_gt=pe["rt_gt"][:-1]))
        with pytest.raises(ValueError, match="num_points"):
            evaluate.pose_errors(**dict(pe, num_points=pe["num_points"][:-1]))
        with pytest.raises(ValueError, match="out"):
            evaluate.pose_errors(**pe, out=torch.zeros((5, 4), device=D))
        with pytest.raises(ValueError, match="first_add"):
            evaluate.pose_tally(**dict(pt, first_add=fa[:, :-1].contiguous()))
        with pytest.raises(ValueError, match="pred_label"):
            evaluate.confusion(**dict(cf, pred_label=cf["pred_label"][:, :-1].contiguous()))
        with pytest.raises(ValueError, match="hist"):
            evaluate.confusion(**dict(cf, num_classes=21))
        assert sum(guard.calls.values()) == 0
    finally:
        _lib._lib = real
    # the guard refuses what the wrappers would never send
    with pytest.raises(abi_guard.AbiContractError):
        guard.pcnn_confusion(_lib.ptr(cf["gt_label"].long()), _lib.ptr(cf["pred_label"]), 91, 22, _lib.ptr(cf["hist"]),
                             _lib.ptr(cf["skipped"]), _lib.stream_ptr())
    with pytest.raises(abi_guard.AbiContractError):
        guard.pcnn_pose_tally(_lib.ptr(pt["errors"].double()), _lib.ptr(pt["cls"]), None, 64, _lib.ptr(pt["symmetry"]),
                              _lib.ptr(pt["thresholds"]), C, _lib.ptr(pt["curve_thr"]), T, _lib.ptr(s), _lib.ptr(c),
                              _lib.ptr(fa), _lib.ptr(fs), _lib.stream_ptr())
    torch.cuda.synchronize()
