"""estimatePose2D on the GPU (csrc/pose2d.hip over csrc/pose_ransac.h, posecnn_amd/synthesize/pose2d.py)
against the restated reference (oracle/orc_pose2d.cpp) on ray-cast box scenes:
the sampled hypotheses (object and pixel indices exact; poses to double
rounding), every preemptive round's inlier counts and the survivors exact, the
(3, 4, C) output against the oracle and -- exact coordinates -- the true pose;
with coordinate noise, object centres within 3 px."""
import numpy as np
import pytest
import torch

from oracle import oracle
from pose2d_scene import make_scene
from posecnn_amd.synthesize import pose2d

pytestmark = pytest.mark.gpu


def _run(sc, **kw):
    C = sc["C"]
    poses = np.zeros((3, 4, C), np.float32)
    _, d = pose2d.estimate_poses_2d(sc["label"], sc["vertmap"], sc["extents"], poses, C, *sc["camera"],
                                    return_diag=True, **kw)
    return poses, {k: v.cpu().numpy() for k, v in d.items()}


@pytest.mark.parametrize("noise,seed", [(0.0, 1), (0.01, 2), (0.003, 5)])
def test_pose2d_matches_oracle(hip, noise, seed):
    sc = make_scene(seed=seed, coord_noise=noise)
    poses, d = _run(sc)
    r = oracle.pose2d(sc["label"], sc["vertmap"], sc["extents"], *sc["camera"])
    np.testing.assert_array_equal(d["hyps"][:, 0], r["hyps"][:, 0])   # object of every hypothesis
    np.testing.assert_array_equal(d["hyp_px"], r["hyp_px"])             # its 4 sampled pixels
    np.testing.assert_allclose(d["hyps"][:, 1:], r["hyps"][:, 1:], atol=1e-5)
    np.testing.assert_array_equal(d["inliers"], r["inliers"])           # every round's counts
    np.testing.assert_array_equal(d["final"], r["final"])               # the survivors
    np.testing.assert_allclose(poses, r["poses"], atol=1e-5)
    fx, fy, px, py = sc["camera"]
    for c, p in sc["poses"].items():
        assert d["final"][c][0] >= 0
        if noise == 0.0:
            np.testing.assert_allclose(poses[:, :3, c], p["R"], atol=2e-5)
            np.testing.assert_allclose(poses[:, 3, c], p["t"], atol=2e-5)
        t = poses[:, 3, c]
        got = np.array([fx * t[0] / t[2] + px, fy * t[1] / t[2] + py])
        want = np.array([fx * p["t"][0] / p["t"][2] + px, fy * p["t"][1] / p["t"][2] + py])
        # the known answer: exact coordinates put the centre on the truth; noisy
        # ones (a 4-point P3P survivor, no refinement) within 3 px on these
        # scenes (the GPU equals the oracle, so this is a property of the
        # scene: 0.2-2.6 px here; over eight 1 %-noise scenes the oracle's
        # centres land at 0.7-3.2 px with one 26 px outlier)
        assert np.abs(got - want).max() < (0.1 if noise == 0.0 else 3.0)


@pytest.mark.parametrize("max_iter", [3, 40])
def test_pose2d_attempt_limit_matches_oracle(hip, max_iter):
    """max_iter bounds each hypothesis's attempts: 3 (< the 32 evaluated at
    once: some hypotheses stay empty) and 40 (attempts past the batch run 64
    at a time, one wave per hypothesis, the first accepted in attempt order);
    hypotheses, survivors and poses against the oracle."""
    sc = make_scene(seed=6, coord_noise=0.01)
    poses, d = _run(sc, max_iter=max_iter)
    r = oracle.pose2d(sc["label"], sc["vertmap"], sc["extents"], *sc["camera"], max_iter=max_iter)
    np.testing.assert_array_equal(d["hyps"][:, 0], r["hyps"][:, 0])
    np.testing.assert_array_equal(d["hyp_px"], r["hyp_px"])
    np.testing.assert_array_equal(d["inliers"], r["inliers"])
    np.testing.assert_array_equal(d["final"], r["final"])
    np.testing.assert_allclose(poses, r["poses"], atol=1e-5)
    if max_iter == 3:
        assert (d["hyps"][:, 0] < 0).any()  # the limit bites


def test_pose2d_device_inputs_and_no_object(hip):
    sc = make_scene(seed=4, n_obj=2)
    dev = torch.device("cuda")
    poses = torch.zeros((3, 4, sc["C"]), device=dev)
    pose2d.estimate_poses_2d(torch.from_numpy(sc["label"]).to(dev), torch.from_numpy(sc["vertmap"]).to(dev),
                             torch.from_numpy(sc["extents"]).to(dev), poses, sc["C"], *sc["camera"])
    r = oracle.pose2d(sc["label"], sc["vertmap"], sc["extents"], *sc["camera"])
    np.testing.assert_allclose(poses.cpu().numpy(), r["poses"], atol=1e-5)
    lab = np.zeros_like(sc["label"])
    lab[:10, :30] = 1  # below minArea
    p2 = np.full((3, 4, sc["C"]), 7.0, np.float32)
    _, d = pose2d.estimate_poses_2d(lab, sc["vertmap"], sc["extents"], p2, sc["C"], *sc["camera"], return_diag=True)
    assert not p2.any() and (d["final"].cpu().numpy() == -1).all()
    with pytest.raises(ValueError):
        pose2d.estimate_poses_2d(lab, sc["vertmap"], sc["extents"], np.zeros((3, 4, 2), np.float32), sc["C"],
                                 *sc["camera"])


def test_pose2d_hypothesis_limit(hip):
    """n_hyp is at most the reference's ransacIterations = 256
    (synthesize.cpp:1601): eight halving rounds then leave one hypothesis per
    object, where getWorkingQueue (:1150-1160) stops."""
    sc = make_scene(seed=4, n_obj=2)
    with pytest.raises(ValueError):
        pose2d.estimate_poses_2d(sc["label"], sc["vertmap"], sc["extents"], np.zeros((3, 4, sc["C"]), np.float32),
                                 sc["C"], *sc["camera"], n_hyp=257)


@pytest.mark.parametrize("H,W,C,n_hyp", [(240, 321, 16, 7), (480, 640, 22, 1), (240, 300, 4, 64)])
def test_pose2d_shapes(hip, H, W, C, n_hyp):
    """Odd and small frames, C = 16 / 4, one hypothesis: hypotheses, rounds,
    survivors and poses against the oracle."""
    sc = make_scene(seed=13, n_obj=min(3, C - 1), C=C, H=H, W=W, coord_noise=0.003)
    poses, d = _run(sc, n_hyp=n_hyp)
    r = oracle.pose2d(sc["label"], sc["vertmap"], sc["extents"], *sc["camera"], n_hyp=n_hyp)
    np.testing.assert_array_equal(d["hyps"][:, 0], r["hyps"][:, 0])
    np.testing.assert_array_equal(d["hyp_px"], r["hyp_px"])
    np.testing.assert_array_equal(d["inliers"], r["inliers"])
    np.testing.assert_array_equal(d["final"], r["final"])
    np.testing.assert_allclose(poses, r["poses"], atol=1e-5)
