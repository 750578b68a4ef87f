"""The scene renderer without a GPU: the invariants of its numpy restatement
(tests/scene_ref.py) on the shared fixture "three", which establish the
fixture before the GPU sees it; the restated ground truth end to end through
the CPU oracle's Hough vote; the host side of the new C-ABI entry points
(pcnn_render_scenes, pcnn_vertex_targets_expand) and the scene sampling of
posecnn_amd/synthesize/scene.py.

Bars: the near-tie share (two fragments closer than 1e-5 m) at most 0.5 % of
the covered pixels, as tests/test_render_ref.py; the voted depth within 1e-4
relative of the instance's tz (measured 2e-5: the vote averages exp(log z) in
float32)."""
import ctypes

import numpy as np
import pytest

from posecnn_amd import synth
from render_ref import CAMERA4
from scene_ref import EXTENTS, H4, W4, alone_ref, expand_ref, meshes, scene_ref, three, three_ref

GAP = 1e-5


def test_three_invariants():
    a, b = three_ref(np.float32), three_ref(np.float64)
    covered = b["inst_id"] >= 0
    assert a["visible"].sum() == (a["inst_id"] >= 0).sum() == covered.sum()
    alone = [int(alone_ref(i, np.float32)["visible"][0]) for i in range(3)]
    overlap = sum((alone_ref(i, np.float32)["inst_id"] >= 0).astype(int) for i in range(3))
    print("visible", a["visible"], "alone", alone, "covered twice or more", int((overlap >= 2).sum()))
    np.testing.assert_array_equal(a["visible"], [1452, 911, 1353])
    assert alone == [1458, 1493, 2227] and (overlap >= 2).sum() == 1462
    close = covered & (b["gap"] < GAP)
    print("near ties", int(close.sum()), "of", int(covered.sum()))
    assert close.sum() <= 0.005 * covered.sum()
    for key in ("inst_id", "face", "label"):
        np.testing.assert_array_equal(a[key][~close], b[key][~close])
    assert np.abs(a["depth"].astype(np.float64) - b["depth"])[~close].max() <= 5e-6
    # consistency of the maps
    assert (a["label"][~covered] == 0).all() and (a["depth"][~covered] == 0).all()
    assert np.isnan(a["vertmap"][~covered]).all() and not np.isnan(a["vertmap"][covered]).any()
    assert (a["vertex3"][~covered] == 0).all()
    np.testing.assert_array_equal(np.round(a["vertmap"][covered][:, 0]), a["label"][covered])
    n = np.hypot(a["vertex3"][..., 0], a["vertex3"][..., 1])[covered]
    assert (np.abs(n - 1) < 1e-6).sum() >= covered.sum() - 3  # unit directions (a pixel on a centre: 0)


def test_equal_depth_goes_to_the_lower_rank():
    mesh, _, pose = three()[0]
    r = scene_ref([(mesh, 2, pose), (mesh, 4, pose)], H4, W4, CAMERA4, np.float32)
    covered = r["inst_id"] >= 0
    assert covered.sum() > 1000 and (r["inst_id"][covered] == 0).all() and (r["label"][covered] == 2).all()
    np.testing.assert_array_equal(r["visible"], [covered.sum(), 0])


def test_restated_targets_through_the_oracle_vote(orc):
    r = three_ref(np.float32)
    C = len(EXTENTS)
    vertex, weights = expand_ref(r["label"][None], r["vertex3"][None], C)
    assert vertex.shape == (1, H4, W4, 3 * C) and (weights[vertex != 0] == 10).all()
    fx, fy, px, py = CAMERA4
    meta = synth.make_meta(np.array([[fx, 0, px], [0, fy, py], [0, 0, 1]]), 1)
    box, pose, _, _, _, n = orc.hough_voting(r["label"][None], vertex, EXTENTS, meta, np.zeros((0, 13), np.float32),
                                             0, -1.0, 0.02, 1, label_threshold=500)
    assert n == 3
    np.testing.assert_array_equal(box[:, 1], [2, 3, 5])
    for row, p in zip(box, pose):
        i = [c for _, c, _ in three()].index(int(row[1]))
        tz = float(three()[i][2][6])
        print("class", int(row[1]), "score", row[6], "visible", r["visible"][i], "tz", p[6], "of", tz,
              "rel", abs(p[6] - tz) / tz)
        assert row[6] in (r["visible"][i], r["visible"][i] - 1)  # the pixel on the centre casts no vote
        assert abs(p[6] - tz) <= 1e-4 * tz


@pytest.fixture(scope="module")
def lib():
    from posecnn_amd import _lib, build
    if build.needs_build():
        build.build()
    return _lib.load()


def test_new_entry_points_are_declared_and_exported(lib):
    from posecnn_amd import _lib
    from test_abi import _declared
    decl = _declared()
    for name, n in (("pcnn_render_scenes", 33), ("pcnn_render_scenes_workspace_size", 6),
                    ("pcnn_vertex_targets_expand", 10)):
        assert decl[name] == n == len(_lib._SIGS[name][1])
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr)
    need = lib.pcnn_render_scenes_workspace_size(8, 48, 480, 640, 1000, 2304)
    assert need >= 8 * 480 * 640 * 8 + 48 * 1000 * 48 + 48 * 2304 * 8
    assert lib.pcnn_render_scenes_workspace_size(8, 48, 480, 640, 1000, (1 << 24) + 1) == 0
    assert lib.pcnn_render_scenes_workspace_size(0, 48, 480, 640, 1000, 12) == 0
    assert lib.pcnn_render_scenes_workspace_size(8, 0, 480, 640, 1000, 12) == 0


def test_argument_validation_without_gpu(lib):
    """Invalid arguments are rejected before any launch (PCNN_EINVAL = 1)."""
    P = ctypes.c_void_p(64)

    def scenes(vertices=P, K=4, S=2, F_max=12, F_total=24, scene_offset=P, label=P, visible=P, inst_id=None,
               workspace=P, H=120, znear=0.25):
        return lib.pcnn_render_scenes(vertices, P, P, P, P, 2, 48, F_total, F_max, P, P, P, K, scene_offset, S, H, 160,
                                      *CAMERA4, znear, 6.0, label, P, P, P, inst_id, visible, P, workspace, 1 << 30,
                                      None)
    assert scenes(vertices=None) == 1 and scenes(scene_offset=None) == 1 and scenes(label=None) == 1
    assert scenes(visible=None) == 1 and scenes(workspace=None) == 1
    assert scenes(K=0) == 1 and scenes(S=0) == 1 and scenes(H=0) == 1 and scenes(znear=0.0) == 1
    assert scenes(F_max=(1 << 24) + 1, F_total=(1 << 24) + 1) == 1
    assert scenes(workspace=ctypes.c_void_p(72)) == 1 and scenes(label=ctypes.c_void_p(66)) == 1
    assert scenes(inst_id=ctypes.c_void_p(65)) == 1

    def expand(label=P, targets=P, weights=P, B=1, C=7):
        return lib.pcnn_vertex_targets_expand(label, P, B, 97, 131, C, 10.0, targets, weights, None)
    assert expand(label=None) == 1 and expand(targets=None) == 1 and expand(B=0) == 1 and expand(C=0) == 1
    assert expand(targets=ctypes.c_void_p(68)) == 1 and expand(weights=ctypes.c_void_p(72)) == 1


def test_sample_scenes():
    from posecnn_amd.synthesize.scene import sample_scenes
    from refine_scene import quat_to_R
    classes = list(range(1, 22))
    off, cls, poses = sample_scenes(16, classes, seed=3)
    assert off.dtype == np.int32 and cls.dtype == np.int32 and poses.dtype == np.float32
    n = np.diff(off)
    assert off[0] == 0 and off[-1] == len(cls) == len(poses) and set(n) <= {5, 6, 7} and len(set(n)) > 1
    for i in range(16):
        c, p = cls[off[i]:off[i + 1]], poses[off[i]:off[i + 1]].astype(np.float64)
        assert len(set(c)) == len(c) and set(c) <= set(classes)
        np.testing.assert_allclose(np.linalg.norm(p[:, :4], axis=1), 1, atol=1e-6)
        assert (np.abs(p[:, 4:6]) <= 0.1).all() and (p[:, 6] >= 0.5).all() and (p[:, 6] <= 2.0).all()
        d = np.linalg.norm(p[:, None, 4:] - p[None, :, 4:], axis=-1) + np.eye(len(p))
        assert d.min() >= 0.2 - 1e-6
    # seeded per global image index: a shard sees the single-device scenes
    o2, c2, p2 = sample_scenes(4, classes, seed=3, image_offset=5)
    np.testing.assert_array_equal(c2, cls[off[5]:off[9]])
    np.testing.assert_array_equal(p2, poses[off[5]:off[9]])
    # redraws are deterministic and differ from the first draw
    a = sample_scenes(2, classes, seed=3, attempts=[0, 2])
    b = sample_scenes(2, classes, seed=3, attempts=[0, 2])
    np.testing.assert_array_equal(a[2], b[2])
    np.testing.assert_array_equal(a[2][:a[0][1]], poses[:off[1]])
    assert not np.array_equal(a[2][a[0][1]:][:3], poses[off[1]:off[2]][:3])
    # the rotation is Rx(roll) Ry(pitch) Rz(yaw): a proper rotation, and the convention itself
    from posecnn_amd.synthesize.scene import _quat_mul
    R = quat_to_R(poses[0, :4])
    np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-6)
    h = np.sqrt(0.5)
    q = _quat_mul(_quat_mul([h, h, 0, 0], [h, 0, h, 0]), [1, 0, 0, 0])  # Rx(90) Ry(90)
    np.testing.assert_allclose(quat_to_R(q), [[0, 0, 1], [1, 0, 0], [0, 1, 0]], atol=1e-12)
    with pytest.raises(ValueError):
        sample_scenes(1, [1, 2, 3], seed=0)
    with pytest.raises(ValueError):  # no second object fits: gives up instead of spinning
        sample_scenes(1, classes, seed=0, min_dist=5.0)


def test_meshes_are_the_render_fixtures():
    assert sorted(meshes()) == [2, 3, 5] and max(len(m.faces) for m in meshes().values()) == 2304
