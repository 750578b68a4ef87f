"""The HIP scene renderer (csrc/render_scene.hip through pcnn_render_scenes,
pcnn_vertex_targets_expand and posecnn_amd/synthesize/scene.py) against the
numpy restatement tests/scene_ref.py, whose own invariants
tests/test_scene_ref.py checks on the CPU.  160 x 120, camera =
refine_scene.CAMERA / 4, the meshes of tests/render_ref.py.

Bars (those of tests/test_gpu_render.py)
 - label, inst_id and coverage: equal to the float32 reference, except at
   pixels whose two nearest fragments (of any instance) are closer than 1e-5 m
   in the float64 reference; at most 0.5 % of the covered pixels may be left
   out this way, and the share is asserted.
 - depth, vertmap minus the class: within 5e-6 m of the float64 reference on
   the compared pixels.
 - visible: exact when no pixel was left out, else within the left-out count.
 - vertex3 channels 0, 1 and centers: the bits of the numpy restatement
   (double subtraction, sqrt and division are correctly rounded on both
   sides, the build does not contract); channel 2 within one float32 ulp
   (libm's and the device's double log may differ in the last bit).
 - background exactly 0 / NaN / -1; every render goes into the middle of
   poisoned buffers whose guard bands must come back untouched.
 - batching, repetition, path threshold, graph replay, a one-instance scene
   against pcnn_render_meshes: bitwise equality."""
import os

import numpy as np
import pytest
import torch

from render_ref import CAMERA4
from scene_ref import EXTENTS, H4, W4, alone_ref, expand_ref, meshes, three, three_ref

pytestmark = pytest.mark.gpu
D = torch.device("cuda")
TOL = 5e-6
GAP = 1e-5
GUARD = 64
POISON = 12345.0
MAPS = ("label", "depth", "vertmap", "vertex3", "inst_id")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(D)


@pytest.fixture(scope="module")
def renderer(hip):
    from posecnn_amd.synthesize import SceneRenderer
    return SceneRenderer(meshes(), H4, W4, CAMERA4, device=D)


def _args(r, scenes):
    """scenes: [[(mesh, class, pose)]] -> scene_offset, mesh_index, class_id, poses (numpy)."""
    slot = {id(m): r.slot[c] for c, m in meshes().items()}
    inst = [i for s in scenes for i in s]
    off = np.concatenate([[0], np.cumsum([len(s) for s in scenes])]).astype(np.int32)
    return (off, np.array([slot[id(m)] for m, _, _ in inst], np.int32), np.array([c for _, c, _ in inst], np.int32),
            np.stack([p for _, _, p in inst]).astype(np.float32).reshape(-1, 7))


def _guarded(shape, dtype, fill):
    n = int(np.prod(shape))
    full = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=D)
    return full, full[GUARD:GUARD + n].view(shape)


def _render(r, off, slots, classes, poses):
    """render_into the middle of poisoned buffers; numpy outputs, guard bands checked."""
    S, K, H, W = len(off) - 1, len(slots), r.H, r.W
    f, i = torch.float32, torch.int32
    bufs = {"label": _guarded((S, H, W), i, 777), "depth": _guarded((S, H, W), f, POISON),
            "vertmap": _guarded((S, H, W, 3), f, POISON), "vertex3": _guarded((S, H, W, 3), f, POISON),
            "inst_id": _guarded((S, H, W), i, 777), "visible": _guarded((K,), i, 777),
            "centers": _guarded((K, 2), f, POISON)}
    r.render_into(T(off), T(slots), T(classes), T(poses), **{k: v[1] for k, v in bufs.items()})
    torch.cuda.synchronize()
    out = {}
    for k, (full, view) in bufs.items():
        a = full.cpu().numpy()
        fill = 777 if a.dtype == np.int32 else np.float32(POISON)
        assert (a[:GUARD] == fill).all() and (a[-GUARD:] == fill).all(), f"{k}: write outside the output"
        out[k] = view.cpu().numpy()
    return out


def _render_scenes(r, scenes):
    return _render(r, *_args(r, scenes))


def _check_background(g):
    bg = g["inst_id"] < 0
    assert (g["label"][bg] == 0).all() and (g["depth"][bg] == 0).all() and (g["vertex3"][bg] == 0).all()
    assert (g["inst_id"][bg] == -1).all()
    assert (np.isnan(g["vertmap"]).all(-1) == bg).all() and (np.isnan(g["vertmap"]).any(-1) == bg).all()
    assert not (g["label"] == 777).any() and not (g["depth"] == POISON).any() and not (g["vertex3"] == POISON).any()


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _check_against(g, a32, b64, classes, what):
    """One scene's maps (no S axis) with its visible / centers rows against the references."""
    _check_background(g)
    covered = b64["inst_id"] >= 0
    skip = covered & (b64["gap"] < GAP)
    share = skip.sum() / max(covered.sum(), 1)
    cmp_ = ~skip
    on = cmp_ & covered
    cls = np.asarray(classes, np.float64)[np.maximum(b64["inst_id"], 0)]
    err_d = np.abs(g["depth"].astype(np.float64) - b64["depth"])[on].max()
    vm, ref = g["vertmap"].astype(np.float64), b64["vertmap"].copy()
    vm[..., 0] -= cls
    ref[..., 0] -= cls
    err_v = np.abs(vm - ref)[on].max()
    dv = np.abs(g["visible"].astype(np.int64) - a32["visible"])
    dir_bits = int((g["vertex3"][..., :2][on] != a32["vertex3"][..., :2][on]).sum())
    log_ulp = int(_ulps(g["vertex3"][..., 2][on], a32["vertex3"][..., 2][on]).max())
    print(f"{what}: covered {int(covered.sum())}, left out {int(skip.sum())} ({share:.4%}), inst_id mismatches "
          f"{int((g['inst_id'] != a32['inst_id'])[cmp_].sum())}, depth err {err_d:.3g}, vertmap err {err_v:.3g}, "
          f"visible {g['visible']} off by {dv}, direction values differing in bits {dir_bits}, log z ulps {log_ulp}")
    assert share <= 0.005
    np.testing.assert_array_equal(g["inst_id"][cmp_], a32["inst_id"][cmp_])
    np.testing.assert_array_equal(g["label"][cmp_], a32["label"][cmp_])
    assert err_d <= TOL and err_v <= TOL
    if skip.sum() == 0:
        np.testing.assert_array_equal(g["visible"], a32["visible"])
    else:
        assert dv.max() <= skip.sum()
    assert dir_bits == 0 and log_ulp <= 1
    np.testing.assert_array_equal(g["centers"].view(np.int32), a32["centers"].view(np.int32))


def _scene(g, s, rows=None):
    out = {k: g[k][s] for k in MAPS}
    if rows is not None:
        out["visible"], out["centers"] = g["visible"][rows], g["centers"][rows]
    return out


def _same(a, b, keys=MAPS):
    for k in keys:
        np.testing.assert_array_equal(a[k].view(np.int32), b[k].view(np.int32), err_msg=k)


@pytest.fixture(scope="module")
def three_alone(renderer):
    """ "three" rendered as the only scene; read-only."""
    return _render_scenes(renderer, [three()])


def test_three_matches_reference(three_alone):
    classes = [c for _, c, _ in three()]
    _check_against(_scene(three_alone, 0, slice(0, 3)), three_ref(np.float32), three_ref(np.float64), classes, "three")
    assert (three_alone["inst_id"] >= 0).sum() > 3000


@pytest.mark.parametrize("i", [0, 1, 2])
def test_single_instance_scene_equals_render_meshes(renderer, i):
    from posecnn_amd.synthesize import MeshRenderer
    mesh, cls, pose = three()[i]
    g = _render_scenes(renderer, [[three()[i]]])
    _check_against(_scene(g, 0, slice(0, 1)), alone_ref(i, np.float32), alone_ref(i, np.float64), [cls], f"alone[{i}]")
    mr = MeshRenderer(meshes(), H4, W4, CAMERA4, device=D)
    vm, pv, pn, depth, tri = mr.render_many([cls], pose[None], return_depth=True, return_tri_id=True)
    np.testing.assert_array_equal(g["vertmap"].view(np.int32), vm.cpu().numpy().view(np.int32))
    np.testing.assert_array_equal(g["depth"].view(np.int32), depth.cpu().numpy().view(np.int32))
    np.testing.assert_array_equal(g["inst_id"] >= 0, tri.cpu().numpy() >= 0)


def test_batch_positions_and_repeats(renderer, three_alone):
    single = [three()[1]]
    one = _render_scenes(renderer, [single])
    for pos in range(3):
        scenes = [[], single]
        scenes.insert(pos, three())
        g = _render_scenes(renderer, scenes)
        again = _render_scenes(renderer, scenes)
        _same(g, again, MAPS + ("visible", "centers"))
        off = np.concatenate([[0], np.cumsum([len(s) for s in scenes])])
        for s, sc in enumerate(scenes):
            rows = slice(off[s], off[s + 1])
            got = _scene(g, s, rows)
            if not sc:
                assert (got["inst_id"] == -1).all()
                _check_background(got)
                continue
            ref = _scene(three_alone if len(sc) == 3 else one, 0, slice(0, len(sc)))
            shifted = dict(ref, inst_id=np.where(ref["inst_id"] >= 0, ref["inst_id"] + off[s], -1).astype(np.int32))
            _same(got, shifted, MAPS + ("visible", "centers"))


def test_both_triangle_paths_give_the_same_bits(renderer, three_alone):
    """Every triangle through the large-triangle queue (threshold 0) and every
    one rasterised by its own thread (threshold above the image)."""
    old = os.environ.get("PCNN_RENDER_SMALL_MAX")
    try:
        for thr in ("0", "1000000"):
            os.environ["PCNN_RENDER_SMALL_MAX"] = thr
            _same(_render_scenes(renderer, [three()]), three_alone, MAPS + ("visible", "centers"))
    finally:
        if old is None:
            os.environ.pop("PCNN_RENDER_SMALL_MAX", None)
        else:
            os.environ["PCNN_RENDER_SMALL_MAX"] = old


def test_graph_replay_on_a_side_stream(renderer):
    scenes = [three(), [], [three()[1]]]
    off, slots, classes, poses = _args(renderer, scenes)
    eager = renderer.render(T(off), T(slots), T(classes), T(poses))
    a = [T(off), T(slots), T(classes), T(poses[::-1].copy())]  # captured with other poses than replayed
    S, K = len(off) - 1, len(slots)
    f, i = dict(dtype=torch.float32, device=D), dict(dtype=torch.int32, device=D)
    out = dict(label=torch.empty((S, H4, W4), **i), depth=torch.empty((S, H4, W4), **f),
               vertmap=torch.empty((S, H4, W4, 3), **f), vertex3=torch.empty((S, H4, W4, 3), **f),
               inst_id=torch.empty((S, H4, W4), **i), visible=torch.empty((K,), **i), centers=torch.empty((K, 2), **f))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up: sizes the stream's workspace outside the capture
        renderer.render_into(*a, stream=s, **out)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        renderer.render_into(*a, stream=s, **out)
    a[3].copy_(T(poses))
    for o in out.values():
        o.fill_(99)
    g.replay()
    torch.cuda.synchronize()
    for k, v in out.items():
        np.testing.assert_array_equal(v.cpu().numpy().view(np.int32), eager[k].cpu().numpy().view(np.int32), err_msg=k)


def test_tie_rule_and_instance_order(renderer, three_alone):
    mesh, _, pose = three()[0]
    g = _render_scenes(renderer, [[(mesh, 2, pose), (mesh, 4, pose)]])
    covered = g["inst_id"][0] >= 0
    assert covered.sum() > 1000 and (g["inst_id"][0][covered] == 0).all() and (g["label"][0][covered] == 2).all()
    np.testing.assert_array_equal(g["visible"], [covered.sum(), 0])
    # ranks 0 and 2 swapped: the same image, the other numbering
    a, b, c = three()
    sw = _render_scenes(renderer, [[c, b, a]])
    _same(sw, three_alone, ("label", "depth", "vertmap", "vertex3"))
    perm = np.array([2, 1, 0, -1])
    np.testing.assert_array_equal(perm[sw["inst_id"]], three_alone["inst_id"])
    np.testing.assert_array_equal(sw["visible"][::-1], three_alone["visible"])
    np.testing.assert_array_equal(sw["centers"][::-1], three_alone["centers"])


def test_invalid_scene_rows_render_background(renderer, three_alone):
    """Rows 0-2 hold "three", rows 3-259 a 12-face box 257 times at one pose."""
    off3, slots, classes, poses = _args(renderer, [three(), [three()[2]] * 257])
    K = len(slots)
    assert K == 260

    def run(off):
        g = _render(renderer, np.asarray(off, np.int32), slots, classes, poses)
        _check_background(g)
        return g
    good = _scene(three_alone, 0)
    for what, off, bad in (("decreasing", [0, 3, 3, 1], [1, 2]), ("beyond K", [0, 3, K + 5], [1]),
                           ("negative start", [-1, 3, 3], [0, 1]), ("257 instances", [0, 3, K], [1])):
        g = run(off)
        for s in range(len(off) - 1):
            if s in bad:
                assert (g["inst_id"][s] == -1).all(), what
            else:
                _same(_scene(g, s), good)
        rows = slice(0, 3) if 0 not in bad else slice(0, 0)
        np.testing.assert_array_equal(g["visible"][rows], three_alone["visible"][rows])
        assert (g["visible"][3:] == 0).all(), what
        np.testing.assert_array_equal(g["centers"][:3].view(np.int32), three_alone["centers"].view(np.int32))
    # 256 instances is the limit, not beyond it: the scene is drawn, every pixel by rank 0
    g = run([0, 3, K - 1])
    _same(_scene(g, 0), good)
    covered = g["inst_id"][1] >= 0
    assert covered.sum() > 1000 and (g["inst_id"][1][covered] == 3).all()
    assert g["visible"][3] == covered.sum() and (g["visible"][4:] == 0).all()


def test_render_into_rejects_outputs_it_would_overrun(renderer):
    off, slots, classes, poses = _args(renderer, [three()])
    f, i = dict(dtype=torch.float32, device=D), dict(dtype=torch.int32, device=D)

    def call(**bad):
        out = dict(label=torch.empty((1, H4, W4), **i), depth=torch.empty((1, H4, W4), **f),
                   vertmap=torch.empty((1, H4, W4, 3), **f), vertex3=torch.empty((1, H4, W4, 3), **f),
                   visible=torch.empty((3,), **i), centers=torch.empty((3, 2), **f))
        out.update(bad)
        renderer.render_into(T(off), T(slots), T(classes), T(poses), **out)
    call()
    for bad in (dict(label=torch.empty((1, H4, W4), **f)), dict(depth=torch.empty((1, H4 - 1, W4), **f)),
                dict(vertmap=torch.empty((1, H4, W4, 4), **f)[..., :3]), dict(visible=torch.empty((2,), **i)),
                dict(centers=torch.empty((3, 2), dtype=torch.float64, device=D)),
                dict(inst_id=torch.empty((1, H4, W4), dtype=torch.int64, device=D)),
                dict(label=torch.empty((1, H4, W4), dtype=torch.int32))):
        with pytest.raises(ValueError):
            call(**bad)
    with pytest.raises(ValueError):  # no scene
        renderer.render(T(off[:1]), T(slots), T(classes), T(poses))
    torch.cuda.synchronize()


def test_expand_matches_the_numpy_scatter(hip):
    from posecnn_amd import _lib
    from posecnn_amd.synthesize.scene import expand
    rng = np.random.default_rng(7)
    B, H, W, C = 2, 97, 131, 7
    label = rng.integers(0, C + 3, size=(B, H, W)).astype(np.int32)  # labels >= C give zero rows
    label[0, 0, :3] = [-1, C, 0]
    v3 = rng.normal(size=(B, H, W, 3)).astype(np.float32)
    rt, rw = expand_ref(label, v3, C)
    assert (B * H * W * 3 * C) % 4 != 0  # the vector stores have a tail
    t, w = expand(T(label), T(v3), C)
    np.testing.assert_array_equal(t.cpu().numpy().view(np.int32), rt.view(np.int32))
    np.testing.assert_array_equal(w.cpu().numpy(), rw)
    assert (rt[label >= C] == 0).all() and (rt[label <= 0] == 0).all() and (rw[label == 3][:, 9:12] == 10).all()
    # into guarded buffers, another weight
    bt, bw = (_guarded((B, H, W, 3 * C), torch.float32, POISON) for _ in range(2))
    rc = hip.pcnn_vertex_targets_expand(_lib.ptr(T(label)), _lib.ptr(T(v3)), B, H, W, C, 2.5, _lib.ptr(bt[1]),
                                        _lib.ptr(bw[1]), _lib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    for full, view, ref in ((bt[0], bt[1], rt), (bw[0], bw[1], rw * np.float32(0.25))):
        a = full.cpu().numpy()
        assert (a[:GUARD] == np.float32(POISON)).all() and (a[-GUARD:] == np.float32(POISON)).all()
        np.testing.assert_array_equal(view.cpu().numpy(), ref)
    with pytest.raises(ValueError):
        expand(T(label), T(v3[..., :2]), C)


def test_vote_consumes_the_rendered_targets(renderer, three_alone, orc):
    from posecnn_amd import synth
    from posecnn_amd.hough_voting_gpu_layer import hough_voting_gpu_op as hv
    from posecnn_amd.synthesize.scene import expand
    C = len(EXTENTS)
    label, v3 = three_alone["label"], three_alone["vertex3"]
    fx, fy, px, py = CAMERA4
    meta = synth.make_meta(np.array([[fx, 0, px], [0, fy, py], [0, 0, 1]]), 1)
    gt = np.zeros((0, 13), np.float32)
    full, _ = expand_ref(label, v3, C)
    ob, op, _, _, _, on = orc.hough_voting(label, full, EXTENTS, meta, gt, 0, -1.0, 0.02, 1, label_threshold=500)
    assert on == 3
    args = (T(EXTENTS), T(meta), T(gt), 0, -1.0, 0.02, 1)
    c = hv.hough_voting_gpu_capacity(T(label), T(v3), *args, label_threshold=500, vertex_compact=True)
    vt, vw = expand(T(label), T(v3), C)
    f = hv.hough_voting_gpu_capacity(T(label), vt, *args, label_threshold=500)
    assert int(c["num_rois"][0].item()) == int(f["num_rois"][0].item()) == on
    for k, ref in (("box", ob), ("pose", op)):
        np.testing.assert_array_equal(c[k][:on].cpu().numpy(), ref, err_msg=k)
        assert torch.equal(c[k][:on], f[k][:on]), k
    np.testing.assert_array_equal(ob[:, 1], [2, 3, 5])


def test_make_scene_frames(renderer):
    from posecnn_amd.synthesize import make_scene_frames
    kw = dict(seed=4, num_objects=(3, 4), tnear=0.5, tfar=0.9, min_dist=0.12, min_pixels=50, full_vertex=True)
    a = make_scene_frames(renderer, 2, **kw)
    b = make_scene_frames(renderer, 2, **kw)
    assert a["label"].shape == (2, H4, W4) and a["vertex3"].shape == (2, H4, W4, 3)
    assert a["depth"].shape == (2, H4, W4, 1) and a["meta"].shape == (2, 1, 1, 48) and a["gt"].shape == (6, 13)
    assert a["vertex"].shape == a["vertex_weights"].shape == (2, H4, W4, 3 * 6) and a["extents"].shape == (6, 3)
    assert all(v.is_cuda for v in a.values())
    vis = a["visible"].cpu().numpy()
    print("visible", vis)
    assert len(vis) == 6 and (vis >= 50).all()
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    gt, lab = a["gt"].cpu().numpy(), a["label"].cpu().numpy()
    for row, n in zip(gt, vis):
        assert (lab[int(row[0])] == int(row[1])).sum() == n  # distinct classes: the label counts are the visible counts
    np.testing.assert_array_equal(gt[:, 0], [0, 0, 0, 1, 1, 1])
    t, w = expand_ref(lab, a["vertex3"].cpu().numpy(), 6)
    np.testing.assert_array_equal(a["vertex"].cpu().numpy(), t)
    np.testing.assert_array_equal(a["vertex_weights"].cpu().numpy(), w)
    # a shard: image 1 alone is image 1 of the pair
    c = make_scene_frames(renderer, 1, image_offset=1, **kw)
    for k in ("label", "vertex3", "depth", "vertex"):
        assert torch.equal(c[k][0].view(torch.int32), a[k][1].view(torch.int32)), k
    np.testing.assert_array_equal(c["gt"].cpu().numpy(), gt[3:])
