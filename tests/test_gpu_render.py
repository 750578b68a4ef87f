"""The HIP mesh rasteriser (csrc/render.hip through pcnn_render_meshes and
posecnn_amd/synthesize/render.py) against the numpy restatement of its rules
(tests/render_ref.py), whose own invariants tests/test_render_ref.py checks on
the CPU.

Bars
 - tri_id and coverage: equal to the float32 reference, except at pixels whose
   two nearest fragments are closer than 1e-5 m in the float64 reference
   (either may win there); at most 0.5 % of the covered pixels may be left out
   this way, and the share is asserted.
 - pred_vertices, vertmap minus the class id, depth: within 5e-6 m of the
   float64 reference on the compared pixels; pred_normals within 5e-6.  That
   is ten times the 5e-7 m measured between the float32 and float64
   restatements (room for another summation order) and over 1000 times below
   ICP's max_error.
 - background: exactly 0 / NaN, written into outputs pre-filled with garbage;
   every render here goes into the middle of a larger poisoned buffer whose
   guard bands must come back untouched.
 - batching, repetition, path threshold, graph replay: bitwise equality."""
import os

import numpy as np
import pytest
import torch

from refine_scene import CAMERA, scene
from render_ref import CAMERA4, box_mesh, fixtures, raster_ref, reference, vertex_pass

pytestmark = pytest.mark.gpu
D = torch.device("cuda")
TOL = 5e-6
GAP = 1e-5
GUARD = 64  # elements on either side of an output
POISON = 12345.0
FIX = [(n, i) for n in ("icosphere", "torus", "box") for i in (0, 1)]
SLOT = {"icosphere": 0, "torus": 1, "box": 2}


def _renderer(names, H, W, camera=CAMERA4, **kw):
    from posecnn_amd.synthesize.render import MeshRenderer
    fx = fixtures()
    return MeshRenderer({fx[n][1]: fx[n][0] for n in names}, H, W, camera, device=D, **kw)


@pytest.fixture(scope="module")
def mixed(hip):
    """All three meshes at 160 x 120 (slots in SLOT's order)."""
    return _renderer(("icosphere", "torus", "box"), 120, 160)


@pytest.fixture(scope="module")
def odd(hip):
    """The box alone at 131 x 97."""
    return _renderer(("box",), 97, 131)


def _guarded(shape, dtype, fill):
    n = int(np.prod(shape))
    full = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=D)
    return full, full[GUARD:GUARD + n].view(shape)


def _render_guarded(r, slots, classes, poses):
    """render_into the middle of poisoned buffers; returns numpy maps after
    checking that the guard bands are untouched."""
    K = len(slots)
    H, W = r.H, r.W
    bufs = {"pred_v": _guarded((K, H, W, 4), torch.float32, POISON), "pred_n": _guarded((K, H, W, 4), torch.float32, POISON),
            "vertmap": _guarded((K, H, W, 3), torch.float32, POISON), "depth": _guarded((K, H, W), torch.float32, POISON),
            "tri_id": _guarded((K, H, W), torch.int32, 777)}
    mi = torch.tensor(slots, dtype=torch.int32, device=D)
    ci = torch.tensor(classes, dtype=torch.int32, device=D)
    P = torch.from_numpy(np.ascontiguousarray(poses, np.float32).reshape(K, 7)).to(D)
    r.render_into(mi, ci, P, bufs["pred_v"][1], bufs["pred_n"][1], bufs["vertmap"][1], bufs["depth"][1],
                  bufs["tri_id"][1])
    torch.cuda.synchronize()
    out = {}
    for k, (full, view) in bufs.items():
        f = full.cpu().numpy()
        fill = 777 if k == "tri_id" else np.float32(POISON)
        assert (f[:GUARD] == fill).all() and (f[-GUARD:] == fill).all(), f"{k}: write outside the output"
        out[k] = view.cpu().numpy()
    return out


def _check_consistent(g):
    """NaN in vertmap <=> w = 0 <=> tri_id = -1; background exactly 0 / NaN."""
    bg = g["tri_id"] < 0
    assert (np.isnan(g["vertmap"]).all(-1) == bg).all() and (np.isnan(g["vertmap"]).any(-1) == bg).all()
    assert ((g["pred_v"][..., 3] == 0) == bg).all() and (g["pred_v"][..., 3][~bg] == 1).all()
    assert (g["pred_v"][bg] == 0).all() and (g["pred_n"][bg] == 0).all() and (g["depth"][bg] == 0).all()
    assert (g["pred_n"][..., 3] == 0).all()


def _check_against(g, a32, b64, cls, label):
    """One rendered image (maps without the K axis) against the float32 and float64 references."""
    _check_consistent(g)
    covered = b64["tri_id"] >= 0
    skip = covered & (b64["gap"] < GAP)
    share = skip.sum() / max(covered.sum(), 1)
    cmp_ = ~skip
    err = {}
    on = cmp_ & covered
    for key in ("pred_v", "pred_n", "depth"):
        err[key] = np.abs(g[key].astype(np.float64) - b64[key])[on].max() if on.any() else 0.0
    vm = g["vertmap"].astype(np.float64)
    vm[..., 0] -= cls
    ref_vm = b64["vertmap"].copy()
    ref_vm[..., 0] -= cls
    err["vertmap"] = np.abs(vm - ref_vm)[on].max() if on.any() else 0.0
    bits = sum(int((g[k][on] != a32[k][on]).sum()) for k in ("pred_v", "pred_n", "vertmap", "depth"))
    print(f"{label}: covered {int(covered.sum())}, left out {int(skip.sum())} ({share:.4%}), "
          f"tri_id mismatches {int((g['tri_id'] != a32['tri_id'])[cmp_].sum())}, errors {err}, "
          f"values differing in bits from the float32 restatement {bits}")
    assert share <= 0.005
    np.testing.assert_array_equal(g["tri_id"][cmp_], a32["tri_id"][cmp_])
    for key, e in err.items():
        assert e <= TOL, key
    return covered


@pytest.mark.parametrize("name,i", FIX)
def test_fixture_matches_reference(mixed, odd, name, i):
    mesh, cls, H, W, poses = fixtures()[name]
    r, slot = (odd, 0) if name == "box" else (mixed, SLOT[name])
    g = _render_guarded(r, [slot], [cls], poses[i])
    covered = _check_against({k: v[0] for k, v in g.items()}, reference(name, i, np.float32),
                             reference(name, i, np.float64), cls, f"{name}[{i}]")
    assert covered.sum() > 300


def _edge_pose(q_seed, t):
    q = np.random.default_rng(q_seed).normal(size=4)
    return np.concatenate([q / np.linalg.norm(q), t]).astype(np.float32)


def test_half_and_fully_outside(mixed):
    mesh, cls, H, W, _ = fixtures()["icosphere"]
    fx, fy, px, py = CAMERA4
    half = _edge_pose(1, [-px / fx * 0.8, (H - 1 - py) / fy * 0.8, 0.8])  # centre on the bottom-left corner pixel
    gone = _edge_pose(2, [-1.0, 0.2, 0.8])
    g = _render_guarded(mixed, [0, 0], [cls, cls], np.stack([half, gone]))
    refs = [raster_ref(mesh, half, cls, H, W, CAMERA4, dtype=t) for t in (np.float32, np.float64)]
    covered = _check_against({k: v[0] for k, v in g.items()}, refs[0], refs[1], cls, "half outside")
    assert 50 < covered.sum() < 400 and covered[-1, 0]
    _check_consistent({k: v[1] for k, v in g.items()})
    assert (g["tri_id"][1] == -1).all()


def test_near_and_far_planes(mixed):
    """Faces with a vertex in front of znear are absent (the far side of the
    sphere shows through the hole) and the rest match; beyond zfar: empty."""
    mesh, cls, H, W, _ = fixtures()["icosphere"]
    near = _edge_pose(3, [0.0, 0.0, 0.27])
    far = _edge_pose(4, [0.0, 0.0, 6.5])
    g = _render_guarded(mixed, [0, 0], [cls, cls], np.stack([near, far]))
    refs = [raster_ref(mesh, near, cls, H, W, CAMERA4, dtype=t) for t in (np.float32, np.float64)]
    covered = _check_against({k: v[0] for k, v in g.items()}, refs[0], refs[1], cls, "near plane")
    assert covered.sum() > 1000
    z = vertex_pass(mesh, near, CAMERA4)[0][:, 2]  # camera z of every vertex, float64
    cut = (z[mesh.faces] < np.float64(np.float32(0.25))).any(1)
    assert 0 < cut.sum() < len(cut)
    drawn = np.unique(g["tri_id"][0][g["tri_id"][0] >= 0])
    assert not cut[drawn].any()
    assert g["depth"][0].max() > 0.27  # the inside of the far half is seen
    _check_consistent({k: v[1] for k, v in g.items()})
    assert (g["tri_id"][1] == -1).all()


def test_degenerate_faces_and_bad_mesh_index(hip, odd):
    from posecnn_amd.synthesize.render import Mesh, MeshRenderer
    mesh, cls, H, W, poses = fixtures()["box"]
    extra = np.concatenate([mesh.faces, [[0, 0, 1], [2, 2, 2], [0, 1, 0]]]).astype(np.int32)
    r = MeshRenderer({cls: Mesh(mesh.vertices, extra, mesh.normals)}, H, W, CAMERA4, device=D)
    g = _render_guarded(r, [0], [cls], poses[0])
    ref = _render_guarded(odd, [0], [cls], poses[0])
    for k in g:
        np.testing.assert_array_equal(g[k], ref[k])
    b = _render_guarded(odd, [1, -1, 0, 1 << 30], [cls] * 4, np.stack([poses[0]] * 4))
    _check_consistent(b)
    assert (b["tri_id"][[0, 1, 3]] == -1).all()
    for k in b:
        np.testing.assert_array_equal(b[k][2], ref[k][0])


def _mix():
    fx = fixtures()
    names = ["box", "icosphere", "torus", "icosphere", "box"]
    objs = [fx[n][1] for n in names]
    poses = np.stack([fx[n][4][j % 2] for j, n in enumerate(names)])
    return names, objs, poses


def test_batch_equals_singles_and_repeats(mixed):
    names, objs, poses = _mix()
    kw = dict(return_depth=True, return_tri_id=True)
    many = [m.cpu().numpy() for m in mixed.render_many(objs, poses, **kw)]
    again = [m.cpu().numpy() for m in mixed.render_many(objs, torch.from_numpy(poses).to(D), **kw)]
    assert many[0].shape == (5, 120, 160, 3) and many[1].shape == (5, 120, 160, 4) and many[4].dtype == np.int32
    for a, b in zip(many, again):
        np.testing.assert_array_equal(a, b)
    for j, (o, p) in enumerate(zip(objs, poses)):
        one = mixed(o, p, **kw)
        assert one[0].shape == (120, 160, 3)
        for a, b in zip(many, one):
            np.testing.assert_array_equal(a[j], b.cpu().numpy())
        assert (many[4][j] >= 0).sum() > 300
    # the torus in the batch against its reference: the shared renderer draws what the fixtures test drew
    np.testing.assert_array_equal(many[4][2] >= 0, reference("torus", 0, np.float32)["tri_id"] >= 0)


def test_both_triangle_paths_give_the_same_bits(mixed):
    """Every triangle through the large-triangle queue (threshold 0), every
    one rasterised by its own thread (threshold above the image), and the
    default split: the same bits."""
    names, objs, poses = _mix()
    kw = dict(return_depth=True, return_tri_id=True)
    base = [m.cpu().numpy() for m in mixed.render_many(objs, poses, **kw)]
    old = os.environ.get("PCNN_RENDER_SMALL_MAX")
    try:
        for thr in ("0", "1000000"):
            os.environ["PCNN_RENDER_SMALL_MAX"] = thr
            got = [m.cpu().numpy() for m in mixed.render_many(objs, poses, **kw)]
            for a, b in zip(base, got):
                np.testing.assert_array_equal(a, b)
    finally:
        if old is None:
            os.environ.pop("PCNN_RENDER_SMALL_MAX", None)
        else:
            os.environ["PCNN_RENDER_SMALL_MAX"] = old


def test_graph_replay_on_a_side_stream(mixed):
    names, objs, poses = _mix()
    K, H, W = len(objs), mixed.H, mixed.W
    mi = torch.tensor([SLOT[n] for n in names], dtype=torch.int32, device=D)
    ci = torch.tensor(objs, dtype=torch.int32, device=D)
    P = torch.from_numpy(poses[::-1].copy()).to(D)  # captured with other poses than replayed
    out = [torch.empty((K, H, W, c), dtype=torch.float32, device=D) for c in (4, 4, 3)]
    tri = torch.empty((K, H, W), dtype=torch.int32, device=D)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up: sizes the stream's workspace outside the capture
        mixed.render_into(mi, ci, P, out[0], out[1], out[2], None, tri, stream=s)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        mixed.render_into(mi, ci, P, out[0], out[1], out[2], None, tri, stream=s)
    P.copy_(torch.from_numpy(poses))
    for o in out:
        o.fill_(POISON)
    g.replay()
    torch.cuda.synchronize()
    vm, pv, pn, tid = mixed.render_many(objs, poses, return_tri_id=True)
    for a, b in zip(out + [tri], (pv, pn, vm, tid)):
        np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())


def test_argument_errors(hip, odd):
    from posecnn_amd import _lib
    mesh, cls, H, W, poses = fixtures()["box"]
    P = torch.from_numpy(poses[0][None]).to(D)
    mi = torch.zeros(1, dtype=torch.int32, device=D)
    ci = torch.full((1,), cls, dtype=torch.int32, device=D)
    pv, pn = (torch.empty((1, H, W, 4), device=D) for _ in range(2))
    vm = torch.empty((1, H, W, 3), device=D)
    with pytest.raises(ValueError):  # K = 0
        odd.render_into(mi[:0], ci[:0], P[:0], pv[:0], pn[:0], vm[:0])
    with pytest.raises(ValueError):  # one pose per object
        odd.render_many([cls, cls], poses[0][None])
    with pytest.raises(KeyError):    # an object without a mesh
        odd.render_many([cls + 1], poses[0][None])
    with pytest.raises(_lib.PcnnError):  # a short workspace
        odd.render_into(mi, ci, P, pv, pn, vm, workspace=torch.empty(256, dtype=torch.uint8, device=D))
    need = hip.pcnn_render_workspace_size(1, H, W, odd.V_total, odd.F_max)
    assert need >= H * W * 8 + odd.V_total * 48 and hip.pcnn_render_workspace_size(1, 0, W, 1, 1) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=D)
    p = _lib.ptr

    def call(vertices=odd.vertices, pred_v=pv, K=1, h=H, w=W, znear=0.25):
        return hip.pcnn_render_meshes(p(vertices), p(odd.normals), p(odd.faces), p(odd.vert_offset),
                                      p(odd.face_offset), odd.M, odd.V_total, odd.F_total, odd.F_max, p(mi), p(ci),
                                      p(P), K, h, w, *CAMERA4, znear, 6.0, p(pred_v), p(pn), p(vm), None, None,
                                      p(ws), ws.numel(), _lib.stream_ptr())
    assert call() == 0
    assert call(vertices=None) == 1 and call(pred_v=None) == 1
    assert call(K=0) == 1 and call(h=0) == 1 and call(w=-3) == 1 and call(znear=0.0) == 1
    with pytest.raises(ValueError):
        _lib.check(call(h=0), "render_meshes")
    torch.cuda.synchronize()


class _Counting:
    def __init__(self, r):
        self.r, self.many = r, 0

    def __call__(self, obj, pose):
        raise AssertionError("solve_icp renders through render_many")

    def render_many(self, objs, poses):
        self.many += 1
        return self.r.render_many(objs, poses)


def test_solve_icp_on_a_mesh(hip):
    """solve_icp with the mesh renderer as its `render`, at 640 x 480, to the
    bars of test_gpu_icp.py::test_solve_icp_end_to_end."""
    from posecnn_amd.synthesize import MeshRenderer
    from posecnn_amd.synthesize import icp as R
    sc = scene(5, perturb_deg=2.0, perturb_t=0.01)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(D)  # noqa: E731
    render = _Counting(MeshRenderer({sc["cls"]: box_mesh(sc["half"])}, 480, 640, CAMERA, device=D))
    params = list(CAMERA) + [0.25, 6.0, 10000.0]
    rois = np.array([[0, sc["cls"], 0, 0, 1, 1]], np.float32)
    poses = sc["init"].astype(np.float32)[None]
    depth = t(sc["live"]["depth"].astype(np.int32)).to(torch.uint16)
    lab = t(sc["live"]["label"])
    pnew, picp = R.solve_icp(lab, depth, params, rois, poses, render, max_error=0.02, nm_evals=0)
    assert render.many == 2  # no search stage
    e_init = np.linalg.norm(poses[0, 4:] - sc["true"][4:])
    e_icp = np.linalg.norm(picp[0, 4:] - sc["true"][4:])
    print("translation error: initial", e_init, "refined", e_icp)
    assert e_icp < e_init and e_icp < 3e-3
    render.many = 0
    pnew2, picp2 = R.solve_icp(lab, depth, params, rois, poses, render, max_error=0.02, nm_evals=50)
    assert render.many == 3
    assert abs(np.linalg.norm(picp2[0, :4]) - 1) < 1e-4
    assert np.linalg.norm(picp2[0, 4:] - sc["true"][4:]) < 5e-3
