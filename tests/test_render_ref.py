"""The mesh renderer's host side (posecnn_amd/synthesize/render.py: Mesh,
load_obj) and the invariants of the numpy rasteriser reference
(tests/render_ref.py) that the GPU tests compare against: they establish the
fixtures before the GPU sees them.  No GPU is needed.

Bars: float32 against float64 raster_ref 5e-6 (m for positions, unitless for
normals): ten times the 5e-7 m measured between the two; the box against the
ray-caster of refine_scene.py likewise 5e-6 m."""
import numpy as np
import pytest

from posecnn_amd.synthesize.render import Mesh, load_obj, vertex_normals
from refine_scene import render_box
from render_ref import CAMERA4, box_mesh, fixtures, icosphere, reference

TOL = 5e-6
FIX = [(n, i) for n in ("icosphere", "torus", "box") for i in (0, 1)]


def test_load_obj_face_forms(tmp_path):
    """All four corner forms, a quad (fan-triangulated) and a comment."""
    p = tmp_path / "forms.obj"
    p.write_text("# four corner forms\n"
                 "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nv 0 0 1\n"
                 "vt 0 0\nvt 1 0\nvt 1 1\n"
                 "vn 0 0 1\nvn 0 0 -1\nvn 1 0 0\n"
                 "f 1 2 3\n"
                 "f 1/1 3/2 4/3\n"
                 "f 1/1/1 2/2/1 3/3/1 4/1/1\n"
                 "f 5//3 1//1 2//1\n")
    m = load_obj(str(p))
    assert m.vertices.shape == (5, 3) and m.vertices.dtype == np.float32
    np.testing.assert_array_equal(m.faces, [[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 3], [4, 0, 1]])
    # every position was given a normal by some corner: taken per position index
    np.testing.assert_array_equal(m.normals, [[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1], [1, 0, 0]])


def test_load_obj_negative_indices(tmp_path):
    p = tmp_path / "neg.obj"
    p.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nf -3//-1 -2//-1 -1//-1\n"
                 "v 0 0 2\nv 1 0 2\nv 0 1 2\nvn 0 0 -1\nf -3//-1 -1//-1 -2//-1\n")
    m = load_obj(str(p))
    np.testing.assert_array_equal(m.faces, [[0, 1, 2], [3, 5, 4]])
    np.testing.assert_array_equal(m.normals[:, 2], [1, 1, 1, -1, -1, -1])


def test_load_obj_missing_normals(tmp_path):
    """No vn lines, or some vertex without one: the normals are computed."""
    p = tmp_path / "tetra.obj"
    p.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nv 0 0 1\nvn 1 0 0\nf 1 3 2\nf 1 2 4\nf 2//1 3 4\nf 1 4 3\n")
    m = load_obj(str(p))
    np.testing.assert_array_equal(m.normals, vertex_normals(m.vertices, m.faces))
    np.testing.assert_allclose(np.linalg.norm(m.normals, axis=1), 1, atol=1e-6)
    np.testing.assert_allclose(m.normals[0], -np.ones(3) / np.sqrt(3), atol=1e-6)
    with pytest.raises(ValueError):
        bad = tmp_path / "bad.obj"
        bad.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n")
        load_obj(str(bad))


def test_computed_normals():
    """Area-weighted vertex normals: unit length; outward on the sphere; the
    flat side normals on the 24-vertex box."""
    s = icosphere(2, 0.05)
    n = Mesh(s.vertices, s.faces).normals
    np.testing.assert_allclose(np.linalg.norm(n, axis=1), 1, atol=1e-6)
    assert ((n * s.vertices).sum(1) > 0.99 * 0.05).all()
    b = box_mesh((0.06, 0.045, 0.035))
    np.testing.assert_allclose(Mesh(b.vertices, b.faces).normals, b.normals, atol=1e-6)
    with pytest.raises(ValueError):
        Mesh(b.vertices, b.faces + 24)


@pytest.mark.parametrize("name,i", FIX)
def test_float32_reference_against_float64(name, i):
    a, b = reference(name, i, np.float32), reference(name, i, np.float64)
    covered = b["tri_id"] >= 0
    assert covered.sum() > 300
    np.testing.assert_array_equal(a["tri_id"], b["tri_id"])
    for key in ("pred_v", "pred_n", "depth"):
        err = np.abs(a[key].astype(np.float64) - b[key]).max()
        print(name, i, key, err)
        assert err <= TOL
    assert np.abs(a["vertmap"].astype(np.float64) - b["vertmap"])[covered].max() <= TOL
    assert np.isnan(a["vertmap"][~covered]).all() and not np.isnan(a["vertmap"][covered]).any()
    assert (a["pred_v"][~covered] == 0).all() and (a["pred_n"][~covered] == 0).all()
    assert (a["pred_v"][covered][:, 3] == 1).all() and (a["pred_n"][..., 3] == 0).all()


@pytest.mark.parametrize("name,i", FIX)
def test_near_ties_are_rare(name, i):
    """At most 0.5 % of the covered pixels have their two nearest fragments
    closer than 1e-5 m (the pixels the GPU tests leave out of the bit-exact
    comparison)."""
    b = reference(name, i, np.float64)
    covered = b["tri_id"] >= 0
    close = covered & (b["gap"] < 1e-5)
    print(name, i, int(close.sum()), "of", int(covered.sum()))
    assert close.sum() <= 0.005 * covered.sum()


@pytest.mark.parametrize("i", [0, 1])
def test_box_against_ray_caster(i):
    mesh, cls, H, W, poses = fixtures()["box"]
    ray = render_box(poses[i].astype(np.float64), (0.06, 0.045, 0.035), cls, H, W, CAMERA4)
    for dt in (np.float32, np.float64):
        a = reference("box", i, dt)
        np.testing.assert_array_equal(a["tri_id"] >= 0, ray["hit"])
        hit = ray["hit"]
        err_v = np.abs(a["pred_v"].astype(np.float64) - ray["pred_v"])[hit].max()
        err_m = np.abs(a["vertmap"].astype(np.float64) - ray["vertmap"])[hit].max()
        print(i, dt.__name__, err_v, err_m)
        # render_box stores float32 maps: half an ulp at 1 m (6e-8) and at cls + x (2.4e-7) is inside the bar
        assert err_v <= TOL and err_m <= TOL


def test_even_fragment_count_on_closed_meshes():
    """The tie rule gives a pixel centre on a shared edge to one triangle:
    every covered pixel of a closed mesh sees an even number of fragments
    (it enters and leaves the solid)."""
    from render_ref import fragment_counts
    for name, (mesh, cls, H, W, poses) in fixtures().items():
        n = fragment_counts(mesh, poses[0], H, W, CAMERA4)
        assert (n % 2 == 0).all(), name
        assert (n > 0).sum() > 300
    # vertices on exact pixel centres and edges through them: an axis-aligned box seen head-on
    mesh = box_mesh((0.0625, 0.046875, 0.03125))
    cam = (256.0, 256.0, 64.0, 48.0)
    n = fragment_counts(mesh, np.array([1, 0, 0, 0, 0, 0, 0.53125], np.float32), 97, 131, cam)
    assert (n % 2 == 0).all() and (n > 0).sum() > 1000
