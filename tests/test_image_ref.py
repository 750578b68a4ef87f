"""CPU checks of the numpy restatements in tests/image_ref.py (the lit resolve
and the picture -> blob pass), of the host-side samplers of
posecnn_amd/synthesize/image.py, of include/posecnn_image.h against the
module's signature table and of load_obj's vertex colours."""
import colorsys
import ctypes
import os

import numpy as np
import pytest

import abi_guard
import image_ref as ir
from render_ref import CAMERA4, raster_ref
from scene_ref import H4, W4, scene_ref, three

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGE_HEADER = os.path.join(ROOT, "include", "posecnn_image.h")
F = np.float32
CAM = (100.0, 100.0, 80.0, 60.0)  # the principal point is the pixel centre (80, 60)
DEPTH = 0.8


def quad(color=(0.2, 0.5, 0.9)):
    """A 0.4 m square in the plane z = 0 facing the camera (normal -z), one colour."""
    from posecnn_amd.synthesize.render import Mesh
    v = np.array([[-0.2, -0.2, 0], [0.2, -0.2, 0], [0.2, 0.2, 0], [-0.2, 0.2, 0]], np.float32)
    return Mesh(v, [[0, 1, 2], [0, 2, 3]], np.tile([0, 0, -1.0], (4, 1)), np.tile(color, (4, 1)))


def shade_quad(light, shininess=60.0, dtype=np.float64):
    mesh = quad()
    inst = [(mesh, 1, np.array([1, 0, 0, 0, 0, 0, DEPTH], np.float32))]
    maps = scene_ref(inst, 120, 160, CAM, dtype)
    col, P = ir.shade_ref(inst, maps, [mesh.colors], light, [shininess], CAM, dtype)
    assert maps["inst_id"][60, 80] == 0 and abs(P[60, 80, 2] - DEPTH) < 1e-6 and np.abs(P[60, 80, :2]).max() < 1e-6
    return col[60, 80], mesh.colors[0].astype(np.float64)


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-9), (np.float32, 2e-6)])
def test_light_on_the_axis_gives_the_hand_derived_colour(dtype, tol):
    """N.L = 1 and V.R = 1 at the principal point: colour = I (ka c + att (c + 1))."""
    I, a, ka = 1.5, float(F(0.01)), 0.5
    got, c = shade_quad([0, 0, 0, 1, I, a, ka, 0], dtype=dtype)
    att = 1 / (1 + a * DEPTH ** 2)
    want = I * (ka * c + att * (c + 1))
    np.testing.assert_allclose(got[:3][::-1], want, atol=tol * 4, rtol=0)
    assert got[3] == 1 and got.dtype == dtype


def test_light_behind_the_surface_gives_the_ambient_term_only():
    I, ka = float(F(1.2)), 0.5
    got, c = shade_quad([0, 0, 2 * DEPTH, 1, I, 0.01, ka, 0])
    np.testing.assert_allclose(got[:3][::-1], ka * c * I, atol=1e-12, rtol=0)


def test_directional_light_has_no_attenuation():
    I, ka = float(F(0.8)), 0.5
    got, c = shade_quad([0, 0, -3.0, 0, I, 0.7, ka, 0])  # w = 0: the attenuation coefficient is not used
    np.testing.assert_allclose(got[:3][::-1], I * (ka * c + (c + 1)), atol=1e-9, rtol=0)


def test_weights_ref_reproduces_the_rasteriser_bits():
    """The recomputed weights give raster_ref's own pred_v and pred_n bit for bit."""
    from render_ref import vertex_pass
    mesh, cls, pose = three()[1]
    r = raster_ref(mesh, pose, cls, H4, W4, CAMERA4, dtype=np.float32)
    (la, lb, lc), (a, b, c) = ir.weights_ref(mesh, pose, r["tri_id"], CAMERA4)
    cam, nrm, _, _ = vertex_pass(mesh, pose, CAMERA4)
    hit = r["tri_id"] >= 0
    assert hit.sum() > 500
    for src, key in ((cam.astype(F), "pred_v"), (nrm.astype(F), "pred_n")):
        mix = (la[..., None] * src[a] + lb[..., None] * src[b]) + lc[..., None] * src[c]
        np.testing.assert_array_equal(mix[hit].view(np.int32), r[key][..., :3][hit].view(np.int32))


def test_shade_ref_background_and_alpha():
    inst = three()
    maps = scene_ref(inst, H4, W4, CAMERA4, np.float32)
    col, _ = ir.shade_ref(inst, maps, [ir.colored(m).colors for m, _, _ in inst], [0.3, -0.4, 0, 1, 1.3, 0.01, 0.5, 0],
                          [40, 80, 120], CAMERA4, np.float32)
    bg = maps["inst_id"] < 0
    assert (col[bg] == 0).all() and (col[~bg][:, 3] == 1).all() and col.dtype == np.float32
    assert np.isfinite(col).all() and col[~bg][:, :3].min() > 0


# ---- HLS ----
def _sampled_colours():
    g = np.arange(0, 256, 4)
    grid = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return np.concatenate([grid, [[255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [1, 0, 0], [254, 255, 255]]])


def test_hls_round_trip_is_the_identity_within_one_level():
    """rgb -> hls -> rgb of the float conversion, on every 4th level of each channel (256^3 / 64 colours)."""
    bgr = _sampled_colours()
    assert len(bgr) >= 256 ** 3 // 64
    back = ir.hls_to_bgr(*ir.bgr_to_hls(bgr))
    assert np.abs(back - bgr).max() <= 1


def test_8bit_hls_round_trip_stays_within_the_hue_quantum():
    """The chromatic step with zero jitter goes through the 8-bit store, whose
    hue quantum of 2 degrees is coarser than a level: a hue error of up to
    1 degree moves a channel by up to (p2 - p1) 255 / 60 <= 4.25 levels, the
    roundings of L, S and of the result add up to 0.5 each, so the round
    trip is the identity within 5 levels (measured: 4, and 27 % of the
    sampled colours move by more than one level); lightness, which the hue
    does not touch, and the grey axis keep to one level / exactly."""
    bgr = _sampled_colours()
    back = ir.chromatic_ref(bgr, 0.0, 0.0, 0.0)
    print("8-bit round trip: max", np.abs(back - bgr).max(), "levels; share above one level",
          (np.abs(back - bgr).max(1) > 1).mean())
    assert np.abs(back - bgr).max() <= 5
    H8, L8, S8 = ir.bgr_to_hls8(bgr)
    H2, L2, S2 = ir.bgr_to_hls8(back)
    assert np.abs(L2 - L8).max() <= 1
    grey = (bgr[:, 0] == bgr[:, 1]) & (bgr[:, 1] == bgr[:, 2])
    np.testing.assert_array_equal(back[grey], bgr[grey])
    assert (H8 >= 0).all() and (H8 < 180).all() and (L8 >= 0).all() and (L8 <= 255).all() and (S8 >= 0).all() and \
        (S8 <= 255).all()
    # the 8-bit inverse is the float inverse at the stored values, within a level
    assert np.abs(ir.hls8_to_bgr(H8, L8, S8) - ir.hls_to_bgr(2 * H8, L8 / 255, S8 / 255)).max() <= 1


def test_hls8_of_representable_values_round_trips_within_one_level():
    """hls -> bgr -> hls on 8-bit HLS triples whose colour the 8-bit BGR cube resolves."""
    rng = np.random.default_rng(3)
    H8, L8, S8 = rng.integers(0, 180, 4000), rng.integers(100, 156, 4000), rng.integers(200, 256, 4000)
    h2, l2, s2 = ir.bgr_to_hls8(ir.hls8_to_bgr(H8, L8, S8))
    dh = np.abs(h2 - H8)
    assert np.minimum(dh, 180 - dh).max() <= 1 and np.abs(l2 - L8).max() <= 1 and np.abs(s2 - S8).max() <= 3


def test_float_conversion_agrees_with_colorsys_within_one_level():
    bgr = _sampled_colours()[::7]
    H8, L8, S8 = ir.bgr_to_hls8(bgr)
    ref = np.array([colorsys.rgb_to_hls(r / 255, g / 255, b / 255) for b, g, r in bgr.tolist()])
    dh = np.abs(H8 - ref[:, 0] * 180)
    assert np.minimum(dh, 180 - dh).max() <= 1 and np.abs(L8 - ref[:, 1] * 255).max() <= 1
    assert np.abs(S8 - ref[:, 2] * 255).max() <= 1
    back = ir.hls8_to_bgr(H8, L8, S8)
    ref_back = np.array([colorsys.hls_to_rgb(h * 2 / 360, l / 255, s / 255) for h, l, s in zip(H8, L8, S8)])[:, ::-1]
    assert np.abs(back - ref_back * 255).max() <= 1


def test_a_hue_shift_of_180_is_the_identity():
    bgr = _sampled_colours()[::5]
    np.testing.assert_array_equal(ir.chromatic_ref(bgr, 180.0, 0.0, 0.0), ir.chromatic_ref(bgr, 0.0, 0.0, 0.0))
    H8, L8, S8 = ir.bgr_to_hls8(bgr)
    np.testing.assert_array_equal(ir.jitter_hls8(H8, L8, S8, 180.0, 0, 0)[0], H8)
    np.testing.assert_array_equal(ir.jitter_hls8(H8, L8, S8, -180.0, 0, 0)[0], H8)


def test_named_pixels_truncation_and_clips():
    q = ir.quantise(np.array([0.0, 1.0, 1.7, -0.3, 0.999, 100 / 255, 0.5, np.nan], F))
    np.testing.assert_array_equal(q, [0, 255, 255, 0, 254, 100, 127, 0])  # 0.999 * 255 = 254.7 and 127.5 truncate
    H8, L8, S8 = np.array([10, 179, 0]), np.array([250, 3, 128]), np.array([5, 250, 128])
    Hn, Ln, Sn = ir.jitter_hls8(H8, L8, S8, 1.8, 25.6, -25.6)
    np.testing.assert_array_equal(Hn, [11, 0, 1])      # 11.8 truncates; 180.8 wraps to 0.8
    np.testing.assert_array_equal(Ln, [255, 28, 153])  # clip at 255; 28.6 truncates
    np.testing.assert_array_equal(Sn, [0, 224, 102])   # clip at 0; 224.4 and 102.4 truncate
    np.testing.assert_array_equal(ir.jitter_hls8(H8, L8, S8, -1.8, 0, 0)[0], [8, 177, 178])  # 8.2, 177.2, -1.8 + 180


# ---- the deviate ----
def test_deviate_moments_and_keying():
    n = 160 * 120
    z = ir.deviate_ref(5, 7, n).astype(np.float64)
    assert np.isfinite(z).all()
    assert abs(z.mean()) <= 4 / np.sqrt(n)             # standard error of the mean
    assert abs(z.var() - 1) <= 4 * np.sqrt(2 / n)      # standard error of the variance of a normal sample
    np.testing.assert_array_equal(ir.deviate_ref(5, 7, 100), z[:100].astype(F))  # the pixel's value, not the image size
    assert (ir.deviate_ref(5, 8, 100) != z[:100].astype(F)).mean() > 0.9
    assert (ir.deviate_ref(6, 7, 100) != z[:100].astype(F)).mean() > 0.9
    assert (ir.deviate_ref(5, 7 + (1 << 32), 100) != z[:100].astype(F)).mean() > 0.9  # the index's high word


def test_blob_ref_noise_depends_on_the_global_image_alone():
    rng = np.random.default_rng(0)
    color = rng.uniform(0, 1, (2, 9, 11, 4)).astype(F)
    color[..., 3] = 1
    jit = np.array([[0, 0, 0, 3.0]] * 2, F)
    two = ir.image_blob_ref(color, None, [-1, -1], jit, seed=9, image_offset=3, noise=True)
    one = ir.image_blob_ref(color[1:], None, [-1], jit[1:], seed=9, image_offset=4, noise=True)
    np.testing.assert_array_equal(two[1], one[0])
    nchw = ir.image_blob_ref(color, None, [-1, -1], jit, seed=9, image_offset=3, noise=True, layout="NCHW")
    np.testing.assert_array_equal(nchw.transpose(0, 2, 3, 1), two)


# ---- the samplers ----
def test_sample_lights_ranges_and_keying():
    from posecnn_amd.synthesize.image import sample_lights
    off = np.array([0, 3, 5, 9, 10])
    L, s = sample_lights(4, 11, 2, off)
    assert L.shape == (4, 8) and L.dtype == F and s.shape == (10,) and s.dtype == F
    assert (np.abs(L[:, :2]) <= 2).all() and (L[:, 2] == 0).all() and (L[:, 3] == 1).all()
    assert (L[:, 4] >= 0.5).all() and (L[:, 4] <= 2).all() and (L[:, 5] == F(0.01)).all() and (L[:, 6] == 0.5).all()
    assert (L[:, 7] == 0).all() and (s >= 40).all() and (s <= 120).all()
    assert len(np.unique(L[:, 4])) == 4 and len(np.unique(s)) == 10
    L1, s1 = sample_lights(1, 11, 4, [0, 4])  # image 2 of the batch alone, by its global index
    np.testing.assert_array_equal(L1[0], L[2])
    np.testing.assert_array_equal(s1, s[5:9])
    many = sample_lights(400, 1)[0]
    assert many[:, 4].min() < 0.6 and many[:, 4].max() > 1.9 and many[:, 0].min() < -1.8 and many[:, 1].max() > 1.8


def test_sample_lights_leaves_sample_scenes_alone():
    from posecnn_amd.synthesize import sample_scenes
    from posecnn_amd.synthesize.image import sample_lights
    a = sample_scenes(2, [1, 2, 3, 4], 3, num_objects=(2, 4))
    sample_lights(2, 3, 0, a[0])
    b = sample_scenes(2, [1, 2, 3, 4], 3, num_objects=(2, 4))
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def test_sample_jitter_ranges_and_keying():
    from posecnn_amd.synthesize.image import sample_jitter
    j = sample_jitter(300, 2, 5, noise=True)
    assert j.shape == (300, 4) and j.dtype == F
    assert np.abs(j[:, 0]).max() <= 1.8 and np.abs(j[:, 1:3]).max() <= 25.6
    assert (j[:, 3] >= 0).all() and j[:, 3].max() <= np.sqrt(0.3 * 256) and j[:, 3].max() > 8
    assert np.abs(j[:, 0]).max() > 1.7 and np.abs(j[:, 1]).max() > 24
    np.testing.assert_array_equal(sample_jitter(1, 2, 12, noise=True)[0], j[7])
    quiet = sample_jitter(300, 2, 5)
    assert (quiet[:, 3] == 0).all()
    np.testing.assert_array_equal(quiet[:, :3], j[:, :3])


# ---- the header ----
def test_header_parses_and_matches_the_signature_table():
    from posecnn_amd import _lib
    from posecnn_amd.synthesize import image
    protos = abi_guard.prototypes(header=IMAGE_HEADER)
    assert set(protos) == set(image.SIGS) and not set(image.SIGS) & set(_lib._SIGS)
    ints = {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t, "uint64_t": ctypes.c_uint64,
            "int64_t": ctypes.c_int64}
    for name, params in protos.items():
        res, args = image.SIGS[name]
        assert len(args) == len(params), name
        for p, a in zip(params, args):
            assert a is (ctypes.c_void_p if p.is_pointer else ints[p.c_type]), (name, p.name)
            assert not p.is_pointer or p.elem_type in abi_guard.ELEM, (name, p.name)
    decl = open(IMAGE_HEADER).read()
    assert "size_t pcnn_render_scenes_lit_workspace_size" in decl and "int pcnn_image_blob" in decl
    # the lit renderer takes every parameter of pcnn_render_scenes, in its order
    plain = [p.name for p in abi_guard.prototypes()["pcnn_render_scenes"]]
    lit = [p.name for p in protos["pcnn_render_scenes_lit"]]
    assert [n for n in lit if n in plain] == plain and set(lit) - set(plain) == {"colors", "shininess", "lights", "color"}


def test_new_source_is_built_and_the_abi_version_is_8():
    from posecnn_amd import build
    assert "render_lit.hip" in build.SOURCES
    assert os.path.abspath(IMAGE_HEADER) in [os.path.abspath(h) for h in build.HEADERS]
    capi = open(os.path.join(ROOT, "posecnn_amd", "csrc", "capi.hip")).read()
    assert "pcnn_abi_version(void) { return 8; }" in capi


# ---- load_obj and Mesh ----
def test_load_obj_reads_vertex_colours(tmp_path):
    from posecnn_amd.synthesize import Mesh, load_obj
    p = tmp_path / "c.obj"
    p.write_text("v 0 0 0 1 0 0\nv 1 0 0 0 1 0\nv 0 1 0 0 0 1\nv 1 1 0 0.25 0.5 0.75\nf 1 2 3\nf 2 4 3\n")
    m = load_obj(str(p))
    np.testing.assert_array_equal(m.colors, np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.25, 0.5, 0.75]], F))
    assert m.colors.dtype == F and m.faces.shape == (2, 3)
    q = tmp_path / "plain.obj"
    q.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nf 1//1 2//1 3//1\n")
    n = load_obj(str(q))
    np.testing.assert_array_equal(n.colors, np.full((3, 3), 0.5, F))
    np.testing.assert_array_equal(n.normals, np.tile([0, 0, 1], (3, 1)).astype(F))
    mixed = tmp_path / "mixed.obj"  # one vertex without a colour: the default for all
    mixed.write_text("v 0 0 0 1 0 0\nv 1 0 0\nv 0 1 0 0 0 1\nf 1 2 3\n")
    np.testing.assert_array_equal(load_obj(str(mixed)).colors, np.full((3, 3), 0.5, F))
    with pytest.raises(ValueError):
        Mesh(n.vertices, n.faces, n.normals, np.zeros((2, 3)))
    plain = Mesh(n.vertices, n.faces)
    np.testing.assert_array_equal(plain.colors, np.full((3, 3), 0.5, F))
