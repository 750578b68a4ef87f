"""The lit scene renderer and the image blob (csrc/render_lit.hip through
include/posecnn_image.h and posecnn_amd/synthesize/image.py) against the numpy
restatements of tests/image_ref.py, whose own checks are in
tests/test_image_ref.py.  160 x 120, camera = refine_scene.CAMERA / 4, the
fixture "three" of tests/scene_ref.py with vertex colours, unless stated.

Bars
 - the seven maps shared with pcnn_render_scenes: its bits.
 - color: within 4 e32 of shade_ref in float64, e32 = max |shade_ref(float32) -
   shade_ref(float64)| on the fixture, computed here on the CPU.  Measured:
   e32 = 1.114e-5 at colours up to 2.70, so the bar is 4.455e-5 (the margin is
   for the device's powf and normalisations differing from libm's by a few
   ulps, each amplified by a shininess of up to 120).  Pixels whose two nearest
   fragments are closer than 1e-5 m in the float64 reference are left out, at
   most 0.5 % of the covered ones, the share asserted.  Background exactly
   (0, 0, 0, 0), alpha exactly 1 on the models.
 - batching, repetition, the path threshold (in a child process), graph
   replay: bitwise-equal color.
 - image_blob, noise off: the bits of image_ref.image_blob_ref; noise on:
   within 2 * 2^-16 (two float32 ulps of a value below 256: libm's and the
   device's double log / cos may differ in the last bit), and the same bits
   for an image whatever batch it comes in.
 - every output goes into the middle of a poisoned buffer whose 64-element
   guard bands must come back untouched.
 - end to end: the quantised levels of make_image_frames' image within one
   level of the float64 restatement everywhere and equal wherever 255 c64 is
   farther than 255 bar from an integer and below 255."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import abi_guard  # noqa: E402
import image_ref as ir  # noqa: E402
from render_ref import CAMERA4  # noqa: E402
from scene_ref import H4, W4, meshes, scene_ref, three, three_ref  # noqa: E402

pytestmark = pytest.mark.gpu
IMAGE_HEADER = os.path.join(ROOT, "include", "posecnn_image.h")
GAP = 1e-5
GUARD = 64
POISON = 12345.0
MAPS = ("label", "depth", "vertmap", "vertex3", "inst_id", "visible", "centers")
LIGHTS = np.array([[0.3, -0.4, 0, 1, 1.3, 0.01, 0.5, 0], [-1.0, 0.5, -2.0, 0, 0.9, 0.3, 0.4, 0]], np.float32)
SHININESS = np.array([40, 80, 120, 55, 100], np.float32)


def D():
    return torch.device("cuda")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(D())


def coloured_meshes():
    """class id -> the fixture's mesh with vertex colours (a phase per class)."""
    return {c: ir.colored(m, 0.3 * i) for i, (c, m) in enumerate(meshes().items())}


def two_scenes():
    """The batch of the tests: "three", then its torus and box alone under a directional light."""
    return [three(), [three()[1], three()[2]]]


def scene_args(slot, scenes):
    inst = [i for s in scenes for i in s]
    off = np.concatenate([[0], np.cumsum([len(s) for s in scenes])]).astype(np.int32)
    return (off, np.array([slot[c] for _, c, _ in inst], np.int32), np.array([c for _, c, _ in inst], np.int32),
            np.stack([p for _, _, p in inst]).astype(np.float32).reshape(-1, 7))


def guarded(shape, dtype, fill):
    n = int(np.prod(shape))
    full = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=D())
    return full, full[GUARD:GUARD + n].view(shape)


def check_guards(full, name):
    a = full.cpu().numpy()
    fill = 777 if a.dtype == np.int32 else np.float32(POISON)
    assert (a[:GUARD] == fill).all() and (a[-GUARD:] == fill).all(), f"{name}: write outside the output"


def render_lit(r, scenes, lights, shininess):
    """render_into the middle of poisoned buffers; numpy outputs, guard bands checked."""
    off, slots, classes, poses = scene_args(r.slot, scenes)
    S, K, H, W = len(off) - 1, len(slots), r.H, r.W
    f, i = torch.float32, torch.int32
    bufs = {"label": guarded((S, H, W), i, 777), "depth": guarded((S, H, W), f, POISON),
            "vertmap": guarded((S, H, W, 3), f, POISON), "vertex3": guarded((S, H, W, 3), f, POISON),
            "inst_id": guarded((S, H, W), i, 777), "visible": guarded((K,), i, 777),
            "centers": guarded((K, 2), f, POISON), "color": guarded((S, H, W, 4), f, POISON)}
    r.render_into(T(off), T(slots), T(classes), T(poses), T(shininess), T(lights), **{k: v[1] for k, v in bufs.items()})
    torch.cuda.synchronize()
    out = {}
    for k, (full, view) in bufs.items():
        check_guards(full, k)
        out[k] = view.cpu().numpy()
    assert not (out["color"] == POISON).any()
    return out


def same_bits(a, b, what):
    np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32), err_msg=what)


@pytest.fixture(scope="module")
def lit(hip):
    from posecnn_amd.synthesize import LitSceneRenderer
    return LitSceneRenderer(coloured_meshes(), H4, W4, CAMERA4, device=D())


@pytest.fixture(scope="module")
def two(lit):
    """The two-scene batch, rendered once; read-only."""
    return render_lit(lit, two_scenes(), LIGHTS, SHININESS)


@pytest.fixture(scope="module")
def e32():
    """max |shade_ref(float32) - shade_ref(float64)| on "three" (CPU) and the float64 colour."""
    cols = [coloured_meshes()[c].colors for _, c, _ in three()]
    a32, b64 = three_ref(np.float32), three_ref(np.float64)
    c32, _ = ir.shade_ref(three(), a32, cols, LIGHTS[0], SHININESS[:3], CAMERA4, np.float32)
    c64, _ = ir.shade_ref(three(), b64, cols, LIGHTS[0], SHININESS[:3], CAMERA4, np.float64)
    covered = b64["inst_id"] >= 0
    on = covered & ~(b64["gap"] < GAP)
    assert ((a32["inst_id"] == b64["inst_id"]) & (a32["face"] == b64["face"]))[on].all()
    e = float(np.abs(c32.astype(np.float64) - c64)[on].max())
    print(f"e32 = {e:.4g}, bar = {4 * e:.4g}, colours up to {c64[on][:, :3].max():.3g}")
    assert 1e-6 < e < 1e-4  # the order the float32 formats give at these magnitudes
    return e, c64


def test_shared_maps_carry_the_plain_renderer_bits(lit, two):
    from posecnn_amd.synthesize import SceneRenderer
    plain = SceneRenderer(coloured_meshes(), H4, W4, CAMERA4, device=D())
    off, slots, classes, poses = scene_args(plain.slot, two_scenes())
    ref = plain.render(T(off), T(slots), T(classes), T(poses))
    torch.cuda.synchronize()
    for k in MAPS:
        same_bits(two[k], ref[k].cpu().numpy(), k)
    assert (two["inst_id"][0] >= 0).sum() > 3000 and (two["inst_id"][1] >= 0).sum() > 1500
    # and those are the maps the existing tests pin: the float32 restatement off the near-tie pixels
    a32, b64 = three_ref(np.float32), three_ref(np.float64)
    keep = ~((b64["inst_id"] >= 0) & (b64["gap"] < GAP))
    np.testing.assert_array_equal(two["inst_id"][0][keep], a32["inst_id"][keep])
    np.testing.assert_array_equal(two["label"][0][keep], a32["label"][keep])


def test_color_matches_the_float64_restatement(two, e32):
    e, c64 = e32
    bar = 4 * e
    b64 = three_ref(np.float64)
    covered = b64["inst_id"] >= 0
    skip = covered & (b64["gap"] < GAP)
    share = skip.sum() / covered.sum()
    on = covered & ~skip
    got = two["color"][0]
    err = float(np.abs(got.astype(np.float64) - c64)[on].max())
    print(f"covered {int(covered.sum())}, left out {int(skip.sum())} ({share:.4%}), colour err {err:.4g}, bar {bar:.4g}")
    assert share <= 0.005
    assert err <= bar
    for s in range(2):
        hit = two["inst_id"][s] >= 0
        assert (two["color"][s][~hit] == 0).all() and (two["color"][s][hit][:, 3] == 1).all()
        assert np.isfinite(two["color"][s]).all() and (two["color"][s][hit][:, :3] > 0).all()
    # the second scene's directional light against its own restatement
    inst = two_scenes()[1]
    cols = [coloured_meshes()[c].colors for _, c, _ in inst]
    m64 = scene_ref(inst, H4, W4, CAMERA4, np.float64)
    d64, _ = ir.shade_ref(inst, m64, cols, LIGHTS[1], SHININESS[3:], CAMERA4, np.float64)
    on1 = (m64["inst_id"] >= 0) & ~(m64["gap"] < GAP)
    assert (~on1 & (m64["inst_id"] >= 0)).sum() <= 0.005 * (m64["inst_id"] >= 0).sum()
    err1 = float(np.abs(two["color"][1].astype(np.float64) - d64)[on1].max())
    print(f"directional scene: colour err {err1:.4g}")
    assert err1 <= bar


def test_batch_position_and_repetition_give_the_same_bits(lit, two):
    alone = render_lit(lit, [two_scenes()[1]], LIGHTS[1:], SHININESS[3:])
    same_bits(alone["color"][0], two["color"][1], "scene 1 alone")
    again = render_lit(lit, two_scenes(), LIGHTS, SHININESS)
    same_bits(again["color"], two["color"], "repetition")
    for k in MAPS:
        same_bits(again[k], two[k], k)


def test_both_triangle_paths_give_the_same_color(two, tmp_path):
    """Every triangle through the large-triangle queue (threshold 0), in a child process."""
    out = str(tmp_path / "color.npy")
    env = dict(os.environ, PCNN_RENDER_SMALL_MAX="0")
    subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, check=True, timeout=300)
    same_bits(np.load(out), two["color"], "threshold 0")


def test_graph_replay_on_a_side_stream(lit, two):
    off, slots, classes, poses = scene_args(lit.slot, two_scenes())
    a = [T(off), T(slots), T(classes), T(poses[::-1].copy()), T(SHININESS[::-1].copy()), T(LIGHTS[::-1].copy())]
    S, K = len(off) - 1, len(slots)
    f, i = dict(dtype=torch.float32, device=D()), dict(dtype=torch.int32, device=D())
    out = dict(label=torch.empty((S, H4, W4), **i), depth=torch.empty((S, H4, W4), **f),
               vertmap=torch.empty((S, H4, W4, 3), **f), vertex3=torch.empty((S, H4, W4, 3), **f),
               inst_id=torch.empty((S, H4, W4), **i), visible=torch.empty((K,), **i), centers=torch.empty((K, 2), **f),
               color=torch.empty((S, H4, W4, 4), **f))
    blob = torch.empty((S, H4, W4, 3), **f)
    from posecnn_amd.synthesize import image_blob
    bg_index, jitter = T(np.array([-1, -1], np.int32)), T(np.array([[1.0, 5, -5, 2.0]] * 2, np.float32))
    means = T(np.asarray(ir.PIXEL_MEANS, np.float32))

    def run(stream):
        lit.render_into(*a, stream=stream, **out)
        image_blob(out["color"], None, bg_index, jitter, means, seed=3, noise=True, out=blob, stream=stream)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up: sizes the stream's workspace outside the capture
        run(s)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        run(s)
    a[3].copy_(T(poses))  # captured with other poses, materials and lights than replayed
    a[4].copy_(T(SHININESS))
    a[5].copy_(T(LIGHTS))
    for o in list(out.values()) + [blob]:
        o.fill_(99)
    g.replay()
    torch.cuda.synchronize()
    same_bits(out["color"].cpu().numpy(), two["color"], "replayed color")
    eager = image_blob(T(two["color"]), None, bg_index, jitter, means, seed=3, noise=True)
    same_bits(blob.cpu().numpy(), eager.cpu().numpy(), "replayed blob")


# ---- image_blob ----
def blob_inputs(H, W, B=3):
    """Host-made inputs: a colour ramp through 0, 1, values above 1, negative
    ones and exact k / 255; alpha 0 and 1; two backgrounds and none; jitters at
    both ends of their ranges."""
    rng = np.random.default_rng(11)
    n = B * H * W
    ramp = np.linspace(-0.25, 1.35, n).astype(np.float32)
    color = np.stack([ramp, ramp[::-1], rng.integers(0, 256, n).astype(np.float32) / np.float32(255),
                      (rng.uniform(size=n) < 0.6).astype(np.float32)], 1).reshape(B, H, W, 4).copy()
    color[0, 0, :6, :3] = np.array([0.0, 1.0, 1.7, -0.3, 0.999, 100 / 255], np.float32)[:, None]
    color[0, 0, :6, 3] = 1
    color[1, :, :, 2] = rng.uniform(0, 1, (H, W)).astype(np.float32)
    bgs = rng.integers(0, 256, (2, H, W, 3)).astype(np.uint8)
    bgs[0, :2] = 255
    bgs[1, :2] = 0
    bg_index = np.array([0, 1, -1], np.int32)[:B]
    jitter = np.array([[1.8, 25.6, -25.6, 0], [-1.8, -25.6, 25.6, 0], [0.9, 12.3, 7.7, 0]], np.float32)[:B]
    return color, bgs, bg_index, jitter


def run_blob(color, bgs, bg_index, jitter, layout, **kw):
    """image_blob into the middle of a poisoned buffer; numpy result."""
    from posecnn_amd.synthesize import image_blob
    B, H, W, _ = color.shape
    shape = (B, H, W, 3) if layout == "NHWC" else (B, 3, H, W)
    full, view = guarded(shape, torch.float32, POISON)
    r = image_blob(T(color), None if bgs is None else T(bgs), T(bg_index), T(jitter), layout=layout, out=view, **kw)
    torch.cuda.synchronize()
    assert r is view
    check_guards(full, "blob")
    got = view.cpu().numpy()
    assert not (got == POISON).any()
    return got


# 157 x 119: odd, the batch ends inside a thread's four pixels; 16 x 12: H W a multiple of 4, NCHW's vector stores
@pytest.mark.parametrize("H,W", [(119, 157), (12, 16)])
@pytest.mark.parametrize("layout", ["NHWC", "NCHW"])
@pytest.mark.parametrize("chromatic", [True, False])
def test_image_blob_matches_the_restatement_bit_for_bit(hip, H, W, layout, chromatic):
    color, bgs, bg_index, jitter = blob_inputs(H, W)
    assert (3 * H * W) % 4 != 0 or (H * W) % 4 == 0
    got = run_blob(color, bgs, bg_index, jitter, layout, chromatic=chromatic, noise=False)
    ref = ir.image_blob_ref(color, bgs, bg_index, jitter, chromatic=chromatic, noise=False, layout=layout)
    same_bits(got, ref, f"{layout} chromatic={chromatic}")
    if not chromatic and layout == "NHWC":  # the named pixels: 0, 1, above 1, negative, truncation, k / 255
        lv = np.rint(got[0, 0, :6, 0] + np.float32(ir.PIXEL_MEANS[0]))
        np.testing.assert_array_equal(lv, [0, 255, 255, 0, 254, 100])
        pasted = color[..., 3] == 0
        assert pasted[0].any() and pasted[2].any() and (~pasted).any()
        np.testing.assert_array_equal(np.rint(got[2][pasted[2]] + np.asarray(ir.PIXEL_MEANS, np.float32)), 0)


def test_image_blob_without_backgrounds_and_other_means(hip):
    color, _, bg_index, jitter = blob_inputs(12, 16)
    means = (1.5, -2.25, 100.0)
    got = run_blob(color, None, bg_index, jitter, "NHWC", pixel_means=means)
    same_bits(got, ir.image_blob_ref(color, None, bg_index, jitter, means), "no backgrounds")


def test_image_blob_noise(hip):
    H, W = 119, 157
    color, bgs, bg_index, jitter = blob_inputs(H, W, B=2)
    jitter[:, 3] = [4.0, 8.7]
    kw = dict(seed=(7 << 32) | 5, chromatic=True, noise=True)
    got = run_blob(color, bgs, bg_index, jitter, "NHWC", image_offset=3, **kw)
    ref = ir.image_blob_ref(color, bgs, bg_index, jitter, image_offset=3, **kw)
    err = float(np.abs(got.astype(np.float64) - ref).max())
    quiet = ir.image_blob_ref(color, bgs, bg_index, jitter, chromatic=True, noise=False)
    print(f"noise: max |kernel - restatement| = {err:.3g}, values moved by the noise: {(ref != quiet).mean():.3f}")
    assert err <= 2 * 2.0 ** -16
    assert (ref != quiet).mean() > 0.9
    # one normal deviate per pixel, shared by the channels, where nothing clipped
    d = got - quiet
    # (chosen by the noiseless value, seven sigma from either end: the choice does not look at the noise)
    inner = (np.abs(quiet + np.asarray(ir.PIXEL_MEANS, np.float32) - 127.5) < 127.5 - 7 * 8.7).all(-1)
    assert np.abs(d[inner][:, 0] - d[inner][:, 1]).max() <= 2.0 ** -15
    z = d[1][inner[1]][:, 0].astype(np.float64) / 8.7
    assert len(z) > 1000
    assert abs(z.mean()) <= 4 / np.sqrt(len(z)) and abs(z.var() - 1) <= 4 * np.sqrt(2 / len(z))  # 4 standard errors
    # the global image index alone: image 1 of (B = 2, offset 3) is image 0 of (B = 1, offset 4)
    one = run_blob(color[1:], bgs, bg_index[1:], jitter[1:], "NHWC", image_offset=4, **kw)
    same_bits(one[0], got[1], "image 4 alone")
    far = run_blob(color[1:], bgs, bg_index[1:], jitter[1:], "NCHW", image_offset=(1 << 32) + 4, **kw)
    ref_far = ir.image_blob_ref(color[1:], bgs, bg_index[1:], jitter[1:], image_offset=(1 << 32) + 4, layout="NCHW", **kw)
    assert np.abs(far.astype(np.float64) - ref_far).max() <= 2 * 2.0 ** -16 and (far[0].transpose(1, 2, 0) != one[0]).any()


# ---- end to end ----
def test_make_image_frames(lit, e32):
    from posecnn_amd.synthesize import SceneRenderer, make_image_frames, make_scene_frames, sample_lights
    bar = 4 * e32[0]
    kw = dict(seed=4, num_objects=(3, 4), tnear=0.5, tfar=0.9, min_dist=0.12, min_pixels=50)
    a = make_image_frames(lit, 2, chromatic=False, **kw)
    plain = make_scene_frames(SceneRenderer(coloured_meshes(), H4, W4, CAMERA4, device=D()), 2, **kw)
    for k in ("label", "vertex3", "gt", "depth", "visible", "scene_offset"):
        assert torch.equal(a[k].view(torch.int32), plain[k].view(torch.int32)), k
    assert set(a) == set(plain) | {"color", "image"}
    assert a["color"].shape == (2, H4, W4, 4) and a["image"].shape == (2, H4, W4, 3) and a["image"].is_cuda
    levels = np.rint(a["image"].cpu().numpy() + np.asarray(ir.PIXEL_MEANS, np.float32)).astype(np.int64)
    gt, off = a["gt"].cpu().numpy(), a["scene_offset"].cpu().numpy()
    cm = coloured_meshes()
    for b in range(2):
        rows = gt[off[b]:off[b + 1]]
        inst = [(cm[int(r[1])], int(r[1]), r[6:13]) for r in rows]
        light, shin = sample_lights(1, 4, b, [0, len(inst)])
        m64 = scene_ref(inst, H4, W4, CAMERA4, np.float64)
        c64, _ = ir.shade_ref(inst, m64, [m.colors for m, _, _ in inst], light[0], shin, CAMERA4, np.float64)
        x = 255.0 * c64[..., :3]
        want = np.floor(np.clip(x, 0, 255)).astype(np.int64)
        diff = np.abs(levels[b] - want)
        firm = (np.abs(x - np.rint(x)) > 255 * bar) & (x < 255)
        print(f"image {b}: levels off by one {int((diff == 1).sum())}, more {int((diff > 1).sum())}, "
              f"firm pixels {firm.mean():.4f}, levels up to {want.max()}")
        assert diff.max() <= 1
        np.testing.assert_array_equal(levels[b][firm], want[firm])
        assert (want > 0).any() and (levels[b][m64["inst_id"] < 0] == 0).all()
    # a shard: image 1 alone is image 1 of the pair, with chromatic jitter, noise, a background and NCHW
    bgs = T(np.random.default_rng(2).integers(0, 256, (3, H4, W4, 3)).astype(np.uint8))
    full = make_image_frames(lit, 2, backgrounds=bgs, noise=True, layout="NCHW", **kw)
    part = make_image_frames(lit, 1, image_offset=1, backgrounds=bgs, noise=True, layout="NCHW", **kw)
    assert full["image"].shape == (2, 3, H4, W4)
    for k in ("image", "color", "label"):
        assert torch.equal(part[k][0].view(torch.int32), full[k][1].view(torch.int32)), k
    bg = (full["label"][1] == 0).cpu().numpy()
    img = full["image"][1].permute(1, 2, 0).cpu().numpy()
    assert np.abs(img[bg]).max() > 50 and not torch.equal(full["image"][1], a["image"][1].permute(2, 0, 1))


# ---- the wrappers' contract, through the guard on the new header ----
def _variants(t):
    """A float64 (for an integer tensor: int64), a strided and a CPU form of `t`."""
    wide = t.to(torch.float64 if t.dtype.is_floating_point else torch.int64)
    if t.dtype == torch.uint8:
        wide = t.to(torch.float64)
    big = torch.zeros(t.shape[:-1] + (2 * t.shape[-1],), dtype=t.dtype, device=t.device)
    strided = big[..., ::2]
    strided.copy_(t)
    assert not strided.is_contiguous() or t.numel() <= 1
    return {"float64": wide, "strided": strided, "cpu": t.cpu()}


def test_wrappers_keep_the_header_contract(lit):
    from posecnn_amd import _lib
    from posecnn_amd.synthesize import image
    real = image._load()
    assert isinstance(real, type(_lib.load())) and real.pcnn_image_blob.argtypes is not None
    guard = abi_guard.GuardedLib(real, header=IMAGE_HEADER)
    off, slots, classes, poses = scene_args(lit.slot, two_scenes())
    S, K = len(off) - 1, len(slots)
    f, i = dict(dtype=torch.float32, device=D()), dict(dtype=torch.int32, device=D())
    rargs = dict(scene_offset=T(off), mesh_index=T(slots), class_id=T(classes), poses=T(poses), shininess=T(SHININESS),
                 lights=T(LIGHTS), label=torch.empty((S, H4, W4), **i), depth=torch.empty((S, H4, W4), **f),
                 vertmap=torch.empty((S, H4, W4, 3), **f), vertex3=torch.empty((S, H4, W4, 3), **f),
                 inst_id=torch.empty((S, H4, W4), **i), visible=torch.empty((K,), **i),
                 centers=torch.empty((K, 2), **f), color=torch.empty((S, H4, W4, 4), **f))
    color, bgs, bg_index, jitter = blob_inputs(12, 16)
    bargs = dict(color=T(color), backgrounds=T(bgs), bg_index=T(bg_index), jitter=T(jitter),
                 pixel_means=T(np.asarray(ir.PIXEL_MEANS, np.float32)), out=torch.empty((3, 12, 16, 3), **f))
    _lib._lib = guard
    try:
        lit.render_into(**rargs)
        lit.render(*(rargs[k] for k in ("scene_offset", "mesh_index", "class_id", "poses", "shininess", "lights")))
        image.image_blob(**bargs)
        image.image_blob(**dict(bargs, backgrounds=None, out=None, layout="NHWC", noise=True))
        torch.cuda.synchronize()
        assert guard.calls["pcnn_render_scenes_lit"] == 2 and guard.calls["pcnn_image_blob"] == 2
        assert guard.launches == 4
        guard.reset()
        for call, args in ((lit.render_into, rargs), (image.image_blob, bargs)):
            for name, t in args.items():
                for what, bad in _variants(t).items():
                    with pytest.raises(ValueError):
                        call(**dict(args, **{name: bad}))
                    assert sum(guard.calls.values()) == 0, (call.__name__, name, what)
        with pytest.raises(ValueError):
            image.image_blob(**dict(bargs, layout="HWC"))
        with pytest.raises(ValueError):
            image.image_blob(**dict(bargs, out=torch.empty((3, 3, 12, 16), **f)))  # NCHW's shape for NHWC
        assert sum(guard.calls.values()) == 0 and guard.launches == 0
    finally:
        _lib._lib = real
    # the guard refuses what the wrappers would have let through
    with pytest.raises(abi_guard.AbiContractError):
        guard.pcnn_image_blob(_lib.ptr(bargs["color"].double()), None, 0, _lib.ptr(bargs["bg_index"]),
                              _lib.ptr(bargs["jitter"]), _lib.ptr(bargs["pixel_means"]), 0, 0, 3, 12, 16, 0,
                              _lib.ptr(bargs["out"]), _lib.stream_ptr())
    torch.cuda.synchronize()


if __name__ == "__main__":  # the child of test_both_triangle_paths_give_the_same_color: argv[1] = where to save color
    from posecnn_amd.synthesize import LitSceneRenderer
    child = LitSceneRenderer(coloured_meshes(), H4, W4, CAMERA4, device=D())
    np.save(sys.argv[1], render_lit(child, two_scenes(), LIGHTS, SHININESS)["color"])
