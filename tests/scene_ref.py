"""Test-only helper for the scene renderer (csrc/render_scene.hip): scene_ref
composes render_ref.raster_ref (the numpy restatement of the rasteriser's
rules) per instance into one depth-tested scene and builds the training
ground truth from it with the numeric types of the reference's
_generate_vertex_targets (lib/gt_synthesize_layer/minibatch.py:556-568).
Also the shared fixture "three" and the numpy scatter that
pcnn_vertex_targets_expand is compared with."""
import functools

import numpy as np

from refine_scene import axis_angle_quat
from render_ref import CAMERA4, box_mesh, icosphere, raster_ref, torus

H4, W4 = 120, 160


def scene_ref(instances, H, W, camera, dtype=np.float32, znear=0.25, zfar=6.0):
    """instances: [(mesh, class id, pose (7,) float32)] in rank order.  The
    scene's maps: the instance of the smallest depth wins a pixel (argmin
    takes the first minimum: an equal depth goes to the lower rank).  Returns
    label, inst_id, face (H,W) int32, depth (H,W) and vertmap (H,W,3) in
    `dtype`, vertex3 (H,W,3) float32, visible (n,) int32, centers (n,2)
    float32 and gap (H,W) float64: the depth between the two nearest
    fragments of the pixel, of any instance (inf with fewer than two)."""
    n = len(instances)
    r = [raster_ref(m, np.asarray(p, np.float32), c, H, W, camera, znear, zfar, dtype=dtype) for m, c, p in instances]
    z = np.stack([np.where(x["tri_id"] >= 0, x["depth"].astype(np.float64), np.inf) for x in r])
    win = z.argmin(0)
    covered = np.isfinite(z).any(0)
    inst = np.where(covered, win, -1).astype(np.int32)
    pick = lambda key: np.take_along_axis(np.stack([x[key] for x in r]), win[None], 0)[0]  # noqa: E731
    cls = np.array([c for _, c, _ in instances], np.int32)
    label = np.where(covered, cls[win], 0).astype(np.int32)
    face = np.where(covered, pick("tri_id"), -1).astype(np.int32)
    depth = np.where(covered, pick("depth"), 0).astype(dtype)
    vertmap = np.take_along_axis(np.stack([x["vertmap"] for x in r]), win[None, ..., None], 0)[0]
    vertmap = np.where(covered[..., None], vertmap, np.nan).astype(dtype)
    zs = np.sort(z, 0)
    with np.errstate(invalid="ignore"):
        between = zs[1] - zs[0] if n > 1 else np.full((H, W), np.inf)
    gap = np.where(covered, np.minimum(pick("gap"), np.where(np.isnan(between), np.inf, between)), np.inf)
    visible = np.array([(inst == i).sum() for i in range(n)], np.int32)
    # synthesize.cpp:558-562, float arithmetic
    fx, fy, px, py = (np.float32(c) for c in camera)
    poses = np.stack([np.asarray(p, np.float32) for _, _, p in instances])
    centers = np.stack([fx * (poses[:, 4] / poses[:, 6]) + px, fy * (poses[:, 5] / poses[:, 6]) + py], 1)
    assert centers.dtype == np.float32
    # The vote target of each pixel's winning instance, with the numeric types
    # of minibatch.py:556-568: float32 centre, the difference to the pixel, its
    # norm (+ 1e-10) and the quotient in float64, float32 on store; log tz in
    # float64, float32 on store.
    vertex3 = np.zeros((H, W, 3), np.float32)
    ys, xs = np.mgrid[0:H, 0:W]
    won = inst >= 0
    own = np.maximum(inst, 0)
    dx = centers[own, 0].astype(np.float64) - xs
    dy = centers[own, 1].astype(np.float64) - ys
    length = np.sqrt(dx * dx + dy * dy) + 1e-10
    logz = np.log(poses[:, 6].astype(np.float64)).astype(np.float32)
    vertex3[..., 0] = np.where(won, dx / length, 0)
    vertex3[..., 1] = np.where(won, dy / length, 0)
    vertex3[..., 2] = np.where(won, logz[own], 0)
    return dict(label=label, inst_id=inst, face=face, depth=depth, vertmap=vertmap, vertex3=vertex3, visible=visible,
                centers=centers, gap=gap)


def pose_of(axis, angle, t):
    return np.concatenate([axis_angle_quat(axis, angle), t]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def meshes():
    """class id -> Mesh: the three closed test meshes of render_ref.py."""
    return {2: icosphere(3, 0.05), 5: torus(0.05, 0.02, 48, 24), 3: box_mesh((0.06, 0.045, 0.035))}


@functools.lru_cache(maxsize=None)
def three():
    """The shared fixture: sphere, torus and box overlapping in one 160 x 120
    image, [(mesh, class, pose)] in rank order.  Treat as read-only."""
    m = meshes()
    return [(m[2], 2, pose_of((1, 2, 3), 0.7, (-0.045, -0.01, 0.62))),
            (m[5], 5, pose_of((0.3, 1, 0.2), 0.9, (0.07, 0.02, 0.72))),
            (m[3], 3, pose_of((1, 0.2, 0.5), 1.1, (0.0, 0.0, 0.66)))]


# extents (C,3) for the vote on "three": class 2 the sphere, 3 the box, 5 the torus
EXTENTS = np.zeros((7, 3), np.float32)
EXTENTS[2] = (0.1, 0.1, 0.1)
EXTENTS[5] = (0.14, 0.14, 0.04)
EXTENTS[3] = (0.12, 0.09, 0.07)


@functools.lru_cache(maxsize=None)
def three_ref(dtype):
    """scene_ref of "three", once per process; treat as read-only."""
    return scene_ref(three(), H4, W4, CAMERA4, dtype)


@functools.lru_cache(maxsize=None)
def alone_ref(i, dtype):
    """Instance i of "three" rendered alone."""
    return scene_ref(three()[i:i + 1], H4, W4, CAMERA4, dtype)


def expand_ref(label, vertex3, C, w_inside=10.0):
    """The scatter of minibatch.py:253-254, 566-574: (targets, weights) (...,3C)."""
    targets = np.zeros(label.shape + (3 * C,), np.float32)
    weights = np.zeros_like(targets)
    for l in range(1, C):
        idx = np.where(label == l)
        for j in range(3):
            targets[idx + (3 * l + j,)] = vertex3[idx + (j,)]
            weights[idx + (3 * l + j,)] = np.float32(w_inside)
    return targets, weights
