"""Multi-object training scenes rendered on the device, backed by
libposecnn_hip.so (csrc/render_scene.hip): the role of the reference's online
frame synthesis -- Synthesizer::render (lib/synthesize/synthesize.cpp:345-609),
its `render` worker (tools/train_net.py:155-260) and _generate_vertex_targets
(lib/gt_synthesize_layer/minibatch.py:517-575).

SceneRenderer(meshes, H, W, camera, ...)   render(scene_offset, mesh_index,
                                           class_id, poses) -> dict of maps,
                                           render_into(...), expand(...)
sample_scenes(B, classes, seed, ...)       the reference's scene sampling
make_scene_frames(renderer, B, ...)        frames in synth.make_frames' layout,
                                           as device tensors

Narrowings: the ground truth only (label, depth, vertex map and vote targets;
image.py renders the lit colour picture and builds the input blob, without a
texture path); no `box` from the model point cloud (train_net.py:236-252); the
depth is metric float32, not the uint16 factor_depth encoding (:205-207).  The
geometry rules are at the top of csrc/render.hip, the scene rules at the top
of csrc/render_scene.hip and in DESIGN.md "Scene renderer".
"""
import numpy as np
import torch

from .. import _lib, synth
from .render import PackedMeshes


class SceneRenderer(PackedMeshes):
    """Renders S scenes of K object instances in all (meshes: dict class id ->
    Mesh), each scene depth-tested across its instances, into the training
    ground truth: label, depth, vertmap, the class-compact vote target
    vertex3, inst_id, visible and centers (include/posecnn_hip.h,
    pcnn_render_scenes).  The instances of scene s are the rows
    [scene_offset[s], scene_offset[s+1]) of mesh_index / class_id / poses."""

    def __init__(self, meshes, H, W, camera, znear=0.25, zfar=6.0, device="cuda"):
        super().__init__(meshes, H, W, camera, znear, zfar, device)
        # box extents of each mesh, for the vote's consumers (the reference reads extents.txt)
        self.extents = {int(o): (m.vertices.max(0) - m.vertices.min(0)).astype(np.float32) for o, m in meshes.items()}

    def render(self, scene_offset, mesh_index, class_id, poses, return_inst_id=True, stream=None):
        """Device tensors in (scene_offset (S+1), mesh_index (K), class_id (K)
        int32, poses (K,7) float32), fresh device tensors out, as a dict:
        label (S,H,W) int32, depth (S,H,W), vertmap (S,H,W,3), vertex3
        (S,H,W,3), inst_id (S,H,W) int32 (unless return_inst_id=False),
        visible (K) int32, centers (K,2).  Nothing is staged from the host and
        nothing is read back: no sync, and the call can be captured in a HIP
        graph once the stream's workspace has been sized by a first call."""
        dev = self.device
        S, K = scene_offset.numel() - 1, mesh_index.numel()
        H, W = self.H, self.W
        f32 = dict(dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        out = dict(label=torch.empty((S, H, W), **i32), depth=torch.empty((S, H, W), **f32),
                   vertmap=torch.empty((S, H, W, 3), **f32), vertex3=torch.empty((S, H, W, 3), **f32),
                   inst_id=torch.empty((S, H, W), **i32) if return_inst_id else None,
                   visible=torch.empty((K,), **i32), centers=torch.empty((K, 2), **f32))
        self.render_into(scene_offset, mesh_index, class_id, poses, stream=stream, **out)
        if not return_inst_id:
            del out["inst_id"]
        return out

    def render_into(self, scene_offset, mesh_index, class_id, poses, label, depth, vertmap, vertex3, visible, centers,
                    inst_id=None, stream=None, workspace=None):
        """The C-ABI call on caller-owned contiguous device tensors (S from
        scene_offset, K from poses, H x W from the renderer); every element of
        every output is written."""
        _lib.require_gpu(scene_offset, mesh_index, class_id, poses, label, depth, vertmap, vertex3, visible, centers,
                         inst_id)
        lib = _lib.load()
        S, K, H, W = scene_offset.numel() - 1, int(poses.shape[0]), self.H, self.W
        if S < 1 or K < 1:
            raise ValueError("SceneRenderer: at least one scene (scene_offset (S+1)) and one instance")
        i32, f32 = torch.int32, torch.float32
        # the kernels write S*H*W / K elements of these types: anything else would be a stray device write
        for name, t, shape, dt in (("scene_offset", scene_offset, (S + 1,), i32), ("mesh_index", mesh_index, (K,), i32),
                                   ("class_id", class_id, (K,), i32), ("poses", poses, (K, 7), f32),
                                   ("label", label, (S, H, W), i32), ("depth", depth, (S, H, W), f32),
                                   ("vertmap", vertmap, (S, H, W, 3), f32), ("vertex3", vertex3, (S, H, W, 3), f32),
                                   ("inst_id", inst_id, (S, H, W), i32), ("visible", visible, (K,), i32),
                                   ("centers", centers, (K, 2), f32)):
            if t is None and name == "inst_id":
                continue
            if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != poses.device:
                raise ValueError(f"SceneRenderer: {name} must be a contiguous {dt} tensor of shape {shape} on the "
                                 f"poses' device (got {tuple(t.shape)}, {t.dtype})")
        if workspace is None:
            workspace = _lib.workspace(lib.pcnn_render_scenes_workspace_size(S, K, H, W, self.V_total, self.F_max),
                                       self.device, "render_scenes", stream)
        fx, fy, px, py = self.camera
        rc = lib.pcnn_render_scenes(*self.mesh_args(), _lib.ptr(mesh_index), _lib.ptr(class_id), _lib.ptr(poses), K,
                                    _lib.ptr(scene_offset), S, H, W, fx, fy, px, py, self.znear, self.zfar,
                                    _lib.ptr(label), _lib.ptr(depth), _lib.ptr(vertmap), _lib.ptr(vertex3),
                                    _lib.ptr(inst_id), _lib.ptr(visible), _lib.ptr(centers), _lib.ptr(workspace),
                                    workspace.numel(), _lib.stream_ptr(stream))
        _lib.check(rc, "render_scenes")

    def expand(self, label, vertex3, C, w_inside=10.0, stream=None):
        """The reference's blobs from the compact target: (vertex_targets,
        vertex_weights), both (B,H,W,3C) (minibatch.py:253-254, 566-574)."""
        return expand(label, vertex3, C, w_inside, stream)


def expand(label, vertex3, C, w_inside=10.0, stream=None):
    """label (B,H,W) int32 and vertex3 (B,H,W,3) float32 on the device ->
    (vertex_targets, vertex_weights) (B,H,W,3C): a pixel with label l in
    [1, C) carries vertex3 at channels 3l..3l+2 and w_inside in the weights
    there; everything else is 0.  No sync."""
    _lib.require_gpu(label, vertex3)
    if label.dim() != 3 or vertex3.shape != (*label.shape, 3):
        raise ValueError("expand: label (B,H,W) and vertex3 (B,H,W,3)")
    if label.dtype != torch.int32 or vertex3.dtype != torch.float32:
        raise ValueError("expand: int32 label and float32 vertex3")
    label, vertex3 = label.contiguous(), vertex3.contiguous()
    B, H, W = label.shape
    targets = torch.empty((B, H, W, 3 * int(C)), dtype=torch.float32, device=label.device)
    weights = torch.empty_like(targets)
    rc = _lib.load().pcnn_vertex_targets_expand(_lib.ptr(label), _lib.ptr(vertex3), B, H, W, int(C), float(w_inside),
                                                _lib.ptr(targets), _lib.ptr(weights), _lib.stream_ptr(stream))
    _lib.check(rc, "vertex_targets_expand")
    return targets, weights


def _quat_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


_MAX_POSE_DRAWS = 10000  # per object, before sample_scenes gives up on min_dist


def _sample_scene(rng, classes, num_objects, tnear, tfar, min_dist):
    """One scene of synthesize.cpp:359-471 (is_sampling, not is_sampling_pose):
    (class ids (n,), poses (n,7) float64)."""
    lo, hi = num_objects
    n = int(rng.integers(lo, hi))  # irand excludes its maximum (thread_rand.h:113)
    cls = rng.choice(np.asarray(classes, np.int64), size=n, replace=False)  # distinct (:368-385)
    poses = np.zeros((n, 7))
    for i in range(n):
        for _ in range(_MAX_POSE_DRAWS):
            roll, pitch, yaw = np.deg2rad(rng.uniform(0.0, 360.0, size=3))  # :426-431, Rx(roll) Ry(pitch) Rz(yaw)
            q = _quat_mul(_quat_mul([np.cos(roll / 2), np.sin(roll / 2), 0, 0], [np.cos(pitch / 2), 0, np.sin(pitch / 2), 0]),
                          [np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)])
            t = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(tnear, tfar)])  # :437-439
            if i == 0 or np.linalg.norm(poses[:i, 4:] - t, axis=1).min() >= min_dist:  # :443-453
                break
        else:  # the reference would spin forever
            raise ValueError(f"sample_scenes: no place for object {i + 1} of {n} at min_dist = {min_dist} in "
                             f"[-0.1, 0.1]^2 x [{tnear}, {tfar}] after {_MAX_POSE_DRAWS} draws")
        poses[i, :4], poses[i, 4:] = q, t
    return cls, poses


def sample_scenes(B, classes, seed, image_offset=0, num_objects=(5, 8), tnear=0.5, tfar=2.0, min_dist=0.2,
                  attempts=None):
    """The reference's scene sampling (synthesize.cpp:359-471 with
    is_sampling=True, is_sampling_pose=False) for B images, on the host: per
    image n ~ U{lo, ..., hi-1} objects of distinct classes drawn from
    `classes`, rotation Rx(roll) Ry(pitch) Rz(yaw) with the angles uniform in
    0-360 degrees, translation U(-0.1, 0.1)^2 x U(tnear, tfar), a pose drawn
    again while it lies within min_dist of an earlier object of its scene.
    Image i draws from numpy.random.default_rng(seed*1000 + image_offset + i)
    (as synth.make_frames does, so a sharded run sees the single-device
    frames); attempts[i] > 0 selects the image's deterministic redraw number
    attempts[i] (make_scene_frames' rejected scenes).  The distribution is the
    reference's, its own random stream (thread_rand.h) is not reproduced.
    Returns numpy scene_offset (B+1) int32, class_id (K) int32, poses (K,7)
    float32 [qw qx qy qz tx ty tz]."""
    lo, hi = num_objects
    if not 0 < lo < hi or hi - 1 > len(classes):
        raise ValueError("sample_scenes: num_objects = (lo, hi) with 0 < lo < hi and hi - 1 distinct classes available")
    off, cls, poses = [0], [], []
    for i in range(B):
        gi = seed * 1000 + image_offset + i
        a = 0 if attempts is None else int(attempts[i])
        rng = np.random.default_rng(gi if a == 0 else [gi, a])
        c, p = _sample_scene(rng, classes, num_objects, tnear, tfar, min_dist)
        cls.append(c)
        poses.append(p)
        off.append(off[-1] + len(c))
    return (np.asarray(off, np.int32), np.concatenate(cls).astype(np.int32), np.concatenate(poses).astype(np.float32))


def make_scene_frames(renderer, B, classes=None, seed=0, image_offset=0, num_objects=(5, 8), tnear=0.5, tfar=2.0,
                      min_dist=0.2, min_pixels=800, num_classes=None, full_vertex=False, w_inside=10.0, voxel=None,
                      max_attempts=100, render=None, extra=()):
    """B training frames rendered by `renderer` (a SceneRenderer whose mesh
    keys are the class ids), in the layout of synth.make_frames but as device
    tensors: label (B,H,W) int32, vertex3 (B,H,W,3) the class-compact vote
    target, depth (B,H,W,1), meta (B,1,1,48) from synth.make_meta, gt rows
    [b, cls, 0,0,0,0, q, t] with b the global image index, extents (C,3) the
    meshes' boxes, K (3,3); full_vertex adds vertex and vertex_weights
    (B,H,W,3C) through expand.  Also visible (K) and scene_offset (B+1).

    As the reference's worker does (train_net.py:222-230), a scene is drawn
    again while any of its objects shows fewer than min_pixels pixels; redraw
    number a of image i is seeded by (seed*1000 + image_offset + i, a), so
    the frames depend on the global image index alone.  This convenience
    renders only the images still rejected (an image's maps do not depend on
    its batch), reads their `visible` back once per attempt and so syncs with
    the device; SceneRenderer.render does not.

    render(global image indices and scene_offset on the host, then
    scene_offset, mesh_index, class_id, poses on the device) -> dict replaces
    renderer.render(..., return_inst_id=False) for the attempts' draws, and each per-image map of its result named in `extra` is carried
    through the rejection loop into the frames under its own name (image.py's
    `color`: an accepted scene is not rendered twice)."""
    classes = sorted(renderer.slot) if classes is None else [int(c) for c in classes]
    C = int(num_classes) if num_classes is not None else max(renderer.slot) + 1
    dev, H, W = renderer.device, renderer.H, renderer.W
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    label = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    depth = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    vertex3 = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
    more = {}  # the maps named in `extra`, allocated from the first attempt's
    scene = [None] * B  # per image: (class ids, poses, visible) of its accepted draw
    todo, attempt = np.arange(B), 0
    while todo.size:
        if attempt > max_attempts:
            raise RuntimeError(f"make_scene_frames: no scene with {min_pixels} visible pixels per object after "
                               f"{max_attempts} redraws (images {(todo + image_offset).tolist()})")
        drawn = [sample_scenes(1, classes, seed, image_offset + int(i), num_objects, tnear, tfar, min_dist, [attempt])
                 for i in todo]
        off = np.concatenate([[0], np.cumsum([len(c) for _, c, _ in drawn])]).astype(np.int32)
        cls = np.concatenate([c for _, c, _ in drawn])
        slots = np.array([renderer.slot[int(c)] for c in cls], np.int32)
        poses = t(np.concatenate([p for _, _, p in drawn]))
        if render is None:
            out = renderer.render(t(off), t(slots), t(cls), poses, return_inst_id=False)
        else:
            out = render(todo + image_offset, off, t(off), t(slots), t(cls), poses)
        visible = out["visible"].cpu().numpy()
        ok = np.array([visible[off[j]:off[j + 1]].min() >= min_pixels for j in range(len(todo))])
        if ok.any():
            src, dst = t(np.flatnonzero(ok)), t(todo[ok])
            label[dst], depth[dst], vertex3[dst] = out["label"][src], out["depth"][src], out["vertex3"][src]
            for k in extra:
                if k not in more:
                    more[k] = torch.empty((B,) + tuple(out[k].shape[1:]), dtype=out[k].dtype, device=dev)
                more[k][dst] = out[k][src]
            for j in np.flatnonzero(ok):
                scene[todo[j]] = (drawn[j][1], drawn[j][2], visible[off[j]:off[j + 1]])
        todo, attempt = todo[~ok], attempt + 1
    fx, fy, px, py = renderer.camera
    K = np.array([[fx, 0, px], [0, fy, py], [0, 0, 1]], np.float64)
    off = np.concatenate([[0], np.cumsum([len(c) for c, _, _ in scene])]).astype(np.int32)
    gt = np.zeros((off[-1], 13), np.float32)
    gt[:, 0] = np.repeat(np.arange(B), np.diff(off)) + image_offset
    gt[:, 1] = np.concatenate([c for c, _, _ in scene])
    gt[:, 6:] = np.concatenate([p for _, p, _ in scene])
    extents = np.zeros((C, 3), np.float32)
    for c, e in renderer.extents.items():
        if c < C:
            extents[c] = e
    frames = dict(label=label, vertex3=vertex3, depth=depth.unsqueeze(-1), meta=t(synth.make_meta(K, B, voxel)),
                  gt=t(gt), extents=t(extents), K=t(K.astype(np.float32)),
                  visible=t(np.concatenate([v for _, _, v in scene]).astype(np.int32)), scene_offset=t(off))
    frames.update(more)
    if full_vertex:
        frames["vertex"], frames["vertex_weights"] = expand(label, vertex3, C, w_inside)
    return frames
