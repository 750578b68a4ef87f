"""Triangle-mesh renderer for the pose-refinement maps, backed by
libposecnn_hip.so (csrc/render.hip): the role of the reference's OpenGL pass
(lib/synthesize/synthesize.cpp:2103-2139 with the canonicalVerts.* and
vertsAndNorms.* shaders of lib/kinect_fusion/shaders).

Mesh(vertices, faces, normals=None,       a triangle mesh with vertex normals
     colors=None)                          and vertex colours
load_obj(path)                             -> Mesh (Wavefront v / vn / f lines)
MeshRenderer(meshes, H, W, camera, ...)    solve_icp's `render`: __call__(obj, pose)
                                           and render_many(objs, poses) ->
                                           (vertmap, pred_vertices, pred_normals)

No texture, colour or lighting here, one object per image (scene.py renders
several into one image, image.py adds the lit colour picture of a scene from
the meshes' vertex colours); the geometry rules are at the top of
csrc/render.hip and in DESIGN.md.
"""
import numpy as np
import torch

from .. import _lib


def vertex_normals(vertices, faces):
    """Area-weighted vertex normals: the sum of the incident faces' cross
    products, normalised (a vertex of no face, or of degenerate ones, keeps 0)."""
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    n = np.zeros_like(v)
    for j in range(3):
        np.add.at(n, f[:, j], fn)
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    return (n / np.where(ln > 0, ln, 1.0)).astype(np.float32)


class Mesh:
    """vertices (V,3) float32 in the model frame, faces (F,3) int32 vertex
    indices, normals (V,3) float32 (computed, area-weighted, when None),
    colors (V,3) float32 RGB in [0, 1] for the lit renderer (image.py), a
    mid-grey 0.5 when None (the reference's own fallback for a mesh without
    colours is a debug red)."""

    def __init__(self, vertices, faces, normals=None, colors=None):
        self.vertices = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
        self.faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
        V = len(self.vertices)
        if V == 0 or len(self.faces) == 0:
            raise ValueError("Mesh: needs at least one vertex and one face")
        if self.faces.min() < 0 or self.faces.max() >= V:
            raise ValueError("Mesh: face index outside the vertices")
        if normals is None:
            normals = vertex_normals(self.vertices, self.faces)
        self.normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        if len(self.normals) != V:
            raise ValueError("Mesh: one normal per vertex")
        if colors is None:
            colors = np.full((V, 3), 0.5, np.float32)
        self.colors = np.ascontiguousarray(colors, np.float32).reshape(-1, 3)
        if len(self.colors) != V:
            raise ValueError("Mesh: one colour per vertex")


def load_obj(path):
    """A small Wavefront reader: `v`, `vn` and `f` lines, the face forms i,
    i/j, i/j/k and i//k, negative (relative) indices, polygons fan-triangulated.
    Normals are taken per position index (the last face corner that names one
    wins); when any vertex is left without one, all are computed.  A file
    whose every `v` line has the form `v x y z r g b` gives the vertex
    colours; otherwise the colours are Mesh's default."""
    pos, col, nrm, faces, n_of = [], [], [], [], {}
    with open(path) as fh:
        for line in fh:
            tok = line.split("#", 1)[0].split()
            if not tok:
                continue
            if tok[0] == "v":
                pos.append([float(x) for x in tok[1:4]])
                if len(tok) == 7:
                    col.append([float(x) for x in tok[4:7]])
            elif tok[0] == "vn":
                nrm.append([float(x) for x in tok[1:4]])
            elif tok[0] == "f":
                corner = []
                for c in tok[1:]:
                    part = c.split("/")
                    i = int(part[0])
                    i = i - 1 if i > 0 else len(pos) + i
                    if not 0 <= i < len(pos):
                        raise ValueError(f"load_obj: {path}: vertex index {part[0]} out of range")
                    if len(part) == 3 and part[2]:
                        k = int(part[2])
                        k = k - 1 if k > 0 else len(nrm) + k
                        if not 0 <= k < len(nrm):
                            raise ValueError(f"load_obj: {path}: normal index {part[2]} out of range")
                        n_of[i] = k
                    corner.append(i)
                if len(corner) < 3:
                    raise ValueError(f"load_obj: {path}: face with fewer than 3 corners")
                faces += [[corner[0], corner[j], corner[j + 1]] for j in range(1, len(corner) - 1)]
    normals = None
    if pos and len(n_of) == len(pos):
        normals = np.asarray(nrm, np.float32)[[n_of[i] for i in range(len(pos))]]
    colors = np.asarray(col, np.float32) if pos and len(col) == len(pos) else None
    return Mesh(np.asarray(pos, np.float32), np.asarray(faces, np.int32), normals, colors)


class PackedMeshes:
    """The view (H x W, camera = (fx, fy, px, py), znear, zfar) and the mesh
    set (dict obj_id -> Mesh) packed onto the device once, in the layout the
    C ABI takes: what MeshRenderer and SceneRenderer share.  slot[obj_id] is
    the mesh's position in the set (the ABI's mesh_index); colors (V_total,3)
    is packed like the vertices, for the lit renderer."""

    def __init__(self, meshes, H, W, camera, znear=0.25, zfar=6.0, device="cuda"):
        self.H, self.W = int(H), int(W)
        self.camera = tuple(float(c) for c in camera)
        self.znear, self.zfar = float(znear), float(zfar)
        self.device = torch.device(device)
        _lib.require_gpu()
        if not meshes:
            raise ValueError(f"{type(self).__name__}: no meshes")
        self.slot = {int(o): i for i, o in enumerate(meshes)}
        ms = list(meshes.values())
        voff = np.concatenate([[0], np.cumsum([len(m.vertices) for m in ms])]).astype(np.int32)
        foff = np.concatenate([[0], np.cumsum([len(m.faces) for m in ms])]).astype(np.int32)
        self.M, self.V_total, self.F_total = len(ms), int(voff[-1]), int(foff[-1])
        self.F_max = max(len(m.faces) for m in ms)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)  # noqa: E731
        self.vertices = dev(np.concatenate([m.vertices for m in ms]))
        self.normals = dev(np.concatenate([m.normals for m in ms]))
        self.colors = dev(np.concatenate([m.colors for m in ms]))
        self.faces = dev(np.concatenate([m.faces for m in ms]))
        self.vert_offset, self.face_offset = dev(voff), dev(foff)

    def mesh_args(self):
        """The packed mesh set as the leading arguments of the C-ABI calls."""
        return (_lib.ptr(self.vertices), _lib.ptr(self.normals), _lib.ptr(self.faces), _lib.ptr(self.vert_offset),
                _lib.ptr(self.face_offset), self.M, self.V_total, self.F_total, self.F_max)


class MeshRenderer(PackedMeshes):
    """Renders meshes (dict obj_id -> Mesh) at H x W through camera = (fx, fy,
    px, py); the meshes are packed onto the device once.  Plugs into solve_icp
    as `render`: render_many(objs, poses (K,7)) -> (vertmap (K,H,W,3),
    pred_vertices (K,H,W,4), pred_normals (K,H,W,4)), fresh tensors per call;
    __call__(obj, pose) renders one pose ((H,W,.) maps).  return_depth /
    return_tri_id append depth (K,H,W) float32 / tri_id (K,H,W) int32.  poses
    may be numpy or a device tensor (no host sync either way); obj ids are
    host integers, the class written into vertmap's x.  An object id without a
    mesh raises KeyError."""

    def render_many(self, objs, poses, return_depth=False, return_tri_id=False, stream=None):
        objs = [int(o) for o in objs]
        K = len(objs)
        index = torch.tensor([[self.slot[o] for o in objs], objs], dtype=torch.int32).to(self.device,
                                                                                      non_blocking=True)
        return self.render_indexed(index[0], index[1], poses, return_depth, return_tri_id, stream)

    def render_indexed(self, mesh_index, class_id, poses, return_depth=False, return_tri_id=False, stream=None):
        """render_many with the mesh slots (positions in the dict given at
        construction) and class ids as device int32 tensors (K): nothing is
        staged from the host, so the call can be captured in a HIP graph.  A
        slot outside the mesh set renders an all-background image."""
        dev = self.device
        K = mesh_index.numel()
        if torch.is_tensor(poses):
            P = poses.to(device=dev, dtype=torch.float32).contiguous()
        else:
            P = torch.from_numpy(np.ascontiguousarray(poses, np.float32)).to(dev, non_blocking=True)
        if P.dim() != 2 or P.shape != (K, 7) or class_id.numel() != K:
            raise ValueError("MeshRenderer: poses (K,7), one object per pose")
        mi = mesh_index.to(device=dev, dtype=torch.int32).contiguous()
        ci = class_id.to(device=dev, dtype=torch.int32).contiguous()
        H, W = self.H, self.W
        f32 = dict(dtype=torch.float32, device=dev)
        vm = torch.empty((K, H, W, 3), **f32)
        pv = torch.empty((K, H, W, 4), **f32)
        pn = torch.empty((K, H, W, 4), **f32)
        depth = torch.empty((K, H, W), **f32) if return_depth else None
        tri = torch.empty((K, H, W), dtype=torch.int32, device=dev) if return_tri_id else None
        self.render_into(mi, ci, P, pv, pn, vm, depth, tri, stream)
        out = (vm, pv, pn)
        if return_depth:
            out += (depth,)
        if return_tri_id:
            out += (tri,)
        return out

    def render_into(self, mesh_index, class_id, poses, pred_vertices, pred_normals, vertmap, depth=None, tri_id=None,
                    stream=None, workspace=None):
        """The C-ABI call on caller-owned contiguous device tensors (K taken
        from poses, H x W from the renderer); every pixel of every map is
        written."""
        lib = _lib.load()
        K, H, W = int(poses.shape[0]), self.H, self.W
        if workspace is None:
            workspace = _lib.workspace(lib.pcnn_render_workspace_size(K, H, W, self.V_total, self.F_max), self.device,
                                       "render", stream)
        fx, fy, px, py = self.camera
        rc = lib.pcnn_render_meshes(*self.mesh_args(), _lib.ptr(mesh_index), _lib.ptr(class_id),
                                    _lib.ptr(poses), K, H, W, fx, fy, px, py, self.znear, self.zfar,
                                    _lib.ptr(pred_vertices), _lib.ptr(pred_normals), _lib.ptr(vertmap),
                                    _lib.ptr(depth), _lib.ptr(tri_id), _lib.ptr(workspace), workspace.numel(),
                                    _lib.stream_ptr(stream))
        _lib.check(rc, "render_meshes")

    def __call__(self, obj, pose, return_depth=False, return_tri_id=False, stream=None):
        p = pose.reshape(1, 7) if torch.is_tensor(pose) else np.asarray(pose, np.float32).reshape(1, 7)
        return tuple(m[0] for m in self.render_many([obj], p, return_depth, return_tri_id, stream))
