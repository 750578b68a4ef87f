"""The network's input for the synthetic training frames, on the device,
backed by libposecnn_hip.so (csrc/render_lit.hip, include/posecnn_image.h):
the Phong-lit colour pass of the reference's Synthesizer::render
(lib/synthesize/synthesize.cpp:473-536, 575-590 with the shaders
canonicalVertsAndColor.*) and its _get_image_blob (lib/gt_synthesize_layer/
minibatch.py:132-187 with chromatic_transform and add_noise,
lib/utils/blob.py:74-129).

LitSceneRenderer(meshes, H, W, camera, ...)  SceneRenderer whose render /
                                             render_into also take shininess (K)
                                             and lights (S,8) and return `color`
sample_lights(B, seed, ...)                  the reference's light and shininess
sample_jitter(B, seed, ...)                  the reference's chromatic / noise draws
image_blob(color, backgrounds, ...)          picture -> mean-subtracted BGR blob
make_image_frames(renderer, B, ...)          make_scene_frames' frames plus
                                             `color` and `image`

Narrowings: the surface colour is the interpolated vertex colour (no texture
path); the vertex normals are normalised after the rotation, per vertex (the
reference normalises the interpolated raw normal; the same for unit mesh
normals); the HLS conversion is the standard hexcone formula with 8-bit
storage, not OpenCV's 8-bit code path, whose own rounding is not pinned;
add_noise's 10 % motion-blur branch, background resizing (backgrounds arrive
at H x W), flipping, multi-scale and the DEPTH / RGBD / NORMAL inputs are not
done.  The rules are in include/posecnn_image.h and DESIGN.md "Scene
renderer"; tests/image_ref.py restates them in numpy.
"""
import ctypes

import numpy as np
import torch

from .. import _lib
from .scene import SceneRenderer, make_scene_frames

PIXEL_MEANS = (102.9801, 115.9465, 122.7717)  # BGR, lib/fcn/config.py:242
CHROMATIC, NOISE, NCHW = 1, 2, 4              # pcnn_image_blob's flags

_v, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
# include/posecnn_image.h: name -> (restype, argtypes); v = device pointer or stream
SIGS = {
    "pcnn_render_scenes_lit_workspace_size": (ctypes.c_size_t, [_i] * 6),
    "pcnn_render_scenes_lit": (_i, [_v, _v, _v, _v, _v, _v, _i, _i, _i, _i, _v, _v, _v, _v, _i, _v, _v, _i, _i, _i,
                                    _f, _f, _f, _f, _f, _f, _v, _v, _v, _v, _v, _v, _v, _v, _v, ctypes.c_size_t, _v]),
    "pcnn_image_blob": (_i, [_v, _v, _i, _v, _v, _v, ctypes.c_uint64, ctypes.c_int64, _i, _i, _i, _i, _v, _v]),
}
_bound = None


def _load():
    """_lib.load()'s handle with this module's prototypes set on it (once).  A
    library without the entry points is an error: there is no other path."""
    global _bound
    lib = _lib.load()
    if isinstance(lib, ctypes.CDLL) and lib is not _bound:
        for name, (res, args) in SIGS.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:
                raise _lib.PcnnError(f"{_lib.LIB_PATH} has no {name} (ABI version {lib.pcnn_abi_version()} < 8); "
                                     "rebuild it: __graft_entry__.build()") from None
            fn.restype = res
            fn.argtypes = args
        _bound = lib
    return lib


def _want(who, name, t, shape, dtype, device):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{who}: {name}: expected a torch.Tensor, got {type(t).__name__}")
    if tuple(t.shape) != tuple(shape) or t.dtype != dtype or not t.is_contiguous() or not t.is_cuda or \
            t.device != device:
        raise ValueError(f"{who}: {name} must be a contiguous {dtype} tensor of shape {tuple(shape)} on {device} "
                         f"(got {tuple(t.shape)}, {t.dtype}, strides {tuple(t.stride())}, {t.device})")
    return t


class LitSceneRenderer(SceneRenderer):
    """SceneRenderer with the colour attachment (include/posecnn_image.h,
    pcnn_render_scenes_lit): the meshes' vertex colours lit by one light per
    scene, lights (S,8) [x y z w, intensity, attenuation, ambient, 0] in the
    camera frame (w = 0: directional), with one specular exponent per
    instance, shininess (K).  The seven maps of SceneRenderer carry the same
    bits; `color` (S,H,W,4) is linear float32 BGRA, alpha 1 on the models and
    all 0 off them."""

    def render(self, scene_offset, mesh_index, class_id, poses, shininess, lights, return_inst_id=True, stream=None):
        """SceneRenderer.render's tensors plus shininess (K) and lights (S,8)
        float32 in; its dict plus color (S,H,W,4) out.  No sync; capturable
        once the stream's workspace has been sized by a first call."""
        dev = self.device
        S, K = scene_offset.numel() - 1, mesh_index.numel()
        H, W = self.H, self.W
        f32 = dict(dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        out = dict(label=torch.empty((S, H, W), **i32), depth=torch.empty((S, H, W), **f32),
                   vertmap=torch.empty((S, H, W, 3), **f32), vertex3=torch.empty((S, H, W, 3), **f32),
                   inst_id=torch.empty((S, H, W), **i32) if return_inst_id else None,
                   visible=torch.empty((K,), **i32), centers=torch.empty((K, 2), **f32),
                   color=torch.empty((S, H, W, 4), **f32))
        self.render_into(scene_offset, mesh_index, class_id, poses, shininess, lights, stream=stream, **out)
        if not return_inst_id:
            del out["inst_id"]
        return out

    def render_into(self, scene_offset, mesh_index, class_id, poses, shininess, lights, label, depth, vertmap, vertex3,
                    visible, centers, color, inst_id=None, stream=None, workspace=None):
        """The C-ABI call on caller-owned contiguous device tensors; every
        element of every output is written."""
        who = "LitSceneRenderer"
        if not isinstance(poses, torch.Tensor) or not isinstance(scene_offset, torch.Tensor):
            raise TypeError(f"{who}: scene_offset and poses must be tensors")
        S, K, H, W = scene_offset.numel() - 1, int(poses.shape[0]) if poses.dim() else 0, self.H, self.W
        if S < 1 or K < 1:
            raise ValueError(f"{who}: at least one scene (scene_offset (S+1)) and one instance")
        i32, f32 = torch.int32, torch.float32
        # the kernels read and write S*H*W / K elements of these types: anything else would be a stray device access
        for name, t, shape, dt in (("scene_offset", scene_offset, (S + 1,), i32), ("mesh_index", mesh_index, (K,), i32),
                                   ("class_id", class_id, (K,), i32), ("poses", poses, (K, 7), f32),
                                   ("shininess", shininess, (K,), f32), ("lights", lights, (S, 8), f32),
                                   ("label", label, (S, H, W), i32), ("depth", depth, (S, H, W), f32),
                                   ("vertmap", vertmap, (S, H, W, 3), f32), ("vertex3", vertex3, (S, H, W, 3), f32),
                                   ("inst_id", inst_id, (S, H, W), i32), ("visible", visible, (K,), i32),
                                   ("centers", centers, (K, 2), f32), ("color", color, (S, H, W, 4), f32)):
            if t is None and name == "inst_id":
                continue
            _want(who, name, t, shape, dt, self.vertices.device)
        lib = _load()
        if workspace is None:
            workspace = _lib.workspace(lib.pcnn_render_scenes_lit_workspace_size(S, K, H, W, self.V_total, self.F_max),
                                       self.device, "render_scenes_lit", stream)
        else:
            _lib.require(workspace, torch.uint8, name=f"{who}: workspace")
        fx, fy, px, py = self.camera
        rc = lib.pcnn_render_scenes_lit(
            _lib.ptr(self.vertices), _lib.ptr(self.normals), _lib.ptr(self.colors), _lib.ptr(self.faces),
            _lib.ptr(self.vert_offset), _lib.ptr(self.face_offset), self.M, self.V_total, self.F_total, self.F_max,
            _lib.ptr(mesh_index), _lib.ptr(class_id), _lib.ptr(poses), _lib.ptr(shininess), K, _lib.ptr(scene_offset),
            _lib.ptr(lights), S, H, W, fx, fy, px, py, self.znear, self.zfar, _lib.ptr(label), _lib.ptr(depth),
            _lib.ptr(vertmap), _lib.ptr(vertex3), _lib.ptr(inst_id), _lib.ptr(visible), _lib.ptr(centers),
            _lib.ptr(color), _lib.ptr(workspace), workspace.numel(), _lib.stream_ptr(stream))
        _lib.check(rc, "render_scenes_lit")


_TAG_LIGHT, _TAG_JITTER = 0x4C495445, 0x4A495454  # the streams of sample_lights / sample_jitter ("LITE", "JITT")


def sample_lights(B, seed, image_offset=0, scene_offset=None):
    """The reference's light and material sampling (synthesize.cpp:476-481,
    498) for B images, on the host: per image one point light of intensity
    U(0.5, 2) at (U(-2, 2), U(-2, 2), 0, 1) in the camera frame with
    attenuation 0.01 and ambient coefficient 0.5, then one shininess
    U(40, 120) per instance of the image in rank order (scene_offset (B+1):
    the instances' CSR; None: no instances).  Image i draws from
    numpy.random.default_rng([seed*1000 + image_offset + i, 0, tag]): a stream
    of its own, so sample_scenes' draws are untouched and the values depend on
    the global image index alone.  Returns numpy lights (B,8) and shininess
    (K) float32."""
    off = np.zeros(B + 1, np.int64) if scene_offset is None else np.asarray(scene_offset, np.int64)
    if off.shape != (B + 1,):
        raise ValueError("sample_lights: scene_offset (B+1)")
    lights = np.zeros((B, 8), np.float32)
    shin = np.zeros(int(off[-1]), np.float32)
    for i in range(B):
        rng = np.random.default_rng([seed * 1000 + image_offset + i, 0, _TAG_LIGHT])
        intensity = rng.uniform(0.5, 2.0)
        lights[i] = [rng.uniform(-2.0, 2.0), rng.uniform(-2.0, 2.0), 0.0, 1.0, intensity, 0.01, 0.5, 0.0]
        shin[off[i]:off[i + 1]] = rng.uniform(40.0, 120.0, size=int(off[i + 1] - off[i]))
    return lights, shin


def sample_jitter(B, seed, image_offset=0, noise=False):
    """The reference's per-image draws of chromatic_transform (blob.py:79-84)
    and add_noise (:111-112): d_h = (U - 0.5) 0.02 180, d_l and d_s =
    (U - 0.5) 0.2 256, sigma = sqrt(U 0.3 256) (0 unless noise), keyed like
    sample_lights.  Returns numpy (B,4) float32 [d_h, d_l, d_s, sigma]."""
    jit = np.zeros((B, 4), np.float32)
    for i in range(B):
        u = np.random.default_rng([seed * 1000 + image_offset + i, 0, _TAG_JITTER]).uniform(size=4)
        jit[i] = [(u[0] - 0.5) * 0.02 * 180, (u[1] - 0.5) * 0.2 * 256, (u[2] - 0.5) * 0.2 * 256,
                  np.sqrt(u[3] * 0.3 * 256) if noise else 0.0]
    return jit


def image_blob(color, backgrounds, bg_index, jitter, pixel_means=PIXEL_MEANS, seed=0, image_offset=0, chromatic=True,
               noise=False, layout="NHWC", out=None, stream=None):
    """color (B,H,W,4) float32 BGRA (LitSceneRenderer's) -> the network's
    input, float32 (B,H,W,3) or, layout="NCHW", (B,3,H,W), in one pass
    (include/posecnn_image.h, pcnn_image_blob): quantise to 8 bits, paste
    backgrounds[bg_index[b]] ((N_bg,H,W,3) uint8 BGR; None or an index outside
    the set: black) where alpha is 0, the chromatic transform by jitter[b] =
    [d_h, d_l, d_s, sigma], Gaussian noise of that sigma, minus pixel_means
    (BGR; 3 numbers or a device tensor).  The noise of image b depends on
    (seed, image_offset + b, pixel) alone.  Device tensors in, `out` or a
    fresh tensor back; no sync, nothing allocated when out and a pixel_means
    tensor are given."""
    who = "image_blob"
    if not isinstance(color, torch.Tensor):
        raise TypeError(f"{who}: color: expected a torch.Tensor, got {type(color).__name__}")
    if color.dim() != 4 or color.shape[-1] != 4:
        raise ValueError(f"{who}: color must have shape (B,H,W,4) (got {tuple(color.shape)})")
    if layout not in ("NHWC", "NCHW"):
        raise ValueError(f"{who}: layout must be 'NHWC' or 'NCHW'")
    B, H, W = (int(d) for d in color.shape[:3])
    dev, f32 = color.device, torch.float32
    _want(who, "color", color, (B, H, W, 4), f32, dev)
    n_bg = 0
    if backgrounds is not None:
        n_bg = int(backgrounds.shape[0]) if isinstance(backgrounds, torch.Tensor) and backgrounds.dim() else 0
        _want(who, "backgrounds", backgrounds, (n_bg, H, W, 3), torch.uint8, dev)
    _want(who, "bg_index", bg_index, (B,), torch.int32, dev)
    _want(who, "jitter", jitter, (B, 4), f32, dev)
    if not isinstance(pixel_means, torch.Tensor):
        pixel_means = torch.tensor([float(m) for m in pixel_means], dtype=f32).to(dev, non_blocking=True)
    _want(who, "pixel_means", pixel_means, (3,), f32, dev)
    shape = (B, H, W, 3) if layout == "NHWC" else (B, 3, H, W)
    if out is None:
        out = torch.empty(shape, dtype=f32, device=dev)
    _want(who, "out", out, shape, f32, dev)
    flags = (CHROMATIC if chromatic else 0) | (NOISE if noise else 0) | (NCHW if layout == "NCHW" else 0)
    rc = _load().pcnn_image_blob(_lib.ptr(color), _lib.ptr(backgrounds if n_bg else None), n_bg, _lib.ptr(bg_index),
                                 _lib.ptr(jitter), _lib.ptr(pixel_means), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                 int(image_offset), B, H, W, flags, _lib.ptr(out), _lib.stream_ptr(stream))
    _lib.check(rc, "image_blob")
    return out


def make_image_frames(renderer, B, seed=0, image_offset=0, backgrounds=None, chromatic=True, noise=False,
                      layout="NHWC", pixel_means=PIXEL_MEANS, **scene_kw):
    """make_scene_frames' B frames (its keyword arguments pass through) from a
    LitSceneRenderer, plus color (B,H,W,4), the lit BGRA picture under
    sample_lights' light and shininess, and image, the network's input:
    image_blob of it under sample_jitter's draws over backgrounds[(image_offset
    + b) mod N_bg] ((N_bg,H,W,3) uint8 BGR on the device; None: black).  Every
    draw is keyed by the global image index, so a shard reproduces the frames
    of a single-device run.  The colour is rendered in make_scene_frames' own
    rejection loop: no host round trip beyond its `visible` read."""
    def render(images, off, scene_offset, mesh_index, class_id, poses):
        rows = [sample_lights(1, seed, int(g), [0, int(off[j + 1] - off[j])]) for j, g in enumerate(images)]
        lights = torch.from_numpy(np.concatenate([l for l, _ in rows])).to(renderer.device)
        shin = torch.from_numpy(np.concatenate([s for _, s in rows])).to(renderer.device)
        return renderer.render(scene_offset, mesh_index, class_id, poses, shin, lights, return_inst_id=False)

    frames = make_scene_frames(renderer, B, seed=seed, image_offset=image_offset, render=render, extra=("color",),
                               **scene_kw)
    dev = renderer.device
    n_bg = 0 if backgrounds is None else int(backgrounds.shape[0])
    idx = (np.arange(B) + image_offset) % n_bg if n_bg else np.full(B, -1)
    frames["image"] = image_blob(frames["color"], backgrounds, torch.from_numpy(idx.astype(np.int32)).to(dev),
                                 torch.from_numpy(sample_jitter(B, seed, image_offset, noise)).to(dev), pixel_means,
                                 seed, image_offset, chromatic, noise, layout)
    return frames
