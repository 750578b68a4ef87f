"""Test-only helper for the network's input side (csrc/render_lit.hip,
include/posecnn_image.h): numpy restatements of the lit resolve and of the
picture -> blob pass.  They are the specification of pcnn_image_blob's steps 1-3
and 5 (float32, the kernel's operation order, bit for bit) and the accuracy
reference of the shading.

weights_ref     the winner's perspective-correct weights, recomputed from a
                raster's tri_id with render_ref.raster_ref's own expressions
shade_ref       the colour attachment of a scene from scene_ref's maps; with
                dtype=float32 the kernel's operations in the kernel's order,
                with float64 the accuracy reference
bgr_to_hls8, hls8_to_bgr, chromatic_ref   the 8-bit HLS round trip and jitter
deviate_ref     the Gaussian deviate of (seed, global image, pixel)
image_blob_ref  the whole pass"""
import numpy as np

from oracle import philox
from render_ref import vertex_pass

F = np.float32
TAG_IMAGE = 0x494D4731
PIXEL_MEANS = (102.9801, 115.9465, 122.7717)


def colored(mesh, phase=0.0):
    """`mesh` with smooth vertex colours in [0, 1], a function of the position."""
    from posecnn_amd.synthesize.render import Mesh
    v = mesh.vertices.astype(np.float64)
    s = 40.0
    col = 0.5 + 0.45 * np.stack([np.sin(s * v[:, 0] + phase), np.cos(s * v[:, 1] - phase), np.sin(s * v[:, 2] + 1.0)], 1)
    return Mesh(mesh.vertices, mesh.faces, mesh.normals, col.astype(np.float32))


def weights_ref(mesh, pose, tri_id, camera, znear=0.25, dtype=np.float32):
    """(la, lb, lc) (H,W) in `dtype` and the winning face's vertices (a, b, c)
    (H,W) int64 in the positive orientation, at the pixels with tri_id >= 0
    (0 elsewhere): render_ref.raster_ref's expressions, vectorised over the
    pixels."""
    T = dtype
    H, W = tri_id.shape
    cam, _, u, v = vertex_pass(mesh, pose, camera)
    with np.errstate(invalid="ignore"):
        ok = (cam[:, 2] >= np.float64(np.float32(znear))) & (np.abs(u) <= 2.0 ** 20) & (np.abs(v) <= 2.0 ** 20)
    su = np.where(ok, np.rint(np.where(ok, u, 0) * 256.0), 0)
    sv = np.where(ok, np.rint(np.where(ok, v, 0) * 256.0), 0)
    ru = np.where(ok, u - su / 256.0, 0).astype(T)
    rv = np.where(ok, v - sv / 256.0, 0).astype(T)
    su, sv = su.astype(np.int64), sv.astype(np.int64)
    z = cam[:, 2].astype(T)
    hit = tri_id >= 0
    f = mesh.faces.astype(np.int64)[np.maximum(tri_id, 0)]
    a, b, c = f[..., 0], f[..., 1], f[..., 2]
    area = (su[b] - su[a]) * (sv[c] - sv[a]) - (sv[b] - sv[a]) * (su[c] - su[a])
    b, c = np.where(area < 0, c, b), np.where(area < 0, b, c)
    ys, xs = np.mgrid[0:H, 0:W]
    X, Y = xs.astype(np.int64) * 256, ys.astype(np.int64) * 256
    k = T(1) / T(256)

    def edge(p, q):
        dx = (su[q] - su[p]).astype(T) * k + (ru[q] - ru[p])
        dy = (sv[q] - sv[p]).astype(T) * k + (rv[q] - rv[p])
        qx = (X - su[p]).astype(T) * k - ru[p]
        qy = (Y - sv[p]).astype(T) * k - rv[p]
        return dx * qy - dy * qx

    with np.errstate(divide="ignore", invalid="ignore"):
        ba, bb, bc = edge(b, c) / z[a], edge(c, a) / z[b], edge(a, b) / z[c]
        s = (ba + bb) + bc
        la, lb, lc = ba / s, bb / s, bc / s
    assert la.dtype == T
    zero = T(0)
    return (np.where(hit, la, zero), np.where(hit, lb, zero), np.where(hit, lc, zero)), (a, b, c)


def _dot(p, q):
    return (p[..., 0] * q[..., 0] + p[..., 1] * q[..., 1]) + p[..., 2] * q[..., 2]


def _unit(p):
    """p / |p|, a zero length left as is."""
    n = np.sqrt(_dot(p, p))
    return p / np.where(n > 0, n, n.dtype.type(1))[..., None]


def apply_light(P, N, c, light, shininess, dtype=np.float32):
    """The shader's ApplyLight with specular colour 1 on arrays (...,3) of the
    camera-frame position, the unit normal and the RGB surface colour; light
    (8,) [x y z w, intensity, attenuation, ambient, 0], shininess (...).
    Returns RGB (...,3) in `dtype`."""
    T = dtype
    P, N, c = P.astype(T), N.astype(T), c.astype(T)
    lt = np.asarray(light, np.float32).astype(T)
    sh = np.asarray(shininess, np.float32).astype(T)
    I, att_k, ka = lt[4], lt[5], lt[6]
    if lt[3] != 0:
        D = lt[:3] - P
        att = T(1) / (T(1) + att_k * _dot(D, D))
    else:
        D = np.broadcast_to(lt[:3], P.shape).copy()
        att = np.ones(P.shape[:-1], T)
    L = _unit(D)
    V = _unit(-P)
    nl = _dot(N, L)
    diffuse = np.maximum(T(0), nl)
    R = (T(2) * nl)[..., None] * N - L
    with np.errstate(invalid="ignore"):
        spec = np.where(diffuse > 0, np.power(np.maximum(T(0), _dot(V, R)), sh), T(0)).astype(T)
    sI = spec * I
    out = (ka * c) * I + att[..., None] * ((diffuse[..., None] * c) * I + sI[..., None])
    assert out.dtype == T
    return out


def shade_ref(instances, maps, colors, light, shininess, camera, dtype=np.float32, znear=0.25):
    """The colour attachment (H,W,4) BGRA in `dtype` of one scene: instances
    [(mesh, class, pose)] in rank order, maps = scene_ref's dict of the scene
    in the same dtype (inst_id and face are read), colors [(V,3)] per
    instance, light (8,), shininess (n,).  Also returns P (H,W,3)."""
    T = dtype
    inst, face = maps["inst_id"], maps["face"]
    H, W = inst.shape
    out = np.zeros((H, W, 4), T)
    Pall = np.zeros((H, W, 3), T)
    for i, (mesh, _, pose) in enumerate(instances):
        own = inst == i
        if not own.any():
            continue
        tri = np.where(own, face, -1)
        (la, lb, lc), (a, b, c) = weights_ref(mesh, np.asarray(pose, np.float32), tri, camera, znear, T)
        cam, nrm, _, _ = vertex_pass(mesh, np.asarray(pose, np.float32), camera)
        cam, nrm, col = cam.astype(T), nrm.astype(T), np.asarray(colors[i], np.float32).astype(T)
        mix = lambda v: (la[..., None] * v[a] + lb[..., None] * v[b]) + lc[..., None] * v[c]  # noqa: E731
        P, N, cc = mix(cam), _unit(mix(nrm)), mix(col)
        rgb = apply_light(P[own], N[own], cc[own], light, np.full(int(own.sum()), shininess[i], np.float32), T)
        out[own, 0], out[own, 1], out[own, 2], out[own, 3] = rgb[:, 2], rgb[:, 1], rgb[:, 0], T(1)
        Pall[own] = P[own]
    return out, Pall


# ---- the image pipeline ----
def quantise(c):
    """Step 1: (uint8)min(max(255 c, 0), 255), truncated; NaN -> 0.  int32 out."""
    q = np.fmin(np.fmax(F(255) * np.asarray(c, F), F(0)), F(255))
    return q.astype(np.int32)


def bgr_to_hls(bgr):
    """(...,3) integer BGR levels -> float32 (h in degrees [0, 360), l, s in
    [0, 1]): the hexcone formula in float32 on level / 255, the float
    conversion that bgr_to_hls8 stores in 8 bits."""
    p = np.asarray(bgr).astype(F) / F(255)
    b, g, r = p[..., 0], p[..., 1], p[..., 2]
    vmax = np.maximum(np.maximum(r, g), b)
    vmin = np.minimum(np.minimum(r, g), b)
    d = vmax - vmin
    l = (vmax + vmin) * F(0.5)
    ds = np.where(d > 0, d, F(1))
    den = np.where(l < F(0.5), vmax + vmin, (F(2) - vmax) - vmin)  # > 0 wherever d > 0
    s = d / np.where(d > 0, den, F(1))
    h = np.where(vmax == r, (F(60) * (g - b)) / ds,
                 np.where(vmax == g, (F(60) * (b - r)) / ds + F(120), (F(60) * (r - g)) / ds + F(240)))
    h = np.where(h < 0, h + F(360), h)
    h, s = np.where(d > 0, h, F(0)), np.where(d > 0, s, F(0))
    assert h.dtype == F and s.dtype == F and l.dtype == F
    return h, l, s


def hls_to_bgr(h, l, s):
    """The float inverse: h in degrees [0, 360), l, s in [0, 1] -> (...,3) BGR
    levels (int32), ending in rint(255 x) saturated.  (hls8_to_bgr is its
    8-bit form, whose sector and fraction come from the integer H.)"""
    h, l, s = (np.asarray(x, F) for x in (h, l, s))
    p2 = np.where(l <= F(0.5), l * (F(1) + s), (l + s) - l * s)
    p1 = F(2) * l - p2
    hs = h / F(60)
    sector = np.clip(np.floor(hs), 0, 5).astype(np.int32)
    f = hs - sector.astype(F)
    up, down = p1 + (p2 - p1) * f, p1 + (p2 - p1) * (F(1) - f)
    r = np.choose(sector, [p2, down, p1, p1, up, p2])
    g = np.choose(sector, [up, p2, p2, down, p1, p1])
    b = np.choose(sector, [p1, p1, up, p2, p2, down])
    grey = s == 0
    return _sat8(np.stack([np.where(grey, l, b), np.where(grey, l, g), np.where(grey, l, r)], -1))


def bgr_to_hls8(bgr):
    """(...,3) integer BGR levels -> H in [0, 180), L, S in [0, 255] (int32):
    bgr_to_hls stored as H = rint(h / 2) with 180 -> 0, L = rint(255 l),
    S = rint(255 s)."""
    h, l, s = bgr_to_hls(bgr)
    H8 = np.rint(h * F(0.5)).astype(np.int32)
    H8 = np.where(H8 >= 180, H8 - 180, H8)
    return H8, np.rint(F(255) * l).astype(np.int32), np.rint(F(255) * s).astype(np.int32)


def _sat8(x):
    return np.fmin(np.fmax(np.rint(F(255) * x), F(0)), F(255)).astype(np.int32)


def hls8_to_bgr(H8, L8, S8):
    """The inverse: 8-bit H in [0, 180), L, S -> (...,3) BGR levels (int32)."""
    H8, L8, S8 = (np.asarray(x, np.int32) for x in (H8, L8, S8))
    l, s = L8.astype(F) / F(255), S8.astype(F) / F(255)
    p2 = np.where(l <= F(0.5), l * (F(1) + s), (l + s) - l * s)
    p1 = F(2) * l - p2
    sector = H8 // 30
    f = (H8 - 30 * sector).astype(F) / F(30)
    up, down = p1 + (p2 - p1) * f, p1 + (p2 - p1) * (F(1) - f)
    r = np.choose(sector, [p2, down, p1, p1, up, p2])
    g = np.choose(sector, [up, p2, p2, down, p1, p1])
    b = np.choose(sector, [p1, p1, up, p2, p2, down])
    grey = S8 == 0
    out = np.stack([np.where(grey, l, b), np.where(grey, l, g), np.where(grey, l, r)], -1)
    assert out.dtype == F
    return _sat8(out)


def jitter_hls8(H8, L8, S8, d_h, d_l, d_s):
    """The jitter in float32: hue modulo 180, the others clipped to [0, 255], all truncated."""
    d_h, d_l, d_s = F(d_h), F(d_l), F(d_s)
    th = H8.astype(F) + d_h
    th = th - F(180) * np.floor(th / F(180))
    Hn = np.fmin(np.fmax(th, F(0)), F(180)).astype(np.int32)
    Hn = np.where(Hn >= 180, Hn - 180, Hn)
    Ln = np.fmin(np.fmax(L8.astype(F) + d_l, F(0)), F(255)).astype(np.int32)
    Sn = np.fmin(np.fmax(S8.astype(F) + d_s, F(0)), F(255)).astype(np.int32)
    return Hn, Ln, Sn


def chromatic_ref(bgr, d_h, d_l, d_s):
    """Step 3 on (...,3) BGR levels."""
    return hls8_to_bgr(*jitter_hls8(*bgr_to_hls8(bgr), d_h, d_l, d_s))


def deviate_ref(seed, image, n_pix):
    """Step 4's normal deviates of pixels 0..n_pix-1 of global image `image` (float32)."""
    pix = np.arange(n_pix, dtype=np.uint64)
    gi = int(image) & 0xFFFFFFFFFFFFFFFF
    ctr = np.stack([pix, np.zeros_like(pix), np.full_like(pix, gi & 0xFFFFFFFF), np.full_like(pix, gi >> 32)], 1)
    key = np.array([[(seed & 0xFFFFFFFF) ^ TAG_IMAGE, (seed >> 32) & 0xFFFFFFFF]], np.uint64)
    o = philox.philox4x32_10(ctr, key)
    u1 = (o[:, 0].astype(np.float64) + 1.0) * (1.0 / 4294967296.0)
    u2 = o[:, 1].astype(np.float64) * (1.0 / 4294967296.0)
    return (np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)).astype(F)


def image_blob_ref(color, backgrounds, bg_index, jitter, pixel_means=PIXEL_MEANS, seed=0, image_offset=0,
                   chromatic=True, noise=False, layout="NHWC"):
    """pcnn_image_blob: color (B,H,W,4) float32 BGRA, backgrounds (N,H,W,3)
    uint8 or None, bg_index (B), jitter (B,4) -> (B,H,W,3) or (B,3,H,W) float32."""
    color = np.asarray(color, F)
    B, H, W, _ = color.shape
    means = np.asarray(pixel_means, F)
    out = np.zeros((B, H, W, 3), F)
    n_bg = 0 if backgrounds is None else len(backgrounds)
    for b in range(B):
        p = quantise(color[b, ..., :3])
        bg = np.zeros((H, W, 3), np.int32)
        if 0 <= int(bg_index[b]) < n_bg:
            bg = backgrounds[int(bg_index[b])].astype(np.int32)
        p = np.where((color[b, ..., 3] == 0)[..., None], bg, p)
        d_h, d_l, d_s, sigma = (F(x) for x in jitter[b])
        if chromatic:
            p = chromatic_ref(p, d_h, d_l, d_s)
        v = p.astype(F)
        if noise:
            e = sigma * deviate_ref(seed, image_offset + b, H * W).reshape(H, W)
            v = np.fmin(np.fmax(v + e[..., None], F(0)), F(255))
        out[b] = v - means
    assert out.dtype == F
    return out if layout == "NHWC" else np.ascontiguousarray(out.transpose(0, 3, 1, 2))
