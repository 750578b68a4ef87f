"""Test-only helper for the mesh rasteriser (csrc/render.hip): small closed
meshes and raster_ref, a numpy restatement of the geometry rules written at
the top of render.hip.  With dtype=float32 it performs the kernel's float
operations in the kernel's order, each rounded to float32; with dtype=float64
it is the accuracy reference.  The vertex pass is float64 in both, as the
kernel's is, so both snap the same coordinates: the two differ only in the
values and in which of two nearly equal depths wins."""
import functools

import numpy as np

from posecnn_amd.synthesize.render import Mesh
from refine_scene import CAMERA

CAMERA4 = tuple(c / 4 for c in CAMERA)


def box_mesh(half):
    """12 faces, 4 vertices per side with the side's flat normal (24 in all), outward winding."""
    h = np.asarray(half, np.float64)
    V, N, F = [], [], []
    for ax in range(3):
        for s in (-1.0, 1.0):
            a, b = (ax + 1) % 3, (ax + 2) % 3
            n = np.zeros(3)
            n[ax] = s
            quad = []
            for ca, cb in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
                p = np.zeros(3)
                p[ax], p[a], p[b] = s * h[ax], ca * h[a], cb * h[b]
                quad.append(p)
            if s < 0:
                quad = quad[::-1]
            o = len(V)
            V += quad
            N += [n] * 4
            F += [[o, o + 1, o + 2], [o, o + 2, o + 3]]
    return Mesh(np.array(V), np.array(F), np.array(N))


def icosphere(level, r=1.0):
    """Icosahedron subdivided `level` times (20 * 4^level faces) on the sphere of radius r."""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return Mesh(np.array(v) * r, np.array(f))


def torus(R, r, nu, nv):
    """nu x nv quads split in two (2 * nu * nv faces), axis z."""
    a = np.arange(nu) * 2 * np.pi / nu
    b = np.arange(nv) * 2 * np.pi / nv
    A, B = np.meshgrid(a, b, indexing="ij")
    v = np.stack([(R + r * np.cos(B)) * np.cos(A), (R + r * np.cos(B)) * np.sin(A), r * np.sin(B)], -1).reshape(-1, 3)
    f = []
    for i in range(nu):
        for j in range(nv):
            p00, p10 = i * nv + j, ((i + 1) % nu) * nv + j
            p01, p11 = i * nv + (j + 1) % nv, ((i + 1) % nu) * nv + (j + 1) % nv
            f += [[p00, p10, p11], [p00, p11, p01]]
    return Mesh(v, np.array(f))


def vertex_pass(mesh, pose, camera):
    """The vertex pass (float64 from the float32 inputs, the kernel's order):
    camera position, rotated normal and projection of every vertex."""
    T = np.float64
    fx, fy, px, py = (T(np.float32(c)) for c in camera)
    q = np.asarray(pose, np.float32).astype(T)
    qw, qx, qy, qz = q[0], q[1], q[2], q[3]
    qn = np.sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz)
    qw, qx, qy, qz = qw / qn, qx / qn, qy / qn, qz / qn
    one, two = T(1), T(2)
    R = [[one - two * (qy * qy + qz * qz), two * (qx * qy - qz * qw), two * (qx * qz + qy * qw)],
         [two * (qx * qy + qz * qw), one - two * (qx * qx + qz * qz), two * (qy * qz - qx * qw)],
         [two * (qx * qz - qy * qw), two * (qy * qz + qx * qw), one - two * (qx * qx + qy * qy)]]
    p = mesh.vertices.astype(T)
    n = mesh.normals.astype(T)
    cam = [((R[i][0] * p[:, 0] + R[i][1] * p[:, 1]) + R[i][2] * p[:, 2]) + q[4 + i] for i in range(3)]
    nr = [(R[i][0] * n[:, 0] + R[i][1] * n[:, 1]) + R[i][2] * n[:, 2] for i in range(3)]
    ln = np.sqrt((nr[0] * nr[0] + nr[1] * nr[1]) + nr[2] * nr[2])
    d = np.where(ln > 0, ln, one)
    nr = [c / d for c in nr]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = fx * cam[0] / cam[2] + px
        v = fy * cam[1] / cam[2] + py
    return np.stack(cam, -1), np.stack(nr, -1), u, v


def raster_ref(mesh, pose, cls, H, W, camera, znear=0.25, zfar=6.0, dtype=np.float32):
    """The rules of render.hip for one mesh and one pose (7,) float32.  The
    vertex pass is float64 as the kernel's; `dtype` is the type its results
    are stored in (camera position, normal, the residual of the snap) and of
    the per-pixel arithmetic.  Returns pred_v / pred_n (H,W,4), vertmap
    (H,W,3), depth (H,W) in `dtype`, tri_id (H,W) int32, gap (H,W) float64:
    the depth between the two nearest fragments of the pixel (inf with fewer
    than two), and frags (H,W) int32: the number of triangles covering the
    pixel, whatever their depth."""
    T = dtype
    cam, nrm, u, v = vertex_pass(mesh, pose, camera)
    with np.errstate(invalid="ignore"):
        ok = (cam[:, 2] >= np.float64(np.float32(znear))) & (np.abs(u) <= 2.0 ** 20) & (np.abs(v) <= 2.0 ** 20)
    su = np.where(ok, np.rint(np.where(ok, u, 0) * 256.0), 0)
    sv = np.where(ok, np.rint(np.where(ok, v, 0) * 256.0), 0)
    ru = np.where(ok, u - su / 256.0, 0).astype(T)
    rv = np.where(ok, v - sv / 256.0, 0).astype(T)
    su, sv = su.astype(np.int64), sv.astype(np.int64)
    cam, nrm = cam.astype(T), nrm.astype(T)
    model = mesh.vertices.astype(T)
    zf = T(np.float32(zfar))
    z1 = np.full((H, W), np.inf, T)
    z2 = np.full((H, W), np.inf, T)
    tri = np.full((H, W), -1, np.int32)
    pv = np.zeros((H, W, 4), T)
    pn = np.zeros((H, W, 4), T)
    vm = np.full((H, W, 3), np.nan, T)
    frags = np.zeros((H, W), np.int32)

    def covers(a, b, X, Y):
        dx, dy = int(su[b] - su[a]), int(sv[b] - sv[a])
        e = dx * (Y - int(sv[a])) - dy * (X - int(su[a]))
        return (e > 0) | ((e == 0) & bool(dy < 0 or (dy == 0 and dx > 0)))

    k = T(1) / T(256)

    def edge(a, b, X, Y):  # X, Y: the pixel centres' snapped coordinates (int64)
        dx = T(su[b] - su[a]) * k + (ru[b] - ru[a])
        dy = T(sv[b] - sv[a]) * k + (rv[b] - rv[a])
        qx = (X - su[a]).astype(T) * k - ru[a]
        qy = (Y - sv[a]).astype(T) * k - rv[a]
        return dx * qy - dy * qx

    for f, (a, b, c) in enumerate(mesh.faces.tolist()):
        if not (ok[a] and ok[b] and ok[c]):
            continue
        area = int(su[b] - su[a]) * int(sv[c] - sv[a]) - int(sv[b] - sv[a]) * int(su[c] - su[a])
        if area == 0:
            continue
        if area < 0:
            b, c = c, b
        x0 = max(-(-int(min(su[a], su[b], su[c])) // 256), 0)
        x1 = min(int(max(su[a], su[b], su[c])) // 256, W - 1)
        y0 = max(-(-int(min(sv[a], sv[b], sv[c])) // 256), 0)
        y1 = min(int(max(sv[a], sv[b], sv[c])) // 256, H - 1)
        if x0 > x1 or y0 > y1:
            continue
        ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1]
        X, Y = xs.astype(np.int64) * 256, ys.astype(np.int64) * 256
        cov = covers(a, b, X, Y) & covers(b, c, X, Y) & covers(c, a, X, Y)
        if not cov.any():
            continue
        ys, xs = ys[cov], xs[cov]
        frags[ys, xs] += 1
        Xf, Yf = X[cov], Y[cov]
        with np.errstate(divide="ignore", invalid="ignore"):
            ba = edge(b, c, Xf, Yf) / cam[a, 2]
            bb = edge(c, a, Xf, Yf) / cam[b, 2]
            bc = edge(a, b, Xf, Yf) / cam[c, 2]
            s = (ba + bb) + bc
            la, lb, lc = ba / s, bb / s, bc / s
            Z = (la * cam[a, 2] + lb * cam[b, 2]) + lc * cam[c, 2]
            keep = (Z > 0) & (Z <= zf)
        assert Z.dtype == T
        ys, xs, la, lb, lc, Z = ys[keep], xs[keep], la[keep], lb[keep], lc[keep], Z[keep]
        win = Z < z1[ys, xs]  # faces come in ascending order: an equal Z stays with the lower index
        lose = ~win
        z2[ys[lose], xs[lose]] = np.minimum(z2[ys[lose], xs[lose]], Z[lose])
        ys, xs, la, lb, lc, Z = ys[win], xs[win], la[win], lb[win], lc[win], Z[win]
        z2[ys, xs] = z1[ys, xs]
        z1[ys, xs] = Z
        tri[ys, xs] = f
        for j in range(2):
            pv[ys, xs, j] = (la * cam[a, j] + lb * cam[b, j]) + lc * cam[c, j]
        pv[ys, xs, 2] = Z
        pv[ys, xs, 3] = 1
        for j in range(3):
            pn[ys, xs, j] = (la * nrm[a, j] + lb * nrm[b, j]) + lc * nrm[c, j]
            vm[ys, xs, j] = (la * model[a, j] + lb * model[b, j]) + lc * model[c, j]
        vm[ys, xs, 0] = vm[ys, xs, 0] + T(cls)
    depth = np.where(tri >= 0, z1, 0).astype(T)
    with np.errstate(invalid="ignore"):
        gap = np.where(tri >= 0, z2.astype(np.float64) - z1.astype(np.float64), np.inf)
    return dict(pred_v=pv, pred_n=pn, vertmap=vm, depth=depth, tri_id=tri, gap=gap, frags=frags)


def fragment_counts(mesh, pose, H, W, camera):
    return raster_ref(mesh, pose, 0, H, W, camera, 1e-3, 1e3)["frags"]


def random_pose(rng, zlo=0.6, zhi=1.0):
    """A float32 pose (7,) with a uniform random rotation in front of the quarter-size camera."""
    q = rng.normal(size=4)
    t = [rng.uniform(-0.08, 0.08), rng.uniform(-0.05, 0.05), rng.uniform(zlo, zhi)]
    return np.concatenate([q / np.linalg.norm(q), t]).astype(np.float32)


def silhouette_clearance(mesh, pose, H, W, camera):
    """Smallest distance (px) from a pixel centre to the outline of a CONVEX
    mesh's projection (the hull of its float64 projected vertices)."""
    _, _, u, v = vertex_pass(mesh, pose, camera)
    pts = sorted(set(zip(u.tolist(), v.tolist())))
    cross = lambda o, a, b: (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])  # noqa: E731
    hull = []
    for seq in (pts, pts[::-1]):  # monotone chain: lower, then upper
        part = []
        for p in seq:
            while len(part) >= 2 and cross(part[-2], part[-1], p) <= 0:
                part.pop()
            part.append(p)
        hull += part[:-1]
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    best = np.inf
    for a, b in zip(hull, hull[1:] + hull[:1]):
        d = np.array([b[0] - a[0], b[1] - a[1]])
        t = np.clip(((xs - a[0]) * d[0] + (ys - a[1]) * d[1]) / (d @ d), 0, 1)
        best = min(best, np.hypot(xs - (a[0] + t * d[0]), ys - (a[1] + t * d[1])).min())
    return best


@functools.lru_cache(maxsize=None)
def fixtures():
    """name -> (mesh, class id, H, W, two poses): the shared fixtures of the
    CPU and GPU rasteriser tests (camera = refine_scene.CAMERA / 4).

    The box is compared for EXACT coverage with the analytic ray-caster of
    refine_scene.py.  Snapping a vertex to 1/256 px moves an edge by up to
    sqrt(2)/512 px, so that comparison is well posed only where no pixel
    centre lies that close to the true outline (about one pose in four at
    this size, by outline length x band width): box poses with a pixel centre
    within 1/256 px of the float64 outline are drawn again.  The criterion
    looks at the geometry alone, never at a rasteriser's output."""
    rng = np.random.default_rng(20240611)
    out = {}
    for name, mesh, cls, H, W in (("icosphere", icosphere(3, 0.05), 2, 120, 160),
                                  ("torus", torus(0.05, 0.02, 48, 24), 5, 120, 160),
                                  ("box", box_mesh((0.06, 0.045, 0.035)), 3, 97, 131)):
        poses = []
        while len(poses) < 2:
            p = random_pose(rng)
            if name != "box" or silhouette_clearance(mesh, p, H, W, CAMERA4) > 1 / 256:
                poses.append(p)
        out[name] = (mesh, cls, H, W, poses)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, i, dtype):
    """raster_ref of fixture `name` at its pose i, computed once per process; treat as read-only."""
    mesh, cls, H, W, poses = fixtures()[name]
    return raster_ref(mesh, poses[i], cls, H, W, CAMERA4, dtype=dtype)
