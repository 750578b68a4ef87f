"""numpy helpers shared by the tests of the ADD-S filtered search: the query
and candidate clouds of a row by the reference's fp32 expressions, the fp32
first-minimum picks, and the filter's emulated verdict on them."""
import numpy as np

# kFiltWin, kFiltM2Min and kFiltM2Max of csrc/average_distance.hip: the tests'
# one copy of the kernel's window and range (test_filter_emulation_error_is_inside_the_bound
# ties the window to the derivation's error terms)
FILT_WIN = 2.8e-4
FILT_M2_MIN, FILT_M2_MAX = 2.0 ** -40, 2.0 ** 40


def filter_emulation(q, c):
    """numpy emulation of the filter of the ADD-S search (csrc/average_distance.hip)
    for query points q (N, 3) and candidates c (P, 3), float32: the filter
    values s~ (N, P) from the bf16 planes with fp32 sums, the item's window
    and whether the item is inside the range the window is proved for."""
    def bf16(x):
        b = np.ascontiguousarray(x, np.float32).view(np.uint32)
        return ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).view(np.float32)

    def split2(x):
        h = bf16(x)
        return h, bf16(x - h)

    q = np.asarray(q, np.float32)
    c = np.asarray(c, np.float32)
    n = c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2]
    qn = q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2]
    m2 = np.float32(max(n.max(), qn.max()))
    in_range = bool(np.isfinite(n).all() and np.isfinite(qn).all() and FILT_M2_MIN <= m2 <= FILT_M2_MAX)
    with np.errstate(all="ignore"):
        nh = bf16(n)
        nm = bf16(n - nh)
        nl = bf16(n - nh - nm)
        s = np.zeros((q.shape[0], c.shape[0]), np.float32)
        for a in range(3):
            ch, cm = split2(c[:, a])
            bh, bm = split2(np.float32(-2) * q[:, a])
            for x, y in ((ch, bh), (ch, bm), (cm, bh), (cm, bm)):
                s += y[:, None] * x[None, :]
        for pl in (nh, nm, nl):
            s += pl[None, :]
    return s, np.float32(FILT_WIN) * m2, in_range


def rot(q):
    s, u, v, w = (np.float32(x) for x in q)
    two = np.float32(2)
    return np.array([[s * s + u * u - v * v - w * w, two * (u * v - s * w), two * (u * w + s * v)],
                     [two * (u * v + s * w), s * s - u * u + v * v - w * w, two * (v * w - s * u)],
                     [two * (u * w - s * v), two * (v * w + s * u), s * s - u * u - v * v + w * w]], np.float32)


def clouds(qp, qt, X):
    """Query points (prediction-rotated) and candidates (GT-rotated) of model X, fp32."""
    X = np.asarray(X, np.float32)
    Rp, Rg = rot(qp), rot(qt)
    q = np.stack([Rp[i, 0] * X[:, 0] + Rp[i, 1] * X[:, 1] + Rp[i, 2] * X[:, 2] for i in range(3)], 1)
    c = np.stack([Rg[i, 0] * X[:, 0] + Rg[i, 1] * X[:, 1] + Rg[i, 2] * X[:, 2] for i in range(3)], 1)
    return q, c


def picks(q, c):
    """fp32 first minimum of the reference expression (numpy does not contract)."""
    e = [q[:, None, i] - c[None, :, i] for i in range(3)]
    d = e[0] * e[0] + e[1] * e[1] + e[2] * e[2]
    return np.argmin(d, 1)


def filter_verdict(q, c):
    """(in range, every fp32 pick inside the window, mean and largest number of
    candidates inside the window per query) of the emulated filter."""
    s, win, ok = filter_emulation(q, c)
    j = picks(q, c)
    inside = s <= s.min(1, keepdims=True) + win
    hits = inside.sum(1)
    return ok, bool(inside[np.arange(len(j)), j].all()), float(hits.mean()), int(hits.max())


def rows_in_range(pred, target, weight, pts, sym):
    """Whether every symmetric row's clouds are inside the filter's proved range."""
    for r in range(pred.shape[0]):
        cls = np.flatnonzero(weight[r, 0::4] > 0)
        if len(cls) == 0 or not sym[cls[0]] > 0:
            continue
        c0 = 4 * cls[0]
        q, c = clouds(pred[r, c0:c0 + 4], target[r, c0:c0 + 4], pts[cls[0]])
        n = np.concatenate([(q * q).sum(1), (c * c).sum(1)])
        if not (np.isfinite(n).all() and FILT_M2_MIN <= n.max() <= FILT_M2_MAX):
            return False
    return True
