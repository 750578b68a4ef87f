"""numpy restatement of the upscore layers (include/posecnn_hip.h,
pcnn_upscore_*): the fixed bilinear transposed conv with a 2s x 2s kernel at
stride s, SAME padding, s in {2,4,8,16}.

An output row y has the taps i1 = (y + s/2) div s, k = y + s/2 - s i1,
i0 = i1 - 1 with weights (2k+1)/(2s) at i1 and (2s-1-2k)/(2s) at i0; a tap
outside [0, h) is absent (zero padding); columns alike; a 2-D weight is the
product of the two.

mode "f32": the pinned order of the generic forward, every op rounded
separately -- acc = ((t00 + t01) + t10) + t11 over the present taps, then
bias, then ReLU -- the device's bits.  mode "f64": everything in double.  The
backward sums have the device's own order, so they are compared against the
f64 mode under the worst-case bound of float32 summation in any order
(`sum_bound`), or exactly on integer inputs.
"""
import numpy as np

STRIDES = (2, 4, 8, 16)
U = 2.0 ** -24


def taps(n, s):
    """Taps of the s*n outputs along an axis of low-res extent n:
    (i0, i1, w0, w1, p0, p1), weights in float64 (exact dyadic fractions)."""
    assert s in STRIDES
    y = np.arange(s * n)
    i1 = (y + s // 2) // s
    k = y + s // 2 - s * i1
    i0 = i1 - 1
    w1 = (2 * k + 1) / (2.0 * s)
    w0 = (2 * s - 1 - 2 * k) / (2.0 * s)
    return i0, i1, w0, w1, i0 >= 0, i1 < n


def matrix(n, s):
    """(s*n, n) float64: out = matrix @ low along one axis."""
    i0, i1, w0, w1, p0, p1 = taps(n, s)
    m = np.zeros((s * n, n))
    y = np.arange(s * n)
    m[y[p0], i0[p0]] = w0[p0]
    m[y[p1], i1[p1]] = w1[p1]
    return m


def upscore_fwd_ref(x, s, bias=None, relu=False, mode="f32"):
    """x (B,h,w,Ch) -> (B, s h, s w, Ch) in `mode`'s type."""
    assert mode in ("f32", "f64")
    ft = np.float32 if mode == "f32" else np.float64
    x = np.asarray(x, ft)
    B, h, w, Ch = x.shape
    if mode == "f64":
        out = np.einsum("yi,bijc,xj->byxc", matrix(h, s), x, matrix(w, s))
    else:
        ri0, ri1, rw0, rw1, rp0, rp1 = taps(h, s)
        ci0, ci1, cw0, cw1, cp0, cp1 = taps(w, s)
        out = np.zeros((B, s * h, s * w, Ch), ft)
        have = np.zeros((s * h, s * w), bool)
        for ri, rw, rp in ((ri0, rw0, rp0), (ri1, rw1, rp1)):
            for ci, cw, cp in ((ci0, cw0, cp0), (ci1, cw1, cp1)):
                wgt = (rw[:, None] * cw[None, :]).astype(ft)   # exact
                pres = rp[:, None] & cp[None, :]
                t = x[:, np.clip(ri, 0, h - 1)][:, :, np.clip(ci, 0, w - 1)] * wgt[None, :, :, None]
                start = (pres & ~have)[None, :, :, None]
                cont = (pres & have)[None, :, :, None]
                out = np.where(start, t, np.where(cont, out + t, out)).astype(ft)
                have |= pres
        assert have.all()
    if bias is not None:
        out = out + np.asarray(bias, ft)
    if relu:
        out = np.where(out > 0, out, ft(0))
    return out.astype(ft)


def term_counts(h, w, s):
    """(h, w): the number of outputs that tap each low-res pixel."""
    return np.outer((matrix(h, s) > 0).sum(axis=0), (matrix(w, s) > 0).sum(axis=0))


def upscore_bwd_ref(d_y, s, y=None):
    """float64: {"d_x" (B,h,w,Ch), "d_bias" (Ch), "abs_x", "abs_b": the sums of
    the terms' magnitudes, "n_x" (h,w), "n_b": term counts}.  y: the forward's
    output, the ReLU mask (y > 0)."""
    g = np.asarray(d_y, np.float64)
    if y is not None:
        g = np.where(np.asarray(y) > 0, g, 0.0)
    B, H, W, Ch = g.shape
    h, w = H // s, W // s
    mr, mc = matrix(h, s), matrix(w, s)
    return {"d_x": np.einsum("yi,byxc,xj->bijc", mr, g, mc), "d_bias": g.sum(axis=(0, 1, 2)),
            "abs_x": np.einsum("yi,byxc,xj->bijc", mr, np.abs(g), mc), "abs_b": np.abs(g).sum(axis=(0, 1, 2)),
            "n_x": term_counts(h, w, s), "n_b": B * H * W}


def live(label, C):
    label = np.asarray(label)
    return (label >= 0) & (label < C)


def gather_class(dense, label):
    """dense (B,H,W,3C) -> (B,H,W,3): the three channels of each pixel's class, 0 where not live."""
    C = dense.shape[-1] // 3
    lv = live(label, C)
    idx = 3 * np.where(lv, label, 0)[..., None] + np.arange(3)
    return np.where(lv[..., None], np.take_along_axis(dense, idx, axis=-1), dense.dtype.type(0))


def scatter_class(g3, label, C):
    """g3 (B,H,W,3) -> (B,H,W,3C) float64: each pixel's three values at its class's channels."""
    lv = live(label, C)
    dense = np.zeros(g3.shape[:3] + (3 * C,))
    idx = 3 * np.where(lv, label, 0)[..., None] + np.arange(3)
    np.put_along_axis(dense, idx, np.where(lv[..., None], np.asarray(g3, np.float64), 0.0), axis=-1)
    return dense


def upscore_compact_fwd_ref(z, bias, label, s, mode="f32"):
    """(B,H,W,3): the generic forward of z with bias, without ReLU, gathered at the label's channels."""
    return gather_class(upscore_fwd_ref(z, s, bias=bias, mode=mode), label)


def upscore_compact_bwd_ref(label, d_vertex3, C, s):
    """float64: {"d_z" (B,h,w,3C), "d_bias" (3C), "abs_z", "abs_b", "n_z"
    (B,h,w,3C): the pixels of the channel's class in the window, "n_b" (3C)}."""
    label = np.asarray(label)
    dense = scatter_class(d_vertex3, label, C)
    r = upscore_bwd_ref(dense, s)
    B, H, W = label.shape
    h, w = H // s, W // s
    nr, nc = (matrix(h, s) > 0).astype(np.float64), (matrix(w, s) > 0).astype(np.float64)
    onehot = np.zeros((B, H, W, C))
    lv = live(label, C)
    np.put_along_axis(onehot, np.where(lv, label, 0)[..., None], lv[..., None].astype(np.float64), axis=-1)
    n_z = np.repeat(np.einsum("yi,byxc,xj->bijc", nr, onehot, nc), 3, axis=-1)
    return {"d_z": r["d_x"], "d_bias": r["d_bias"], "abs_z": r["abs_x"], "abs_b": r["abs_b"], "n_z": n_z,
            "n_b": np.repeat(onehot.sum(axis=(0, 1, 2)), 3)}


def sum_bound(n, abs_sum):
    """Worst-case error of n float32 terms (each a rounded product) summed in
    float32 in any order, against the float64 sum: (n + 1) * 2^-24 * sum |terms|
    to first order, 1 % for the higher orders."""
    return 1.01 * (np.asarray(n, np.float64) + 1) * U * abs_sum
