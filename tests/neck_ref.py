"""numpy restatement of the embedding neck (include/posecnn_neck.h,
csrc/neck.hip, posecnn_amd/neck.py): the layers between conv4_3 / conv5_3 and
the two heads, lib/networks/vgg16_convs.py:128-137 (score branch, ReLU) and
:152-161 (vertex branch, no ReLU), with both branches side by side in the
columns: [0, U) score, [U, N) vertex.

    t4 = act(z4 + b4),  t5 = act(z5 + b5),  up = upscore(t5, 2),
    a = t4 + up,  out = (a / keep_prob) * keep

neck_fwd_ref / neck_bwd_ref are the two passes behind the GEMMs z4 = x4 W4,
z5 = x5 W5.  mode "f32": the device's pinned order, every op rounded
separately -- the forward's bits, and of the backward dz4 (one product chain
per element) and dz5 (the 4x4 window row major, added to 0); the bias sums have
the device's own blocking and are compared against mode "f64" under
upscore_ref.sum_bound, or exactly on integers.  mode "f64": everything in
double.  layer_f64 is the whole layer, GEMMs included, forward and backward, in
double; with `masks` it evaluates the same expression on other operands (their
absolute values: the error bounds of the tests).

Built on tests/upscore_ref.py (the stride-2 taps) and oracle.philox (the keep
bits).
"""
import numpy as np

import upscore_ref as up
from oracle import philox


def keep_maps(M4, U, V, seed, step, stream_ids, keep_prob):
    """(keep_score (M4,U), keep_vertex (M4,V)) uint8: dense dropout masks of
    those shapes, one Philox stream id per branch."""
    return (philox.dropout_mask(M4, U, seed, step, stream_ids[0], keep_prob),
            philox.dropout_mask(M4, V, seed, step, stream_ids[1], keep_prob))


def _join_keep(keep, shape):
    """The two keep maps side by side as a float64 0 / 1 array of `shape` (B,h,w,N)."""
    return np.concatenate([np.asarray(k, np.float64) for k in keep], axis=1).reshape(shape)


def _relu_cols(a, U):
    out = a.copy()
    out[..., :U] = np.where(a[..., :U] > 0, a[..., :U], a.dtype.type(0))
    return out


def neck_fwd_ref(z4, z5, b4, b5, U, keep_prob=1.0, keep=None, mode="f32"):
    """z4 (B,h,w,N), z5 (B,h/2,w/2,N), b4, b5 (N) -> (add_score (B,h,w,U),
    add_score_vertex (B,h,w,N-U)) in `mode`'s type.  keep = (keep_score,
    keep_vertex), needed below keep_prob 1."""
    assert mode in ("f32", "f64")
    ft = np.float32 if mode == "f32" else np.float64
    z4, z5, b4, b5 = (np.asarray(a, ft) for a in (z4, z5, b4, b5))
    t4 = _relu_cols((z4 + b4).astype(ft), U)
    t5 = _relu_cols((z5 + b5).astype(ft), U)
    a = (t4 + up.upscore_fwd_ref(t5, 2, mode=mode)).astype(ft)
    if keep_prob != 1.0:
        a = ((a / ft(keep_prob)).astype(ft) * _join_keep(keep, a.shape).astype(ft)).astype(ft)
    return np.ascontiguousarray(a[..., :U]), np.ascontiguousarray(a[..., U:])


def _window_sum(g, ft):
    """dz5 before its mask: per low-res pixel the 4x4 window of g (B,h,w,N),
    rows 2i-1+u, columns 2j-1+v, weights 1/4 3/4 3/4 1/4, row major, each
    product rounded to `ft` and added to a sum that starts at 0."""
    B, h, w, N = g.shape
    hl, wl = h // 2, w // 2
    wt = np.array([0.25, 0.75, 0.75, 0.25], ft)
    acc = np.zeros((B, hl, wl, N), ft)
    i, j = np.arange(hl), np.arange(wl)
    for u in range(4):
        yy = 2 * i - 1 + u
        py = (yy >= 0) & (yy < h)
        for v in range(4):
            xx = 2 * j - 1 + v
            px = (xx >= 0) & (xx < w)
            t = (g[:, np.clip(yy, 0, h - 1)][:, :, np.clip(xx, 0, w - 1)] * ft(wt[u] * wt[v])).astype(ft)
            pres = (py[:, None] & px[None, :])[None, :, :, None]
            acc = np.where(pres, (acc + t).astype(ft), acc)
    return acc


def neck_bwd_ref(d_s, d_v, keep, z4, z5, b4, b5, U, keep_prob=1.0, mode="f32"):
    """{"dz4" (B,h,w,N), "dz5" (B,h/2,w/2,N), "db4", "db5" (N)} in `mode`'s
    type (mode "f32": db4, db5 are numpy's float32 sums, not the device's
    order).  mode "f64" adds the sums of the terms' magnitudes "abs_dz5",
    "abs_db4", "abs_db5" and the term counts "n_dz5" (hl,wl), "n_db4", "n_db5"."""
    assert mode in ("f32", "f64")
    ft = np.float32 if mode == "f32" else np.float64
    z4, z5, b4, b5 = (np.asarray(a, ft) for a in (z4, z5, b4, b5))
    g = np.concatenate([np.asarray(d_s, ft), np.asarray(d_v, ft)], axis=-1)
    if keep_prob != 1.0:
        g = ((g / ft(keep_prob)).astype(ft) * _join_keep(keep, g.shape).astype(ft)).astype(ft)
    m4 = np.ones(z4.shape, bool)
    m5 = np.ones(z5.shape, bool)
    m4[..., :U] = (z4 + b4).astype(ft)[..., :U] > 0
    m5[..., :U] = (z5 + b5).astype(ft)[..., :U] > 0
    dz4 = np.where(m4, g, ft(0))
    dz5 = np.where(m5, _window_sum(g, ft), ft(0))
    out = {"dz4": dz4, "dz5": dz5, "db4": dz4.sum(axis=(0, 1, 2), dtype=ft), "db5": dz5.sum(axis=(0, 1, 2), dtype=ft)}
    if mode == "f64":
        B, h, w, _ = g.shape
        abs5 = np.where(m5, _window_sum(np.abs(g), ft), 0.0)
        out.update(abs_dz5=abs5, abs_db4=np.abs(dz4).sum(axis=(0, 1, 2)), abs_db5=abs5.sum(axis=(0, 1, 2)),
                   n_dz5=up.term_counts(h // 2, w // 2, 2), n_db4=B * h * w, n_db5=B * h * w // 4)
    return out


def layer_f64(x4, x5, W4, b4, W5, b5, U, keep_prob=1.0, keep=None, d=None, masks=None):
    """The whole layer in float64.  x4 (B,h,w,K), x5 (B,h/2,w/2,K), W4, W5
    (K,N), b4, b5 (N); d = (d_add_score, d_add_score_vertex) adds the six
    gradients.  Returns a dict: "add_score", "add_score_vertex", "z4", "z5",
    "masks" = (act'(z4 + b4), act'(z5 + b5)) as booleans (True on the vertex
    columns) and, with d, "dz4", "dz5", "x4", "x5", "W4", "b4", "W5", "b5".
    With `masks` given, the activations are those masks instead of the
    operands' own signs: layer_f64 of the operands' absolute values under the
    true masks is the sum of the magnitudes of every term."""
    x4, x5, W4, b4, W5, b5 = (np.asarray(a, np.float64) for a in (x4, x5, W4, b4, W5, b5))
    z4, z5 = x4 @ W4, x5 @ W5
    if masks is None:
        m4, m5 = np.ones(z4.shape, bool), np.ones(z5.shape, bool)
        m4[..., :U] = (z4 + b4)[..., :U] > 0
        m5[..., :U] = (z5 + b5)[..., :U] > 0
    else:
        m4, m5 = masks
    t4, t5 = np.where(m4, z4 + b4, 0.0), np.where(m5, z5 + b5, 0.0)
    a = t4 + up.upscore_fwd_ref(t5, 2, mode="f64")
    kq = np.ones(a.shape) if keep_prob == 1.0 else _join_keep(keep, a.shape)
    a = (a / keep_prob) * kq
    out = {"add_score": a[..., :U], "add_score_vertex": a[..., U:], "z4": z4, "z5": z5, "masks": (m4, m5)}
    if d is not None:
        g = np.concatenate([np.asarray(d[0], np.float64), np.asarray(d[1], np.float64)], axis=-1)
        g = (g / keep_prob) * kq
        dz4 = np.where(m4, g, 0.0)
        dz5 = np.where(m5, up.upscore_bwd_ref(g, 2)["d_x"], 0.0)
        K, N = W4.shape
        out.update(dz4=dz4, dz5=dz5, x4=dz4 @ W4.T, x5=dz5 @ W5.T, W4=x4.reshape(-1, K).T @ dz4.reshape(-1, N),
                   W5=x5.reshape(-1, K).T @ dz5.reshape(-1, N), b4=dz4.sum(axis=(0, 1, 2)), b5=dz5.sum(axis=(0, 1, 2)))
    return out
