"""numpy restatement of the backward of the class-compact vertex_pred layer
(include/posecnn_hip.h, pcnn_vertex_pred_compact_bwd): the 1x1 conv K -> 3C
plus bias of lib/networks/vgg16_convs.py:152-163 evaluated at each pixel's own
class.  With g = d_vertex3[p], l = label[p], a pixel is live if 0 <= l < C:

    d_feat[p][k]       = (g0 * w[k][3l] + g1 * w[k][3l+1]) + g2 * w[k][3l+2]
    d_weights[k][3l+j] = sum of feat[p][k] * g_j over the live pixels of class l
    d_bias[3l+j]       = sum of g_j over the same pixels

mode "f32": d_feat in float32 in the pinned order, every op rounded
separately (the device's bits); the sums in float64 from float32 products.
mode "f64": everything in double.  The sums' order on the device is its own,
so they are compared against the f64 mode under the worst-case bound of
float32 summation (`sum_bounds`), or exactly on integer inputs.
"""
import numpy as np


def vertex_pred_fwd_ref(feat, weights, bias, label):
    """(B,H,W,3) in double: feat @ W + b gathered at the label's three channels, 0 where not live."""
    K = feat.shape[-1]
    w = np.asarray(weights, np.float64).reshape(K, -1)
    C = w.shape[1] // 3
    live = (label >= 0) & (label < C)
    idx = 3 * np.where(live, label, 0)[..., None] + np.arange(3)
    dense = np.asarray(feat, np.float64) @ w + np.asarray(bias, np.float64)
    return np.where(live[..., None], np.take_along_axis(dense, idx, axis=-1), 0.0)


def vertex_pred_bwd_ref(feat, weights, label, d_vertex3, mode="f32"):
    """{"d_feat" (B,H,W,K), "d_weights" (K,3C), "d_bias" (3C), "n" (C) live
    pixels per class, "abs_w" (K,3C) = sum |feat * g|, "abs_b" (3C) = sum |g|}."""
    assert mode in ("f32", "f64")
    ft = np.float32 if mode == "f32" else np.float64
    K = feat.shape[-1]
    w = np.asarray(weights, ft).reshape(K, -1)
    C = w.shape[1] // 3
    label = np.asarray(label).reshape(-1)
    f = np.asarray(feat, ft).reshape(-1, K)
    g = np.asarray(d_vertex3, ft).reshape(-1, 3)
    live = (label >= 0) & (label < C)
    l = np.where(live, label, 0)
    wc = w.T.reshape(C, 3, K)[l]  # (n_pix, 3, K): the class's three weight columns
    t = g[:, 0:1] * wc[:, 0]
    t = t + g[:, 1:2] * wc[:, 1]
    t = t + g[:, 2:3] * wc[:, 2]
    d_feat = np.where(live[:, None], t, ft(0)).astype(ft)
    d_w = np.zeros((K, 3 * C), np.float64)
    d_b = np.zeros(3 * C, np.float64)
    abs_w = np.zeros((K, 3 * C), np.float64)
    abs_b = np.zeros(3 * C, np.float64)
    n = np.zeros(C, np.int64)
    for c in range(C):
        m = live & (label == c)
        n[c] = m.sum()
        if not n[c]:
            continue
        fc, gc = f[m], g[m]
        for j in range(3):
            prod = (fc * gc[:, j:j + 1]).astype(np.float64)  # rounded to ft first: float32 products in f32 mode
            d_w[:, 3 * c + j] = prod.sum(axis=0)
            abs_w[:, 3 * c + j] = np.abs(prod).sum(axis=0)
        d_b[3 * c:3 * c + 3] = gc.astype(np.float64).sum(axis=0)
        abs_b[3 * c:3 * c + 3] = np.abs(gc.astype(np.float64)).sum(axis=0)
    return {"d_feat": d_feat.reshape(feat.shape), "d_weights": d_w, "d_bias": d_b, "n": n, "abs_w": abs_w,
            "abs_b": abs_b}


def sum_bounds(r64):
    """Worst-case error of float32 products summed in float32 in any order,
    against the f64 reference: (n_l + 1) * 2^-24 * sum |feat * g| for a weight
    gradient (one rounding per product, at most n_l - 1 per sum, first order
    terms with 1 % for the higher ones), n_l * 2^-24 * sum |g| for a bias
    gradient."""
    n3 = np.repeat(r64["n"], 3).astype(np.float64)
    u = 2.0 ** -24
    return 1.01 * (n3 + 1) * u * r64["abs_w"], 1.01 * n3 * u * r64["abs_b"]
