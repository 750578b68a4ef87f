"""numpy restatement of the backbone's arithmetic (include/posecnn_backbone.h)
-- CPU only.

Maps are NHWC, weights HWIO (3,3,Cin,Cout), padding TF SAME.

 * conv3x3_f64: the MFMA conv's reference, float64, with |.| twin for bounds;
 * conv3x3_direct_f32: conv1_1's stated float32 order, to the bit;
 * max_pool2x2: the stated compare order, to the bit;
 * im2col: the implicit matrix (M, 9 Cin), k = (dy 3 + dx) Cin + c, for the
   plane-product bookkeeping of gemm_exact_cases.kept_products;
 * vgg16_shapes: the map shapes of the whole stack.
"""
import numpy as np


def _shifted(x, dy, dx):
    """x (B,H,W,C) -> the tap (dy, dx) view: out[b, y, x] = x[b, y+dy-1, x+dx-1]
    where that is inside the map, as (destination slices, source slices) or
    None if no output pixel sees the tap."""
    H, W = x.shape[1], x.shape[2]
    y0, y1 = max(0, 1 - dy), min(H, H + 1 - dy)
    x0, x1 = max(0, 1 - dx), min(W, W + 1 - dx)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy - 1, y1 + dy - 1), slice(x0 + dx - 1, x1 + dx - 1))


def conv3x3_f64(x, w, bias=None, relu=True):
    """float64 act(conv3x3(x, w) + bias), SAME; returns (value, magnitude):
    magnitude = conv3x3(|x|, |w|) + |bias|, the scale of the error bounds."""
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    B, H, W, _ = x.shape
    out = np.zeros((B, H, W, w.shape[3]), np.float64)
    mag = np.zeros_like(out)
    for dy in range(3):
        for dx in range(3):
            sl = _shifted(x, dy, dx)
            if sl is None:
                continue
            (dys, dxs), (sys_, sxs) = sl
            out[:, dys, dxs] += x64[:, sys_, sxs] @ w64[dy, dx]
            mag[:, dys, dxs] += np.abs(x64[:, sys_, sxs]) @ np.abs(w64[dy, dx])
    if bias is not None:
        out += bias.astype(np.float64)
        mag += np.abs(bias.astype(np.float64))
    if relu:
        out = np.maximum(out, 0.0)
    return out, mag


def conv3x3_direct_f32(x, w, bias=None, relu=True):
    """conv1_1's order in float32: s = 0; for dy, dx, c nested: s = s + x * w,
    product and sum rounded separately, taps outside the image skipped; then
    s + bias, then v > 0 ? v : 0."""
    assert x.dtype == np.float32 and w.dtype == np.float32
    B, H, W, Cin = x.shape
    s = np.zeros((B, H, W, w.shape[3]), np.float32)
    for dy in range(3):
        for dx in range(3):
            sl = _shifted(x, dy, dx)
            if sl is None:
                continue
            (dys, dxs), (sys_, sxs) = sl
            for c in range(Cin):
                prod = (x[:, sys_, sxs, c, None] * w[dy, dx, c][None, None, None, :]).astype(np.float32)
                s[:, dys, dxs] = s[:, dys, dxs] + prod
    if bias is not None:
        s = s + bias.astype(np.float32)
    if relu:
        s = np.where(s > 0, s, np.float32(0))
    return s.astype(np.float32)


def max_pool2x2(x):
    """2x2, stride 2, SAME: m = the top-left value, then v > m ? v : m over
    the present ones of (0,1), (1,0), (1,1); keeps the dtype."""
    B, H, W, C = x.shape
    OH, OW = (H + 1) // 2, (W + 1) // 2
    m = x[:, 0::2, 0::2].copy()
    assert m.shape == (B, OH, OW, C)
    for oy, ox in ((0, 1), (1, 0), (1, 1)):
        v = x[:, oy::2, ox::2]
        h, w = v.shape[1], v.shape[2]
        if h == 0 or w == 0:
            continue
        sub = m[:, :h, :w]
        m[:, :h, :w] = np.where(v > sub, v, sub)
    return m


def im2col(x):
    """(B,H,W,C) -> the implicit matrix (B H W, 9 C), zeros for taps outside the image."""
    B, H, W, C = x.shape
    A = np.zeros((B, H, W, 9, C), x.dtype)
    for dy in range(3):
        for dx in range(3):
            sl = _shifted(x, dy, dx)
            if sl is None:
                continue
            (dys, dxs), (sys_, sxs) = sl
            A[:, dys, dxs, dy * 3 + dx] = x[:, sys_, sxs]
    return A.reshape(B * H * W, 9 * C)


def border_mask(B, H, W):
    """(B,H,W) bool: the pixels whose window reaches outside the image."""
    m = np.zeros((B, H, W), bool)
    m[:, 0] = m[:, -1] = True
    m[:, :, 0] = m[:, :, -1] = True
    return m


def vgg16_shapes(layers, B, H, W):
    """{name: (B,h,w,C)} of every layer of the table for a (B,H,W,3) blob."""
    out, h, w, c = {}, H, W, 3
    for layer in layers:
        if len(layer) == 3:
            assert layer[1] == c, layer
            c = layer[2]
        else:
            h, w = (h + 1) // 2, (w + 1) // 2
        out[layer[0]] = (B, h, w, c)
    return out
