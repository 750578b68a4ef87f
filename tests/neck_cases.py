"""Shapes and operands of the embedding-neck tests (tests/test_neck_ref.py on
the CPU, tests/test_gpu_neck.py on the device), generated once per shape and
shared."""
import functools

import numpy as np

# (B, h, w, K, U, V)
SHAPES = [
    (2, 6, 10, 40, 12, 20),     # low-res 3 x 5: odd extents, absent taps at every border, widths far from any tile
    (3, 6, 10, 40, 12, 20),     # M4 = 180: no multiple of 32
    (1, 8, 12, 512, 64, 128),   # the real widths; two blocks in the backward
    (2, 4, 4, 40, 16, 0),       # the score branch alone
    (2, 4, 4, 40, 0, 8),        # the vertex branch alone
]
REAL = SHAPES[2]
SEED, STREAM_IDS = 0x1234567887654321, (1, 2)
IDS = ["x".join(str(v) for v in s) for s in SHAPES]


def _shapes(shape):
    B, h, w, K, U, V = shape
    N = U + V
    return dict(x4=(B, h, w, K), x5=(B, h // 2, w // 2, K), W4=(K, N), W5=(K, N), b4=(N,), b5=(N,),
                d_s=(B, h, w, U), d_v=(B, h, w, V), z4=(B, h, w, N), z5=(B, h // 2, w // 2, N))


def mask_room(c, shape):
    """(|x W + b|, (K + 16) 2^-24 (|x| |W| + |b|)) on the ReLU columns, in float64, for both maps: a float32
    pre-activation computed in any order has the sign of the exact one wherever the first exceeds the second."""
    K, U = shape[3], shape[4]
    out = []
    for x, W, b in ((c["x4"], c["W4"], c["b4"]), (c["x5"], c["W5"], c["b5"])):
        x, W, b = (np.asarray(a, np.float64) for a in (x, W, b))
        out.append((np.abs(x @ W + b)[..., :U], ((K + 16) * 2.0 ** -24 * (np.abs(x) @ np.abs(W) + np.abs(b)))[..., :U]))
    return out


@functools.lru_cache(maxsize=None)
def float_case(shape):
    """float32 operands: x, W and b of order 1 (z = x W of order sqrt(K) W's scale), gradients of order 1.
    The backward of a ReLU is discontinuous at 0, so a comparison of gradients against float64 is well posed
    only if no pre-activation is within float32's reach of 0 (mask_room): the first draw for which that holds
    is taken (at K = 512 a draw has a couple of such elements among its 6912 more often than not)."""
    s = _shapes(shape)
    K = shape[3]
    for attempt in range(200):
        rng = np.random.default_rng(1000 * (1 + SHAPES.index(shape)) + attempt)
        c = {n: rng.standard_normal(s[n]).astype(np.float32)
             for n in ("x4", "x5", "b4", "b5", "d_s", "d_v", "z4", "z5")}
        for n in ("W4", "W5"):
            c[n] = (rng.standard_normal(s[n]) / np.sqrt(K)).astype(np.float32)
        if all((pre > room).all() for pre, room in mask_room(c, shape)):
            return c
    raise AssertionError(f"no well-posed draw for {shape}")


@functools.lru_cache(maxsize=None)
def integer_case(shape):
    """Small integers as float32: |x| <= 4, |W| <= 2, |b| <= 3, incoming gradients |g| <= 4.  With keep_prob
    0.5 every intermediate is an integer or a multiple of 1/16 far below 2^24 / 16: float32 is exact in any order."""
    rng = np.random.default_rng(200 + SHAPES.index(shape))
    s = _shapes(shape)
    lim = dict(x4=4, x5=4, W4=2, W5=2, b4=3, b5=3, d_s=4, d_v=4, z4=40, z5=40)
    return {n: rng.integers(-lim[n], lim[n] + 1, size=s[n]).astype(np.float32) for n in lim}
