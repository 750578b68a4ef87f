"""Shapes and operands of the backbone tests -- CPU only (numpy).

Shapes are (B, H, W, Cin, Cout), the smallest at which each path of
csrc/backbone.hip can still go wrong.  The exact classes carry the idea of
tests/gemm_exact_cases.py to the conv: integer operands for which every kept
bf16 plane product and every partial sum of them is an integer below 2^24, so
any accumulation order, tiling or split of the contraction must equal the
float64 result bit for bit.
"""
import functools

import numpy as np

# the MFMA conv
MFMA_SHAPES = (
    (2, 5, 7, 16, 20),      # less than one patch; rows cross image rows and the batch seam; a ragged column edge
    (1, 18, 20, 48, 132),   # several patches, three channel steps per tap, columns crossing 128
    (3, 4, 4, 512, 64),     # K = 4608, the workload's longest contraction; a tiny map (the planner splits)
    (1, 1, 1, 16, 4),       # every tap but the centre is padding
    (1, 1, 9, 16, 4),       # every vertical tap is padding
)
FLOAT_SHAPES = MFMA_SHAPES[:3]
SPLIT_SHAPE = MFMA_SHAPES[2]
DIRECT_SHAPES = ((2, 5, 7, 3, 64), (1, 1, 1, 3, 4))          # conv1_1
POOL_SHAPES = ((2, 5, 7, 8), (1, 4, 6, 64), (1, 1, 1, 4))     # (B, H, W, C)
STACK_SHAPES = ((2, 32, 48), (1, 17, 23))                     # (B, H, W) of the blob


def ident(shape):
    return "x".join(str(s) for s in shape)


# class -> the kept plane products (activation plane * weight plane) it must light
CLASSES = {
    "dense4": ("hi*hi",),
    "x19": ("hi*hi", "mid*hi", "lo*hi"),
    "w19": ("hi*hi", "hi*mid", "hi*lo"),
    "mm10": ("hi*hi", "mid*mid"),
    "const": ("hi*hi",),   # the halo case: a constant non-zero map against dense 4-bit weights
}
ALL_KEPT = ("hi*hi", "hi*mid", "mid*hi", "mid*mid", "hi*lo", "lo*hi")
SPARSE_NNZ = 8
CONST = 3.0
LIMIT = float(1 << 24)


def _ints(rng, bits, shape):
    if bits == 0:
        return rng.choice(np.array([-1.0, 1.0], np.float32), size=shape)
    return rng.integers(-(1 << bits) + 1, 1 << bits, size=shape).astype(np.float32)


def _sparse_weights(rng, bits, Cin, Cout):
    """(3,3,Cin,Cout) with at most SPARSE_NNZ non-zeros per output channel."""
    K = 9 * Cin
    Wm = np.zeros((K, Cout), np.float32)
    ks = rng.integers(0, K, size=(SPARSE_NNZ, Cout))
    Wm[ks, np.arange(Cout)[None, :]] = _ints(rng, bits, (SPARSE_NNZ, Cout))
    return Wm.reshape(3, 3, Cin, Cout)


def _one_channel(rng, B, H, W, Cin):
    """+-1 in one random channel per pixel: at most 9 non-zeros per window."""
    x = np.zeros((B * H * W, Cin), np.float32)
    x[np.arange(B * H * W), rng.integers(0, Cin, size=B * H * W)] = _ints(rng, 0, B * H * W)
    return x.reshape(B, H, W, Cin)


@functools.lru_cache(maxsize=None)
def exact_case(cls, shape, seed=0):
    """(x (B,H,W,Cin), weights (3,3,Cin,Cout), bias (Cout)) of a class: integers stored as float32."""
    B, H, W, Cin, Cout = shape
    rng = np.random.default_rng([seed, *shape, sorted(CLASSES).index(cls)])
    if cls == "dense4":
        x, w = _ints(rng, 4, (B, H, W, Cin)), _ints(rng, 4, (3, 3, Cin, Cout))
    elif cls == "x19":
        x, w = _ints(rng, 19, (B, H, W, Cin)), _sparse_weights(rng, 0, Cin, Cout)
    elif cls == "w19":
        x, w = _one_channel(rng, B, H, W, Cin), _ints(rng, 19, (3, 3, Cin, Cout))
    elif cls == "mm10":
        x, w = _ints(rng, 10, (B, H, W, Cin)), _sparse_weights(rng, 10, Cin, Cout)
    elif cls == "const":
        x, w = np.full((B, H, W, Cin), CONST, np.float32), _ints(rng, 4, (3, 3, Cin, Cout))
    else:
        raise KeyError(cls)
    bias = rng.integers(-255, 256, size=Cout).astype(np.float32)
    for a in (x, w, bias):
        a.setflags(write=False)
    return x, w, bias


@functools.lru_cache(maxsize=None)
def float_case(shape, seed=0):
    """Normal activations, weights scaled by K^-1/2 (all three planes populated), a normal bias."""
    B, H, W, Cin, Cout = shape
    rng = np.random.default_rng([seed, *shape, 1234])
    x = rng.standard_normal((B, H, W, Cin)).astype(np.float32)
    w = (rng.standard_normal((3, 3, Cin, Cout)) / np.sqrt(9 * Cin)).astype(np.float32)
    bias = rng.standard_normal(Cout).astype(np.float32)
    for a in (x, w, bias):
        a.setflags(write=False)
    return x, w, bias


@functools.lru_cache(maxsize=None)
def negative_map(shape, seed=0):
    """Negative-only normal floats: a zero from padding would win a max wrongly."""
    rng = np.random.default_rng([seed, *shape, 99])
    x = (-np.abs(rng.standard_normal(shape)) - 0.5).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def stack_params(seed=0, scale=1.0):
    """{name: (weights, biases)} for the thirteen layers: He-scaled normal
    weights (so that activations neither die nor blow up through the stack)
    and small biases."""
    from posecnn_amd.backbone import CONVS
    rng = np.random.default_rng([seed, 4321])
    out = {}
    for name, cin, cout in CONVS:
        w = (rng.standard_normal((3, 3, cin, cout)) * (scale * np.sqrt(2.0 / (9 * cin)))).astype(np.float32)
        b = (0.1 * rng.standard_normal(cout)).astype(np.float32)
        out[name] = (w, b)
    return out


@functools.lru_cache(maxsize=None)
def blob(shape, seed=0):
    B, H, W = shape
    rng = np.random.default_rng([seed, *shape, 7])
    x = rng.standard_normal((B, H, W, 3)).astype(np.float32)
    x.setflags(write=False)
    return x
