"""Exact test operands for the split-bf16 GEMMs, and the table of GEMM calls
the exact tests run -- CPU only (numpy; torch only inside poison()).

The idea: on integer operands chosen so that every kept bf16 plane product
and every partial sum of them is an integer below 2^24, the fp32 accumulation
of v_mfma_f32_32x32x16_bf16 is exact whatever the order, the tile plan or the
split-K slicing, and the GEMM must equal an fp64 matmul bit for bit.  A lost
or doubled plane product, a wrong fragment, a K-tail slip or a stale slab is
then a plain mismatch at shapes of a few hundred, with no tolerance.

 * bf16 / split3 / split2 model x_split3 (gemm_common.h) and x_split2
   (gemm_x3.hip); kept_products says which plane products a pair of operands
   lights up, what the family's kept products sum to, and the largest term
   the family drops (0 for every class below).
 * operands(cls, ...) draws a class; reference(...) is the fp64 result with
   the same epilogue.
 * CASES is the table of calls: tests/test_gemm_exact_cases.py evaluates it
   through the plan checker (every kernel instantiation present, every edge
   case on the plan property it is named for) and tests/test_gpu_gemm_exact.py
   runs it on the GPU.
"""
from collections import namedtuple

import numpy as np

# ---------------------------------------------------------------------------
# bf16 and the split models


def bf16(x):
    """fp32 -> bf16 (round to nearest even) -> fp32; finite values only."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def split3(x):
    """x_split3: (hi, mid, lo) bf16 planes as fp32, and the residue x - hi - mid - lo."""
    x = np.asarray(x, dtype=np.float32)
    hi = bf16(x)
    r = x - hi
    mid = bf16(r)
    s = r - mid
    lo = bf16(s)
    return hi, mid, lo, s - lo


def split2(x):
    """x_split2: (hi, lo) bf16 planes as fp32, and the residue x - hi - lo."""
    x = np.asarray(x, dtype=np.float32)
    hi = bf16(x)
    r = x - hi
    lo = bf16(r)
    return hi, lo, r - lo


# kept plane products (A plane, B plane) of a family, in the kernels' names
KEPT = {
    "x6": [("hi", "hi"), ("hi", "mid"), ("mid", "hi"), ("mid", "mid"), ("hi", "lo"), ("lo", "hi")],
    "x3": [("hi", "hi"), ("hi", "lo"), ("lo", "hi")],
}

Products = namedtuple("Products", "active dropped model abs_sum")


def kept_products(A, B, family):
    """A (M, K), B (K, N) fp32 (A the summed A + A2).  active: {"hi*mid": bool}
    -- whether a kept plane product has a non-zero term; dropped: the largest
    |term| among the products the family leaves out (the split's residue
    counts as a plane); model: the fp64 sum of the kept products; abs_sum: the
    largest sum of |kept terms| of one output element (below 2^24: every
    partial sum in any order is an exact fp32 integer)."""
    if family == "x6":
        ah, am, al, ar = split3(A)
        bh, bm, bl, br = split3(B)
        pa = {"hi": ah, "mid": am, "lo": al, "res": ar}
        pb = {"hi": bh, "mid": bm, "lo": bl, "res": br}
    else:
        ah, al, ar = split2(A)
        bh, bl, br = split2(B)
        pa = {"hi": ah, "lo": al, "res": ar}
        pb = {"hi": bh, "lo": bl, "res": br}
    kept = KEPT[family]
    active, dropped = {}, 0.0
    model = np.zeros((A.shape[0], B.shape[1]), np.float64)
    abs_sum = np.zeros_like(model)
    for na, a in pa.items():
        ca = np.abs(a).max(axis=0, initial=0.0).astype(np.float64)  # per k
        for nb, b in pb.items():
            rb = np.abs(b).max(axis=1, initial=0.0).astype(np.float64)
            top = float((ca * rb).max(initial=0.0))
            if (na, nb) in kept:
                active[f"{na}*{nb}"] = top != 0.0
                model += a.astype(np.float64) @ b.astype(np.float64)
                abs_sum += np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)
            else:
                dropped = max(dropped, top)
    return Products(active, dropped, model, float(abs_sum.max(initial=0.0)))


# ---------------------------------------------------------------------------
# Operand classes: integers stored as fp32.  "<= b bits": uniform in
# (-2^b, 2^b).  Sparse: at most 8 non-zeros per output column (B) or output
# row (A), at random k.  Per class: (A kind, A bits, B kind, B bits, the plane
# products it must light up).
CLASSES = {
    "dense4": ("dense", 4, "dense", 4, ("hi*hi",)),
    "a19": ("dense", 19, "sparse", 0, ("hi*hi", "mid*hi", "lo*hi")),
    "b19": ("sparse", 0, "dense", 19, ("hi*hi", "hi*mid", "hi*lo")),
    "mm10": ("dense", 10, "sparse", 10, ("hi*hi", "mid*mid")),
    "a15": ("dense", 15, "sparse", 5, ("hi*hi", "lo*hi")),
    "b15": ("sparse", 5, "dense", 15, ("hi*hi", "hi*lo")),
}
# bits 0: +-1.  19-bit operands leave x3 a split residue: never give it a19 / b19
FAMILY_CLASSES = {"x6": ("dense4", "a19", "b19", "mm10"), "x3": ("dense4", "a15", "b15"), "f32": ("dense4", "a19")}
FAMILY = {0: "f32", 1: "x3", 2: "x6"}
SPARSE_NNZ = 8


def _ints(rng, bits, shape):
    if bits == 0:
        return rng.choice(np.array([-1.0, 1.0], np.float32), size=shape)
    return rng.integers(-(1 << bits) + 1, 1 << bits, size=shape).astype(np.float32)


def _dense(rng, bits, rows, cols):
    return _ints(rng, bits, (rows, cols))


def _sparse_cols(rng, bits, K, N):
    """(K, N) with at most SPARSE_NNZ non-zeros per column."""
    X = np.zeros((K, N), np.float32)
    ks = rng.integers(0, K, size=(SPARSE_NNZ, N))
    X[ks, np.arange(N)[None, :]] = _ints(rng, bits, (SPARSE_NNZ, N))
    return X


def operands(cls, M, N, K, seed=0, a2=False):
    """A (M, K), A2 (M, K) or None, B (K, N) of a class, fp32.  With a2 the fp32
    sum A + A2 stays inside the class: dense A and A2 are one bit narrower
    each; a sparse A is S - T and A2 = T with T dense (<= 4 bits), so the
    kernel must add A2 at every position to get the sparse S back."""
    ak, ab, bk, bb, _ = CLASSES[cls]
    rng = np.random.default_rng([seed, M, N, K, sorted(CLASSES).index(cls), int(a2)])
    A2 = None
    if ak == "dense":
        A = _dense(rng, ab - 1 if a2 else ab, M, K)
        if a2:
            A2 = _dense(rng, ab - 1, M, K)
    else:
        A = np.ascontiguousarray(_sparse_cols(rng, ab, K, M).T)
        if a2:
            A2 = _dense(rng, 4, M, K)
            A = A - A2
    B = _dense(rng, bb, K, N) if bk == "dense" else _sparse_cols(rng, bb, K, N)
    return A, A2, B


def epilogue_operands(M, N, seed=0):
    """Epilogue inputs that keep an integer result exact: an integer bias, a
    +-1 relu-backward mask, a 0 / 1 drop mask (for keep_prob = 0.5: v / 0.5
    doubles)."""
    rng = np.random.default_rng([seed, M, N, 77])
    bias = rng.integers(-255, 256, size=N).astype(np.float32)
    mask = rng.choice(np.array([-1.0, 1.0], np.float32), size=(M, N))
    drop = rng.integers(0, 2, size=(M, N)).astype(np.uint8)
    return bias, mask, drop


def reference(A, A2, B, bias=None, act=0, mask=None, drop=None, keep_prob=1.0, rows=None, k=None):
    """fp64 epilogue((A + A2)[:rows, :k] @ B[:k]): bias, relu, mask > 0, then the
    dropout (v / keep_prob) * drop -- the live rows only."""
    rows = A.shape[0] if rows is None else rows
    k = A.shape[1] if k is None else k
    a = A[:rows, :k].astype(np.float64)
    if A2 is not None:
        a = a + A2[:rows, :k]
    v = a @ B[:k].astype(np.float64)
    if bias is not None:
        v = v + bias.astype(np.float64)
    if act == 1:
        v = np.maximum(v, 0.0)
    if mask is not None:
        v = np.where(mask[:rows] > 0, v, 0.0)
    if keep_prob != 1.0:
        v = v / keep_prob
    if drop is not None:
        v = v * drop[:rows]
    return v


def poison(t):
    """Fill a (contiguous) torch buffer with 0xFF bytes: NaN as fp32."""
    assert t.is_contiguous()
    t.view(-1).view(__import__("torch").uint8).fill_(0xFF)
    return t


# ---------------------------------------------------------------------------
# The table of calls.  m_dev / k_dev: the value of the device-side counter, or
# None for a static dimension.  want: the plan properties the call is in the
# table for (PROPERTIES below; checked on the CPU through the plan checker).
Case = namedtuple("Case", "group prec M N K at bt a2 m_dev k_dev want")
LAYOUTS = ((0, 0), (0, 1), (1, 0), (1, 1))
EDGE_LAYOUTS = ((0, 0), (1, 0), (0, 1))
FORMS = ("t128", "t256gen", "t256lean")

# form -> ((base shape, device M), (ragged twin, device M))
MATRIX_SHAPES = {
    "t128": (((160, 96, 72), None), ((163, 97, 75), 131)),
    "t256gen": (((300, 320, 1024), None), ((301, 323, 1023), None)),
    "t256lean": (((300, 320, 200), None), ((301, 323, 199), None)),
}
FORM_WANT = {"t128": ("tile128",), "t256gen": ("tile256", "gen", "split"), "t256lean": ("tile256", "lean", "whole")}

LIVE256 = (0, 1, 31, 32, 33, 64, 65, 96, 97, 128, 129, 160, 224, 256, 257, 300, 320)
LIVE128 = (0, 1, 33, 64, 65, 128, 129, 163)
KSTEPS = {2: (1, 4, 15, 16, 17, 32, 33, 48), 1: (1, 31, 32, 33, 64, 65, 96)}
KDEV = (0, 1, 5, 77)
SPLIT_SHAPE = (300, 320, 4224)  # x6: ns 264, S 32, kstep 9 -> slices 30, 31 empty; x3: ns 132, kstep 5 -> 27 .. 31
SPLIT_MDEV = (1, 150, 300)
MULTI = {"t128": (3072, 3072, 64), "t256lean": (4352, 4352, 144)}
F32_SHAPES = ((200, 300, 1000), (203, 301, 999))
TP_SHAPES = (((300, 320, 200), None, None), ((320, 512, 192), 300, None), ((512, 384, 320), None, 77))


def matrix_case(prec, form, at, bt, ragged, a2):
    (M, N, K), mdev = MATRIX_SHAPES[form][ragged]
    return Case("matrix", prec, M, N, K, at, bt, a2, mdev, None, FORM_WANT[form] + (("ragged",) if ragged else ("whole4",)))


def _cases():
    out = []
    for prec in (1, 2):
        for form in FORMS:
            for at, bt in LAYOUTS:
                for ragged in (0, 1):
                    for a2 in (0, 1):
                        out.append(matrix_case(prec, form, at, bt, ragged, a2))
        for at, bt in EDGE_LAYOUTS:
            for m in LIVE256:
                out.append(Case("live256", prec, 320, 512, 192, at, bt, 0, m, None, ("tile256", "gen", "dev_m_whole")))
            for m in LIVE128:
                out.append(Case("live128", prec, 163, 97, 75, at, bt, 0, m, None, ("tile128", "dev_m_whole")))
            for k in KSTEPS[prec]:
                out.append(Case("ksteps", prec, 160, 96, k, at, bt, 0, None, None, ("tile128", f"steps{prec}")))
            out.append(Case("splitk", prec, *SPLIT_SHAPE, at, bt, 0, None, None, ("tile256", "gen", "empty_slice")))
            for m in SPLIT_MDEV:
                out.append(Case("splitk_mdev", prec, *SPLIT_SHAPE, at, bt, 0, m, None, ("tile256", "gen", "split")))
            out.append(Case("multi", prec, *MULTI["t128"], at, bt, 0, None, None, ("tile128", "multi_item")))
            out.append(Case("multi", prec, *MULTI["t256lean"], at, bt, 0, None, None, ("tile256", "lean", "multi_item")))
            out.append(Case("keep", prec, 160, 96, 72, at, bt, 0, None, None, ("tile128", "whole")))
        for k in KDEV:  # the dW layout, on a tile-128 and on a tile-256 capacity shape
            out.append(Case("kdev", prec, 160, 96, 80, 1, 0, 0, None, k, ("tile128", "kdev")))
            out.append(Case("kdev", prec, 300, 320, 200, 1, 0, 0, None, k, ("tile256", "lean", "kdev")))
    for (M, N, K) in F32_SHAPES:
        for at, bt in LAYOUTS:
            for mdev in (None, M - 70):
                out.append(Case("f32", 0, M, N, K, at, bt, 0, mdev, None, ()))
    return out


CASES = _cases()


def cases(group, prec=None):
    return [c for c in CASES if c.group == group and (prec is None or c.prec == prec)]


# Plan rows of the checker's --variant mode
Plan = namedtuple("Plan", "tile gen at bt ragged a2 mode S tiles active kstep ns grid")


def checker_args(c):
    return [c.M, c.N, c.K, int(c.m_dev is not None), int(c.k_dev is not None), c.at, c.bt, c.a2, c.prec,
            c.M if c.m_dev is None else c.m_dev, c.K if c.k_dev is None else c.k_dev]


def _steps_ok(prec):
    bk = 16 if prec == 2 else 32
    return lambda c, p: p.S == 1 and p.ns == (c.K + bk - 1) // bk


# property name -> predicate(case, plan)
PROPERTIES = {
    "tile128": lambda c, p: p.tile == 128 and p.gen == 1,
    "tile256": lambda c, p: p.tile == 256,
    "gen": lambda c, p: p.gen == 1,
    "lean": lambda c, p: p.gen == 0 and p.mode == 0 and p.S == 1,
    "split": lambda c, p: p.mode == 1 and p.S > 1,
    "whole": lambda c, p: p.mode == 0 and p.S == 1,
    "ragged": lambda c, p: p.ragged == 1,
    "whole4": lambda c, p: p.ragged == 0,
    # device-side M on a shape that runs whole tiles for every M
    "dev_m_whole": lambda c, p: c.m_dev is not None and p.S == 1 and p.mode == 0 and (p.tiles > 0) == (c.m_dev > 0),
    # split-K whose last slice(s) get no K step
    "empty_slice": lambda c, p: p.mode == 1 and p.S > 1 and (p.ns + p.kstep - 1) // p.kstep < p.S,
    # a persistent workgroup takes more than one item
    "multi_item": lambda c, p: p.mode == 0 and p.tiles > p.active and p.active == p.grid,
    "kdev": lambda c, p: c.k_dev is not None and p.S == 1,
    "steps1": _steps_ok(1),
    "steps2": _steps_ok(2),
}
