"""CPU checks of the numpy restatement of the fused momentum-SGD update
(tests/optim_ref.py) against float64 and hand-computed values, of
include/posecnn_train.h against posecnn_amd/optim.py's signature table and
the built library's exports, and of the entry point's host-side refusals."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import abi_guard
import optim_ref as orf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN_HEADER = os.path.join(ROOT, "include", "posecnn_train.h")
F = np.float32
EPS = 2.0 ** -24  # the unit roundoff of float32


def _problem(n=100003, seed=0):
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal(n) * 1e-3).astype(F)
    gs = [(rng.standard_normal(n) * 1e-4).astype(F) for _ in range(3)]
    return w, gs


def test_float32_order_against_float64():
    """3 steps on 100 003 normal values.  A step rounds g + t, momentum * m,
    a + g2, lr * m' and w - u: five roundings at full weight per element (the
    sixth, of t = weight_reg * w, enters at 1e-4 of g's size), three steps,
    slack 8: |w32 - w64| <= 8 2^-24 (|w| + lr |m|)."""
    w, gs = _problem()
    lr, mom, reg = F(1e-3), F(0.9), F(1e-4)
    w32, m32 = w.copy(), np.zeros_like(w)
    w64, m64 = w.astype(np.float64), np.zeros(w.size)
    for g in gs:
        w32, m32 = orf.update(w32, g, m32, lr, mom, reg)
        w64, m64 = orf.update64(w64, g, m64, float(lr), float(mom), float(reg))
    assert w32.dtype == F and m32.dtype == F
    bound = 8 * EPS * (np.abs(w64) + float(lr) * np.abs(m64))
    err = np.abs(w32.astype(np.float64) - w64)
    print("max error / bound:", float((err / bound).max()))
    assert (err <= bound).all()
    assert not np.array_equal(w32, w)  # it moved


def test_reg_loss_reduction_against_float64():
    """Positive terms, at most 16 serial + 8 tree + 2 roundings per term
    (the square, the float32 sums of a chunk; the float64 sums and the final
    rounding add one more): gamma_26 = 26 2^-24 = 1.6e-6, asserted at 1e-5."""
    w, _ = _problem()
    more = [w, w[:4097] * F(3), w[:5]]
    flags = [True, True, False]
    got = orf.reg_loss(more, flags, 1e-4)
    want = orf.reg_loss64(more, flags, float(F(1e-4)))
    print("reg_loss relative error:", abs(float(got) - want) / want)
    assert got.dtype == F and abs(float(got) - want) <= 1e-5 * want
    # an unflagged tensor adds nothing, whatever it holds
    assert orf.reg_loss(more, flags, 1e-4) == orf.reg_loss([w, w[:4097] * F(3), w[:5] * F(1e6)], flags, 1e-4)
    assert orf.reg_loss([], [], 1e-4) == 0


def test_chunk_partials_shape():
    c = orf.CHUNK
    x = np.ones(2 * c + 3, F)
    np.testing.assert_array_equal(orf.chunk_partials(x), [c, c, 3])
    assert orf.chunk_partials(np.zeros(0, F)).shape == (0,)
    # the order matters: 2^24 + 1 + 1 ... stays 2^24 when the large term comes first in a thread's serial sum
    y = np.zeros(c, F)
    y[0] = 4096.0   # its square is 2^24; thread 0 owns the elements 0..3
    y[1:4] = 1.0
    assert orf.chunk_partials(y)[0] == 2.0 ** 24
    y[[0, 3]] = y[[3, 0]]  # the small terms first: 3 + 2^24 rounds once, to the even neighbour
    assert orf.chunk_partials(y)[0] == 2.0 ** 24 + 4


def test_known_answer_two_steps():
    """Two steps on three values, written out; lr 0.5, momentum 0.5, weight_reg 0.25 (all exact in binary)."""
    w = np.array([1.0, -2.0, 4.0], F)
    g1 = np.array([0.5, 1.0, -1.0], F)
    g2 = np.array([0.25, 0.0, 1.0], F)
    m = np.zeros(3, F)
    # step 1: g + reg w = [0.75, 0.5, 0]; m = that; w -= 0.5 m
    w, m = orf.update(w, g1, m, 0.5, 0.5, 0.25)
    np.testing.assert_array_equal(m, [0.75, 0.5, 0.0])
    np.testing.assert_array_equal(w, [0.625, -2.25, 4.0])
    # step 2: g + reg w = [0.25 + 0.15625, -0.5625, 2]; m = 0.5 m + that; w -= 0.5 m
    w, m = orf.update(w, g2, m, 0.5, 0.5, 0.25)
    np.testing.assert_array_equal(m, [0.375 + 0.40625, 0.25 - 0.5625, 2.0])
    np.testing.assert_array_equal(w, [0.625 - 0.390625, -2.25 + 0.15625, 3.0])
    # without the flag the weight does not enter the gradient
    w2, m2 = orf.update(np.array([8.0], F), np.array([1.0], F), np.array([2.0], F), 0.5, 0.5, 0.25, regularize=False)
    np.testing.assert_array_equal(m2, [2.0])
    np.testing.assert_array_equal(w2, [7.0])
    # the L2 value of [1, -2, 4] at weight_reg 0.25: 0.125 * 21
    assert orf.reg_loss([np.array([1.0, -2.0, 4.0], F)], [True], 0.25) == F(2.625)


def test_staircase():
    got = [orf.lr_at(n, 0.001, 0.1, 2) for n in range(6)]
    lr0, g = np.float64(F(0.001)), np.float64(F(0.1))
    want = [F(lr0), F(lr0), F(lr0 * g), F(lr0 * g), F(lr0 * g * g), F(lr0 * g * g)]
    assert got == want and all(x.dtype == F for x in got)
    assert got[0] == F(0.001) and got[1] > got[2] > got[4] > 0
    assert abs(float(got[4]) - 1e-5) < 1e-11
    assert orf.lr_at(1000, 0.001, 0.1, 0) == F(0.001)  # stepsize 0: constant
    ws, ms, loss, lr = orf.apply([np.ones(3, F)], [np.ones(3, F)], [np.zeros(3, F)], [False], 4, 0.001, 0.9, 0.0,
                                 0.1, 2)
    assert lr == got[4] and loss == 0
    np.testing.assert_array_equal(ws[0], np.ones(3, F) - got[4] * np.ones(3, F))


# ---- the header, the build and the library ----
def test_new_source_and_header_are_built():
    from posecnn_amd import build
    assert "momentum.hip" in build.SOURCES and "momentum.hip" not in build.NO_SLP
    assert os.path.abspath(TRAIN_HEADER) in [os.path.abspath(h) for h in build.HEADERS]


def test_header_parses_and_matches_the_signature_table():
    from posecnn_amd import _lib, optim
    protos = abi_guard.prototypes(header=TRAIN_HEADER)
    assert set(protos) == set(optim.SIGS) and not set(optim.SIGS) & set(_lib._SIGS)
    ints = {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t, "long": ctypes.c_long}
    for name, params in protos.items():
        res, args = optim.SIGS[name]
        assert len(args) == len(params), name
        for p, a in zip(params, args):
            assert a is (ctypes.c_void_p if p.is_pointer else ints[p.c_type]), (name, p.name)
            assert not p.is_pointer or p.elem_type in abi_guard.ELEM, (name, p.name)
    decl = open(TRAIN_HEADER).read()
    assert "size_t pcnn_momentum_workspace_size" in decl and "int pcnn_momentum_sgd" in decl


def test_library_exports_every_declared_function():
    from posecnn_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in out.stdout.splitlines() if line.strip()}
    missing = set(abi_guard.declarations(TRAIN_HEADER)) - exported
    assert not missing, missing


@pytest.fixture(scope="module")
def lib():
    from posecnn_amd import optim
    return optim._load()


def test_versions_and_queries(lib):
    assert lib.pcnn_train_abi_version() == 1
    assert lib.pcnn_abi_version() == 8
    assert lib.pcnn_momentum_chunk() == orf.CHUNK
    assert lib.pcnn_momentum_workspace_size(0) >= 4
    assert lib.pcnn_momentum_workspace_size(1000) >= 4000
    assert lib.pcnn_momentum_workspace_size(1000) % 256 == 0


def test_host_side_refusals_need_no_gpu(lib):
    """Each of these is refused by the argument check, before any HIP call; the
    pointers are never dereferenced."""
    fake = ctypes.c_void_p(0x1000)
    ok = dict(table=fake, chunk_start=fake, T=1, total_chunks=1, lr0=0.001, gamma=0.1, stepsize=0, momentum=0.9,
              weight_reg=1e-4, step_dev=fake, reg_loss=None, lr_out=None, workspace=None, workspace_bytes=0,
              stream=None)

    def call(**kw):
        return lib.pcnn_momentum_sgd(*dict(ok, **kw).values())

    assert call(table=None) == 1
    assert call(chunk_start=None) == 1
    assert call(step_dev=None) == 1
    assert call(T=-1) == 1
    assert call(momentum=1.0) == 1
    assert call(momentum=-0.1) == 1
    assert call(momentum=float("nan")) == 1
    assert call(lr0=-1.0) == 1
    assert call(weight_reg=-1.0) == 1
    assert call(gamma=0.0) == 1
    assert call(stepsize=-1) == 1
    assert call(total_chunks=-1) == 1
    assert call(total_chunks=1 << 31) == 1
    assert call(T=0, total_chunks=1) == 1
    # the L2 value needs the workspace of the query
    need = lib.pcnn_momentum_workspace_size(1)
    assert call(reg_loss=fake, workspace=None) == 1
    assert call(reg_loss=fake, workspace=fake, workspace_bytes=need - 1) == 1
    assert lib.pcnn_strerror(1) == b"invalid argument"
