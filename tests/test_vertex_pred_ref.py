"""The backward of the class-compact vertex_pred layer without a GPU:
tests/vertex_pred_ref.py (the reference the GPU tests compare against) against
torch autograd of the dense layer and a hand-derived known answer, and the
library's host-side answers (size queries, argument validation; no launch is
made: PCNN_EINVAL = 1, PCNN_ECAPACITY = 3)."""
import ctypes

import numpy as np
import pytest
import torch

import vertex_pred_ref as ref

P = ctypes.c_void_p(1 << 20)   # any 16-byte aligned non-NULL address: nothing is dereferenced
ODD = ctypes.c_void_p((1 << 20) + 4)
BIG = 1 << 40


@pytest.fixture(scope="module")
def lib():
    from posecnn_amd import _lib, build
    if build.needs_build():
        build.build()
    return _lib.load()


@pytest.mark.parametrize("shape", [(2, 6, 7, 8, 5), (1, 3, 5, 4, 1)])
def test_f64_reference_is_autograd_of_the_dense_layer(shape):
    B, H, W, K, C = shape
    rng = np.random.default_rng(sum(shape))
    feat = rng.standard_normal((B, H, W, K))
    w = rng.standard_normal((K, 3 * C))
    b = rng.standard_normal(3 * C)
    g = rng.standard_normal((B, H, W, 3))
    label = rng.integers(0, C, size=(B, H, W))
    label.reshape(-1)[:4] = [-1, C, C + 5, -100]
    r = ref.vertex_pred_bwd_ref(feat, w, label, g, mode="f64")

    tf, tw, tb = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (feat, w, b))
    live = (label >= 0) & (label < C)
    idx = torch.tensor(3 * np.where(live, label, 0)[..., None] + np.arange(3))
    out = torch.gather(tf @ tw + tb, 3, idx) * torch.tensor(live[..., None].astype(np.float64))
    np.testing.assert_allclose(out.detach().numpy(), ref.vertex_pred_fwd_ref(feat, w, b, label), rtol=1e-12,
                               atol=1e-12)
    out.backward(torch.tensor(g))
    for name, t in (("d_feat", tf), ("d_weights", tw), ("d_bias", tb)):
        got, want = r[name], t.grad.numpy()
        assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), name
    assert r["n"].sum() == live.sum() and not r["d_feat"].reshape(-1, K)[~live.reshape(-1)].any()


def test_f32_mode_rounds_every_op_of_d_feat():
    rng = np.random.default_rng(5)
    feat = rng.standard_normal((1, 4, 4, 4)).astype(np.float32)
    w = rng.standard_normal((4, 6)).astype(np.float32)
    g = rng.standard_normal((1, 4, 4, 3)).astype(np.float32)
    label = rng.integers(0, 2, size=(1, 4, 4))
    r = ref.vertex_pred_bwd_ref(feat, w, label, g, mode="f32")
    assert r["d_feat"].dtype == np.float32
    f32 = np.float32
    for (y, x, k) in ((0, 0, 0), (3, 2, 1), (1, 3, 3)):
        l, gg = label[0, y, x], g[0, y, x]
        t = f32(gg[0] * w[k, 3 * l])
        t = f32(t + f32(gg[1] * w[k, 3 * l + 1]))
        t = f32(t + f32(gg[2] * w[k, 3 * l + 2]))
        assert r["d_feat"][0, y, x, k] == t


@pytest.mark.parametrize("mode", ["f32", "f64"])
def test_one_pixel_per_class_unit_gradient(mode):
    """Pixel c has label c, feat[c] = (c + 1) * (1, 2, .., K) and g = (1, 1, 1):
    d_weights[k][3c+j] = (c + 1) (k + 1), d_bias = 1, d_feat[c][k] = the sum of class c's three weights of row k."""
    C, K = 3, 4
    feat = np.stack([(c + 1) * np.arange(1, K + 1) for c in range(C)]).reshape(1, 1, C, K).astype(np.float32)
    w = np.arange(K * 3 * C, dtype=np.float32).reshape(K, 3 * C)
    label = np.arange(C).reshape(1, 1, C)
    g = np.ones((1, 1, C, 3), np.float32)
    r = ref.vertex_pred_bwd_ref(feat, w, label, g, mode=mode)
    want_w = np.repeat(np.outer(np.arange(1, K + 1), np.arange(1, C + 1)), 3, axis=1)
    np.testing.assert_array_equal(r["d_weights"], want_w)
    np.testing.assert_array_equal(r["d_bias"], np.ones(3 * C))
    want_f = np.stack([w[:, 3 * c:3 * c + 3].sum(axis=1) for c in range(C)]).reshape(1, 1, C, K)
    np.testing.assert_array_equal(r["d_feat"], want_f)
    np.testing.assert_array_equal(r["n"], [1, 1, 1])
    bw, bb = ref.sum_bounds(r)
    assert (bw > 0).all() and (bb > 0).all()


def test_entry_points_are_declared_and_exported(lib):
    from posecnn_amd import _lib
    from test_abi import _declared
    decl = _declared()
    for name, n in (("pcnn_vertex_pred_compact_bwd", 15), ("pcnn_vertex_pred_compact_bwd_workspace_size", 5),
                    ("pcnn_vertex_pred_compact_bwd_partials", 5)):
        assert decl[name] == n == len(_lib._SIGS[name][1]), name
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr)
    assert lib.pcnn_abi_version() >= 6


def test_size_queries(lib):
    size, parts = lib.pcnn_vertex_pred_compact_bwd_workspace_size, lib.pcnn_vertex_pred_compact_bwd_partials
    P8 = parts(8, 480, 640, 128, 22)
    assert P8 > 0 and size(8, 480, 640, 128, 22) >= P8 * 66 * 129 * 4
    assert parts(1, 5, 7, 4, 1) == 1 and size(1, 5, 7, 4, 1) > 0
    assert parts(2, 120, 160, 16, 4) >= 3
    assert size(1, 3, 5, 252, 21) > 0   # 252 * 63 * 4 = 63,504 B: inside the LDS image's limit
    for bad in ((2, 24, 32, 6, 22), (2, 24, 32, 256, 22), (2, 24, 32, 128, 43), (0, 24, 32, 128, 22),
                (2, 24, 32, 128, 0), (2, 24, 32, 0, 22), (2, -1, 32, 128, 22), (64, 480, 640, 128, 22)):
        assert size(*bad) == 0 and parts(*bad) == 0, bad   # K % 4, K * 3C * 4 > 64 KiB, non-positive, >= 2^31 elements


def test_argument_validation(lib):
    shape = (2, 24, 32, 128, 22)
    need = lib.pcnn_vertex_pred_compact_bwd_workspace_size(*shape)

    def bwd(feat=P, w=P, label=P, g=P, d_feat=P, d_w=P, d_b=P, workspace=P, nbytes=BIG, shape=shape):
        return lib.pcnn_vertex_pred_compact_bwd(feat, w, label, g, *shape, d_feat, d_w, d_b, workspace, nbytes, None)
    assert bwd(d_feat=None, d_w=None, d_b=None) == 1
    assert bwd(d_feat=ODD) == 1 and bwd(feat=ODD) == 1 and bwd(g=ODD) == 1
    assert bwd(shape=(2, 24, 32, 6, 22)) == 1 and bwd(shape=(2, 24, 32, 256, 22)) == 1
    assert bwd(shape=(0, 24, 32, 128, 22)) == 1 and bwd(shape=(2, 24, 32, 128, 0)) == 1
    assert bwd(label=None) == 1 and bwd(g=None) == 1
    assert bwd(feat=None) == 1 and bwd(w=None) == 1           # needed by d_weights / by d_feat
    assert bwd(workspace=None) == 1 and bwd(workspace=None, d_feat=None) == 1
    assert bwd(nbytes=need - 1) == 3 and bwd(nbytes=0, d_feat=None, d_w=None) == 3
