"""The segmentation and vertex losses without a GPU: the C-ABI surface of the
four ops (include/posecnn_hip.h against posecnn_amd._lib), their host-side
argument validation (no launch is made: PCNN_EINVAL = 1, PCNN_ECAPACITY = 3),
and hand-derived known answers that pin tests/seg_loss_ref.py, the reference
the GPU tests compare against."""
import ctypes
import math

import numpy as np
import pytest

import seg_loss_ref as ref

P = ctypes.c_void_p(1 << 20)   # any 16-byte aligned non-NULL address: nothing is dereferenced
ODD = ctypes.c_void_p((1 << 20) + 4)
BIG = 1 << 40


@pytest.fixture(scope="module")
def lib():
    from posecnn_amd import _lib, build
    if build.needs_build():
        build.build()
    return _lib.load()


def test_entry_points_are_declared_and_exported(lib):
    from posecnn_amd import _lib
    from test_abi import _declared
    decl = _declared()
    for name, n in (("pcnn_seg_loss", 17), ("pcnn_seg_loss_workspace_size", 4), ("pcnn_cross_entropy", 10),
                    ("pcnn_cross_entropy_workspace_size", 2), ("pcnn_vertex_loss", 11),
                    ("pcnn_vertex_loss_workspace_size", 1), ("pcnn_vertex_loss_compact", 17),
                    ("pcnn_vertex_loss_compact_workspace_size", 4)):
        assert decl[name] == n == len(_lib._SIGS[name][1]), name
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr)
    assert lib.pcnn_abi_version() >= 5


def test_workspace_sizes(lib):
    n_pix = 8 * 480 * 640
    assert lib.pcnn_seg_loss_workspace_size(8, 480, 640, 22) >= n_pix * 8 + (n_pix // 256) * 16
    assert lib.pcnn_seg_loss_workspace_size(8, 480, 640, 0) == 0
    assert lib.pcnn_seg_loss_workspace_size(0, 480, 640, 22) == 0
    assert lib.pcnn_seg_loss_workspace_size(8, 4800, 6400, 22) == 0  # 2^31 elements or more
    assert 0 < lib.pcnn_cross_entropy_workspace_size(n_pix, 22) <= 1 << 20
    assert lib.pcnn_cross_entropy_workspace_size(n_pix, 0) == 0
    assert 0 < lib.pcnn_vertex_loss_workspace_size(n_pix * 66) <= 1 << 20
    assert lib.pcnn_vertex_loss_workspace_size(0) == 0 and lib.pcnn_vertex_loss_workspace_size(1 << 31) == 0
    assert 0 < lib.pcnn_vertex_loss_compact_workspace_size(8, 480, 640, 22) <= 1 << 20
    assert lib.pcnn_vertex_loss_compact_workspace_size(8, 480, 640, 0) == 0


def test_seg_loss_validation(lib):
    need = lib.pcnn_seg_loss_workspace_size(2, 48, 64, 22)

    def seg(score=P, gt=P, C=22, threshold=1.0, log_prob=None, d_score=P, label=P, loss=P, workspace=P, nbytes=BIG,
            B=2):
        return lib.pcnn_seg_loss(score, gt, B, 48, 64, C, threshold, 1.0, log_prob, None, label, None, d_score, loss,
                                 workspace, nbytes, None)
    assert seg(score=None) == 1 and seg(gt=None) == 1 and seg(loss=None) == 1 and seg(workspace=None) == 1
    assert seg(C=0) == 1 and seg(B=0) == 1 and seg(B=-1) == 1
    assert seg(threshold=0.0) == 1 and seg(threshold=-1.0) == 1
    assert seg(score=ODD) == 1 and seg(d_score=ODD) == 1 and seg(log_prob=ODD) == 1 and seg(workspace=ODD) == 1
    assert seg(label=ctypes.c_void_p((1 << 20) + 2)) == 1
    assert seg(B=1 << 20) == 1  # 2^31 elements or more
    assert seg(nbytes=need - 1) == 3


def test_cross_entropy_validation(lib):
    need = lib.pcnn_cross_entropy_workspace_size(1000, 22)

    def ce(scores=P, labels=P, n_pix=1000, C=22, d=P, loss=P, workspace=P, nbytes=BIG):
        return lib.pcnn_cross_entropy(scores, labels, n_pix, C, 1.0, d, loss, workspace, nbytes, None)
    assert ce(scores=None) == 1 and ce(labels=None) == 1 and ce(loss=None) == 1 and ce(workspace=None) == 1
    assert ce(C=0) == 1 and ce(n_pix=0) == 1 and ce(n_pix=1 << 30, C=2) == 1
    assert ce(scores=ODD) == 1 and ce(labels=ODD) == 1 and ce(d=ODD) == 1
    assert ce(nbytes=need - 1) == 3


def test_vertex_loss_validation(lib):
    need = lib.pcnn_vertex_loss_workspace_size(66000)

    def vl(pred=P, tgt=P, w=P, n=66000, sigma=1.0, d=P, loss=P, workspace=P, nbytes=BIG):
        return lib.pcnn_vertex_loss(pred, tgt, w, n, sigma, 1.0, d, loss, workspace, nbytes, None)
    assert vl(pred=None) == 1 and vl(tgt=None) == 1 and vl(w=None) == 1 and vl(loss=None) == 1
    assert vl(workspace=None) == 1 and vl(n=0) == 1 and vl(n=1 << 31) == 1
    assert vl(sigma=0.0) == 1 and vl(sigma=-2.0) == 1
    assert vl(pred=ODD) == 1 and vl(tgt=ODD) == 1 and vl(w=ODD) == 1 and vl(d=ODD) == 1
    assert vl(nbytes=need - 1) == 3

    need = lib.pcnn_vertex_loss_compact_workspace_size(2, 48, 64, 22)

    def vc(label=P, v3=P, pred=P, pred_ch=66, C=22, sigma=1.0, d=P, d_ch=3, loss=P, workspace=P, nbytes=BIG):
        return lib.pcnn_vertex_loss_compact(label, v3, pred, pred_ch, 2, 48, 64, C, 10.0, sigma, 1.0, d, d_ch, loss,
                                            workspace, nbytes, None)
    assert vc(label=None) == 1 and vc(v3=None) == 1 and vc(pred=None) == 1 and vc(loss=None) == 1
    assert vc(workspace=None) == 1 and vc(C=0) == 1 and vc(sigma=0.0) == 1
    assert vc(pred_ch=4) == 1 and vc(d_ch=5) == 1
    assert vc(pred=ODD) == 1 and vc(d=ODD) == 1 and vc(workspace=ODD) == 1
    assert vc(nbytes=need - 1) == 3


# ---------------------------------------------------------------------------
# known answers of the reference module

@pytest.mark.parametrize("mode", ["f32", "f64"])
def test_two_equal_scores(mode):
    r = ref.seg_ref(np.zeros((1, 2), np.float32), np.array([1]), 1.0, mode=mode)
    assert abs(float(r["loss"]) - math.log(2)) < 1e-7 and r["n"] == 1
    np.testing.assert_allclose(r["d_score"], [[0.5, -0.5]], rtol=1e-7)
    np.testing.assert_array_equal(r["prob_normalized"], [[0.5, 0.5]])
    np.testing.assert_array_equal(r["label_2d"], [0])  # the first maximum
    np.testing.assert_array_equal(r["gt_label_weight"], [[0, 1]])


@pytest.mark.parametrize("mode", ["f32", "f64"])
def test_ignored_pixels_give_zero(mode):
    rng = np.random.default_rng(0)
    r = ref.seg_ref(rng.standard_normal((5, 7, 4)).astype(np.float32), np.full((5, 7), -1), 1.0, mode=mode)
    assert r["n"] == 0 and float(r["loss"]) == 0.0 and not r["d_score"].any() and not r["gt_label_weight"].any()
    assert np.isfinite(r["d_score"]).all()


def test_background_threshold_and_out_of_range_labels():
    score = np.zeros((4, 3), np.float32)
    score[1, 0] = 100.0   # p_0 == 1.0f exactly: not below the threshold 1.0
    r = ref.seg_ref(score, np.array([0, 0, 3, -7]), 1.0)
    assert r["prob_normalized"][1, 0] == np.float32(1.0)
    np.testing.assert_array_equal(r["hard"], [True, False, False, False])
    assert abs(float(r["loss"]) - math.log(3)) < 1e-6
    assert not r["d_score"][1:].any()
    assert not ref.seg_ref(score, np.array([0, 0, 3, -7]), 0.3)["hard"].any()  # p_0 = 1/3 >= 0.3
    # grad_scale scales the gradient alone
    a, b = ref.seg_ref(score, np.array([0, 1, 2, 1]), 1.0), ref.seg_ref(score, np.array([0, 1, 2, 1]), 1.0, 2.5)
    assert a["loss"] == b["loss"]
    np.testing.assert_allclose(b["d_score"], 2.5 * a["d_score"], rtol=1e-6, atol=1e-30)  # exp(-100) is subnormal


def test_cross_entropy_is_the_seg_loss_of_its_maps():
    rng = np.random.default_rng(1)
    score = rng.standard_normal((50, 5)).astype(np.float32)
    gt = rng.integers(-1, 5, 50)
    r = ref.seg_ref(score, gt, 1.0)
    loss, d = ref.cross_entropy_ref(r["log_prob"], r["gt_label_weight"])
    assert abs(float(loss) - float(r["loss"])) <= np.spacing(np.float32(r["loss"]))
    np.testing.assert_allclose(d, -r["gt_label_weight"] / r["n"], rtol=1e-6)


@pytest.mark.parametrize("mode", ["f32", "f64"])
def test_smooth_l1_known_answers(mode):
    delta = np.array([0.5, 1.0, 2.0], np.float32)
    r = ref.vertex_ref(delta, np.zeros(3, np.float32), np.ones(3, np.float32), 1.0, mode=mode)
    np.testing.assert_array_equal(r["in_loss"], [0.125, 0.5, 1.5])
    np.testing.assert_array_equal(r["near"], [True, False, False])
    np.testing.assert_allclose(r["d_pred"], np.array([0.5, 1, 1]) / 3, rtol=1e-7)
    assert abs(float(r["loss"]) - 2.125 / 3) < 1e-7
    # the sign of the far branch, zero at zero
    r = ref.vertex_ref(-delta, np.zeros(3, np.float32), np.ones(3, np.float32), 1.0, mode=mode)
    np.testing.assert_allclose(r["d_pred"], -np.array([0.5, 1, 1]) / 3, rtol=1e-7)
    z = ref.vertex_ref(np.zeros(2), np.zeros(2), np.array([1, 0]), 1.0, mode=mode)
    assert not z["d_pred"].any() and float(z["loss"]) == 0.0 and z["near"].all()


def test_sigma_moves_the_branch_point():
    c_inv, c_half, c_off, c_s2 = ref.smooth_l1_constants(3.0)
    assert (c_inv, c_half, c_off, c_s2) == (np.float32(1 / 9), np.float32(4.5), np.float32(0.5 / 9), np.float32(9))
    delta = np.array([0.1, 0.12, -0.5], np.float32)  # 1/9 = 0.111...
    r = ref.vertex_ref(delta, np.zeros(3), np.ones(3), 3.0, mode="f64")
    np.testing.assert_array_equal(r["near"], [True, False, False])
    d = delta.astype(np.float64)
    np.testing.assert_allclose(r["in_loss"], [4.5 * d[0] ** 2, d[1] - 0.5 / 9, 0.5 - 0.5 / 9], rtol=1e-12)
    np.testing.assert_allclose(r["d_pred"], np.array([9 * d[0], 1, -1]) / 3, rtol=1e-9)
    # weights enter the difference and the gradient once more, and the denominator
    r = ref.vertex_ref(np.array([0.01, 1.0]), np.zeros(2), np.array([10.0, 10.0]), 1.0, mode="f64")
    np.testing.assert_allclose(r["in_loss"], [0.5 * 0.1 ** 2, 10 - 0.5], rtol=1e-6)
    np.testing.assert_allclose(r["d_pred"], np.array([10 * 0.1, 10 * 1.0]) / 20, rtol=1e-6)
