"""The segmentation and vertex losses on the GPU against tests/seg_loss_ref.py.

Tolerances of the segmentation op are measured, not chosen: E_ref = max |f32
mode - f64 mode| of the reference is the error float32 arithmetic makes on the
input, and the device must stay within 4 x E_ref of the f64 mode (OCML's and
numpy's expf / logf may each differ by an ulp, and the maxima are taken over
different roundings).  With C = 1 every output is exact in both modes
(log_prob = 0, prob = 1, no hard pixel): E_ref is 0 there and the device must
match exactly; everywhere else E_ref > 0 is asserted.  Scores lie on a grid of
1/8 with exact ties, so label_2d and the hard mask are unambiguous and are
compared exactly.  The vertex ops have no transcendentals: gradients are
compared bit for bit and losses (double sums rounded once) to one float32 ulp.
"""
import functools

import numpy as np
import pytest
import torch

import seg_loss_ref as ref

pytestmark = pytest.mark.gpu

SEG_SHAPES = [(2, 48, 64, 22), (1, 7, 9, 3), (3, 33, 65, 16), (1, 17, 19, 130), (2, 5, 13, 1)]
THRESHOLDS = [1.0, 0.5]
VERTEX_SHAPES = [(2, 48, 64, 22), (1, 7, 9, 3), (1, 5, 13, 2)]
FLOAT_OUTPUTS = ("log_prob", "prob_normalized", "d_score")
ALL = ("log_prob", "prob_normalized", "label_2d", "gt_label_weight", "d_score")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def ulp(x):
    return float(np.spacing(np.abs(np.float32(x))))


# ---------------------------------------------------------------------------
# segmentation inputs and references, built once per (shape, threshold); read-only

@functools.lru_cache(maxsize=None)
def seg_case(shape, threshold):
    B, H, W, C = shape
    rng = np.random.default_rng(1000 * sum(shape) + int(10 * threshold))
    score = (rng.integers(-32, 33, size=shape) / 8).astype(np.float32)
    if C > 1:  # an exact tie for the maximum on one pixel in ten
        tie = rng.random((B, H, W)) < 0.1
        other = rng.integers(0, C, size=(B, H, W))
        top = score.max(axis=-1)
        idx = np.nonzero(tie)
        score[idx + (other[idx],)] = top[idx]
    gt = rng.integers(-1, C, size=(B, H, W)).astype(np.int32)
    flat = gt.reshape(-1)
    flat[rng.choice(flat.size, 4, replace=False)] = [C, C + 5, -2, -100]
    score[0, 0, 0, :] = 0   # p_0 == 1.0f exactly: not hard at threshold 1.0
    score[0, 0, 0, 0] = 100
    gt[0, 0, 0] = 0
    if threshold < 1.0:  # keep background pixels off the threshold
        p0 = ref.seg_ref(score, gt, threshold, mode="f64")["prob_normalized"][..., 0]
        near = (gt == 0) & (np.abs(p0 - threshold) < 1e-4)
        score[near, 0] += 1
    r64 = ref.seg_ref(score, gt, threshold, mode="f64")
    r32 = ref.seg_ref(score, gt, threshold, mode="f32")
    if threshold < 1.0:  # no pixel was left on it, so no case is left out
        assert not ((gt == 0) & (np.abs(r64["prob_normalized"][..., 0] - threshold) < 1e-4)).any()
    return score, gt, r32, r64


@functools.lru_cache(maxsize=None)
def seg_device(shape, threshold):
    from posecnn_amd.losses import seg_loss
    score, gt, _, _ = seg_case(shape, threshold)
    loss, out = seg_loss(dev(score), dev(gt), threshold, want=ALL)
    return loss, out


@pytest.mark.parametrize("threshold", THRESHOLDS)
@pytest.mark.parametrize("shape", SEG_SHAPES)
def test_seg_loss_against_the_reference(hip, shape, threshold):
    score, gt, r32, r64 = seg_case(shape, threshold)
    C = shape[3]
    loss, out = seg_device(shape, threshold)
    np.testing.assert_array_equal(r32["label_2d"], r64["label_2d"])
    np.testing.assert_array_equal(r32["hard"], r64["hard"])
    np.testing.assert_array_equal(host(out["label_2d"]), r64["label_2d"])
    np.testing.assert_array_equal(host(out["gt_label_weight"]), r64["gt_label_weight"])
    assert not host(out["d_score"])[~r64["hard"]].any()
    valid = (gt >= 0) & (gt < C)
    assert not r64["hard"][0, 0, 0] and r64["prob_normalized"][0, 0, 0, 0] == 1.0
    assert host(out["prob_normalized"])[0, 0, 0, 0] == np.float32(1.0)
    if threshold == 1.0 and C > 1:  # every other pixel with an in-range label is hard
        expect = valid.copy()
        expect[0, 0, 0] = False
        np.testing.assert_array_equal(r64["hard"], expect)
    got = {k: host(out[k]).astype(np.float64) for k in FLOAT_OUTPUTS}
    got["loss"] = np.float64(loss.item())
    for k in FLOAT_OUTPUTS + ("loss",):
        e_ref = float(np.max(np.abs(np.asarray(r32[k], np.float64) - r64[k])))
        err = float(np.max(np.abs(got[k] - r64[k])))
        print(f"{shape} thr {threshold} {k}: E_ref {e_ref:.3e} device {err:.3e} ratio {err / e_ref if e_ref else 0:.3f}")
        assert np.isfinite(got[k]).all()
        if C > 1:
            assert e_ref > 0
        else:
            assert e_ref == 0
        assert err <= 4 * e_ref, k


def test_seg_loss_ignored_pixels(hip):
    from posecnn_amd.losses import seg_loss
    score = seg_case(SEG_SHAPES[0], 1.0)[0]
    loss, out = seg_loss(dev(score), torch.full(score.shape[:3], -1, dtype=torch.int32, device="cuda"), 1.0,
                         want=("d_score", "gt_label_weight"))
    assert loss.item() == 0.0
    assert not host(out["d_score"]).any() and np.isfinite(host(out["d_score"])).all()
    assert not host(out["gt_label_weight"]).any()


def test_seg_loss_grad_scale(hip):
    from posecnn_amd.losses import seg_loss
    shape = SEG_SHAPES[2]
    score, gt, _, _ = seg_case(shape, 1.0)
    loss1, out1 = seg_device(shape, 1.0)
    loss2, out2 = seg_loss(dev(score), dev(gt), 1.0, want=("d_score",), grad_scale=2.5)
    assert bits(host(loss1)) == bits(host(loss2))
    # five roundings apart (two products, two factors, the 2.5 x here): 5 * 2^-24 relative
    np.testing.assert_allclose(host(out2["d_score"]), 2.5 * host(out1["d_score"]), rtol=2.0 ** -21, atol=1e-30)
    assert host(out2["d_score"]).any()


@pytest.mark.parametrize("shape", [SEG_SHAPES[2], SEG_SHAPES[3]])
def test_seg_loss_outputs_alone_and_twice(hip, shape):
    from posecnn_amd.losses import seg_loss
    score, gt, _, _ = seg_case(shape, 0.5)
    loss, out = seg_device(shape, 0.5)
    s, g = dev(score), dev(gt)
    for k in ALL:
        l1, o1 = seg_loss(s, g, 0.5, want=(k,))
        assert list(o1) == [k] and torch.equal(o1[k], out[k]), k
        assert torch.equal(l1, loss)
    l0, o0 = seg_loss(s, g, 0.5, want=())
    assert o0 == {} and torch.equal(l0, loss)
    l2, o2 = seg_loss(s, g, 0.5, want=ALL)
    assert torch.equal(l2, loss)
    for k in ALL:
        assert np.array_equal(host(o2[k]).view(np.int32), host(out[k]).view(np.int32)), k


@pytest.mark.parametrize("shape", [SEG_SHAPES[0], SEG_SHAPES[3], SEG_SHAPES[4]])
def test_softmax_maps_and_cross_entropy(hip, shape):
    from posecnn_amd import losses
    from posecnn_amd.label_2d import argmax_2d
    from posecnn_amd.hard_label_layer.hard_label_op import hard_label
    score, gt, _, _ = seg_case(shape, 1.0)
    loss, out = seg_device(shape, 1.0)
    s = dev(score)
    prob = losses.softmax_high_dimension(s)
    assert torch.equal(prob, out["prob_normalized"])
    assert torch.equal(losses.log_softmax_high_dimension(s), out["log_prob"])
    assert torch.equal(argmax_2d(prob), out["label_2d"])
    assert torch.equal(hard_label(prob, dev(gt), 1.0), out["gt_label_weight"])
    ce = losses.loss_cross_entropy_single_frame(out["log_prob"], out["gt_label_weight"])
    print(shape, "seg loss", loss.item(), "cross entropy", ce.item())
    # both round a double sum whose relative error is bounded by n * 2^-53
    assert abs(ce.item() - loss.item()) <= ulp(loss.item())
    ce2, d = losses.loss_cross_entropy_single_frame(out["log_prob"], out["gt_label_weight"], want_grad=True,
                                                    grad_scale=2.0)
    assert torch.equal(ce2, ce)
    r_loss, r_d = ref.cross_entropy_ref(host(out["log_prob"]), host(out["gt_label_weight"]), 2.0)
    assert abs(ce.item() - float(r_loss)) <= ulp(r_loss)
    np.testing.assert_array_equal(bits(host(d)), bits(r_d))


def test_segmentation_loss_module(hip):
    from posecnn_amd.losses import seg_loss
    from posecnn_amd.pth import SegmentationLoss
    shape = SEG_SHAPES[2]
    score, gt, _, _ = seg_case(shape, 1.0)
    loss0, out0 = seg_device(shape, 1.0)
    s = dev(score).requires_grad_(True)
    loss, label = SegmentationLoss(1.0)(s, dev(gt))
    assert loss.dim() == 0 and torch.equal(loss.detach(), loss0) and torch.equal(label, out0["label_2d"])
    (3 * loss).backward()
    _, want = seg_loss(dev(score), dev(gt), 1.0, want=("d_score",), grad_scale=3.0)
    assert torch.equal(s.grad, want["d_score"]) and s.grad.abs().max().item() > 0


def test_seg_wrapper_validation(hip):
    from posecnn_amd import losses
    from posecnn_amd.pth import SegmentationLoss
    shape = SEG_SHAPES[1]
    score, gt, _, _ = seg_case(shape, 1.0)
    loss0, out0 = seg_device(shape, 1.0)
    s, g = dev(score), dev(gt)
    with pytest.raises(ValueError):
        losses.seg_loss(s, g[:, :-1], 1.0)
    with pytest.raises(ValueError):
        losses.seg_loss(s[0], g, 1.0)
    with pytest.raises(ValueError):
        losses.seg_loss(s, g, 0.0)
    with pytest.raises(ValueError):
        losses.seg_loss(s, g, -1.0)
    with pytest.raises(ValueError):
        losses.seg_loss(s, g, 1.0, want=("logits",))
    with pytest.raises(ValueError):
        SegmentationLoss(0.0)
    with pytest.raises(ValueError):
        losses.loss_cross_entropy_single_frame(s, s[..., :-1])
    # float64, int64 and non-contiguous inputs: the results of their float32 / int32 contiguous copies
    nchw = s.permute(0, 3, 1, 2).contiguous()
    for sv, gv in ((s.double(), g.long()), (nchw.permute(0, 2, 3, 1), g)):
        assert not (sv.is_contiguous() and sv.dtype == torch.float32)
        loss, out = losses.seg_loss(sv, gv, 1.0, want=ALL)
        assert torch.equal(loss, loss0)
        for k in ALL:
            assert torch.equal(out[k], out0[k]), k


# ---------------------------------------------------------------------------
# vertex losses

@functools.lru_cache(maxsize=None)
def vertex_case(shape, sigma, w_inside):
    """Host inputs: label, vertex3, the blob pair (numpy restatement of the
    expand op, compared with the op in the test), pred (B,H,W,3C)."""
    from scene_ref import expand_ref
    B, H, W, C = shape
    rng = np.random.default_rng(7 * sum(shape) + int(10 * sigma) + int(100 * w_inside))
    label = rng.integers(0, C, size=(B, H, W)).astype(np.int32)
    flat = label.reshape(-1)
    flat[rng.choice(flat.size, 5, replace=False)] = [0, -1, C, C + 3, -9]
    vertex3 = rng.standard_normal((B, H, W, 3)).astype(np.float32)
    tgt, wt = expand_ref(label, vertex3, C, w_inside)
    # |w * noise| up to twice the branch point 1 / sigma^2, and exactly 0 on one element in ten
    noise = rng.uniform(-1, 1, size=tgt.shape) * 2.0 / (sigma * sigma * w_inside)
    noise[rng.random(tgt.shape) < 0.1] = 0
    pred = (tgt + noise).astype(np.float32)
    return label, vertex3, tgt, wt, pred


def gather3(dense, label, C):
    """(B,H,W,3C) -> (B,H,W,3) at the label's channels, 0 where the label is outside [1, C)."""
    on = (label >= 1) & (label < C)
    idx = 3 * np.where(on, label, 0)[..., None] + np.arange(3)
    return np.where(on[..., None], np.take_along_axis(dense, idx, axis=-1), np.float32(0))


@pytest.mark.parametrize("w_inside", [10.0, 2.5])
@pytest.mark.parametrize("sigma", [1.0, 3.0])
@pytest.mark.parametrize("shape", VERTEX_SHAPES)
def test_vertex_losses(hip, shape, sigma, w_inside):
    from posecnn_amd import losses
    from posecnn_amd.synthesize.scene import expand
    C = shape[3]
    label, vertex3, tgt, wt, pred = vertex_case(shape, sigma, w_inside)
    d_label, d_v3, d_pred_in = dev(label), dev(vertex3), dev(pred)
    d_tgt, d_wt = expand(d_label, d_v3, C, w_inside)
    np.testing.assert_array_equal(host(d_tgt), tgt)
    np.testing.assert_array_equal(host(d_wt), wt)
    r = ref.vertex_ref(pred, tgt, wt, sigma, 1.5)
    live = wt > 0
    assert (r["near"] & live & (r["diff"] != 0)).any() and (~r["near"]).any() and ((r["diff"] == 0) & live).any()
    assert live.any() and (~live).any()

    # dense op
    loss, d = losses.smooth_l1_loss_vertex(d_pred_in, d_tgt, d_wt, sigma, want_grad=True, grad_scale=1.5)
    print(shape, sigma, w_inside, "loss", loss.item(), "reference", float(r["loss"]))
    np.testing.assert_array_equal(bits(host(d)), bits(r["d_pred"]))
    assert abs(loss.item() - float(r["loss"])) <= ulp(r["loss"])
    assert torch.equal(losses.smooth_l1_loss_vertex(d_pred_in, d_tgt, d_wt, sigma), loss)

    # compact op: every combination of the prediction's and the gradient's layout
    dense_d = host(d)
    pred3 = dev(gather3(pred, label, C))
    for p in (d_pred_in, pred3):
        for dense_grad in (True, False):
            lc, dc = losses.vertex_loss_compact(p, d_label, d_v3, C, w_inside, sigma, dense_grad=dense_grad,
                                                want_grad=True, grad_scale=1.5)
            assert abs(lc.item() - loss.item()) <= ulp(loss.item())
            if dense_grad:
                assert dc.shape == d.shape
                np.testing.assert_array_equal(host(dc), dense_d)
                np.testing.assert_array_equal(bits(host(dc))[live], bits(dense_d)[live])
            else:
                assert dc.shape == (*label.shape, 3)
                np.testing.assert_array_equal(bits(host(dc)), bits(gather3(dense_d, label, C)))
            assert torch.equal(losses.vertex_loss_compact(p, d_label, d_v3, C, w_inside, sigma), lc)


def test_vertex_all_background(hip):
    from posecnn_amd import losses
    from posecnn_amd.synthesize.scene import expand
    shape = VERTEX_SHAPES[1]
    C = shape[3]
    _, vertex3, _, _, pred = vertex_case(shape, 1.0, 10.0)
    label = torch.zeros(shape[:3], dtype=torch.int32, device="cuda")
    tgt, wt = expand(label, dev(vertex3), C, 10.0)
    loss, d = losses.smooth_l1_loss_vertex(dev(pred), tgt, wt, 1.0, want_grad=True)
    assert loss.item() == 0.0 and not host(d).any() and np.isfinite(host(d)).all()
    for dense_grad in (True, False):
        loss, d = losses.vertex_loss_compact(dev(pred), label, dev(vertex3), C, 10.0, 1.0, dense_grad=dense_grad,
                                             want_grad=True)
        assert loss.item() == 0.0 and not host(d).any() and np.isfinite(host(d)).all()


def test_vertex_loss_module(hip):
    from posecnn_amd import losses
    from posecnn_amd.pth import VertexLoss
    shape = VERTEX_SHAPES[0]
    C = shape[3]
    label, vertex3, tgt, wt, pred = vertex_case(shape, 3.0, 2.5)
    mod = VertexLoss(sigma=3.0, w_inside=2.5)
    _, want = losses.smooth_l1_loss_vertex(dev(pred), dev(tgt), dev(wt), 3.0, want_grad=True, grad_scale=3.0)
    p = dev(pred).requires_grad_(True)
    loss = mod(p, dev(tgt), dev(wt))
    assert loss.dim() == 0
    (3 * loss).backward()
    assert torch.equal(p.grad, want) and p.grad.abs().max().item() > 0
    # the compact ground truth, dense and 3-channel predictions
    p = dev(pred).requires_grad_(True)
    lc = mod(p, dev(label), dev(vertex3))
    assert abs(lc.item() - loss.item()) <= ulp(loss.item())
    (3 * lc).backward()
    assert torch.equal(p.grad, want)
    p3 = dev(gather3(pred, label, C)).requires_grad_(True)
    with pytest.raises(ValueError):
        mod(p3, dev(label), dev(vertex3))
    l3 = VertexLoss(sigma=3.0, w_inside=2.5, num_classes=C)(p3, dev(label), dev(vertex3))
    (3 * l3).backward()
    np.testing.assert_array_equal(bits(host(p3.grad)), bits(gather3(host(want), label, C)))


def test_vertex_wrapper_validation(hip):
    from posecnn_amd import losses
    from posecnn_amd.pth import VertexLoss
    shape = VERTEX_SHAPES[2]
    C = shape[3]
    label, vertex3, tgt, wt, pred = vertex_case(shape, 1.0, 10.0)
    p, t, w, lb, v3 = dev(pred), dev(tgt), dev(wt), dev(label), dev(vertex3)
    with pytest.raises(ValueError):
        losses.smooth_l1_loss_vertex(p, t[..., :-1], w)
    with pytest.raises(ValueError):
        losses.smooth_l1_loss_vertex(p, t, w, 0.0)
    with pytest.raises(ValueError):
        losses.vertex_loss_compact(p, lb, v3, C, 10.0, -1.0)
    with pytest.raises(ValueError):
        losses.vertex_loss_compact(p[..., :-1], lb, v3, C, 10.0)
    with pytest.raises(ValueError):
        losses.vertex_loss_compact(p, lb, v3[..., :2], C, 10.0)
    with pytest.raises(ValueError):
        VertexLoss(sigma=0.0)
    loss0, d0 = losses.smooth_l1_loss_vertex(p, t, w, 1.0, want_grad=True)
    lc0, dc0 = losses.vertex_loss_compact(p, lb, v3, C, 10.0, want_grad=True)
    # float64 / int64 / non-contiguous inputs: the results of their float32 / int32 contiguous copies
    pt = p.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    assert not pt.is_contiguous()
    for pv in (p.double(), pt):
        loss, d = losses.smooth_l1_loss_vertex(pv, t.double(), w, 1.0, want_grad=True)
        assert torch.equal(loss, loss0) and torch.equal(d, d0)
        lc, dc = losses.vertex_loss_compact(pv, lb.long(), v3.double(), C, 10.0, want_grad=True)
        assert torch.equal(lc, lc0) and torch.equal(dc, dc0)
