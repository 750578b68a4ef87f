"""fc8 fused into the split-K reduces around it (posecnn_amd/csrc/fc8_fused.hip)
against the launches it replaces, bit for bit (torch.equal):

    forward   pcnn_gemm_drop_gen / pcnn_gemm_drop (fc7) -> pcnn_gemm (fc8) ->
              pcnn_pose_head_fwd   vs   pcnn_gemm_partial -> pcnn_fc8_fwd_fused
              -> pcnn_fc8_reduce_head_fwd
    backward  pcnn_gemm_drop(b_trans=1, mask=y7, keep)  vs  pcnn_fc8_dx_skinny

at the flagship's units (4096) and row capacity (1152), D = 88 and 64, with
the device row count at 1, 32, 33 (32-row block edges), 256, 257 (the fc7 plan
goes from 16 to 8 slabs), 405 (the bench's count), 513 and 1152 (the
capacity).  Output buffers are pre-filled with the same pattern on both sides
and compared whole, so rows past the count must be left as the old path
leaves them.  Then one PoseStep step with fuse_fc8 on and off."""
import numpy as np
import pytest
import torch

from posecnn_amd import pose_head as ph
from posecnn_amd import synth
from posecnn_amd.pipeline import PoseStep

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
UNITS, CAP = 4096, 1152
COUNTS = (1, 32, 33, 256, 257, 405, 513, 1152)
SEED, SID = 0x5EED, 7


@pytest.fixture(scope="module")
def fc(hip):
    """Shared, read-only operands: y6 (CAP, UNITS), W7, b7, and per D: W8, b8, poses_weight."""
    g = torch.Generator(device=DEV).manual_seed(17)
    r = lambda *s: torch.randn(s, device=DEV, generator=g)
    d = dict(y6=torch.relu(r(CAP, UNITS)), w7=r(UNITS, UNITS) * 0.02, b7=r(UNITS) * 0.1)
    for D in (64, 88, 132):
        pw = (torch.rand((CAP, D), device=DEV, generator=g) < 0.3).float()
        d[D] = dict(w8=r(UNITS, D) * 0.02, b8=r(D) * 0.1, pw=pw)
    return d


def _same(a, b):
    """torch.equal, and the same bits (+0 / -0 told apart)."""
    bits = lambda x: x.view(torch.int32) if x.dtype == torch.float32 else x
    return torch.equal(a, b) and torch.equal(bits(a), bits(b))


def _outputs(D):
    f = lambda n, v: torch.full((CAP, n), v, dtype=torch.float32, device=DEV)
    return dict(y7=f(UNITS, 3.0), drop=torch.full((CAP, UNITS), 0x55, dtype=torch.uint8, device=DEV), y8=f(D, 5.0),
                t8=f(D, 6.0), pred=f(D, 7.0))


def _forward(fc, D, keep, n, fuse, external=None):
    o = _outputs(D)
    nr = torch.tensor([n], dtype=torch.int32, device=DEV)
    step = torch.tensor([3], dtype=torch.int64, device=DEV)
    kw = {}
    if keep < 1.0:
        if external is not None:
            o["drop"].copy_(external)
            kw = dict(drop=o["drop"], keep_prob=keep)
        else:
            kw = dict(drop=o["drop"], keep_prob=keep, drop_gen=(SEED, step, SID))
    w = fc[D]
    ph.fc7_fc8_head_fwd(fc["y6"], fc["w7"], fc["b7"], o["y7"], w["w8"], w["b8"], o["y8"], w["pw"], o["t8"],
                        o["pred"], M_dev=nr, fuse=fuse, **kw)
    return o


@pytest.mark.parametrize("keep", [0.5, 1.0])
@pytest.mark.parametrize("D", [88, 64])
def test_fc8_forward_chain_bitwise(fc, D, keep):
    assert ph.fc8_fused_ok(UNITS, D)
    for n in COUNTS:
        old = _forward(fc, D, keep, n, fuse=False)
        new = _forward(fc, D, keep, n, fuse=True)
        torch.cuda.synchronize()
        for k in ("y7", "drop", "y8", "t8", "pred"):
            assert _same(old[k], new[k]), (k, D, keep, n)
        if keep < 1.0:  # the draw is a real Bernoulli(keep) mask over the live rows, untouched past them
            live = old["drop"][:n].float().mean().item()
            assert abs(live - keep) < 0.05 and set(old["drop"][:n].unique().tolist()) <= {0, 1}
            assert n == CAP or bool((new["drop"][n:] == 0x55).all())
        assert bool((new["y8"][:n] != 5.0).any()) and (n == CAP or bool((new["pred"][n:] == 7.0).all()))


def test_fc8_forward_chain_external_mask_bitwise(fc):
    """keep bits supplied by the caller (PoseStep.set_drop_masks) rather than drawn."""
    g = torch.Generator(device=DEV).manual_seed(5)
    m = (torch.rand((CAP, UNITS), device=DEV, generator=g) < 0.5).to(torch.uint8)
    for n in (33, 405):
        old = _forward(fc, 88, 0.5, n, fuse=False, external=m)
        new = _forward(fc, 88, 0.5, n, fuse=True, external=m)
        for k in ("y7", "drop", "y8", "t8", "pred"):
            assert _same(old[k], new[k]), (k, n)


def test_fc8_wide_head_takes_the_generic_path(fc):
    """D = 132 > 128: the dispatch keeps today's launches, and the fused entry points refuse the shape."""
    assert not ph.fc8_fused_ok(UNITS, 132)
    old = _forward(fc, 132, 0.5, 405, fuse=False)
    new = _forward(fc, 132, 0.5, 405, fuse=True)
    for k in ("y7", "drop", "y8", "t8", "pred"):
        assert _same(old[k], new[k]), k
    o = _outputs(132)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        ph.fc8_fwd_fused(ws, UNITS, fc["b7"], o["y7"], fc[132]["w8"])
    with pytest.raises(ValueError):
        ph.fc8_reduce_head_fwd(fc[132]["b8"], UNITS, fc[132]["pw"], o["y8"], o["t8"], o["pred"])
    # the backward wrapper falls back by itself
    dy8 = torch.randn((CAP, 132), device=DEV)
    nr = torch.tensor([405], dtype=torch.int32, device=DEV)
    a, b = (torch.full((CAP, UNITS), 2.0, device=DEV) for _ in range(2))
    ph.fc8_dx(dy8, fc[132]["w8"], a, mask=fc["y6"], keep_prob=0.5, M_dev=nr)
    ph.gemm(dy8, fc[132]["w8"], b, b_trans=1, mask=fc["y6"], keep_prob=0.5, M_dev=nr)
    assert _same(a, b)


@pytest.mark.parametrize("keep", [0.5, 1.0])
@pytest.mark.parametrize("D", [88, 64])
def test_fc8_dx_skinny_bitwise(fc, D, keep):
    g = torch.Generator(device=DEV).manual_seed(23)
    dy8 = torch.randn((CAP, D), device=DEV, generator=g)
    dy8[5] = 0.0  # a row of zero gradients (all-zero accumulators)
    # y7 as the forward leaves it: positive values, exact zeros (relu / dropped), and -0.0
    y7 = torch.relu(torch.randn((CAP, UNITS), device=DEV, generator=g))
    y7[torch.rand((CAP, UNITS), device=DEV, generator=g) < 0.1] = -0.0
    assert bool((y7 == 0).any()) and bool(torch.signbit(y7).any())
    for n in COUNTS:
        nr = torch.tensor([n], dtype=torch.int32, device=DEV)
        old, new = (torch.full((CAP, UNITS), 2.0, device=DEV) for _ in range(2))
        ph.gemm(dy8, fc[D]["w8"], old, b_trans=1, mask=y7, keep_prob=keep, M_dev=nr)
        ph.fc8_dx(dy8, fc[D]["w8"], new, mask=y7, keep_prob=keep, M_dev=nr)
        assert _same(old, new), (D, keep, n)
        assert bool((new[:n] != 2.0).any()) and (n == CAP or bool((new[n:] == 2.0).all()))


def test_pose_step_fuse_fc8_is_bitwise_neutral(hip):
    """One PoseStep step at B = 1 with fuse_fc8 on and off: the loss, pred, the
    ADD gradient, every weight / bias gradient and both feature-map gradients."""
    B, H, W, C, CH, UN = 1, 120, 160, 22, 64, 256
    fr = synth.make_frames(B, H=H, W=W, num_classes=C, objects_per_image=4, seed=93)
    g = torch.Generator().manual_seed(9)
    conv4 = torch.randn((B, H // 8, W // 8, CH), generator=g)
    conv5 = torch.randn((B, H // 16, W // 16, CH), generator=g)
    pts, sym = synth.rescaled_points(C)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    inputs = dict(label=t(fr["label"]), vertex=t(fr["vertex"]), extents=t(fr["extents"]), meta=t(fr["meta"]),
                  gt=t(fr["gt"]), conv4=conv4.to(DEV), conv5=conv5.to(DEV), points=t(pts), symmetry=t(sym))
    outs, weights = [], None
    for fuse in (True, False):
        step = PoseStep(B, H, W, C, DEV, channels=CH, units=UN, is_train=1, skip_pixels=3, weights=weights,
                        fuse_fc8=fuse)
        assert step.fuse_fc8 == fuse
        if weights is None:
            weights = step.weights
            for b in (weights.b6, weights.b7, weights.b8):
                b.copy_(torch.randn(b.shape, generator=g) * 1e-3)
        loss = step.step(inputs)
        torch.cuda.synchronize()
        assert int(step.hough["num_rois"][1].item()) > 4
        res = dict(loss=loss, pred=step.pred, diff=step.diff, y7=step.y7, y8=step.y8, drop7=step.drop7,
                   dy7=step.dy7, dx=step.dx, dconv4=step.dconv4, dconv5=step.dconv5)
        res.update({"g_" + k: v for k, v in step.grads.items()})
        outs.append({k: v.clone() for k, v in res.items()})
    for k in outs[0]:
        assert _same(outs[0][k], outs[1][k]), k
    assert bool(outs[0]["dconv4"].any()) and bool(outs[0]["g_w7"].any())
