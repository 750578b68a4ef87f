"""Segmentation / vertex loss microbench at the bench size (B=8, 640x480, C=22):
each op of posecnn_amd.losses next to the same formulas composed from torch's
own device ops on the same tensors (the only baseline: no earlier version of
these ops exists).  One pair of HIP events per run on the launch stream;
median, p10 and p90 over --iters runs after --warmup; bytes are what the
algorithm has to move, computed from the shapes, over the median time.
    python scripts/seg_loss_bench.py [--iters 100] [--warmup 10] [--out FILE]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from posecnn_amd import losses  # noqa: E402
from posecnn_amd.synthesize.scene import expand  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--iters", type=int, default=100)
p.add_argument("--warmup", type=int, default=10)
p.add_argument("--batch", type=int, default=8)
p.add_argument("--out", default=None)
a = p.parse_args()
D = torch.device("cuda")
B, H, W, C = a.batch, 480, 640, 22
THR, SIGMA, W_IN, GS = 1.0, 1.0, 10.0, 1.0
g = torch.Generator(device=D).manual_seed(1)
n_pix = B * H * W

# a frame-like ground truth: 70 % background, the rest spread over the classes
gt = torch.randint(1, C, (B, H, W), generator=g, device=D, dtype=torch.int32)
gt[torch.rand((B, H, W), generator=g, device=D) < 0.7] = 0
score = torch.randn((B, H, W, C), generator=g, device=D)
score.scatter_add_(3, gt.long().unsqueeze(3), torch.full((B, H, W, 1), 2.0, device=D))
vertex3 = torch.randn((B, H, W, 3), generator=g, device=D)
tgt, wt = expand(gt, vertex3, C, W_IN)
pred = tgt + torch.randn(tgt.shape, generator=g, device=D) * (1.0 / W_IN)
pred3 = torch.gather(pred, 3, (3 * gt.long()).unsqueeze(3) + torch.arange(3, device=D)).contiguous()


def torch_seg(want_grad):
    lp = torch.log_softmax(score, 3)
    prob = torch.softmax(score, 3)
    label = prob.argmax(3).int()
    hard = (gt >= 0) & (gt < C) & ((gt > 0) | (prob[..., 0] < THR))
    w = ((torch.arange(C, device=D) == gt.unsqueeze(3)) & hard.unsqueeze(3)).float()
    n = w.sum()
    loss = -(lp * w).sum() / (n + 1e-10)
    d = (prob - w) * hard.unsqueeze(3) * (GS / (n + 1e-10)) if want_grad else None
    return loss, label, d


def torch_ce(lp, w):
    return -(lp * w).sum() / (w.sum() + 1e-10)


def torch_vertex(want_grad):
    s2 = SIGMA * SIGMA
    diff = wt * (pred - tgt)
    ab = diff.abs()
    near = ab < 1.0 / s2
    wsum = wt.sum()
    loss = torch.where(near, diff * diff * (s2 / 2), ab - 0.5 / s2).sum() / (wsum + 1e-10)
    d = wt * torch.where(near, diff * s2, diff.sign()) * (GS / (wsum + 1e-10)) if want_grad else None
    return loss, d


def timeit(fn):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    t = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)
    return {"median_us": t[len(t) // 2], "p10_us": t[len(t) // 10], "p90_us": t[(9 * len(t)) // 10]}


MAP, V = n_pix * C * 4, n_pix * 3 * C * 4          # the score map and one vertex blob, bytes
PX = n_pix * 4
LIVE = int((gt > 0).sum().item())                  # pixels on an object: the only ones whose prediction is read
# bytes the two-pass structure moves (include/posecnn_hip.h): reads + writes
BYTES = {
    "seg_fwd": MAP + PX + PX + 2 * PX,                              # score, gt -> label_2d, (m, s)
    "seg_fwd_bwd": 2 * MAP + 2 * PX + PX + 4 * PX + MAP,            # + score, gt, (m, s) -> d_score
    "seg_all_outputs": 3 * MAP + 2 * PX + PX + 4 * PX + 4 * MAP,    # + log_prob (score read again), prob, weight
    "cross_entropy": 2 * MAP,
    "vertex_dense_fwd": 3 * V,
    "vertex_dense_fwd_bwd": V + 3 * V + V,                          # weights; pred, targets, weights -> d_pred
    # label, vertex3 and, per labelled pixel, one 64-byte sector of the 3C-channel map
    "vertex_compact_fwd_pred3C": PX + 3 * PX + LIVE * 64,
    "vertex_compact_fwd_bwd_pred3C": 2 * (PX + 3 * PX + LIVE * 64) + V + LIVE * 64,   # + the zero fill and the scatter
    "vertex_compact_fwd_pred3": PX + 3 * PX + 3 * PX,
    "vertex_compact_fwd_bwd_pred3": 2 * (PX + 3 * PX + 3 * PX) + 3 * PX,
}
lp_w = losses.seg_loss(score, gt, THR, want=("log_prob", "gt_label_weight"))[1]
OPS = {
    "seg_fwd": (lambda: losses.seg_loss(score, gt, THR, want=("label_2d",)), lambda: torch_seg(False)),
    "seg_fwd_bwd": (lambda: losses.seg_loss(score, gt, THR, want=("label_2d", "d_score"), grad_scale=GS),
                    lambda: torch_seg(True)),
    "seg_all_outputs": (lambda: losses.seg_loss(score, gt, THR, want=losses.SEG_OUTPUTS), None),
    "cross_entropy": (lambda: losses.loss_cross_entropy_single_frame(lp_w["log_prob"], lp_w["gt_label_weight"]),
                      lambda: torch_ce(lp_w["log_prob"], lp_w["gt_label_weight"])),
    "vertex_dense_fwd": (lambda: losses.smooth_l1_loss_vertex(pred, tgt, wt, SIGMA), lambda: torch_vertex(False)),
    "vertex_dense_fwd_bwd": (lambda: losses.smooth_l1_loss_vertex(pred, tgt, wt, SIGMA, want_grad=True,
                                                                  grad_scale=GS), lambda: torch_vertex(True)),
    "vertex_compact_fwd_pred3C": (lambda: losses.vertex_loss_compact(pred, gt, vertex3, C, W_IN, SIGMA), None),
    "vertex_compact_fwd_bwd_pred3C": (lambda: losses.vertex_loss_compact(pred, gt, vertex3, C, W_IN, SIGMA,
                                                                         dense_grad=True, want_grad=True), None),
    "vertex_compact_fwd_pred3": (lambda: losses.vertex_loss_compact(pred3, gt, vertex3, C, W_IN, SIGMA), None),
    "vertex_compact_fwd_bwd_pred3": (lambda: losses.vertex_loss_compact(pred3, gt, vertex3, C, W_IN, SIGMA,
                                                                        want_grad=True), None),
}

# the two sides compute the same thing
l_seg, o_seg = losses.seg_loss(score, gt, THR, want=("label_2d", "d_score"), grad_scale=GS)
t_loss, t_label, t_d = torch_seg(True)
assert abs(l_seg.item() - t_loss.item()) <= 1e-5 * abs(t_loss.item())
assert (o_seg["label_2d"] != t_label).float().mean().item() < 1e-4  # near-ties may round apart
assert (o_seg["d_score"] - t_d).abs().max().item() <= 1e-5 * t_d.abs().max().item()
l_v, d_v = losses.smooth_l1_loss_vertex(pred, tgt, wt, SIGMA, want_grad=True, grad_scale=GS)
t_lv, t_dv = torch_vertex(True)
assert abs(l_v.item() - t_lv.item()) <= 1e-5 * abs(t_lv.item())
assert (d_v - t_dv).abs().max().item() <= 1e-5 * t_dv.abs().max().item()
del t_d, t_dv, d_v, o_seg, t_label

res = {"shape": [B, H, W, C], "labelled_pixels": LIVE, "iters": a.iters, "device": torch.cuda.get_device_name(0), "ops": {}}
for name, (ours, theirs) in OPS.items():
    r = {"bytes": BYTES[name], "hip": timeit(ours)}
    r["hip"]["TBps"] = BYTES[name] / (r["hip"]["median_us"] * 1e-6) / 1e12
    if theirs is not None:
        r["torch"] = timeit(theirs)
        r["speedup"] = r["torch"]["median_us"] / r["hip"]["median_us"]
    res["ops"][name] = r
    print(name, json.dumps(r), flush=True)
line = json.dumps(res)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
print(line, flush=True)
