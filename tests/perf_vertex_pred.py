"""Measurement of the class-compact vertex_pred backward
(csrc/vertex_pred_bwd.hip) at the workload's size: B = 8 frames of 640x480,
K = 128 features, C = 22 classes; labels and vote targets from
make_scene_frames scenes (boxes of the LOV extents), the gradient from
vertex_loss_compact on the compact forward's output.  Warm, by HIP events,
median of --reps:
  compact_*_us   pcnn_vertex_pred_compact_bwd on preallocated outputs: all
                 three gradients, and each alone
  dense_*_us     what a user does without it: torch's backward of the dense
                 (N,128) x (128,66) layer from the dense (B,H,W,66) gradient of
                 vertex_loss_compact(..., dense_grad=True): d_feat = g W^T,
                 d_weights = x^T g, d_bias = column sums of g
  loss_grad_*_us the loss gradient in the compact and in the dense format
  copy_*         device-to-device copies of each pass's algorithmic bytes
                 (read once and written once: 2 x bytes moved), buffers taken
                 in turn so that they do not stay in the last-level cache
One JSON object, printed and written to --out.
    python tests/perf_vertex_pred.py [--reps 30] [--out profiles/vertex_pred_bwd.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from posecnn_amd import _lib, losses, synth  # noqa: E402
from posecnn_amd.synthesize import SceneRenderer, make_scene_frames  # noqa: E402
from posecnn_amd.vertex_pred import vertex_pred_compact  # noqa: E402
from refine_scene import CAMERA  # noqa: E402
from render_ref import box_mesh  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--reps", type=int, default=30)
p.add_argument("--out", default=os.path.join(ROOT, "profiles", "vertex_pred_bwd.json"))
a = p.parse_args()
D = torch.device("cuda")
B, H, W, K, C = 8, 480, 640, 128, 22
N = B * H * W


def median_us(fn, reps=a.reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return round(float(np.median(ts)), 1)


ext = synth.models()["lov_extents"][:C]
meshes = {c: box_mesh(ext[c] / 2) for c in range(1, C)}
frames = make_scene_frames(SceneRenderer(meshes, H, W, CAMERA, device=D), B, seed=0, num_classes=C)
label, vertex3 = frames["label"], frames["vertex3"]
gen = torch.Generator(device=D).manual_seed(0)
feat = torch.randn((B, H, W, K), device=D, generator=gen)
wts = torch.randn((K, 3 * C), device=D, generator=gen) * 0.05
bias = torch.randn((3 * C,), device=D, generator=gen)
pred3 = vertex_pred_compact(feat, wts, bias, label)
_, g3 = losses.vertex_loss_compact(pred3, label, vertex3, C, 10.0, want_grad=True)
_, g_dense = losses.vertex_loss_compact(pred3, label, vertex3, C, 10.0, want_grad=True, dense_grad=True)
live = (label >= 0) & (label < C)
summed = live & (g3 != 0).any(dim=-1)   # the pixels whose feat rows the sums read
n_summed = int(summed.sum())

lib = _lib.load()
P = lib.pcnn_vertex_pred_compact_bwd_partials(B, H, W, K, C)
ws = torch.empty(lib.pcnn_vertex_pred_compact_bwd_workspace_size(B, H, W, K, C), dtype=torch.uint8, device=D)
d_feat = torch.empty((B, H, W, K), device=D)
d_w = torch.empty((K, 3 * C), device=D)
d_b = torch.empty((3 * C,), device=D)


def compact(want_f, want_w, want_b):
    rc = lib.pcnn_vertex_pred_compact_bwd(_lib.ptr(feat), _lib.ptr(wts), _lib.ptr(label), _lib.ptr(g3), B, H, W, K, C,
                                          _lib.ptr(d_feat if want_f else None), _lib.ptr(d_w if want_w else None),
                                          _lib.ptr(d_b if want_b else None), _lib.ptr(ws), ws.numel(),
                                          _lib.stream_ptr())
    assert rc == 0, rc


x2, g2 = feat.view(N, K), g_dense.view(N, 3 * C)
dense = {"feat": lambda: g2 @ wts.t(), "weights": lambda: x2.t() @ g2, "bias": lambda: g2.sum(0)}


def dense_all():
    return [f() for f in dense.values()]


# same results first (reordered float32 sums: compared against the magnitudes summed)
compact(True, True, True)
t_f, t_w, t_b = dense_all()
scale_w = (x2.abs().t() @ g2.abs()).clamp_min(1e-30)
agree = {"d_feat_max_abs_diff": float((d_feat.view(N, K) - t_f).abs().max()),
         "d_weights_max_diff_over_sum_abs": float(((d_w - t_w).abs() / scale_w).max()),
         "d_bias_max_abs_diff": float((d_b - t_b).abs().max())}

# algorithmic bytes: label + gradient in (16 B/px) for every pass; d_feat writes K floats per pixel; the sums read
# the summed pixels' feat rows, write each partial once and read it back once
scan = 16 * N
part_bytes = 2 * P * 3 * C * (K + 1) * 4
bytes_feat = scan + 4 * N * K
bytes_w = scan + 4 * K * n_summed + part_bytes
bytes_b = scan + 2 * P * 3 * C * 4


def copy_rate(nbytes):
    """(us, GB/s) of a device-to-device copy that reads nbytes / 2 and writes nbytes / 2."""
    half = max(nbytes // 2, 1)
    n_pairs = max(2, -(-(1 << 30) // half))   # at least 1 GiB of sources between two uses of a buffer
    pairs = [(torch.empty(half, dtype=torch.uint8, device=D), torch.empty(half, dtype=torch.uint8, device=D))
             for _ in range(min(n_pairs, 64))]
    turn = [0]

    def cp():
        s, d = pairs[turn[0] % len(pairs)]
        turn[0] += 1
        d.copy_(s)
    us = median_us(cp)
    return us, round(2 * half / (us * 1e-6) / 1e9, 1)


res = {"metric": f"pcnn_vertex_pred_compact_bwd, B = {B}, {W}x{H}, K = {K}, C = {C}, make_scene_frames labels",
       "unit": "us (median of %d, HIP events, warm)" % a.reps, "device": torch.cuda.get_device_name(0),
       "pixels": N, "live_pixels": int(live.sum()), "summed_pixels": n_summed, "partials": P,
       "compact_all_us": median_us(lambda: compact(True, True, True)),
       "compact_d_feat_us": median_us(lambda: compact(True, False, False)),
       "compact_d_weights_us": median_us(lambda: compact(False, True, False)),
       "compact_d_bias_us": median_us(lambda: compact(False, False, True)),
       "dense_all_us": median_us(dense_all),
       "dense_d_feat_us": median_us(dense["feat"]),
       "dense_d_weights_us": median_us(dense["weights"]),
       "dense_d_bias_us": median_us(dense["bias"]),
       "loss_grad_compact_us": median_us(lambda: losses.vertex_loss_compact(pred3, label, vertex3, C, 10.0,
                                                                            want_grad=True)),
       "loss_grad_dense_us": median_us(lambda: losses.vertex_loss_compact(pred3, label, vertex3, C, 10.0,
                                                                          want_grad=True, dense_grad=True)),
       "agreement_with_dense": agree}
for name, nbytes in (("d_feat", bytes_feat), ("d_weights", bytes_w)):
    us, rate = copy_rate(nbytes)
    own = nbytes / (res[f"compact_{name}_us"] * 1e-6) / 1e9
    res[f"{name}_bytes"] = nbytes
    res[f"copy_{name}_us"], res[f"copy_{name}_GBps"] = us, rate
    res[f"compact_{name}_GBps"] = round(own, 1)
    res[f"compact_{name}_share_of_copy_rate"] = round(own / rate, 3)
res["d_bias_bytes"] = bytes_b
res["speedup_all"] = round(res["dense_all_us"] / res["compact_all_us"], 2)
res["speedup_with_loss_grad"] = round((res["dense_all_us"] + res["loss_grad_dense_us"]) /
                                      (res["compact_all_us"] + res["loss_grad_compact_us"]), 2)
res["note"] = ("bytes are the algorithm's: 16 B/px of label and gradient, 4K B/px written for d_feat, the summed "
               "pixels' feat rows plus the partials written and read once for d_weights; a copy of n bytes reads "
               "n/2 and writes n/2")
print(json.dumps(res), flush=True)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as fh:
    fh.write(json.dumps(res, indent=1) + "\n")
