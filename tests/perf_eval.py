"""Measurement of the evaluation ops (csrc/pose_eval.hip).  Warm, on
preallocated tensors, median of --reps with the spread (min, max), two ways:
"call": one HIP event pair around one call of the Python wrapper -- for a
kernel of a few microseconds this is the host's time to validate and launch
(the 4-pixel confusion call is that floor); "graph": 20 calls captured in one
graph, one event pair around a replay, divided by 20 -- the kernels and the
gaps between them, without the host.  The ratios are taken on "graph".
  pose_errors   N = 64 rows, P = 2620 (the dataset's models, C = 22): ADD and
                ADD-S are always both computed, so this is the full cost;
                beside it the wall time of the float64 kd-tree form
                (tests/pose_eval_ref.py: pose_errors64, scipy cKDTree) for
                the same rows on the host
  pose_tally    the same 64 rows, 1000 curve thresholds
  confusion     B = 8, 480 x 640, C = 22: a synth.make_frames label map
                against a shifted copy of itself, and the all-background pair
                (every lane on one counter); beside them a device-to-device
                copy of the same 19.7 MB (gt and pred), the floor of a pass
                that reads them once
No time bar: the ratios are the result.
    python tests/perf_eval.py [--reps 50] [--out profiles/eval_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pose_eval_ref as per  # noqa: E402
from posecnn_amd import evaluate, synth  # noqa: E402
from test_pose_eval_ref import random_pair  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--reps", type=int, default=50)
p.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_bench.json"))
a = p.parse_args()
D = torch.device("cuda")
F = np.float32


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(D)


GRAPH_CALLS = 20


def _events(fn, reps, div):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / div)
    return {"us": round(float(np.median(ts)), 2), "min_us": round(float(np.min(ts)), 2),
            "max_us": round(float(np.max(ts)), 2)}


def timed(fn, reps=a.reps):
    """{"call": {"us": median, "min_us", "max_us"}, "graph": {...}} of fn, warm."""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    call = _events(fn, reps, 1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(GRAPH_CALLS):
            fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    return {"call": call, "graph": _events(g.replay, reps, GRAPH_CALLS)}


mdl = synth.models()
C, N = 22, 64
points = mdl["lov_points"][:C].astype(F)
P = points.shape[1]
num = np.full(C, P, np.int32)
K = mdl["K"].astype(F)
rng = np.random.default_rng(0)
cls = rng.integers(1, C, N).astype(np.int32)
pairs = [random_pair(rng, 10 ** rng.uniform(-4, -1.3), 10 ** rng.uniform(-3, 0)) for _ in range(N)]
rt_e, rt_g = np.stack([q[0] for q in pairs]), np.stack([q[1] for q in pairs])
d_args = [dev(x) for x in (cls, rt_e, rt_g, points, num, K)]
out = torch.empty((N, 5), device=D)
pose = timed(lambda: evaluate.pose_errors(*d_args, out=out))
got = out.cpu().numpy()

t0 = time.perf_counter()
host = np.stack([per.pose_errors64(rt_e[i], rt_g[i], points[cls[i]], K) for i in range(N)])
host_s = time.perf_counter() - t0
worst = np.abs(got.astype(np.float64) - host).max(axis=0)

sym = dev(mdl["lov_symmetry"][:C].astype(F))
thr = dev((0.1 * np.linalg.norm(mdl["lov_extents"][:C], axis=1)).astype(F))
T = 1000
curve = dev(((np.arange(T) + 1.0) * 0.1 / T).astype(F))
counts = [torch.zeros(s, dtype=torch.int64, device=D) for s in ((C,), (C,), (C, T + 1), (C, T + 1))]
tally = timed(lambda: evaluate.pose_tally(out, d_args[0], sym, thr, curve, *counts))

B, H, W = 8, 480, 640
fr = synth.make_frames(B, H, W, num_classes=C, objects_per_image=6, seed=3)
gt = fr["label"].astype(np.int32)
pred = np.roll(gt, 5, axis=2)
both = torch.stack([dev(gt), dev(pred)])
sink = torch.empty_like(both)
hist = torch.zeros((C, C), dtype=torch.int64, device=D)
skipped = torch.zeros((1,), dtype=torch.int64, device=D)
conf = timed(lambda: evaluate.confusion(both[0], both[1], C, hist, skipped))
hist.zero_()
evaluate.confusion(both[0], both[1], C, hist, skipped)
exact = bool(np.array_equal(hist.cpu().numpy(), per.confusion(gt, pred, C)[0]))
zeros = torch.zeros_like(both)
conf_bg = timed(lambda: evaluate.confusion(zeros[0], zeros[1], C, hist, skipped))
copy = timed(lambda: sink.copy_(both))
four = torch.zeros((4,), dtype=torch.int32, device=D)
conf_4px = timed(lambda: evaluate.confusion(four, four, C, hist, skipped))
nbytes = both.numel() * 4

res = {"device": torch.cuda.get_device_name(0),
       "unit": "us (median of %d with min and max, warm; call: one HIP event pair per wrapper call; graph: per call "
               "of a replayed graph of %d calls)" % (a.reps, GRAPH_CALLS),
       "pose_errors": dict(pose, rows=N, P=P, pairs_per_row=P * P),
       "pose_errors_host_kdtree_float64": {"s": round(host_s, 3), "rows": N,
                                           "note": "wall time of pose_errors64 over the same rows, one run"},
       "pose_errors_host_over_device": round(host_s * 1e6 / pose["graph"]["us"], 1),
       "pose_errors_worst_difference_from_float64": [float(x) for x in worst],
       "pose_tally": dict(tally, rows=N, T=T),
       "confusion_frames": dict(conf, pixels=gt.size, bytes=nbytes, exact=exact,
                                background_fraction=round(float((gt == 0).mean()), 4)),
       "confusion_all_background": conf_bg,
       "confusion_4_pixels": conf_4px,
       "copy_d2d_same_bytes": dict(copy, bytes=nbytes, note="reads 19.7 MB and writes 19.7 MB"),
       "confusion_over_copy": round(conf["graph"]["us"] / copy["graph"]["us"], 2),
       "confusion_all_background_over_copy": round(conf_bg["graph"]["us"] / copy["graph"]["us"], 2)}
print(json.dumps(res), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as fh:
    fh.write(json.dumps(res, indent=1) + "\n")
sys.exit(0 if exact else 1)
