"""Measurement of the mesh rasteriser (csrc/render.hip): MeshRenderer.render_many
for K poses at 640x480 on an icosphere of level 5 (20 480 faces, small
triangles) and on the box of tests/refine_scene.py (12 large triangles), warm,
by HIP events, median of --reps.  Beside it: the time the same outputs' bytes
take at the measured device-to-device copy bandwidth (the floor of the resolve
pass), GraphBoxRenderer.render_many at the same K, and the A/B of the
threshold between the two triangle paths (PCNN_RENDER_SMALL_MAX).  One JSON line.
    python tests/perf_render.py [--k 64] [--reps 50]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from posecnn_amd.synthesize.render import MeshRenderer  # noqa: E402
from refine_scene import CAMERA, GraphBoxRenderer  # noqa: E402
from render_ref import box_mesh, icosphere, random_pose  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--k", type=int, default=64)
p.add_argument("--reps", type=int, default=50)
p.add_argument("--thresholds", default="0,16,64,256,1024,1000000")
a = p.parse_args()
D = torch.device("cuda")
H, W, K = 480, 640, a.k
HALF = (0.06, 0.045, 0.035)


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


rng = np.random.default_rng(0)
poses = np.stack([random_pose(rng, 0.6, 1.0) for _ in range(K)])
poses[:, 4:6] *= 2  # spread over the full-size image
poses_d = torch.from_numpy(poses).to(D)
r = MeshRenderer({1: icosphere(5, 0.05), 2: box_mesh(HALF)}, H, W, CAMERA, device=D)
out_bytes = K * H * W * (16 + 16 + 12)
src = torch.empty(out_bytes, dtype=torch.uint8, device=D)
dst = torch.empty_like(src)
copy_us = median_us(lambda: dst.copy_(src))
res = {"metric": f"render_many, K = {K} poses at {W}x{H}", "unit": "us (median of %d, HIP events, warm)" % a.reps,
       "output_bytes": out_bytes, "d2d_copy_us": copy_us,
       "d2d_copy_GBps": round(2 * out_bytes / (copy_us * 1e-6) / 1e9, 1),
       "note": "d2d_copy_us reads and writes the outputs' bytes once each; the resolve pass writes them once and "
               "reads 8 B of z-buffer per pixel"}
# the op alone (render_into on preallocated maps) and the public call (fresh output tensors)
mi = {n: torch.full((K,), s, dtype=torch.int32, device=D) for n, s in (("icosphere5", 0), ("box", 1))}
ci = {n: torch.full((K,), c, dtype=torch.int32, device=D) for n, c in (("icosphere5", 1), ("box", 2))}
pv, pn = (torch.empty((K, H, W, 4), device=D) for _ in range(2))
vm = torch.empty((K, H, W, 3), device=D)
for name, obj in (("icosphere5", 1), ("box", 2)):
    res[name] = {"render_many_us": median_us(lambda: r.render_many([obj] * K, poses_d)),
                 "op_us": median_us(lambda: r.render_into(mi[name], ci[name], poses_d, pv, pn, vm))}
    ab = {}
    for thr in a.thresholds.split(","):
        os.environ["PCNN_RENDER_SMALL_MAX"] = thr
        ab[thr] = median_us(lambda: r.render_into(mi[name], ci[name], poses_d, pv, pn, vm))
    os.environ.pop("PCNN_RENDER_SMALL_MAX")
    res[name]["op_us_by_small_max"] = ab
covered = int((r.render_many([1] * K, poses_d, return_tri_id=True)[3] >= 0).sum().item())
res["icosphere5"]["covered_pixels_per_pose"] = covered // K
g = GraphBoxRenderer(lambda o: HALF)
res["graph_box_renderer_us"] = median_us(lambda: g.render_many([2] * K, list(poses.astype(np.float64))), reps=max(10, a.reps // 5))
print(json.dumps(res), flush=True)
