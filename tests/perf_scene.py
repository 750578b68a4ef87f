"""Measurement of the scene renderer (csrc/render_scene.hip): B = 8 scenes of 6
class boxes each (LOV extents, sample_scenes' poses) at 640x480, warm, by HIP
events, median of --reps:
  op_us              pcnn_render_scenes on preallocated outputs (render_into)
  render_us          SceneRenderer.render, fresh output tensors per call
  meshes_composite_us what a user did before: pcnn_render_meshes on the same 48
                     poses (one image each), then a torch min-composite of the
                     depths per scene with label and vertex map gathered from
                     the winner (no vote targets)
  make_frames_host_us wall time of synth.make_frames(8) on the host plus the
                     copy of label and vertex map to the device
  d2d_copy_us        a device-to-device copy of the resolve pass's traffic
                     (48 B per scene pixel: 8 B key read, 32 B of maps, 8 B clear)
One JSON object, printed and written to --out.
    python tests/perf_scene.py [--reps 50] [--out profiles/scene_bench.json]"""
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
from posecnn_amd import synth  # noqa: E402
from posecnn_amd.synthesize import MeshRenderer, SceneRenderer, sample_scenes  # noqa: E402
from refine_scene import CAMERA  # noqa: E402
from render_ref import box_mesh  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--reps", type=int, default=50)
p.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_bench.json"))
a = p.parse_args()
D = torch.device("cuda")
H, W, B, N = 480, 640, 8, 6


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


ext = synth.models()["lov_extents"][:22]
meshes = {c: box_mesh(ext[c] / 2) for c in range(1, 22)}
off, cls, poses = sample_scenes(B, list(meshes), seed=0, num_objects=(N, N + 1))
r = SceneRenderer(meshes, H, W, CAMERA, device=D)
mr = MeshRenderer(meshes, H, W, CAMERA, device=D)
t = lambda x: torch.from_numpy(x).to(D)  # noqa: E731
off_d, cls_d, poses_d = t(off), t(cls), t(poses)
slots_d = t(np.array([r.slot[int(c)] for c in cls], np.int32))
K = len(cls)
out = r.render(off_d, slots_d, cls_d, poses_d)


def composite():
    vm, pv, pn, depth = mr.render_indexed(slots_d, cls_d, poses_d, return_depth=True)
    z = torch.where(depth > 0, depth, torch.full_like(depth, float("inf"))).view(B, N, H, W)
    zmin, win = z.min(1)
    hit = torch.isfinite(zmin)
    label = torch.where(hit, cls_d.view(B, N)[torch.arange(B, device=D)[:, None, None], win], 0)
    vmap = torch.gather(vm.view(B, N, H, W, 3), 1, win[:, None, :, :, None].expand(B, 1, H, W, 3))[:, 0]
    return label, torch.where(hit, zmin, 0.0), vmap


lab_c, depth_c, vm_c = composite()
same = bool(torch.equal(lab_c.to(torch.int32), out["label"]) and torch.equal(depth_c, out["depth"]))
traffic = B * H * W * 48
# four source / destination pairs taken in turn (944 MB in all): the copy's bytes come from HBM, not from a
# last-level cache that one pair (236 MB) would largely fit
pairs = [(torch.empty(traffic, dtype=torch.uint8, device=D), torch.empty(traffic, dtype=torch.uint8, device=D))
         for _ in range(4)]
turn = [0]


def d2d_copy():
    s, d = pairs[turn[0] % len(pairs)]
    turn[0] += 1
    d.copy_(s)



def host_frames():
    fr = synth.make_frames(B, H, W, num_classes=22, objects_per_image=N, seed=0)
    lab, ver = torch.from_numpy(fr["label"]).to(D), torch.from_numpy(fr["vertex"]).to(D)
    torch.cuda.synchronize()
    return lab, ver


host_frames()
t0 = time.perf_counter()
host_frames()
host_us = round((time.perf_counter() - t0) * 1e6, 1)
copy_us = median_us(d2d_copy)
res = {"metric": f"pcnn_render_scenes, {B} scenes of {N} class boxes (K = {K}) at {W}x{H}",
       "unit": "us (median of %d, HIP events, warm)" % a.reps,
       "op_us": median_us(lambda: r.render_into(off_d, slots_d, cls_d, poses_d, **out)),
       "render_us": median_us(lambda: r.render(off_d, slots_d, cls_d, poses_d)),
       "meshes_composite_us": median_us(composite),
       "make_frames_host_us": host_us,
       "resolve_traffic_bytes": traffic, "d2d_copy_us": copy_us,
       "d2d_copy_GBps": round(2 * traffic / (copy_us * 1e-6) / 1e9, 1),
       "visible_min_max": [int(out["visible"].min()), int(out["visible"].max())],
       "covered_share": round(float((out["label"] > 0).float().mean()), 4),
       "composite_equals_scene_label_and_depth": same,
       "note": "make_frames_host_us is one wall-clock run (host numpy, then the copy of label and the (B,H,W,66) "
               "vertex map); d2d_copy_us reads and writes resolve_traffic_bytes once each, four buffer pairs in turn (944 MB)"}
print(json.dumps(res), flush=True)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as fh:
    fh.write(json.dumps(res, indent=1) + "\n")
