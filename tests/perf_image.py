"""Measurement of the lit scene renderer and the image blob
(csrc/render_lit.hip): B = 8 scenes of 6 class boxes each (LOV extents,
sample_scenes' poses, sample_lights' lights) at 640x480, warm, by HIP events,
median of --reps:
  lit_us        pcnn_render_scenes_lit on preallocated outputs (render_into)
  plain_us      pcnn_render_scenes of the same build on the same scenes
  blob_us       pcnn_image_blob, chromatic and noise on, NHWC, over 4 backgrounds
  blob_quiet_us the same with chromatic and noise off
  blob_floor_us a device-to-device copy of the blob's traffic (16 B colour read,
                3 B background read, 12 B written per pixel: 76 MB), four
                buffer pairs in turn so the bytes come from HBM
One JSON object, printed and written to --out.
    python tests/perf_image.py [--reps 50] [--out profiles/image_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from posecnn_amd import synth  # noqa: E402
from posecnn_amd.synthesize import (LitSceneRenderer, SceneRenderer, image_blob, sample_jitter,  # noqa: E402
                                    sample_lights, sample_scenes)
from refine_scene import CAMERA  # noqa: E402
from render_ref import box_mesh  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--reps", type=int, default=50)
p.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_bench.json"))
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
lights, shin = sample_lights(B, 0, 0, off)
lit = LitSceneRenderer(meshes, H, W, CAMERA, device=D)
plain = SceneRenderer(meshes, H, W, CAMERA, device=D)
t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(D)  # noqa: E731
off_d, cls_d, poses_d, lights_d, shin_d = t(off), t(cls), t(poses), t(lights), t(shin)
slots_d = t(np.array([lit.slot[int(c)] for c in cls], np.int32))
out = lit.render(off_d, slots_d, cls_d, poses_d, shin_d, lights_d)
color = out.pop("color")
ref = plain.render(off_d, slots_d, cls_d, poses_d)
same = all(torch.equal(out[k].view(torch.int32), ref[k].view(torch.int32)) for k in ref)

bgs = torch.randint(0, 256, (4, H, W, 3), dtype=torch.uint8, device=D)
bg_index = t((np.arange(B) % 4).astype(np.int32))
jitter = t(sample_jitter(B, 0, 0, noise=True))
means = t(np.asarray((102.9801, 115.9465, 122.7717), np.float32))
blob = torch.empty((B, H, W, 3), dtype=torch.float32, device=D)
traffic = B * H * W * (16 + 3 + 12)
pairs = [(torch.empty(traffic // 2, dtype=torch.uint8, device=D), torch.empty(traffic // 2, dtype=torch.uint8, device=D))
         for _ in range(4)]
turn = [0]


def d2d_copy():
    s, d = pairs[turn[0] % len(pairs)]
    turn[0] += 1
    d.copy_(s)


floor_us = median_us(d2d_copy)
res = {"metric": f"pcnn_render_scenes_lit and pcnn_image_blob, {B} scenes of {N} class boxes (K = {len(cls)}) at {W}x{H}",
       "unit": "us (median of %d, HIP events, warm)" % a.reps,
       "lit_us": median_us(lambda: lit.render_into(off_d, slots_d, cls_d, poses_d, shin_d, lights_d, color=color, **out)),
       "plain_us": median_us(lambda: plain.render_into(off_d, slots_d, cls_d, poses_d, **ref)),
       "blob_us": median_us(lambda: image_blob(color, bgs, bg_index, jitter, means, chromatic=True, noise=True, out=blob)),
       "blob_quiet_us": median_us(lambda: image_blob(color, bgs, bg_index, jitter, means, chromatic=False, noise=False,
                                                     out=blob)),
       "blob_traffic_bytes": traffic, "blob_floor_us": floor_us,
       "blob_floor_GBps": round(traffic / (floor_us * 1e-6) / 1e9, 1),
       "covered_share": round(float((out["label"] > 0).float().mean()), 4),
       "shared_maps_equal_the_plain_renderer": bool(same),
       "note": "blob_floor_us copies blob_traffic_bytes / 2 bytes (read once, written once: blob_traffic_bytes moved), "
               "four buffer pairs in turn"}
print(json.dumps(res), flush=True)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as fh:
    fh.write(json.dumps(res, indent=1) + "\n")
