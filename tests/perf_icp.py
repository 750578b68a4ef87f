"""Measurement of the pose-refinement row on the synthetic
box scene (tests/refine_scene.py): live vertices, df::icp for N problems
(solveICP's 8 hypotheses) x iterations, one JSON line with per-kernel HIP-event
times, the step kernel's bandwidth against HBM, and the oracle's CPU ICP
(oracle/orc_icp.cpp, one thread) timed on the same problems beside it.
    python tests/perf_icp.py [--n 8] [--iters 8] [--reps 20] [--no-cpu]"""
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
from posecnn_amd.synthesize import icp as R  # noqa: E402
from refine_scene import CAMERA, scene  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--n", type=int, default=8)
p.add_argument("--iters", type=int, default=8)
p.add_argument("--reps", type=int, default=20)
p.add_argument("--no-cpu", action="store_true")
a = p.parse_args()
D = torch.device("cuda")
t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(D)
sc = scene(0)
depth = t(sc["live"]["depth"].astype(np.int32)).to(torch.uint16)
lab = t(sc["live"]["label"])
obj = torch.tensor([sc["cls"]], dtype=torch.int32)
pv = t(np.repeat(sc["pred"]["pred_v"][None], a.n, 0))
pn = t(np.repeat(sc["pred"]["pred_n"][None], a.n, 0))
li = torch.zeros(a.n, dtype=torch.int32, device=D)
lv = R.live_vertices(depth, lab, obj, 10000.0, CAMERA)


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.reps * 1e3


H, W = sc["live"]["label"].shape
recs = int(((sc["pred"]["pred_v"][..., 2] >= 0.25) & (sc["pred"]["pred_v"][..., 2] <= 6.0)).sum())
icp_us = timed(lambda: R.icp(lv, pv, pn, CAMERA, max_error=0.05, iterations=a.iters, live_index=li))
icp0_us = timed(lambda: R.icp(lv, pv, pn, CAMERA, max_error=0.05, iterations=0, live_index=li))
per_iter = (icp_us - icp0_us) / max(a.iters, 1)
# algorithmic bytes of one iteration: each record (vertex + normal, 32 B) and
# its live-vertex gather (12 B), every problem
iter_bytes = a.n * recs * (32 + 12)
res = {"metric": "refined hypotheses/s (8-iteration df::icp on 640x480 maps)",
       "value": round(a.n / (icp_us * 1e-6), 1), "unit": "hypotheses/s",
       "n_problems": a.n, "iterations": a.iters, "records_per_problem": recs,
       "live_vertices_us": round(timed(lambda: R.live_vertices(depth, lab, obj, 10000.0, CAMERA)), 1),
       "icp_us": round(icp_us, 1), "compaction_us": round(icp0_us, 1), "us_per_iteration": round(per_iter, 1),
       "roofline": {"bound": "hbm", "achieved": round(iter_bytes / (per_iter * 1e-6) / 1e9, 1), "peak": 8000.0,
                    "unit": "GB/s", "frac": round(iter_bytes / (per_iter * 1e-6) / 8e12, 4),
                    "bytes_per_iteration": iter_bytes,
                    "note": "step + solve launches per iteration; latency-bound at this size"},
       "data": "synthetic (ray-cast box, tests/refine_scene.py)"}
# SegICP score of 8 hypotheses (grid-bucketed nearest-point search) on the
# scene's object and on a dense 640x480 cloud (every pixel one object point)
hyps8 = t(np.repeat(sc["init"].astype(np.float32)[None], 8, 0))
vm_obj = t(sc["pred"]["vertmap"])
score_scene_us = timed(lambda: R.icp_score(lv[0], lab, sc["cls"], vm_obj, hyps8))
rng = np.random.default_rng(0)
dense_live = (rng.uniform(-0.15, 0.15, (H, W, 3)) + np.array([0, 0, 1.0])).astype(np.float32)
dense_vm = rng.uniform(-0.15, 0.15, (H, W, 3)).astype(np.float32)
dense_vm[..., 0] += 1.0
dense_lab = t(np.ones((H, W), np.int32))
dh = np.zeros((8, 7), np.float32)
dh[:, 0] = 1.0
dh[:, 6] = 1.0 + 0.002 * np.arange(8)
dl, dv, dhy = t(dense_live), t(dense_vm), t(dh)
score_dense_us = timed(lambda: R.icp_score(dl, dense_lab, 1, dv, dhy))
res["icp_score_us"] = {"scene_object": round(score_scene_us, 1), "dense_640x480": round(score_dense_us, 1),
                       "scene_object_points": int(((sc["live"]["label"] == sc["cls"])).sum()),
                       "dense_points": H * W, "hypotheses": 8,
                       "note": "pcnn_icp_score: compaction, hashed half-radius cells searched ring by ring, nearest depth point "
                               "per model point, per-hypothesis flag counts"}
# solve_icp end to end (live vertices, re-centring, Nelder-Mead on optEnergy,
# 8 hypotheses x ICP, SegICP score) for a RoIs of one frame, the renderer a
# GPU ray-caster standing in for the reference's OpenGL pass
from refine_scene import GraphBoxRenderer, render_box_torch  # noqa: E402
params = list(CAMERA) + [0.25, 6.0, 10000.0]
half = sc["half"]
render = lambda o, p: render_box_torch(np.asarray(p, np.float64), half, o)  # noqa: E731
e2e = {}


def wall(fn, reps=3):
    fn()  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


renderers = {"eager": render, "graph": GraphBoxRenderer(lambda o: half)}
for rname, rnd in renderers.items():
    pre = "" if rname == "eager" else "graph_"
    for nroi in (1, 4):
        rois = np.tile(np.array([[0, sc["cls"], 0, 0, 1, 1]], np.float32), (nroi, 1))
        poses = np.tile(sc["init"].astype(np.float32)[None], (nroi, 1))
        for nm in (0, 50):
            key = f"{pre}rois{nroi}_nm{nm}"
            e2e[f"{key}_ms"] = round(wall(lambda: R.solve_icp(lab, depth, params, rois, poses, rnd,
                                                              max_error=0.02, nm_evals=nm)), 2)
            if nm and rname == "eager":  # the host-driven searches (one energy launch + host read per round)
                e2e[f"{key}_host_search_ms"] = round(wall(lambda: R.solve_icp(
                    lab, depth, params, rois, poses, rnd, max_error=0.02, nm_evals=nm, nm_device=False)), 2)
            # the caller's renders alone (1 initial + 1 for the search + 8 hypotheses per RoI): the
            # reference's OpenGL pass, here a torch ray-caster (eager per pose, or replayed from a HIP
            # graph once per stage through render_many)
            if rname == "eager":
                n_render = nroi * (1 + (1 if nm else 0) + 8)
                e2e[f"{key}_renders_ms"] = round(wall(lambda: [rnd(sc["cls"], sc["init"]) for _ in
                                                                range(n_render)]), 2)
            else:
                stages = [nroi] + ([nroi] if nm else []) + [8 * nroi]
                e2e[f"{key}_renders_ms"] = round(wall(lambda: [rnd.render_many([sc["cls"]] * k, [sc["init"]] * k)
                                                                for k in stages]), 2)
            e2e[f"{key}_minus_renders_ms"] = round(e2e[f"{key}_ms"] - e2e[f"{key}_renders_ms"], 2)
# the Nelder-Mead searches alone (pcnn_nelder_mead_energy: one workgroup per RoI, 50 evaluations)
pv0 = render(sc["cls"], sc["init"])[1]
r_ = np.array([0.1, 0.1, 0.1, 0.1, 0.01, 0.01, 0.1])
for nroi in (1, 4):
    rec, cnt = R.energy_records(lv[:1].contiguous(), lab, [sc["cls"]] * nroi,
                                [0] * nroi, pv0[None].expand(nroi, -1, -1, -1).contiguous())
    X0 = np.tile(np.array([[1, 0, 0, 0, 0, 0, 0]], np.float64), (nroi, 1))
    e2e[f"nelder_mead_device_rois{nroi}_us"] = round(
        wall(lambda: R.nelder_mead_device(rec, cnt, X0, X0 - r_, X0 + r_, 50), reps=10) * 1e3, 1)
# each launch path of the search (csrc/pose_search.hip): 4 problems forced to the speculative (1),
# cooperative (2) and one-workgroup (3) kernels, then the sizes at which the default moves to 2 and 3
for nroi, force in ((4, 1), (4, 2), (4, 3), (40, 0), (130, 0)):
    rec, cnt = R.energy_records(lv[:1].contiguous(), lab, [sc["cls"]] * nroi,
                                [0] * nroi, pv0[None].expand(nroi, -1, -1, -1).contiguous())
    X0 = np.tile(np.array([[1, 0, 0, 0, 0, 0, 0]], np.float64), (nroi, 1))
    key = f"nelder_mead_device_rois{nroi}_path{force}_us" if force else f"nelder_mead_device_rois{nroi}_auto_us"
    e2e[key] = round(wall(lambda: R.nelder_mead_device(rec, cnt, X0, X0 - r_, X0 + r_, 50, force_path=force),
                          reps=10) * 1e3, 1)
res["solve_icp_end_to_end"] = {**e2e, "records_per_roi": int(cnt[0].item()),
                               "note": "wall time per solve_icp call (host orchestration, renders, all launches and "
                                       "host reads); rois share one frame; *_renders_ms = the caller's renders alone, "
                                       "*_minus_renders_ms the rest; *_host_search_ms the searches driven from the "
                                       "host (nm_device=False); graph_* with the ray-caster replayed from captured "
                                       "HIP graphs, one batched render per stage (GraphBoxRenderer.render_many)"}
if not a.no_cpu:
    from oracle import oracle
    ref_lv = oracle.icp_live_vertices(sc["live"]["depth"], sc["live"]["label"], sc["cls"], 10000.0, CAMERA)
    t0 = time.perf_counter()
    oracle.icp(ref_lv, sc["pred"]["pred_v"], sc["pred"]["pred_n"], CAMERA, max_error=0.05, iterations=a.iters)
    cpu_s = time.perf_counter() - t0
    res["cpu_baseline"] = {"value": round(1.0 / cpu_s, 2), "unit": "hypotheses/s", "cores": 1, "kind": "port",
                           "sample": f"one problem x {a.iters} iterations of the oracle's df::icp restatement "
                                     "(full-frame per-pixel pass per iteration, as icp.cu)"}
print(json.dumps(res), flush=True)
