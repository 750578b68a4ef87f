"""Measurement of the fused momentum-SGD update (csrc/momentum.hip) at the
pose head's real sizes: C = 22, w6 25088x4096, w7 4096x4096, w8 4096x88 and
the three biases, 119.9 M float32 parameters.  Warm, one HIP event pair per
call on preallocated tensors, median of --reps with the spread (min, max):
  new        one plan.apply over the six tensors, with the L2 loss value
  new_noreg  the same plan without it (reg_loss NULL)
  base       torch.optim.SGD(foreach=True, momentum=0.9, weight_decay=1e-4)
             .step() on the same weights and gradients, in this process on
             this GPU: what a user of the library had to do without the op
  step / step_apply   PoseStep at the benchmark's configuration (B = 8,
             640x480, pipelined, eager): step() alone and step() +
             apply_gradients(), wall time per step over runs of --steps steps
             between device synchronisations, median of 5 runs
bytes = 20 B per parameter (read w, g, m; write w, m).
Condition: new runs strictly under base with disjoint [min, max] ranges.  The
script exits 1 if it fails, after writing the JSON.
    python tests/perf_optim.py [--reps 30] [--steps 20] [--out profiles/optim.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from posecnn_amd import optim, synth  # noqa: E402
from posecnn_amd import pose_head as ph  # noqa: E402
from posecnn_amd.pipeline import PoseStep  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--reps", type=int, default=30)
p.add_argument("--steps", type=int, default=20)
p.add_argument("--skip-step", action="store_true", help="leave out the PoseStep lines")
p.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim.json"))
a = p.parse_args()
D = torch.device("cuda")
C = 22
LR, MOM, REG = 0.001, 0.9, 1e-4
PEAK = (4.8, 5.3)  # TB/s, the practical HBM peak of DESIGN.md


def timed(fn, reps=a.reps):
    """{"us": median, "min_us", "max_us"} of fn, warm."""
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
    return {"us": round(float(np.median(ts)), 1), "min_us": round(float(np.min(ts)), 1),
            "max_us": round(float(np.max(ts)), 1)}


names = ("w6", "b6", "w7", "b7", "w8", "b8")
wts = ph.PoseHeadWeights(C, D)
params = [getattr(wts, k) for k in names]
gen = torch.Generator(device=D).manual_seed(0)
grads = [torch.randn(t.shape, device=D, generator=gen) * 1e-4 for t in params]
n_params = sum(t.numel() for t in params)
nbytes = 20 * n_params

plan = optim.momentum_sgd_plan(params, grads, [torch.zeros_like(t) for t in params])
plan_noreg = optim.momentum_sgd_plan(params, grads, plan.bufs, reg_loss=False)
new = timed(lambda: plan.apply(LR, MOM, REG))
new_noreg = timed(lambda: plan_noreg.apply(LR, MOM, REG))

for t, g in zip(params, grads):
    t.requires_grad_()
    t.grad = g
sgd = torch.optim.SGD(params, lr=LR, momentum=MOM, weight_decay=REG, foreach=True)
base = timed(sgd.step)
for t in params:
    t.grad = None
    t.requires_grad_(False)
del sgd

new["bytes"] = nbytes
new["TBps"] = round(nbytes / (new["us"] * 1e-6) / 1e12, 3)
new_noreg["TBps"] = round(nbytes / (new_noreg["us"] * 1e-6) / 1e12, 3)
base["TBps_at_20B"] = round(nbytes / (base["us"] * 1e-6) / 1e12, 3)
res = {"metric": f"momentum-SGD update of the pose head, C = {C}, {n_params} float32 parameters in 6 tensors",
       "unit": "us (median of %d with min and max, one HIP event pair per call, warm)" % a.reps,
       "device": torch.cuda.get_device_name(0), "parameters": n_params, "chunks": plan.total_chunks,
       "new": new, "new_noreg": new_noreg, "base_torch_sgd_foreach": base,
       "new_us": new["us"], "new_noreg_us": new_noreg["us"], "base_us": base["us"], "bytes": nbytes,
       "speedup_over_base": round(base["us"] / new["us"], 2),
       "fraction_of_practical_peak": [round(new["TBps"] / PEAK[1], 3), round(new["TBps"] / PEAK[0], 3)],
       "practical_peak_TBps": list(PEAK)}

if not a.skip_step:
    del plan, plan_noreg, grads
    torch.cuda.empty_cache()
    B, H, W = 8, 480, 640
    fr = synth.make_frames(B, H, W, num_classes=C, objects_per_image=6, seed=3)
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(D)  # noqa: E731
    inputs = dict(label=to(fr["label"]), vertex=to(fr["vertex"]), extents=to(fr["extents"]), meta=to(fr["meta"]),
                  gt=to(fr["gt"]), conv4=torch.randn((B, H // 8, W // 8, 512), generator=gen, device=D),
                  conv5=torch.randn((B, H // 16, W // 16, 512), generator=gen, device=D))
    pts, sym = synth.rescaled_points(C)
    inputs["points"], inputs["symmetry"] = to(pts), to(sym)
    batches = [inputs, {k: (v.clone() if k not in ("points", "symmetry") else v) for k, v in inputs.items()}]
    step = PoseStep(B, H, W, C, D, is_train=1, skip_pixels=10, weights=wts, pipeline=True, defer_side_join=True)
    step.make_optimizer(lr=LR, momentum=MOM, weight_reg=REG)
    count = [0]

    def one(apply):
        i = count[0]
        count[0] = i + 1
        step.step(batches[i % 2], batches[(i + 1) % 2])
        if apply:
            step.apply_gradients()

    def per_step(apply):
        for _ in range(5):
            one(apply)
        step.join()
        torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(a.steps):
                one(apply)
            step.join()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / a.steps * 1e6)
        return {"us": round(float(np.median(ts)), 1), "min_us": round(float(np.min(ts)), 1),
                "max_us": round(float(np.max(ts)), 1)}

    res["step"] = per_step(False)
    res["step_apply"] = per_step(True)
    res["step_us"], res["step_apply_us"] = res["step"]["us"], res["step_apply"]["us"]
    res["step_unit"] = "us per step, wall time of %d eager pipelined steps between device syncs, median of 5" % a.steps
    res["loss_finite"] = bool(torch.isfinite(step.loss).all())

res["condition_met"] = bool(new["max_us"] < base["min_us"])
res["note"] = ("bytes are the algorithm's: 20 B per parameter; torch's foreach path makes separate passes for the "
               "weight-decay add, the momentum update and the parameter update (at least 36 B per parameter)")
print(json.dumps(res), flush=True)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as fh:
    fh.write(json.dumps(res, indent=1) + "\n")
sys.exit(0 if res["condition_met"] else 1)
