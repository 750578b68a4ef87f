"""Time the ADD loss forward on the bench's own rows (configs[2]: B=8 train-mode
Hough targets/weights, 22 classes, random predictions normalised as the
step's l2_normalize does: a unit quaternion on the row's class) with HIP
events, `--repeats` times over, and check that every repeat gives the same bits.
    python scripts/add_bench.py [--iters 20] [--repeats 3] [--near]
PCNN_ADD_SEARCH=scan in the environment times the exact scan instead of the
MFMA filter; the search counters of the last call are printed either way."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from posecnn_amd import synth  # noqa: E402
from posecnn_amd.hough_voting_gpu_layer import hough_voting_gpu_op as hv  # noqa: E402
from posecnn_amd.average_distance_loss import average_distance_loss_op as adl  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--iters", type=int, default=20)
p.add_argument("--near", action="store_true", help="predictions within a few degrees of the targets")
p.add_argument("--repeats", type=int, default=3)
a = p.parse_args()
D = torch.device("cuda")
B, H, W, C = 8, 480, 640, 22
fr = synth.make_frames(B, H, W, num_classes=C, objects_per_image=6, seed=3)
to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(D)
o = hv.hough_voting_gpu_capacity(to(fr["label"]), to(fr["vertex"]), to(fr["extents"]), to(fr["meta"]), to(fr["gt"]),
                                 1, -1.0, 0.02, 10)
nr = o["num_rois"][1:2]
pts, sym = synth.rescaled_points(C)
pts, sym = to(pts), to(sym)
g = torch.Generator(device=D).manual_seed(7)
raw = torch.randn(o["target"].shape, generator=g, device=D)
if a.near:
    raw = o["target"] + 0.03 * raw
pred = torch.nn.functional.normalize(raw * o["weight"], dim=1)  # unit quaternion on the class, as the step's
loss = torch.zeros((1,), device=D)
diff = torch.zeros_like(pred)
R = pred.shape[0]
ws = torch.empty(adl.workspace_bytes(R, C, pts.shape[1]), dtype=torch.uint8, device=D)
fn = lambda: adl.average_distance_loss(pred, o["target"], o["weight"], pts, sym, 0.01, num_rois=nr, out=(loss, diff),
                                       workspace=ws)
import hashlib  # noqa: E402
res = set()
print(f"workspace {ws.numel()} bytes (R {R}, C {C}, P {pts.shape[1]})", flush=True)
for _ in range(a.repeats):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    dig = hashlib.sha256(diff.cpu().numpy().tobytes()).hexdigest()[:16]
    res.add((loss.item(), dig))
    print(f"rows {int(nr.item())} add_fwd {e0.elapsed_time(e1) / a.iters * 1e3:9.1f} us "
          f"loss {float(loss.item()).hex()} diff sha {dig}", flush=True)
assert len(res) == 1, "repeats differ"
# the ADD-S search of the last call: items by path, exact evaluations, and the
# passing (query, 32-candidate block, half) triples per query point
st = adl.search_stats(ws, R, C, pts.shape[1])
live = int(nr.item())
cls = (o["weight"][:live, 0::4] > 0).float().argmax(1)
has = (o["weight"][:live, 0::4] > 0).any(1)
nsym = int((has & (sym[cls] > 0)).sum().item())
queries = max(1, nsym * pts.shape[1])
print(f"search {os.environ.get('PCNN_ADD_SEARCH', 'filter')}: symmetric rows {nsym}, filter items "
      f"{st['filter_items']}, scan items {st['scan_items']}, exact evaluations {st['exact_evals']} "
      f"({st['exact_evals'] / queries:.2f} per query, {st['exact_evals'] / 16 / queries:.2f} passing block halves "
      f"per query)", flush=True)
