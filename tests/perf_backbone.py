"""Measurement of the backbone's forward (csrc/backbone.hip,
posecnn_amd/backbone.py) at the workload's size: B = 8 frames of 640x480.
Warm, HIP events around --inner back-to-back calls on preallocated operands,
median of --reps with the spread (min, max).  Per layer and for the whole stack:
  conv     backbone.conv3x3 into a preallocated map: time and fp32-equivalent
           TFLOP/s (2 M 9 Cin Cout flops; the MFMA kernel issues six bf16
           products per one of them)
  gemm     beside each MFMA layer, pose_head.gemm at precision 2 on a plain
           (M, 9 Cin) x (9 Cin, Cout) product of the same dimensions: the rate
           the project's own MFMA loop reaches with no gather.  Where the plain
           A matrix would pass 2^31 bytes (the GEMM's own limit; conv1_2's is
           5.7 GB) it runs on the largest row count that fits and the time is
           scaled by the row ratio (gemm_rows says so)
  torch    torch.nn.functional.conv2d in float32 on the same tensors (NHWC
           memory through channels_last views) with bias and ReLU -- what a
           user would otherwise call; if it fails or is unavailable offline the
           script records that and goes on
  pools    bytes moved and GB/s
No threshold is asserted: the script reports.
    python tests/perf_backbone.py [--reps 10] [--inner 3] [--batch 8] [--no-torch] [--out profiles/backbone.json]"""
import argparse
import json
import os
import sys

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")  # the torch yardstick: no exhaustive kernel search

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from posecnn_amd import backbone, pose_head  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--reps", type=int, default=10)
p.add_argument("--inner", type=int, default=3)
p.add_argument("--batch", type=int, default=8)
p.add_argument("--height", type=int, default=480)
p.add_argument("--width", type=int, default=640)
p.add_argument("--no-torch", action="store_true")
p.add_argument("--out", default=os.path.join(ROOT, "profiles", "backbone.json"))
a = p.parse_args()
D = torch.device("cuda")
B, H, W = a.batch, a.height, a.width
LIMIT = (1 << 31) - 1

gen = torch.Generator(device=D).manual_seed(0)


def rand(*s):
    return torch.randn(s, device=D, generator=gen)


def timed(fn, reps=a.reps, inner=a.inner):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / inner)
    return {"us": round(float(np.median(ts)), 1), "min_us": round(float(np.min(ts)), 1),
            "max_us": round(float(np.max(ts)), 1)}


def tflops(flops, t):
    return round(flops / (t["us"] * 1e-6) / 1e12, 1)


params = {}
for name, cin, cout in backbone.CONVS:
    params[name] = (rand(3, 3, cin, cout) * (2.0 / (9 * cin)) ** 0.5, 0.1 * rand(cout))
blob = rand(B, H, W, 3)


def write(res):
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


res = {"metric": f"VGG16 backbone forward, B = {B}, {W}x{H}",
       "unit": "us per call (median of %d windows of %d calls with min and max, one HIP event pair per window, warm); "
               "TFLOPs are fp32-equivalent: 2 M 9 Cin Cout flops per conv" % (a.reps, a.inner),
       "device": torch.cuda.get_device_name(0), "layers": {}}

# ---- the whole stack (also sizes the buffers and gives every layer its real input)
c4, c5, kept = backbone.vgg16_convs(blob, params, keep=tuple(layer[0] for layer in backbone.LAYERS))
torch.cuda.synchronize()
total_flops = 0
cur = blob
for layer in backbone.LAYERS:
    name = layer[0]
    x, y = cur, kept[name]
    _, h, w, c = (int(s) for s in x.shape)
    M = B * h * w
    row = {"in": list(x.shape), "out": list(y.shape)}
    if len(layer) == 3:
        cin, cout = layer[1], layer[2]
        wts, bias = params[name]
        flops = 2 * M * 9 * cin * cout
        total_flops += flops
        out = torch.empty_like(y)
        t = timed(lambda: backbone.conv3x3(x, wts, bias, out=out))
        row["conv"] = dict(t, TFLOPs=tflops(flops, t), kernel="direct f32" if cin == 3 else "mfma x6",
                           workspace_bytes=int(backbone._load().pcnn_conv3x3_workspace_size(B, h, w, cin, cout, 2)))
        if cin != 3:
            K = 9 * cin
            m_run = min(M, LIMIT // (4 * max(K, cout)) // 256 * 256)
            try:
                A = torch.empty((m_run, K), device=D).normal_(generator=gen)
                C = torch.empty((m_run, cout), device=D)
                Wm = wts.view(K, cout)
                tg = timed(lambda: pose_head.gemm(A, Wm, C, bias=bias, act=1, precision=2))
                scale = M / m_run
                tg = {k: round(v * scale, 1) for k, v in tg.items()}
                row["gemm"] = dict(tg, TFLOPs=tflops(flops, tg), gemm_rows=m_run, rows=M)
                row["conv_over_gemm_time"] = round(t["us"] / tg["us"], 2)
                del A, C
            except Exception as e:  # the yardstick, not the subject: record and go on
                row["gemm"] = {"error": f"{type(e).__name__}: {e}"[:300]}
    else:
        out = torch.empty_like(y)
        t = timed(lambda: backbone.max_pool2x2(x, out=out))
        nbytes = 4 * (x.numel() + y.numel())
        row["pool"] = dict(t, bytes=int(nbytes), GBps=round(nbytes / (t["us"] * 1e-6) / 1e9, 1))
    res["layers"][name] = row
    print(name, json.dumps(row), flush=True)
    cur = y

t = timed(lambda: backbone.vgg16_convs(blob, params))
res["stack"] = dict(t, TFLOPs=tflops(total_flops, t), GMAC_per_frame=round(total_flops / 2 / B / 1e9, 1),
                    frames_per_s=round(B / (t["us"] * 1e-6), 1))
print("stack", json.dumps(res["stack"]), flush=True)
write(res)

# ---- torch's own conv2d on the same tensors
if not a.no_torch:
    torch_total, failed = 0.0, None
    cur = blob
    for layer in backbone.LAYERS:
        name = layer[0]
        if len(layer) == 3 and failed is None:
            wts, bias = params[name]
            xn = cur.permute(0, 3, 1, 2)                    # NCHW view of the NHWC map: channels_last
            wn = wts.permute(3, 2, 0, 1).contiguous(memory_format=torch.channels_last)
            try:
                with torch.no_grad():
                    tt = timed(lambda: torch.relu_(torch.nn.functional.conv2d(xn, wn, bias, padding=1)))
                    got = torch.relu_(torch.nn.functional.conv2d(xn, wn, bias, padding=1)).permute(0, 2, 3, 1)
                    diff = float((got - kept[name]).abs().max())
                    del got
                flops = 2 * cur.shape[0] * cur.shape[1] * cur.shape[2] * 9 * layer[1] * layer[2]
                res["layers"][name]["torch"] = dict(tt, TFLOPs=tflops(flops, tt), max_abs_diff=diff)
                res["layers"][name]["conv_over_torch_time"] = round(res["layers"][name]["conv"]["us"] / tt["us"], 2)
                torch_total += tt["us"]
            except Exception as e:
                failed = f"{name}: {type(e).__name__}: {e}"[:300]
            print(name, "torch", json.dumps(res["layers"][name].get("torch", failed)), flush=True)
            write(res)
        cur = kept[name]
    res["torch_conv2d"] = {"error": failed} if failed else {
        "convs_us": round(torch_total, 1),
        "own_convs_us": round(sum(r["conv"]["us"] for r in res["layers"].values() if "conv" in r), 1)}
else:
    res["torch_conv2d"] = {"skipped": "--no-torch"}
print(json.dumps(res), flush=True)
write(res)
