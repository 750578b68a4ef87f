"""Measurement of the embedding neck (csrc/neck.hip, posecnn_amd/neck.py) at
the workload's size: B = 8 frames of 640x480, conv4_3 at 60x80 and conv5_3 at
30x40 with K = 512 channels, U = 64 score and V = 128 vertex units, keep_prob
0.5.  Warm, HIP events around --inner back-to-back calls on preallocated
operands, median of --reps with the spread (min, max); the two forward paths
alternate inside every repetition, so drift of the machine hits both:
  fused_forward    neck.embedding: two GEMMs over all N = 192 columns, then
                   pcnn_neck_fwd (bias, ReLU, stride-2 taps, add, dropout with
                   the keep bits drawn in place)
  base_forward     the composition without the neck: four pose_head.gemm calls
                   with bias and activation (64 and 128 columns on conv4_3 and
                   on conv5_3), two upscore(., 2) calls, a torch add per
                   branch, dropout_mask per branch and a torch multiply per
                   branch (by the keep bytes; the 1 / keep_prob factor is left
                   out, which favours this path)
  fused_backward   neck.embedding_bwd with all six gradients (no composition of
                   existing ops computes it), and its parts: pcnn_neck_bwd
                   alone and the four GEMMs alone
  fused_*_pass     pcnn_neck_fwd / pcnn_neck_bwd alone, with the bytes they
                   move and the rate that gives
No threshold is asserted: the script reports.
    python tests/perf_neck.py [--reps 30] [--inner 10] [--out profiles/neck.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from posecnn_amd import neck, pose_head, upscore  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--reps", type=int, default=30)
p.add_argument("--inner", type=int, default=10)
p.add_argument("--out", default=os.path.join(ROOT, "profiles", "neck.json"))
a = p.parse_args()
D = torch.device("cuda")
B, h, w, K, U, V, KEEP, SEED = 8, 60, 80, 512, 64, 128, 0.5, 1234
N, M4, M5 = U + V, B * h * w, B * h * w // 4

gen = torch.Generator(device=D).manual_seed(0)
rand = lambda *s: torch.randn(s, device=D, generator=gen)  # noqa: E731
x4, x5 = rand(B, h, w, K), rand(B, h // 2, w // 2, K)
W4, W5 = rand(K, N) / K ** 0.5, rand(K, N) / K ** 0.5
b4, b5 = rand(N), rand(N)
d_s, d_v = rand(B, h, w, U), rand(B, h, w, V)
step = torch.zeros(1, dtype=torch.int64, device=D)
drop_gen = (SEED, step, neck.STREAM_IDS)


def fused_forward():
    return neck.embedding(x4, x5, W4, b4, W5, b5, U, keep_prob=KEEP, drop_gen=drop_gen)


# ---- the composition of the ops that exist without the neck, on preallocated buffers
x4m, x5m = x4.view(M4, K), x5.view(M5, K)
cols = ((0, U, 1, neck.STREAM_IDS[0]), (U, N, 0, neck.STREAM_IDS[1]))
Wb = [(W4[:, lo:hi].contiguous(), b4[lo:hi].contiguous(), W5[:, lo:hi].contiguous(), b5[lo:hi].contiguous())
      for lo, hi, _, _ in cols]
y4 = [torch.empty((M4, hi - lo), device=D) for lo, hi, _, _ in cols]
y5 = [torch.empty((M5, hi - lo), device=D) for lo, hi, _, _ in cols]
up5 = [torch.empty((B, h, w, hi - lo), device=D) for lo, hi, _, _ in cols]
masks = [torch.empty((M4, hi - lo), dtype=torch.uint8, device=D) for lo, hi, _, _ in cols]
outs = [torch.empty((B, h, w, hi - lo), device=D) for lo, hi, _, _ in cols]


def base_forward():
    for i, (lo, hi, act, sid) in enumerate(cols):
        w4, bb4, w5, bb5 = Wb[i]
        pose_head.gemm(x4m, w4, y4[i], bias=bb4, act=act)
        pose_head.gemm(x5m, w5, y5[i], bias=bb5, act=act)
        upscore.upscore(y5[i].view(B, h // 2, w // 2, hi - lo), 2, out=up5[i])
        torch.add(y4[i].view(B, h, w, hi - lo), up5[i], out=outs[i])
        pose_head.dropout_mask(masks[i], KEEP, SEED, step_dev=step, stream_id=sid)
        torch.mul(outs[i], masks[i].view(B, h, w, hi - lo), out=outs[i])
    return outs


def timed_pair(fns, reps=a.reps, inner=a.inner):
    """[{"us": median per call, "min_us", "max_us"}] of the callables, warm, alternating in every repetition."""
    for _ in range(3):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1) * 1e3 / inner)
    return [{"us": round(float(np.median(t)), 1), "min_us": round(float(np.min(t)), 1),
             "max_us": round(float(np.max(t)), 1)} for t in ts]


def with_rate(t, nbytes):
    t["bytes"] = int(nbytes)
    t["TBps"] = round(nbytes / (t["us"] * 1e-6) / 1e12, 3)
    return t


s, v, ctx = fused_forward()
base = base_forward()
torch.cuda.synchronize()
agree = {"add_score_max_abs_diff": float((s * KEEP - base[0]).abs().max()),
         "add_score_vertex_max_abs_diff": float((v * KEEP - base[1]).abs().max()),
         "max_abs": float(torch.maximum(s.abs().max(), v.abs().max())) * KEEP,
         "keep_bytes_equal": bool(torch.equal(ctx["keep_score"], masks[0]) and torch.equal(ctx["keep_vertex"], masks[1]))}

z4, z5, ks, kv = ctx["z4"], ctx["z5"], ctx["keep_score"], ctx["keep_vertex"]


def fwd_pass():
    return neck.neck_fwd(z4, z5, b4, b5, U, keep_prob=KEEP, drop_gen=drop_gen)


def bwd_pass():
    return neck.neck_bwd(d_s, d_v, ks, kv, z4, z5, b4, b5, U, keep_prob=KEEP)


dz4, dz5, _, _ = bwd_pass()
d_x4, d_x5 = torch.empty_like(x4), torch.empty_like(x5)
d_W4, d_W5 = torch.empty_like(W4), torch.empty_like(W5)


def bwd_gemms():
    pose_head.gemm(dz4.view(M4, N), W4, d_x4.view(M4, K), b_trans=1)
    pose_head.gemm(x4m, dz4.view(M4, N), d_W4, a_trans=1)
    pose_head.gemm(dz5.view(M5, N), W5, d_x5.view(M5, K), b_trans=1)
    pose_head.gemm(x5m, dz5.view(M5, N), d_W5, a_trans=1)


def fused_backward():
    return neck.embedding_bwd(ctx, d_s, d_v)


f4 = 4  # bytes of a float
x_b, z_b, w_b = f4 * (M4 + M5) * K, f4 * (M4 + M5) * N, f4 * 2 * K * N
out_b, keep_b = f4 * M4 * N, M4 * N
# the forward: the GEMMs read x and W and write z; the fused pass reads z and writes the two maps and the keep bytes
fused_fwd_bytes = x_b + w_b + z_b + (z_b + out_b + keep_b)
# the composition: x and W twice (per branch), y4 / y5 written, y5 read and its upscore written, y4 and the
# upscore read and the sum written, the keep bytes written, sum and keep bytes read and the product written
base_fwd_bytes = 2 * x_b + w_b + z_b + (f4 * M5 * N + out_b) + 3 * out_b + keep_b + (2 * out_b + keep_b)
# the backward pass: d, keep bytes, z4, z5 read; dz4, dz5 written
bwd_pass_bytes = out_b + keep_b + z_b + z_b
fwd, basef = timed_pair([fused_forward, base_forward])
res = {"metric": f"embedding neck, B = {B}, conv4_3 {w}x{h}, conv5_3 {w // 2}x{h // 2}, K = {K}, U = {U}, V = {V}, "
                 f"keep_prob {KEEP}",
       "unit": "us per call (median of %d windows of %d calls with min and max, one HIP event pair per window, warm; "
               "the two forwards alternate)" % (a.reps, a.inner),
       "device": torch.cuda.get_device_name(0),
       "fused_forward": with_rate(fwd, fused_fwd_bytes), "base_forward": with_rate(basef, base_fwd_bytes),
       "fused_forward_pass": with_rate(timed_pair([fwd_pass])[0], z_b + out_b + keep_b),
       "fused_backward": timed_pair([fused_backward])[0],
       "fused_backward_pass": with_rate(timed_pair([bwd_pass])[0], bwd_pass_bytes),
       "fused_backward_gemms": timed_pair([bwd_gemms])[0],
       "agreement_with_base": agree}
res["forward_speedup"] = round(res["base_forward"]["us"] / res["fused_forward"]["us"], 2)
res["fused_forward_is_faster"] = res["fused_forward"]["us"] < res["base_forward"]["us"]
res["note"] = ("bytes are the algorithm's: every operand and result of every launch once; base_forward multiplies "
               "by the keep bytes without the 1 / keep_prob factor")
print(json.dumps(res), flush=True)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as fh:
    fh.write(json.dumps(res, indent=1) + "\n")
