"""Measurement of the upscore layers (csrc/upscore.hip) at the workload's
size: B = 8 frames of 640x480, the 1/8-resolution feature map 60x80 with
K = 128 channels, C = 22 classes, stride 8; labels and vote targets from
make_scene_frames scenes, the gradient from vertex_loss_compact.  Warm, one HIP
event pair per call on preallocated buffers, median of --reps with the spread
(min, max):
  base_*   the path without the folded head, in this process on this GPU:
           torch's depthwise conv_transpose2d producing the (8,480,640,128)
           map, then vertex_pred_compact; backward: vertex_pred_compact_bwd
           with all three outputs, then torch's input gradient of the deconv
           (a strided depthwise conv2d)
  new_*    forward: z = x_low @ W (torch.mm) and pcnn_upscore_compact_fwd;
           backward: pcnn_upscore_compact_bwd (d_z, d_bias), d_x = d_z @ W^T
           and d_W = x_low^T @ d_z
  generic_* pcnn_upscore_fwd (bias, ReLU) and pcnn_upscore_bwd (mask, d_bias)
           alone at Ch = 22 and 64
Condition (from the byte counts): the new forward runs under the baseline's
vertex_pred_compact alone and the new backward under the baseline's
vertex_pred_compact_bwd alone, the deconv excluded from both baselines.  The
script exits 1 if either fails, after writing the JSON.
    python tests/perf_upscore.py [--reps 30] [--out profiles/upscore.json]"""
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
p.add_argument("--out", default=os.path.join(ROOT, "profiles", "upscore.json"))
a = p.parse_args()
D = torch.device("cuda")
B, h, w, K, C, S = 8, 60, 80, 128, 22, 8
H, W = S * h, S * w
N, n = B * H * W, B * h * w
lib = _lib.load()


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


def with_rate(t, nbytes):
    t["bytes"] = int(nbytes)
    t["TBps"] = round(nbytes / (t["us"] * 1e-6) / 1e12, 3)
    return t


ext = synth.models()["lov_extents"][:C]
meshes = {c: box_mesh(ext[c] / 2) for c in range(1, C)}
frames = make_scene_frames(SceneRenderer(meshes, H, W, CAMERA, device=D), B, seed=0, num_classes=C)
label, vertex3 = frames["label"].to(torch.int32).contiguous(), frames["vertex3"]
gen = torch.Generator(device=D).manual_seed(0)
x_low = torch.randn((B, h, w, K), device=D, generator=gen)
wts = torch.randn((K, 3 * C), device=D, generator=gen) * 0.05
bias = torch.randn((3 * C,), device=D, generator=gen)
live = (label >= 0) & (label < C)

# ---- the baseline: deconv to the full-resolution map, then the compact layer and its backward
t = torch.arange(2 * S, dtype=torch.float32, device=D)
hat = 1.0 - (t / S - (2 * S - 1) / (2.0 * S)).abs()
kern = torch.outer(hat, hat).expand(K, 1, 2 * S, 2 * S).contiguous()
x_nchw = x_low.permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)


def deconv():
    return torch.nn.functional.conv_transpose2d(x_nchw, kern, stride=S, padding=S // 2, groups=K)


feat = deconv().permute(0, 2, 3, 1).contiguous()   # (B,H,W,K) NHWC
pred_base = torch.empty((B, H, W, 3), device=D)
vertex_pred_compact(feat, wts, bias, label, out=pred_base)
_, g3 = losses.vertex_loss_compact(pred_base, label, vertex3, C, 10.0, want_grad=True)
ws_vp = torch.empty(lib.pcnn_vertex_pred_compact_bwd_workspace_size(B, H, W, K, C), dtype=torch.uint8, device=D)
d_feat = torch.empty((B, H, W, K), device=D)
d_w_base = torch.empty((K, 3 * C), device=D)
d_b_base = torch.empty((3 * C,), device=D)


def base_bwd():
    rc = lib.pcnn_vertex_pred_compact_bwd(_lib.ptr(feat), _lib.ptr(wts), _lib.ptr(label), _lib.ptr(g3), B, H, W, K, C,
                                          _lib.ptr(d_feat), _lib.ptr(d_w_base), _lib.ptr(d_b_base), _lib.ptr(ws_vp),
                                          ws_vp.numel(), _lib.stream_ptr())
    assert rc == 0, rc


base_bwd()
d_feat_nchw = d_feat.permute(0, 3, 1, 2)   # channels-last view


def deconv_grad():
    return torch.nn.functional.conv2d(d_feat_nchw, kern, stride=S, padding=S // 2, groups=K)


d_x_base = deconv_grad().permute(0, 2, 3, 1).contiguous()

# ---- the folded head
z = torch.empty((n, 3 * C), device=D)
pred_new = torch.empty((B, H, W, 3), device=D)
d_z = torch.empty((B, h, w, 3 * C), device=D)
d_b = torch.empty((3 * C,), device=D)
d_x = torch.empty((n, K), device=D)
d_w = torch.empty((K, 3 * C), device=D)
ws_c = torch.empty(lib.pcnn_upscore_compact_bwd_workspace_size(B, h, w, C, S), dtype=torch.uint8, device=D)
x2 = x_low.view(n, K)
x2_t, w_t = x2.t(), wts.t()


def new_mm():
    torch.mm(x2, wts, out=z)


def new_op3():
    rc = lib.pcnn_upscore_compact_fwd(_lib.ptr(z), _lib.ptr(bias), _lib.ptr(label), B, h, w, C, S, _lib.ptr(pred_new),
                                      _lib.stream_ptr())
    assert rc == 0, rc


def new_fwd():
    new_mm()
    new_op3()


def new_op4():
    rc = lib.pcnn_upscore_compact_bwd(_lib.ptr(label), _lib.ptr(g3), B, h, w, C, S, _lib.ptr(d_z), _lib.ptr(d_b),
                                      _lib.ptr(ws_c), ws_c.numel(), _lib.stream_ptr())
    assert rc == 0, rc


def new_mms():
    torch.mm(d_z.view(n, 3 * C), w_t, out=d_x)
    torch.mm(x2_t, d_z.view(n, 3 * C), out=d_w)


def new_bwd():
    new_op4()
    new_mms()


new_fwd()
new_bwd()
torch.cuda.synchronize()
agree = {"pred_max_abs_diff": float((pred_new - pred_base).abs().max()),
         "pred_max_abs": float(pred_base.abs().max()),
         "d_x_max_abs_diff": float((d_x.view(B, h, w, K) - d_x_base).abs().max()),
         "d_x_max_abs": float(d_x_base.abs().max()),
         "d_weights_max_abs_diff": float((d_w - d_w_base).abs().max()),
         "d_weights_max_abs": float(d_w_base.abs().max()),
         "d_bias_max_abs_diff": float((d_b - d_b_base).abs().max())}

# algorithmic bytes: labels 4 B/px, vertex3 or its gradient 12 B/px, the low-resolution maps once
lab_b, v3_b, z_b, x_b = 4 * N, 12 * N, 4 * n * 3 * C, 4 * n * K
res = {"metric": f"upscore layers, B = {B}, {W}x{H}, low resolution {w}x{h}, K = {K}, C = {C}, stride {S}, "
                 "make_scene_frames labels",
       "unit": "us (median of %d with min and max, one HIP event pair per call, warm)" % a.reps,
       "device": torch.cuda.get_device_name(0), "pixels": N, "low_res_pixels": n, "live_pixels": int(live.sum()),
       "base_deconv": with_rate(timed(deconv), x_b + 4 * N * K),
       "base_vertex_pred_compact": with_rate(timed(lambda: vertex_pred_compact(feat, wts, bias, label, out=pred_base)),
                                             4 * N * K + lab_b + v3_b),
       "base_vertex_pred_compact_bwd": with_rate(timed(base_bwd), lab_b + v3_b + 2 * 4 * N * K),
       "base_deconv_input_grad": with_rate(timed(deconv_grad), x_b + 4 * N * K),
       "new_forward": with_rate(timed(new_fwd), x_b + 2 * z_b + lab_b + v3_b),
       "new_forward_matmul": timed(new_mm),
       "new_forward_compact_fwd": with_rate(timed(new_op3), z_b + lab_b + v3_b),
       "new_backward": with_rate(timed(new_bwd), lab_b + v3_b + 3 * z_b + 2 * x_b),
       "new_backward_compact_bwd": with_rate(timed(new_op4), lab_b + v3_b + z_b),
       "new_backward_matmuls": timed(new_mms),
       "agreement_with_base": agree}
del feat, d_feat, d_feat_nchw, d_x_base
torch.cuda.empty_cache()

for Ch in (22, 64):
    xg = torch.randn((B, h, w, Ch), device=D, generator=gen)
    bg = torch.randn((Ch,), device=D, generator=gen)
    yg = torch.empty((B, H, W, Ch), device=D)
    gg = torch.randn((B, H, W, Ch), device=D, generator=gen)
    dxg = torch.empty((B, h, w, Ch), device=D)
    dbg = torch.empty((Ch,), device=D)
    wsg = torch.empty(lib.pcnn_upscore_bwd_workspace_size(B, h, w, Ch, S), dtype=torch.uint8, device=D)

    def g_fwd():
        rc = lib.pcnn_upscore_fwd(_lib.ptr(xg), B, h, w, Ch, S, _lib.ptr(bg), 1, _lib.ptr(yg), _lib.stream_ptr())
        assert rc == 0, rc

    def g_bwd():
        rc = lib.pcnn_upscore_bwd(_lib.ptr(gg), _lib.ptr(yg), B, h, w, Ch, S, _lib.ptr(dxg), _lib.ptr(dbg),
                                  _lib.ptr(wsg), wsg.numel(), _lib.stream_ptr())
        assert rc == 0, rc

    low, full = 4 * n * Ch, 4 * N * Ch
    res[f"generic_fwd_Ch{Ch}"] = with_rate(timed(g_fwd), low + full)
    res[f"generic_bwd_Ch{Ch}"] = with_rate(timed(g_bwd), 2 * full + low)
    del xg, yg, gg

res["forward_speedup_with_deconv"] = round((res["base_deconv"]["us"] + res["base_vertex_pred_compact"]["us"]) /
                                           res["new_forward"]["us"], 2)
res["backward_speedup_with_deconv"] = round((res["base_vertex_pred_compact_bwd"]["us"] +
                                             res["base_deconv_input_grad"]["us"]) / res["new_backward"]["us"], 2)
res["condition_forward_met"] = res["new_forward"]["us"] < res["base_vertex_pred_compact"]["us"]
res["condition_backward_met"] = res["new_backward"]["us"] < res["base_vertex_pred_compact_bwd"]["us"]
res["note"] = ("bytes are the algorithm's: labels 4 B/px, vertex3 or its gradient 12 B/px, each low-resolution map "
               "and each full-resolution map of a pass once; the baselines of the condition exclude the deconv")
print(json.dumps(res), flush=True)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as fh:
    fh.write(json.dumps(res, indent=1) + "\n")
sys.exit(0 if res["condition_forward_met"] and res["condition_backward_met"] else 1)
