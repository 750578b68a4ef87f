#!/usr/bin/env python
"""bench.py — frames/sec of PoseCNN's Hough-vote + RoI + ADD-loss hot path on MI355X.

Workload (BASELINE.json configs[2] at N = 1, configs[3] at N = 8): per rank,
B = 8 synthetic 640x480 frames with 21 YCB classes (C = 22), train mode:
hough_voting_gpu (skip 10, single instance, 9 jittered RoIs per max) ->
roi_pool x2 (conv5_3 1/16, conv4_3 1/8) -> fc6/fc7/fc8 -> tanh * weight ->
l2_normalize -> ADD loss (margin 0.01) -> backward through loss, FC and both
RoI pools.  Weak scaling: every rank processes B images of the global batch
B*N (index_size = 128 / (B*N) as the reference computes it).  N > 1 runs the
step's RCCL collectives inside the timed region: the row-count and loss
all-reduces and the row-block reduction of the fc6/fc7/fc8 weight gradients
(all-to-all of the layer inputs + all-gather of dY, exchange.GradShard).

A step = one pass over one batch; inputs are resident in HBM before timing.
Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times --steps
eager steps, writes the last step's outputs when --dump-outputs DIR is given,
and prints the line; --full adds every secondary measurement (per-op and
roofline passes, HIP-graph replay timing, other precisions, step distribution,
CPU baseline, one-GPU reference of an N > 1 run).
--workload vote_roi times configs[1]
(hough_voting_gpu + 2x roi_pool forward, B = 1, test mode) instead;
--workload linemod times configs[4] per rank: LINEMOD C = 16, 4 objects per
frame, the configs[2] step plus backproject forward + backward (G = 64,
Ch = 64, NC = 16, kernel_size 1, threshold 0.02).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X HBM3E spec (MI355X_MICROARCH.md, chip parameters)
FP32_MFMA_PEAK_TFS = 157.3   # MI355X f32-input MFMA dense peak (same guide)
BF16_MFMA_PEAK_TFS = 2500.0  # MI355X bf16 MFMA dense peak (same guide; no sparsity)
SETTLE_CALLS = 200           # untimed step calls in front of every timed region (measure())


def parse(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--workload", choices=["full", "vote_roi", "linemod"], default="full")
    p.add_argument("--batch", type=int, default=0, help="images per rank (default 8 full / 1 vote_roi)")
    p.add_argument("--classes", type=int, default=22)
    p.add_argument("--full", action="store_true",
                   help="beside the timed steps also run the secondary measurements: the per-op and in-step GEMM "
                        "breakdown passes and the rooflines, the HIP-graph replay timing (the faster of replay and "
                        "eager launches is then reported), the other GEMM precisions and the no-dropout step, the "
                        "per-step distribution, the practical HBM peak, the CPU baseline, and for N > 1 the one-GPU "
                        "reference.  Without it: set up, warm up, time --steps eager steps, print the line")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps write what the last one computed as DIR/<name>.npy (float32 / "
                        "float64; outputs above 2^20 elements as a fixed seeded sample); the inputs and weights are "
                        "seeded, so two builds run with the same arguments can be compared output for output")
    p.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    p.add_argument("--cpu-seconds", type=float, default=20.0, help="CPU baseline budget (bounded sample)")
    p.add_argument("--no-graph", action="store_true",
                   help="--full: time eager launches only, no HIP-graph replay")
    p.add_argument("--flat-argmax", action="store_true",
                   help="RoI-pool argmax as the reference's int32 flat index instead of uint16 pixel indices (A/B)")
    p.add_argument("--precision", type=int, choices=[0, 1, 2], default=2,
                   help="FC GEMMs: 2 = exact 3-way split-bf16 x6 MFMA (fp32-faithful, default), "
                        "1 = split-bf16 x3 MFMA (~2^-16 per product), 0 = fp32 MFMA")
    p.add_argument("--mask-kernel", action="store_true",
                   help="draw the dropout masks with their own kernel (PoseStep drop_in_reduce=False), for A/Bs")
    p.add_argument("--prep-on-main", action="store_true",
                   help="dropout masks and ADD row classification on the step's stream (PoseStep side_prep=False)")
    p.add_argument("--no-fp32-leg", "--no-precision-legs", dest="no_legs", action="store_true",
                   help="--full: skip the secondary steps at the other GEMM precisions reported beside the main line")
    p.add_argument("--global-batch", type=int, default=0,
                   help="global batch the vote's index_size = 128 / global_batch is taken from (default: per-rank "
                        "batch x ranks; e.g. 64 runs one rank at configs[3]'s per-rank geometry, index_size 2)")
    p.add_argument("--pipeline", choices=["on", "off"], default="on",
                   help="full workloads: run the next minibatch's vote + RoI-pool forward + ADD row classification "
                        "beside the current step's loss and backward (PoseStep(pipeline=True)); two alternating "
                        "synthetic minibatches")
    p.add_argument("--prefetch-at", choices=["start", "fwd", "loss", "bwd", "tail"], default="loss",
                   help="with --pipeline on: where the next minibatch's front chain forks off the step")
    p.add_argument("--pool-at-tail", action="store_true",
                   help="pipelined: issue the prefetched minibatch's RoI-pool forward only once fc6 dX is launched")
    p.add_argument("--defer-side-join", choices=["on", "off"], default="on",
                   help="pipelined, one GPU: do not join the weight-gradient stream at the end of a step; the next "
                        "step waits for it only where it first rewrites what that stream reads")
    p.add_argument("--graph-repeat", type=int, default=1,
                   help="--full, HIP-graph timing: capture this many times the minimal step group (2 steps pipelined, else 1) "
                        "in one replay (the streams are joined once per replay)")
    p.add_argument("--step-priority", choices=["normal", "high"], default="normal",
                   help="run the step's own stream at high HIP stream priority (its side / prefetch streams stay "
                        "normal), so the dispatcher serves the critical chain first")
    p.add_argument("--no-fuse-loss-tail", action="store_true",
                   help="ADD loss row tail and pose-head backward as separate launches (PoseStep fuse_loss_tail=False)")
    p.add_argument("--no-n1-reference", action="store_true",
                   help="--full, N > 1: skip rank 0's one-GPU run of its own shard at the same geometry")
    return p.parse_args(argv)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def launch_plan(n, argv, env, port):
    """The N local rank processes `python bench.py --gpus N ...` starts when
    no launcher set WORLD_SIZE: one process per GPU, rank r on GPU r, the
    torch.distributed env of torch.distributed.run (127.0.0.1 rendezvous).
    Returns [(argv, env)] -- built before anything touches a GPU."""
    plan = []
    for r in range(n):
        e = dict(env)
        e.update(RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), GROUP_RANK="0",
                 MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        plan.append(([sys.executable, os.path.abspath(__file__)] + list(argv), e))
    return plan


def check_world(args, env):
    """None when this process should run a rank itself, else the number of
    local ranks to start.  A launcher's WORLD_SIZE must equal --gpus."""
    ws = env.get("WORLD_SIZE")
    if ws is None:
        return args.gpus if args.gpus > 1 else None
    if int(ws) != args.gpus:
        raise SystemExit(f"bench.py: WORLD_SIZE={ws} from the launcher but --gpus {args.gpus}; they must agree")
    return None


def run_local(n, argv):
    """Start the N rank processes (children, never an exec), wait for all,
    stop the rest if one fails; exit status = the first failure's."""
    import signal
    import socket
    import subprocess
    try:
        import torch  # counting devices does not initialise the GPU on this image
        have = torch.cuda.device_count()
    except Exception:  # pragma: no cover
        have = n
    if have < n:
        raise SystemExit(f"bench.py --gpus {n}: only {have} GPU(s) visible")
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    procs = [subprocess.Popen(a, env=e) for a, e in launch_plan(n, argv, os.environ, port)]
    rc = 0
    try:
        live = list(procs)
        while live:
            for p in list(live):
                r = p.poll()
                if r is None:
                    continue
                live.remove(p)
                if r != 0 and rc == 0:
                    rc = r
                    for q in live:  # the exact PIDs this launcher started
                        q.send_signal(signal.SIGTERM)
            time.sleep(0.2)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return rc if rc >= 0 else 128 - rc


def main():
    args = parse()
    n_local = check_world(args, os.environ)
    if n_local:
        sys.exit(run_local(n_local, sys.argv[1:]))
    import numpy as np
    import torch
    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if args.step_priority == "high":  # every launch of this thread on a high-priority stream
        torch.cuda.set_stream(torch.cuda.Stream(device=dev, priority=-1))
    dist = None
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=dev)
    from posecnn_amd import _lib, synth
    from posecnn_amd.pipeline import PoseStep
    from posecnn_amd.hough_voting_gpu_layer import hough_voting_gpu_op as hv
    from posecnn_amd.roi_pooling_layer import roi_pooling_op as rp
    _lib.load()  # fails loudly without the HIP library

    linemod = args.workload == "linemod"
    full = args.workload in ("full", "linemod")
    B = args.batch or (8 if full else 1)
    C = 16 if linemod else args.classes
    H, W = 480, 640
    gB = args.global_batch or B * world
    if gB < B * world or gB > 128:
        raise SystemExit(f"--global-batch {gB}: needs per-rank batch x ranks ({B * world}) <= it <= MAX_ROI (128)")
    pipelined = full and args.pipeline == "on"
    defer_join = pipelined and world == 1 and args.defer_side_join == "on"
    # seed = config index: configs[2] / configs[1] / configs[4]
    seed = 5 if linemod else (3 if full else 2)
    t0 = time.time()
    if linemod:
        G_BP, CH_BP = 64, 64
        # the voxel grid spans the camera frustum over the scene's 0.9-2.1 m depth range
        voxel = ([1.2 / G_BP, 0.9 / G_BP, 1.2 / G_BP], [-0.6, -0.45, 0.9])
        # RGB-D frames: depth at every pixel (objects over a floor plane), so surfaces cross the voxel grid
        fr = synth.make_frames(B, H, W, num_classes=C, objects_per_image=4, seed=seed, image_offset=rank * B,
                               extents=synth.models()["linemod_extents"], with_depth=True, voxel=voxel,
                               depth_background=(1.0, 2.0))
    else:
        fr = synth.make_frames(B, H, W, num_classes=C, objects_per_image=6, seed=seed, image_offset=rank * B)
    log(f"[rank {rank}] synthetic frames in {time.time() - t0:.1f}s")
    g = torch.Generator(device=dev)
    g.manual_seed(1234 + rank)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    inputs = dict(label=to(fr["label"]), vertex=to(fr["vertex"]), extents=to(fr["extents"]), meta=to(fr["meta"]),
                  gt=to(fr["gt"]),
                  conv4=torch.randn((B, H // 8, W // 8, 512), generator=g, device=dev),
                  conv5=torch.randn((B, H // 16, W // 16, 512), generator=g, device=dev))
    pts, sym = synth.linemod_points() if linemod else synth.rescaled_points(C)
    inputs["points"], inputs["symmetry"] = to(pts), to(sym)
    batches = [inputs]
    if pipelined:
        # the second minibatch: a copy of the first in buffers of its own, so
        # every timed step does exactly the unpipelined line's work (the same
        # RoI rows); the parity test (tests/test_gpu_pipeline.py) runs the
        # pipelined step over distinct minibatches
        batches.append({k: (v.clone() if k not in ("points", "symmetry") else v) for k, v in inputs.items()})

    def runner(st):
        """One step per call; pipelined: minibatches alternate, each call
        prefetching the next one's front chain."""
        if not pipelined:
            return lambda: st.step(inputs)
        k = [0]

        def go():
            i = k[0]
            k[0] = i + 1
            st.step(batches[i % 2], batches[(i + 1) % 2])
        return go

    if full:
        step = PoseStep(B, H, W, C, dev, is_train=1, skip_pixels=10, global_batch=gB, batch_base=rank * B,
                        dist=dist, precision=args.precision, pixel_argmax=not args.flat_argmax,
                        side_prep=not args.prep_on_main, drop_in_reduce=not args.mask_kernel,
                        pipeline=pipelined, prefetch_at=args.prefetch_at, fuse_loss_tail=not args.no_fuse_loss_tail,
                        defer_side_join=defer_join, pool_at_tail=args.pool_at_tail)
        run = runner(step)
        step_run = run
    if linemod:  # + the depth back-projection op, forward and backward (no reference caller)
        from posecnn_amd.backprojecting_layer import backprojecting_op as bpo
        bp_in = dict(data=torch.randn((B, H, W, CH_BP), generator=g, device=dev),
                     label=torch.rand((B, H, W, C), generator=g, device=dev),
                     depth=to(fr["depth"]), label3d=torch.rand((B, G_BP, G_BP, G_BP, C), generator=g, device=dev),
                     grad=torch.randn((B, G_BP, G_BP, G_BP, CH_BP), generator=g, device=dev))
        bp_out = {}  # the last step's back-projection outputs (--dump-outputs)

        def run():
            step_run()
            with step._t("backproject_fwd"):
                bp_out["fwd"] = bpo.backproject(bp_in["data"], bp_in["label"], bp_in["depth"], inputs["meta"],
                                                bp_in["label3d"], G_BP, 1, 0.02)
            with step._t("backproject_bwd"):
                bp_out["bwd"] = bpo.backproject_grad(bp_in["data"], bp_in["depth"], inputs["meta"], bp_in["grad"],
                                                     G_BP, 1, 0.02)
    if not full:  # vote_roi
        hout = {}
        pool = {}
        vr_timer = {}  # op -> [(event, event)] while the breakdown pass runs

        def timed(name, fn):
            if "on" not in vr_timer:
                return fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn()
            e1.record()
            vr_timer.setdefault(name, []).append((e0, e1))
            return r

        def run():
            o = timed("hough_voting_gpu", lambda: hv.hough_voting_gpu_capacity(
                inputs["label"], inputs["vertex"], inputs["extents"], inputs["meta"], inputs["gt"], 0, -1.0, 0.02, 10,
                global_batch=gB, batch_base=rank * B, out=hout.get("o")))
            hout["o"] = o
            nr = o["num_rois"][1:2]
            pool["p5"] = timed("roi_pool_conv5", lambda: rp.roi_pool(
                inputs["conv5"], o["box"], 7, 7, 1.0 / 16, 0, num_rois=nr, batch_base=rank * B, out=pool.get("p5")))
            pool["p4"] = timed("roi_pool_conv4", lambda: rp.roi_pool(
                inputs["conv4"], o["box"], 7, 7, 1.0 / 8, 0, num_rois=nr, batch_base=rank * B, out=pool.get("p4")))
        step = None

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        run()
    barrier()

    # (1) per-op breakdown: eager steps with HIP events around every op on the
    # stream the kernels run on (feeds the roofline objects); --full only
    ops = {}
    if args.full and step is not None:
        step.timer = {}
        nb = max(3, min(args.steps, 10))
        for _ in range(nb):
            run()
        barrier()
        for k, evs in step.timer.items():
            ops[k] = sum(a.elapsed_time(b) for a, b in evs) / nb
        step.timer = None
    elif args.full:
        vr_timer["on"] = True
        nb = max(3, min(args.steps, 20))
        for _ in range(nb):
            run()
        barrier()
        del vr_timer["on"]
        for k, evs in vr_timer.items():
            ops[k] = sum(a.elapsed_time(b) for a, b in evs) / nb
        vr_timer.clear()

    # (1b) in-step GEMM times: eager steps with the stream overlap left on and
    # HIP events around each FC GEMM on the stream it is launched on (the
    # weight gradients run on the side stream beside the data-gradient
    # chain), i.e. each kernel's duration as it runs in the timed step; --full only
    gemm_in_step = {}
    if args.full and step is not None:
        step.gemm_timer = {}
        nb = max(3, min(args.steps, 10))
        for _ in range(nb):
            run()
        barrier()
        for k, evs in step.gemm_timer.items():
            gemm_in_step[k] = sum(a.elapsed_time(b) for a, b in evs) / len(evs)
        step.gemm_timer = None

    # (2) timed region: K steps bracketed by a barrier + device sync on both
    # sides, max over ranks, as eager launches on the step's two streams (the
    # weight-gradient branch overlaps the data-gradient chain).  --full on one
    # GPU: the step also runs as a HIP-graph replay (no host launch cost)
    # before that; both execute the same kernels on the same data, and the
    # faster is reported (both times are in the JSON line; the eager form has
    # been the faster one in every recorded line).  N > 1: eager, with the RCCL
    # collectives inside the step.
    graph_replay = None
    # pipelined: one replay = two steps (both minibatches; the prefetch stream
    # is joined at the replay's end, as capture requires), so K must be even
    per_replay = (2 if pipelined else 1) * args.graph_repeat
    if args.full and world == 1 and not args.no_graph and args.steps % per_replay == 0:
        def run_replay_body():
            for _ in range(per_replay):
                run()
            if pipelined:
                step.join()  # the prefetch and weight-gradient streams, as capture requires
        try:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                run_replay_body()
            torch.cuda.current_stream().wait_stream(s)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                run_replay_body()
            graph.replay()
            torch.cuda.synchronize()
            graph_replay = graph.replay
        except Exception as e:  # pragma: no cover - report and time eagerly
            log(f"graph capture failed ({e}); timing eager launches")
            torch.cuda.synchronize()

    def measure(fn, per_call=1):
        # untimed calls first, so the timed steps run at the GPU's running
        # clocks whatever came before: straight after 5 warm-up steps a 20-step
        # line read 3-4 % slower than after 200 (1.78-1.80 vs 1.725 ms per
        # step on one MI355X).  A fixed count: every rank runs the same steps
        for _ in range(SETTLE_CALLS):
            fn()
        ev0 = torch.cuda.Event(enable_timing=True)
        ev1 = torch.cuda.Event(enable_timing=True)
        barrier()
        w0 = time.perf_counter()
        ev0.record()
        for _ in range(args.steps // per_call):
            fn()
        ev1.record()
        barrier()
        wall = time.perf_counter() - w0
        el = max(wall, ev0.elapsed_time(ev1) / 1e3)
        if dist is not None:
            t = torch.tensor([el], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        return el

    modes = {}
    if graph_replay is not None:
        modes["hipgraph"] = measure(graph_replay, per_replay)
    modes["eager"] = measure(run)
    mode = min(modes, key=modes.get)
    if args.dump_outputs:  # the state the last timed (eager) step left; nothing has run since
        torch.cuda.synchronize()  # every stream of the step
        dump_outputs(args.dump_outputs if world == 1 else os.path.join(args.dump_outputs, f"rank{rank}"),
                     step_outputs(step, bp_out if linemod else None) if full else
                     vote_roi_outputs(hout["o"], pool["p5"], pool["p4"]))
    # the same step with the FC GEMMs at the other precisions, eager, reported
    # beside the line as labelled secondary keys: split-bf16 x3 (~2^-16 per
    # product: fp32-class for the 1e-4 quaternion bound, not fp32-faithful) and
    # plain fp32 MFMA
    legs = {}
    if args.full and args.workload == "full" and world == 1 and not args.no_legs:
        for prec, key, desc in ((1, "bf16x3_step", "split-bf16 x3 MFMA (k_gemm_x3, hi*hi + hi*lo + lo*hi)"),
                                (0, "fp32_mfma_step", "fp32 MFMA (k_gemm_f32, 32x32x2f32)")):
            if prec == args.precision:
                continue
            step0 = PoseStep(B, H, W, C, dev, is_train=1, skip_pixels=10, global_batch=gB, batch_base=rank * B,
                             dist=dist, precision=prec, weights=step.weights, pipeline=pipelined,
                             prefetch_at=args.prefetch_at, defer_side_join=defer_join,
                             pool_at_tail=args.pool_at_tail)
            run0 = runner(step0)
            run0()
            t0_ = measure(run0)
            legs[key] = {"value": round(gB * args.steps / t0_, 2), "unit": "frames/s",
                         "ms_per_step": round(t0_ / args.steps * 1e3, 4), "fc_gemm": desc, "timing": "eager"}
            del step0
        # the same step without drop6 / drop7 (keep_prob 1, the test-time
        # graph's pose head): what the reference's training dropout costs
        step0 = PoseStep(B, H, W, C, dev, is_train=1, skip_pixels=10, global_batch=gB, batch_base=rank * B,
                         dist=dist, precision=args.precision, weights=step.weights, keep_prob=1.0,
                         pipeline=pipelined, prefetch_at=args.prefetch_at, defer_side_join=defer_join,
                         pool_at_tail=args.pool_at_tail)
        run0 = runner(step0)
        run0()
        t0_ = measure(run0)
        legs["no_dropout_step"] = {"value": round(gB * args.steps / t0_, 2), "unit": "frames/s",
                                   "ms_per_step": round(t0_ / args.steps * 1e3, 4), "keep_prob": 1.0,
                                   "timing": "eager",
                                   "note": "the same step without drop6 / drop7; the line itself trains at 0.5"}
        del step0
    elapsed = modes[mode]
    frames = gB * args.steps
    # per-step distribution of the reported mode (after the timed region, which
    # it does not touch): one HIP event pair per step (median and
    # p10 / p90), and the practical HBM peak (device-to-device copy) beside the
    # spec peak of the roofline; --full only
    dist_steps = practical = None
    if args.full:
        dist_steps = distribution(graph_replay if mode == "hipgraph" else run, min(max(args.steps, 100), 200),
                                  per_replay if mode == "hipgraph" else 1,
                                  group=2 if defer_join and mode != "hipgraph" else 1)
        if defer_join and mode != "hipgraph":
            dist_steps["grouping"] = "pairs of steps (deferred weight-gradient join), per step"
        dist_steps["mode"] = mode
        practical = d2d_gbs(dev)
    value = frames / elapsed
    if step is not None:  # pipelined: both minibatches' sets (the last trained and the prefetched one)
        rows_sets = [int(st["hough"]["num_rois"][0].item()) for st in step._sets]
    else:
        rows_sets = [int(hout["o"]["num_rois"][0].item())]
    nrows = rows_sets[0]
    rows_mean = sum(rows_sets) / len(rows_sets)
    rows_per_rank = [rows_mean]
    if dist is not None:  # each rank's RoI row count (its shard's work), rank-major
        t = torch.tensor([rows_mean], device=dev, dtype=torch.float64)
        lst = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(lst, t)
        rows_per_rank = [float(x.item()) for x in lst]

    # roofline objects
    C3 = 3 * C
    vote_bytes = (H * W * 4 + H * W * C3 * 4) * B  # label + vertex contract read
    roof = None
    roof_vote = None
    if "hough_voting_gpu" in ops:
        t_vote = ops["hough_voting_gpu"] / 1e3
        ach = vote_bytes / t_vote / 1e9
        roof_vote = {"bound": "hbm", "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": None,
                     "kernel": "hough_voting_gpu op (label compaction + interval vote + peak + emit)",
                     "bytes_per_launch": vote_bytes, "practical_peak": practical,
                     "frac_of_practical": round(ach / practical["GB/s"], 4)}
    if full and gemm_in_step:
        # dominant kernel: the slowest fc6 GEMM by its in-step HIP-event time
        # (pass 1b: the launch as it runs in the overlapped step, on its own
        # stream); algorithmic fp32 flops 2 R K N per launch
        R = max(rows_mean, 1)
        K6, U = 49 * 512, 4096
        # fc6 dW: one GEMM over this rank's rows, or, image-sharded, this
        # rank's K6 / N row block of the global gradient over every rank's
        # rows (exchange.GradShard) -- algorithmic flops count live rows only
        dw = 2.0 * R * K6 * U if world == 1 else 2.0 * (K6 / world) * U * sum(rows_per_rank)
        gem = {"fc6_fwd": 2.0 * R * K6 * U, "fc6_dx": 2.0 * R * K6 * U, "fc6_dw": dw}
        gem = {k: v for k, v in gem.items() if k in gemm_in_step}
        dom = max(gem, key=lambda k: gemm_in_step.get(k, 0.0))
        tf = gem[dom] / (gemm_in_step[dom] / 1e3) / 1e12
        fam, peak, form = {2: ("k_gemm_x6", BF16_MFMA_PEAK_TFS / 6, "3-way split-bf16 x6 MFMA 32x32x16"),
                           1: ("k_gemm_x3", BF16_MFMA_PEAK_TFS / 3, "split-bf16 x3 MFMA 32x32x16"),
                           0: ("k_gemm_f32", FP32_MFMA_PEAK_TFS, "fp32 MFMA 32x32x2")}[args.precision]
        # the split kernels' peak: the bf16 dense MFMA rate over the MFMA passes per fp32 product;
        # fc6_fwd runs split-K (+ k_gemm_reduce, inside its time)
        kname = f"{fam} ({dom}{' + k_gemm_reduce' if dom == 'fc6_fwd' else ''}, {form}, R={R:g}" + \
            (f", rank's K6/{world} row block over {sum(rows_per_rank):g} rows of {world} ranks)" if world > 1 and
             dom == "fc6_dw" else ")")
        roof = {"bound": "mfma", "achieved": round(tf, 2), "peak": round(peak, 1), "unit": "TFLOP/s",
                "frac": round(tf / peak, 4), "traffic": None, "kernel": kname, "flops_per_launch": gem[dom],
                "us_per_launch_in_step": round(gemm_in_step[dom] * 1e3, 1),
                "us_per_launch_serialised": round(ops.get(f"gemm_{dom}", 0.0) * 1e3, 1),
                "timing": "HIP events on the launching stream, overlapped step (bench pass 1b)"}
    else:
        roof = roof_vote
    # HBM traffic of the same launches from the committed rocprofv3 FETCH_SIZE /
    # WRITE_SIZE passes (scripts/gpu.sh pmc -> scripts/pmc_traffic.py)
    pmc_path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if args.full and os.path.exists(pmc_path) and world == 1 and gB == B:  # the committed passes' shapes
        try:
            pmc = json.load(open(pmc_path))
            wl = pmc.get(args.workload, {})
            if roof is not None and full and args.precision in (1, 2):
                ent = wl.get(f"{fam}:{dom}")
                if ent:
                    roof["traffic"] = round(ent["traffic_bytes"])
                    roof["traffic_unit"] = "bytes/launch (rocprofv3 2*FETCH_SIZE + WRITE_SIZE)"
            if roof_vote is not None and "hough_voting_gpu op" in wl:
                hop = wl["hough_voting_gpu op"]
                roof_vote["traffic"] = round(hop["traffic_bytes"])
                roof_vote["traffic_unit"] = "bytes/launch (rocprofv3 2*FETCH_SIZE + WRITE_SIZE, every op kernel)"
                roof_vote["traffic_kernels"] = hop.get("kernels")
                # the op's real HBM rate: counter bytes over the op's measured time, against the
                # spec peak (`frac` above is SURVEY 8(d)'s contract-byte metric)
                cnt_gbs = hop["traffic_bytes"] / t_vote / 1e9
                roof_vote["achieved_counters"] = round(cnt_gbs, 1)
                roof_vote["hbm_frac_counters"] = round(cnt_gbs / HBM_PEAK_GBS, 4)
                if "valu_busy_pct" in hop:  # the voting limiter is VALU / LDS, not HBM
                    roof_vote["valu_busy_pct"] = hop["valu_busy_pct"]
                    # the trace key carries the template arguments (k_hough_vote<4, 512>)
                    vk = [v for k, v in wl.items() if k.split("<", 1)[0] == "k_hough_vote"]
                    roof_vote["valu_busy_vote_kernel_pct"] = vk[0].get("valu_busy_pct") if vk else None
        except Exception as e:  # pragma: no cover - a stale file must not break the bench
            log(f"pmc traffic unavailable: {e}")

    # N > 1: rank 0 also times its own shard alone on its GPU at the same
    # geometry (same frames, same index_size, no collectives), the per-GPU
    # reference a like-for-like scaling ratio divides by; the other ranks wait
    n1_ref = None
    if args.full and dist is not None and full and not args.no_n1_reference:
        if rank == 0:
            step1 = PoseStep(B, H, W, C, dev, is_train=1, skip_pixels=10, global_batch=gB, batch_base=rank * B,
                             dist=None, precision=args.precision, weights=step.weights, pipeline=pipelined,
                             prefetch_at=args.prefetch_at, defer_side_join=defer_join,
                             pool_at_tail=args.pool_at_tail)
            run1 = runner(step1)
            for _ in range(max(2, args.warmup)):
                run1()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            w0 = time.perf_counter()
            e0.record()
            for _ in range(args.steps):
                run1()
            e1.record()
            torch.cuda.synchronize()
            el1 = max(time.perf_counter() - w0, e0.elapsed_time(e1) / 1e3)
            n1_ref = {"value": round(B * args.steps / el1, 2), "unit": "frames/s",
                      "ms_per_step": round(el1 / args.steps * 1e3, 4), "timing": "eager", "n_gpus": 1,
                      "per_rank_batch": B, "index_size": 128 // gB,
                      "note": "rank 0's shard on its GPU alone at this line's geometry (no collectives, full "
                              "local fc weight gradients): the one-GPU point of a fixed per-frame-work curve"}
            del step1
        dist.barrier()

    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline and not linemod:
        cpu = cpu_baseline(fr, full, args.cpu_seconds)

    if rank == 0:
        log(f"timed mode: {mode}; RoI rows per step (rank 0): {rows_sets}; per rank: {rows_per_rank}")
        if args.full:
            log("per-op ms/step (eager breakdown pass): " +
                json.dumps({k: round(v, 4) for k, v in sorted(ops.items(), key=lambda x: -x[1])}))
        out = {
            "metric": "frames/sec 640x480x21-class Hough-vote+RoI+ADD-loss, 1/2/4/8 MI355X",
            "value": round(value, 2),
            "unit": "frames/s",
            "n_gpus": world,
            "ranks": {"world_size": dist.get_world_size() if dist is not None else 1,
                      "backend": dist.get_backend() if dist is not None else None,
                      "roi_rows_per_rank": rows_per_rank},
            "steps": args.steps,
            "warmup": args.warmup,
            "settle_calls": SETTLE_CALLS,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4),
            "higher_is_better": True,
            "scaling": "weak",
            # no published GPU number exists: the ratio to the
            # measured CPU baseline of BASELINE.md §2, on this host
            "vs_baseline": round(value / cpu["value"], 2) if cpu and cpu.get("value") else None,
            "vs_baseline_basis": "cpu_baseline.value (reference CPU Houghvoting op, BASELINE.md §2)",
            "dtype": {2: "f32 (FC GEMMs: exact 3-way split-bf16 x6 MFMA, products within 2^-24, fp32 accumulate: "
                         "fp32-faithful)",
                      1: "f32 (FC GEMMs split-bf16x3 MFMA, fp32 accumulate)", 0: "f32"}[args.precision],
            "data": "synthetic (seeded label/vertex maps per minibatch.py:517-575; random conv4_3/conv5_3; "
                    "random-init FC weights" + ("; LINEMOD box-surface model points, rendered box depth over a floor plane, random "
                                                "backprojection features" if linemod else "") + ")",
            "config": {
                "workload": ("configs[4]: LINEMOD 15-class hough_voting_gpu(train) + roi_pool x2 + fc6/7/8 + "
                             "l2norm + average_distance_loss fwd/bwd + backproject fwd/bwd (G=64, Ch=64)" if linemod
                             else "configs[2]/[3]: hough_voting_gpu(train) + roi_pool x2 + fc6/7/8 + l2norm + "
                             "average_distance_loss fwd/bwd" if full else
                             "configs[1]: hough_voting_gpu(test) + roi_pool x2 forward"),
                "global_batch": gB, "per_rank_batch": B, "height": H, "width": W, "num_classes": C,
                "skip_pixels": 10, "index_size": 128 // gB, "roi_rows_rank0": nrows,
                "step_stream_priority": args.step_priority,
                "pipelined": pipelined, **({"prefetch_at": args.prefetch_at, "deferred_side_join": defer_join,
                                            "minibatches": "two alternating minibatches (the second a copy of "
                                                           "the first in its own buffers: the same work per "
                                                           "step); the next one's vote + RoI-pool forward + ADD "
                                                           "row classes run on a prefetch stream beside the "
                                                           "current step; K timed steps hold K votes",
                                            "roi_rows_minibatches_rank0": rows_sets} if pipelined else {}),
                "fc_gemm": {2: "3-way split-bf16 x6 MFMA (fp32-faithful)", 1: "split-bf16x3 MFMA, fp32 accumulate",
                            0: "fp32 MFMA"}[args.precision],
                "parallelism": (f"image-shard x{world} (RCCL: row-count/loss all-reduce, fc weight-gradient "
                                f"row blocks via all-to-all + all-gather)") if world > 1 else "single",
            },
            "timing": mode,
            "timing_ms_per_step": {k: round(v / args.steps * 1e3, 4) for k, v in modes.items()},
            "full": args.full,
        }
        if args.full:  # the secondary measurements
            out.update({
                "roofline": roof,
                "roofline_vote": roof_vote,
                "ops_ms_per_step": {k: round(v, 4) for k, v in ops.items()},
                "gemm_us_in_step": {k: round(v * 1e3, 1) for k, v in gemm_in_step.items()},
                "step_ms_distribution": dist_steps,
                "hbm_practical_peak": practical,
                "cpu_baseline": cpu,
                "n1_same_geometry": n1_ref,
                **legs,
            })
        if args.dump_outputs:
            out["outputs_dir"] = args.dump_outputs
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.destroy_process_group()


DUMP_SAMPLE = 1 << 20        # elements kept of an output with more than this many
DUMP_MAX_BYTES = 64 << 20    # cap on everything one --dump-outputs run writes


def step_outputs(step, bp_out=None):
    """What a caller of PoseStep.step() holds after the call: the loss, the
    vote's RoI rows, the pose prediction and the loss's bottom_diff (live
    rows), every weight / bias gradient and both feature-map gradients
    (linemod: + the back-projection's forward and backward outputs)."""
    h = step.hough  # the set the last step trained on
    n = int(h["num_rois"][1].item())
    out = [("loss", step.loss), ("num_rois", h["num_rois"])]
    out += [(f"hough_{k}", h[k][:n]) for k in ("box", "pose", "target", "weight", "domain")]
    out += [("pose_pred", step.pred[:n]), ("loss_diff", step.diff[:n])]
    out += [(f"grad_{k}", g) for k, g in step.grads.items()]
    out += [("grad_conv4", step.dconv4), ("grad_conv5", step.dconv5)]
    if bp_out is not None:
        out += [(f"backproject_top{i}", t) for i, t in enumerate(bp_out["fwd"])]
        out += [("backproject_grad", bp_out["bwd"])]
    return out


def vote_roi_outputs(o, p5, p4):
    """The vote_roi step's outputs: the vote's RoI rows and both pools' (top,
    argmax) over the live rows."""
    n = int(o["num_rois"][1].item())
    out = [("num_rois", o["num_rois"])]
    out += [(f"hough_{k}", o[k][:n]) for k in ("box", "pose", "target", "weight", "domain")]
    for name, (top, arg) in (("conv5", p5), ("conv4", p4)):
        out += [(f"roi_pool_{name}_top", top[:n]), (f"roi_pool_{name}_argmax", arg[:n])]
    return out


def dump_outputs(dirname, named):
    """Write each (name, device tensor) as dirname/<name>.npy: float32 as it
    is, every other dtype as float64; a tensor above DUMP_SAMPLE elements as
    the 1-D sample at DUMP_SAMPLE sorted indices drawn from a fixed seed (a
    function of its size only, so two runs sample the same elements)."""
    import numpy as np
    import torch
    os.makedirs(dirname, exist_ok=True)
    total = 0
    for name, t in named:
        t = t.detach()
        if t.numel() > DUMP_SAMPLE:
            idx = np.sort(np.random.default_rng(2024).integers(0, t.numel(), DUMP_SAMPLE))
            t = t.reshape(-1)[torch.from_numpy(idx).to(t.device)]
        a = t.cpu().numpy()
        a = np.ascontiguousarray(a, dtype=np.float32 if a.dtype == np.float32 else np.float64)
        total += a.nbytes
        if total > DUMP_MAX_BYTES:
            raise SystemExit(f"--dump-outputs: more than {DUMP_MAX_BYTES >> 20} MB of outputs")
        np.save(os.path.join(dirname, name + ".npy"), a)
    log(f"wrote {len(named)} outputs ({total / 1e6:.1f} MB) to {dirname}")


def distribution(fn, n, per_call=1, group=1):
    """ms per step of n steps, timed in groups of `group` calls of `per_call`
    steps each between one HIP event pair on the current stream, divided back.
    group 2 with the deferred weight-gradient join: a step's events on its own
    stream close before its fc6 dW ends and the next step absorbs the rest, so
    single-step samples alternate short / long around the same mean."""
    import numpy as np
    import torch
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
           for _ in range(max(1, n // (per_call * group)))]
    for a, b in evs:
        a.record()
        for _ in range(group):
            fn()
        b.record()
    torch.cuda.synchronize()
    t = np.array([a.elapsed_time(b) for a, b in evs]) / (per_call * group)
    return {"median": round(float(np.median(t)), 4), "p10": round(float(np.percentile(t, 10)), 4),
            "p90": round(float(np.percentile(t, 90)), 4), "n": n}


def d2d_gbs(dev, nbytes=1 << 30, reps=5):
    """Measured device-to-device copy rate (read + write bytes / time): the
    practical HBM peak reported next to the 8 TB/s spec."""
    import torch
    src = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    dst = torch.empty_like(src)
    dst.copy_(src)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        dst.copy_(src)
    b.record()
    torch.cuda.synchronize()
    gbs = 2.0 * nbytes * reps / (a.elapsed_time(b) / 1e3) / 1e9
    del src, dst
    return {"GB/s": round(gbs, 1), "method": f"torch copy_ D2D of {nbytes >> 20} MiB x{reps} (read + write bytes)"}


def host_cpu():
    """CPU model and core counts of this host (recorded beside the baseline)."""
    import subprocess
    info = {"model": None, "logical_cpus": os.cpu_count(), "physical_cores": None,
            "affinity_cpus": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else None}
    try:
        cores, model = set(), None
        phys = core = None
        for line in open("/proc/cpuinfo"):
            k, _, v = line.partition(":")
            k, v = k.strip(), v.strip()
            if k == "model name" and model is None:
                model = v
            elif k == "physical id":
                phys = v
            elif k == "core id":
                core = v
            elif not k and phys is not None:
                cores.add((phys, core))
                phys = core = None
        info["model"] = model
        info["physical_cores"] = len(cores) or None
    except OSError:
        pass
    try:  # GNU nproc: the processing units available to this process (honours OMP_NUM_THREADS)
        info["nproc"] = int(subprocess.run(["nproc"], capture_output=True, text=True, timeout=10).stdout)
    except Exception:
        info["nproc"] = info["affinity_cpus"] or os.cpu_count()
    # the process's real CPU allowance: the cgroup quota (v2 cpu.max "quota period",
    # v1 cfs_quota_us / cfs_period_us), the affinity mask and the OpenMP caps
    info["cgroup_cpu_max"] = None
    quota = None
    for path in ("/sys/fs/cgroup/cpu.max",):
        try:
            txt = open(path).read().strip()
            info["cgroup_cpu_max"] = txt
            q, per = txt.split()[:2]
            if q != "max":
                quota = int(q) / int(per)
        except (OSError, ValueError):
            pass
    if info["cgroup_cpu_max"] is None:
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            info["cgroup_cpu_max"] = f"cfs {q} {per}"
            if q > 0:
                quota = q / per
        except (OSError, ValueError):
            pass
    info["cgroup_cpus"] = quota
    info["OMP_NUM_THREADS"] = os.environ.get("OMP_NUM_THREADS")
    info["OMP_THREAD_LIMIT"] = os.environ.get("OMP_THREAD_LIMIT")
    allow = info["affinity_cpus"] or os.cpu_count() or 1
    if quota is not None:
        allow = min(allow, max(1, int(quota)))
    if info["OMP_THREAD_LIMIT"]:
        try:
            allow = min(allow, int(info["OMP_THREAD_LIMIT"]))
        except ValueError:
            pass
    info["allowance_threads"] = allow
    return info


def cpu_baseline(fr, train, budget_s):
    """Reference CPU Houghvoting op (oracle restatement, OpenMP) on a bounded
    sample of the same frames, on this host's cores: a thread sweep (1, 2, 4,
    ... up to the process's CPU allowance -- cgroup quota, affinity mask,
    OMP_THREAD_LIMIT -- plus nproc and the allowance itself); `value` is the
    best rate at a thread count the allowance permits (all the
    host cores the process may use), `single_thread` the 1-thread rate.  The
    vertex map is given in the CPU op's raw-distance convention
    (synth.cpu_vertex)."""
    try:
        from oracle import oracle
        oracle.build()
    except Exception as e:  # the oracle is test infrastructure; absence is reported, not fatal
        return {"value": None, "error": f"oracle unavailable: {e}"}
    from posecnn_amd import synth
    cpu = host_cpu()
    threads = cpu["nproc"]
    vert = synth.cpu_vertex(fr["vertex"])
    B = fr["label"].shape[0]

    def rate(nt, budget):
        oracle.ransac_hough(fr["label"][:1], vert[:1], fr["extents"], fr["meta"][:1], int(train), nt)  # warm-up
        n, t0 = 0, time.perf_counter()
        while True:
            i = n % B
            oracle.ransac_hough(fr["label"][i:i + 1], vert[i:i + 1], fr["extents"], fr["meta"][i:i + 1],
                                int(train), nt)
            n += 1
            if (time.perf_counter() - t0 > budget and n >= B) or n >= 400:
                break
        return n, n / (time.perf_counter() - t0)

    allow = cpu["allowance_threads"]
    counts = sorted({c for c in (1, 2, 4, 8, 16, 32, 64, 128, 256) if c <= allow} | {min(threads, allow), allow})
    # three interleaved sweeps (1, 2, 4, ..., then again): each thread count's
    # rate is the median of its three samples, so one busy moment of the host's
    # other tenants moves one sample, not the value
    n_sweeps = 3
    per = max(0.7, budget_s / (len(counts) * n_sweeps))
    samples = {c: [] for c in counts}
    for _ in range(n_sweeps):
        for c in counts:
            samples[c].append(rate(c, per))
    sweep = {}
    for c in counts:
        fs = sorted(f for _, f in samples[c])
        sweep[c] = {"frames_per_s": round(fs[len(fs) // 2], 2), "samples_frames_per_s": [round(f, 2) for f in fs],
                    "frames": sum(n for n, _ in samples[c])}
    best = max(sweep, key=lambda c: sweep[c]["frames_per_s"])
    fps, n = sweep[best]["frames_per_s"], sweep[best]["frames"]
    return {"value": round(fps, 2), "unit": "frames/s", "cores": best, "kind": "port",
            "single_thread": {"value": sweep[1]["frames_per_s"], "unit": "frames/s", "cores": 1,
                              "frames": sweep[1]["frames"]},
            "thread_sweep": {str(c): v for c, v in sweep.items()},
            "host": cpu,
            "sample": f"{n} frames ({B} distinct synthetic 640x480 frames cycled) at the best thread count of "
                      f"{counts} within the process's allowance of {allow} threads, each count's rate the median "
                      f"of {n_sweeps} interleaved sweeps of about {per:.1f} s per point; reference Houghvoting op "
                      f"(preemptive RANSAC, {'train' if train else 'test'} mode) restated in oracle/orc_ransac.cpp "
                      f"(OpenMP)"}


if __name__ == "__main__":
    main()
