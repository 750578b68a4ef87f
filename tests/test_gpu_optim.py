"""The fused momentum-SGD update on the GPU (csrc/momentum.hip,
posecnn_amd/optim.py) against its numpy restatement tests/optim_ref.py, bit
for bit: the chunk edges and both alignment paths, the device-side staircase
and step counter, a captured graph, determinism, the torch optimizer, the
state_dict round trip, PoseStep.apply_gradients and the header's contract at
the ctypes boundary."""
import copy

import numpy as np
import pytest
import torch

import abi_guard
import optim_ref as orf
from test_optim_ref import TRAIN_HEADER

pytestmark = pytest.mark.gpu
D = torch.device("cuda")
F = np.float32
SENTINEL = -777.25
EPS = 2.0 ** -24


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, F)
    return np.ascontiguousarray(a, F).view(np.int32)


def same(a, b, what=""):
    np.testing.assert_array_equal(bits(a).ravel(), bits(b).ravel(), err_msg=what)


class Arena:
    """Tensors carved out of one sentinel-filled device buffer: `take(n, odd)`
    gives n elements at a 16-byte aligned offset (odd: one element past one),
    with sentinel elements on both sides."""

    def __init__(self, capacity):
        self.buf = torch.full((capacity,), SENTINEL, dtype=torch.float32, device=D)
        assert self.buf.data_ptr() % 16 == 0
        self.cursor, self.used = 8, np.zeros(capacity, bool)

    def take(self, n, odd=False):
        off = (self.cursor + 3) // 4 * 4 + (1 if odd else 0)
        self.cursor = off + n + 8
        assert self.cursor + 8 <= self.buf.numel()
        self.used[off:off + n] = True
        t = self.buf[off:off + n]
        assert t.data_ptr() % 16 == (4 if odd else 0) and t.is_contiguous()
        return t

    def outside_untouched(self):
        return bool((self.buf.cpu().numpy()[~self.used] == F(SENTINEL)).all())


def make_set(sizes, odd=None, seed=0):
    """(params, grads, bufs) on the device, each inside its own arena, and the host copies.
    odd[i] = (param, grad, buf) misalignment of tensor i."""
    rng = np.random.default_rng(seed)
    cap = sum(sizes) + 16 * len(sizes) + 64
    arenas = [Arena(cap) for _ in range(3)]
    dev, host = ([], [], []), ([], [], [])
    for i, n in enumerate(sizes):
        o = (odd or {}).get(i, (False, False, False))
        for k, scale in enumerate((0.1, 0.01, 0.01)):
            a = (rng.standard_normal(n) * scale).astype(F)
            t = arenas[k].take(n, o[k])
            t.copy_(torch.from_numpy(a))
            dev[k].append(t)
            host[k].append(a)
    return dev, host, arenas


def restore(dev, host):
    for ts, hs in zip(dev, host):
        for t, h in zip(ts, hs):
            t.copy_(torch.from_numpy(h))


def test_edge_set_is_bit_exact(hip):
    from posecnn_amd import optim
    c = optim.chunk()
    assert c == orf.CHUNK
    sizes = [0, 1, 3, 4, 5, c - 1, c, c + 1, 3 * c + 7, c + 5, c + 2, 7, 2 * c + 1]
    odd = {9: (True, True, True),       # the view base[1 : 1 + c + 5] on all three
           10: (False, True, False)}    # the gradient alone
    flags = [True] * 11 + [False, False]
    (ps, gs, ms), (hp, hg, hm), arenas = make_set(sizes, odd)
    plan = optim.momentum_sgd_plan(ps, gs, ms, regularize=flags)
    assert plan.total_chunks == sum((n + c - 1) // c for n in sizes)
    lr0, mom, reg, gamma, stepsize = 0.01, 0.9, 0.01, 0.5, 2
    w, m = [a.copy() for a in hp], [a.copy() for a in hm]
    for n in range(3):
        plan.apply(lr0, mom, reg, gamma=gamma, stepsize=stepsize)
        torch.cuda.synchronize()
        want64 = orf.reg_loss64(w, flags, float(F(reg)))
        w, m, loss, lr = orf.apply(w, hg, m, flags, n, lr0, mom, reg, gamma, stepsize)
        same(plan.reg_loss, [loss], f"reg_loss of step {n}")
        assert abs(float(plan.reg_loss) - want64) <= 1e-5 * want64
        same(plan.lr_used, [lr], f"lr of step {n}")
        assert int(plan.step_dev) == n + 1
    assert float(plan.lr_used) == float(F(np.float64(F(lr0)) * np.float64(F(gamma))))  # n = 2: one decay
    for i, n in enumerate(sizes):
        same(ps[i], w[i], f"weights of tensor {i} ({n} elements)")
        same(ms[i], m[i], f"momentum of tensor {i} ({n} elements)")
        same(gs[i], hg[i], f"gradient of tensor {i} ({n} elements)")
        if n:
            assert not np.array_equal(w[i], hp[i])
    for a, what in zip(arenas, ("params", "grads", "bufs")):
        assert a.outside_untouched(), what
    same(arenas[1].buf[torch.from_numpy(arenas[1].used).to(D)], np.concatenate(hg))


def test_staircase_on_the_device(hip):
    from posecnn_amd import optim
    (ps, gs, ms), (hp, hg, hm), _ = make_set([orf.CHUNK + 5], seed=1)
    plan = optim.momentum_sgd_plan(ps, gs, ms)
    w, m = [hp[0].copy()], [hm[0].copy()]
    lrs = []
    for n in range(5):
        plan.apply(0.001, 0.9, 1e-4, gamma=0.1, stepsize=2)
        w, m, _, lr = orf.apply(w, hg, m, [True], n, 0.001, 0.9, 1e-4, 0.1, 2)
        same(plan.lr_used, [lr], f"lr of step {n}")
        lrs.append(float(lr))
    torch.cuda.synchronize()
    assert lrs[0] == lrs[1] > lrs[2] == lrs[3] > lrs[4] and int(plan.step_dev) == 5
    same(ps[0], w[0])
    same(ms[0], m[0])


def _run(plan, k, **kw):
    for _ in range(k):
        plan.apply(0.01, 0.9, 0.01, **kw)
    torch.cuda.synchronize()
    return [t.clone() for t in plan.params + plan.bufs + [plan.step_dev, plan.reg_loss, plan.lr_used]]


def test_graph_replay_trains_across_a_staircase_boundary(hip):
    """One captured apply, replayed 4 times with stepsize 3: the counter and the
    learning rate live on the device, so the replays are 4 eager applies."""
    from posecnn_amd import optim
    c = orf.CHUNK
    dev, host, _ = make_set([c + 3, 5, 2 * c], {1: (True, False, True)}, seed=2)
    plan = optim.momentum_sgd_plan(*dev, regularize=[True, True, False])
    kw = dict(gamma=0.1, stepsize=3)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside the capture
        plan.apply(0.01, 0.9, 0.01, **kw)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan.apply(0.01, 0.9, 0.01, **kw)
    torch.cuda.synchronize()
    restore(dev, host)
    plan.step_dev.zero_()
    for _ in range(4):
        g.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in plan.params + plan.bufs + [plan.step_dev, plan.reg_loss, plan.lr_used]]
    restore(dev, host)
    plan.step_dev.zero_()
    eager = _run(plan, 4, **kw)
    assert int(plan.step_dev) == 4
    for a, b in zip(replayed, eager):
        assert torch.equal(a, b) and (a.dtype != torch.float32 or np.array_equal(bits(a), bits(b)))
    same(plan.lr_used, [orf.lr_at(3, 0.01, 0.1, 3)])
    assert float(plan.lr_used) < 0.002


def test_two_runs_give_the_same_bits(hip):
    from posecnn_amd import optim
    c = orf.CHUNK
    dev, host, _ = make_set([5 * c + 1, 3, c], seed=3)
    plan = optim.momentum_sgd_plan(*dev)
    first = _run(plan, 1)
    restore(dev, host)
    plan.step_dev.zero_()
    second = _run(plan, 1)
    for a, b in zip(first, second):
        assert torch.equal(a, b) and (a.dtype != torch.float32 or np.array_equal(bits(a), bits(b)))
    assert float(first[-2]) > 0


def _linear(seed=0):
    torch.manual_seed(seed)
    lin = torch.nn.Linear(37, 5).to(D)
    extra = torch.nn.Parameter(torch.ones(3, device=D))  # never in the loss: its .grad stays None
    x = torch.randn(11, 37, device=D)
    return lin, extra, x


def test_momentum_sgd_optimizer(hip):
    from posecnn_amd import optim
    lin, extra, x = _linear()
    lr, mom, reg = 0.1, 0.9, 1e-2
    opt = optim.MomentumSGD(list(lin.parameters()) + [extra], lr=lr, momentum=mom, weight_reg=reg)
    twin = [p.detach().clone().requires_grad_() for p in lin.parameters()]
    sgd = torch.optim.SGD(twin, lr=lr, momentum=mom, weight_decay=reg)
    w = [p.detach().cpu().numpy().copy() for p in lin.parameters()]
    m = [np.zeros_like(a) for a in w]
    held, plans = [], []
    for n in range(2):
        lin(x).square().sum().backward()
        grads = [p.grad.detach().clone() for p in lin.parameters()]
        opt.step()
        torch.cuda.synchronize()
        plans.append(opt.plans[0])
        w, m, loss, _ = orf.apply(w, [g.cpu().numpy() for g in grads], m, [True, True], n, lr, mom, reg)
        same(opt.plans[0].reg_loss, [loss])
        for p, ref in zip(lin.parameters(), w):
            same(p, ref, f"step {n}")
        for t, g in zip(twin, grads):
            t.grad = g.clone()
        sgd.step()
        held.append([p.grad for p in lin.parameters()])  # kept alive: the next gradients land elsewhere
        opt.zero_grad(set_to_none=True)
    assert plans[0] is not plans[1] and plans[0].key != plans[1].key  # the table was rebuilt
    assert plans[0].step_dev is plans[1].step_dev and int(plans[1].step_dev) == 2
    assert plans[1].T == 2 and extra.grad is None and bool((extra == 1).all()) and extra not in opt.state
    # torch's SGD: the same update up to its own rounding order (it may fuse g + wd p): a semantic check,
    # |dw| <= 8 2^-24 (|w| + lr |m|) per step taken
    for p, t, ref_m in zip(lin.parameters(), twin, m):
        a, b = p.detach().double().cpu().numpy(), t.detach().double().cpu().numpy()
        bound = 2 * 8 * EPS * (np.abs(a) + lr * np.abs(ref_m.astype(np.float64)))
        print("torch.optim.SGD: differing elements", int((a != b).sum()), "of", a.size, "max",
              float(np.abs(a - b).max()))
        assert (np.abs(a - b) <= bound).all()
        same(opt.state[p]["momentum_buffer"], ref_m)


def test_state_dict_round_trip_continues_bit_identically(hip):
    from posecnn_amd import optim
    lin, _, x = _linear(1)
    kw = dict(lr=0.1, momentum=0.9, weight_reg=1e-2, gamma=0.5, stepsize=2)
    opt = optim.MomentumSGD(lin.parameters(), **kw)
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        lin(x).square().sum().backward()
        opt.step()
    sd = copy.deepcopy(opt.state_dict())
    assert sd["param_groups"][0]["step"] == 2
    lin2 = copy.deepcopy(lin)
    opt2 = optim.MomentumSGD(lin2.parameters())  # other settings: the loaded ones replace them
    opt2.load_state_dict(sd)
    for o, l in ((opt, lin), (opt2, lin2)):
        o.zero_grad(set_to_none=True)
        l(x).square().sum().backward()
        o.step()
    torch.cuda.synchronize()
    for a, b in zip(lin.parameters(), lin2.parameters()):
        same(a, b)
        same(opt.state[a]["momentum_buffer"], opt2.state[b]["momentum_buffer"])
        assert opt.state[a]["momentum_buffer"].data_ptr() != opt2.state[b]["momentum_buffer"].data_ptr()
    # the third update is past the staircase's first edge: the count travelled
    for o in (opt, opt2):
        assert int(o.plans[0].step_dev) == 3
        same(o.plans[0].lr_used, [orf.lr_at(2, 0.1, 0.5, 2)])
    assert opt2.state_dict()["param_groups"][0]["step"] == 3


def test_pose_step_applies_its_gradients(hip):
    """step() + apply_gradients() at the step tests' small geometry: every
    weight is the reference update of the pre-step weight with step.grads, the
    L2 value is that of the pre-step weights, and the next step sees the new
    weights."""
    from posecnn_amd import synth
    from posecnn_amd.pipeline import PoseStep
    B, H, W, C, CH, UN = 1, 120, 160, 22, 64, 256
    fr = synth.make_frames(B, H=H, W=W, num_classes=C, objects_per_image=4, seed=93)
    g = torch.Generator().manual_seed(9)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(D)  # noqa: E731
    pts, sym = synth.rescaled_points(C)
    inputs = dict(label=t(fr["label"]), vertex=t(fr["vertex"]), extents=t(fr["extents"]), meta=t(fr["meta"]),
                  gt=t(fr["gt"]), conv4=torch.randn((B, H // 8, W // 8, CH), generator=g).to(D),
                  conv5=torch.randn((B, H // 16, W // 16, CH), generator=g).to(D), points=t(pts), symmetry=t(sym))
    step = PoseStep(B, H, W, C, D, channels=CH, units=UN, is_train=1, skip_pixels=3, keep_prob=1.0)
    names = ("w6", "b6", "w7", "b7", "w8", "b8")
    for b in (step.weights.b6, step.weights.b7, step.weights.b8):
        b.copy_(torch.randn(b.shape, generator=g) * 1e-3)
    with pytest.raises(Exception, match="make_optimizer"):
        step.apply_gradients()
    kw = dict(lr=0.05, momentum=0.9, weight_reg=1e-3, gamma=0.1, stepsize=30000)
    plan = step.make_optimizer(**kw)
    before = [getattr(step.weights, k).cpu().numpy().copy() for k in names]
    loss1 = float(step.step(inputs))
    step.apply_gradients()
    torch.cuda.synchronize()
    grads = [step.grads[k].cpu().numpy() for k in names]
    assert all(np.abs(a).max() > 0 for a in grads)
    want, _, reg_loss, lr = orf.apply(before, grads, [np.zeros_like(a) for a in before], [True] * 6, 0, kw["lr"],
                                      kw["momentum"], kw["weight_reg"], kw["gamma"], kw["stepsize"])
    for k, ref, old in zip(names, want, before):
        same(getattr(step.weights, k), ref, k)
        assert not np.array_equal(ref, old), k
    same(plan.reg_loss, [reg_loss])
    same(plan.lr_used, [lr])
    assert int(plan.step_dev) == 1 and float(plan.reg_loss) > 0
    loss2 = float(step.step(inputs))
    step.apply_gradients()
    torch.cuda.synchronize()
    assert loss1 > 0 and loss2 > 0 and loss2 != loss1 and int(plan.step_dev) == 2
    step.dist = object()  # the image-sharded step: refused
    try:
        with pytest.raises(NotImplementedError, match="dist"):
            step.apply_gradients()
        with pytest.raises(NotImplementedError, match="dist"):
            step.make_optimizer()
    finally:
        step.dist = None


def _variants(t):
    """A float64, a strided and a CPU form of `t`."""
    big = torch.zeros((2 * t.numel(),), dtype=t.dtype, device=t.device)
    strided = big[::2]
    strided.copy_(t)
    assert not strided.is_contiguous()
    return {"float64": t.double(), "strided": strided, "cpu": t.cpu()}


def test_wrappers_keep_the_header_contract(hip):
    from posecnn_amd import _lib, optim
    real = optim._load()
    assert isinstance(real, type(_lib.load())) and real.pcnn_momentum_sgd.argtypes is not None
    guard = abi_guard.GuardedLib(real, header=TRAIN_HEADER)
    (ps, gs, ms), host, _ = make_set([orf.CHUNK + 1, 6], seed=4)
    lists = dict(params=ps, grads=gs, bufs=ms)
    _lib._lib = guard
    try:
        plan = optim.momentum_sgd_plan(ps, gs, ms)
        guard.reset()
        plan.apply(0.01, 0.9, 1e-4)  # the canonical call: one entry point with a stream (its two kernels)
        torch.cuda.synchronize()
        assert guard.calls["pcnn_momentum_sgd"] == 1 and sum(guard.calls.values()) == 1 and guard.launches == 1
        assert int(plan.step_dev) == 1
        guard.reset()
        for name, ts in lists.items():
            for i in range(len(ts)):
                for what, bad in _variants(ts[i]).items():
                    with pytest.raises(ValueError, match=rf"{name}\[{i}\]"):
                        optim.momentum_sgd_plan(**dict(lists, **{name: ts[:i] + [bad] + ts[i + 1:]}))
                    assert sum(guard.calls.values()) == 0, (name, i, what)
        with pytest.raises(ValueError, match="overlaps"):   # the momentum in the parameter's memory
            optim.momentum_sgd_plan(ps, gs, [ps[0], ms[1]])
        with pytest.raises(ValueError, match="overlaps"):   # two row blocks that share a row
            optim.momentum_sgd_plan([ps[0][:100], ps[0][99:200]], [gs[0][:100], gs[0][100:201]],
                                    [ms[0][:100], ms[0][100:201]])
        with pytest.raises(ValueError, match="elements"):
            optim.momentum_sgd_plan(ps, [gs[0][:-1], gs[1]], ms)
        with pytest.raises(ValueError, match="regularize"):
            optim.momentum_sgd_plan(ps, gs, ms, regularize=[True])
        with pytest.raises(ValueError):
            plan.apply(0.01, 1.0, 1e-4)  # momentum 1: refused by the library, nothing launched
        assert guard.calls["pcnn_momentum_sgd"] == 1 and int(plan.step_dev) == 1
        # disjoint row blocks of one matrix are fine (GradShard's slabs)
        mat = [torch.zeros((6, 10), device=D) for _ in range(3)]
        rows = optim.momentum_sgd_plan(*[[a[:3], a[3:]] for a in mat])
        assert rows.T == 2
    finally:
        _lib._lib = real
    # the guard refuses what the wrapper would never send
    with pytest.raises(abi_guard.AbiContractError):
        guard.pcnn_momentum_sgd(_lib.ptr(plan.table.float()), _lib.ptr(plan.chunk_start), plan.T, plan.total_chunks,
                                0.01, 0.1, 0, 0.9, 1e-4, _lib.ptr(plan.step_dev), None, None, None, 0,
                                _lib.stream_ptr())
    torch.cuda.synchronize()
