"""The weight update of the training step, on the device, backed by
libposecnn_hip.so (csrc/momentum.hip, include/posecnn_train.h): the
reference's train_op, MomentumOptimizer(lr, 0.9).minimize(loss) with the L2
regularisation term in the loss and the staircase exponential_decay learning
rate (lib/fcn/train.py:481,530-534; network.py:417-419; config.py:54,99-102).

momentum_sgd_plan(params, grads, bufs, ...)  validate a set of (parameter,
                                             gradient, momentum) triples once and
                                             build its device table
plan.apply(lr, momentum, weight_reg, ...)    one library call: every tensor of the
                                             set updated in place, the step counter
                                             bumped, the L2 loss value and the
                                             learning rate used left on the device
MomentumSGD(params, lr=..., ...)             the same as a torch.optim.Optimizer
                                             (the pth.py modules, any backbone)

Per element, float32, every operation rounded separately:
    g2 = g + weight_reg * w   (regularised tensors; else g2 = g)
    m' = momentum * m + g2
    w' = w - lr * m'
with lr = (float)(lr0 gamma^(n // stepsize)) in float64 by repeated
multiplication, n = the updates applied so far (plan.step_dev, int64 on the
device: a captured graph that holds an apply trains on replay).
tests/optim_ref.py restates all of it in numpy.
"""
import ctypes

import numpy as np
import torch

from . import _lib

REGULARIZE = 1  # PCNN_MOMENTUM_REGULARIZE

_v, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
# include/posecnn_train.h: name -> (restype, argtypes); v = device pointer or stream
SIGS = {
    "pcnn_train_abi_version": (_i, []),
    "pcnn_momentum_chunk": (_i, []),
    "pcnn_momentum_workspace_size": (ctypes.c_size_t, [ctypes.c_long]),
    "pcnn_momentum_sgd": (_i, [_v, _v, _i, ctypes.c_long, _f, _f, _i, _f, _f, _v, _v, _v, _v, ctypes.c_size_t, _v]),
}
_bound = None


def _load():
    """_lib.load()'s handle with this module's prototypes set on it (once).  A
    library without the entry points is an error: there is no other path."""
    global _bound
    lib = _lib.load()
    if isinstance(lib, ctypes.CDLL) and lib is not _bound:
        for name, (res, args) in SIGS.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:
                raise _lib.PcnnError(f"{_lib.LIB_PATH} has no {name}; rebuild it: __graft_entry__.build()") from None
            fn.restype = res
            fn.argtypes = args
        _bound = lib
    return lib


def chunk():
    """Elements per unit of work (pcnn_momentum_chunk): a tensor of n elements
    takes ceil(n / chunk()) chunks."""
    return int(_load().pcnn_momentum_chunk())


def _flags(regularize, T, who):
    if regularize is None or regularize is True:
        return [True] * T
    if regularize is False:
        return [False] * T
    flags = [bool(r) for r in regularize]
    if len(flags) != T:
        raise ValueError(f"{who}: regularize has {len(flags)} entries for {T} parameters")
    return flags


class MomentumPlan:
    """A validated set of (parameter, gradient, momentum) triples with its
    device table; made by momentum_sgd_plan.  step_dev (1) int64, reg_loss (1)
    float32 (None without the L2 value) and lr_used (1) float32 are device
    tensors an apply() writes; nothing is read back."""

    def __init__(self, params, grads, bufs, flags, device, step_dev, reg_loss):
        self.params, self.grads, self.bufs, self.flags, self.device = params, grads, bufs, flags, device
        c = chunk()
        T = len(params)
        start = np.zeros(T + 1, np.int64)
        rows = np.zeros((max(T, 1), 5), np.int64)
        for t, (p, g, m, r) in enumerate(zip(params, grads, bufs, flags)):
            rows[t] = (p.data_ptr(), g.data_ptr(), m.data_ptr(), p.numel(), REGULARIZE if r else 0)
            start[t + 1] = start[t] + (p.numel() + c - 1) // c
        if start[-1] >= 1 << 31:
            raise ValueError("momentum_sgd_plan: the set has 2^31 chunks or more")
        self.T, self.total_chunks = T, int(start[-1])
        self.key = tuple(int(a) for a in rows[:T, :3].ravel())
        # fresh pinned tensors: the host allocator keeps them until the copies have run
        self.table = torch.from_numpy(rows).pin_memory().to(device, non_blocking=True)
        self.chunk_start = torch.from_numpy(start.astype(np.int32)).pin_memory().to(device, non_blocking=True)
        self.step_dev = step_dev if step_dev is not None else torch.zeros((1,), dtype=torch.int64, device=device)
        self.lr_used = torch.zeros((1,), dtype=torch.float32, device=device)
        self.reg_loss = self.workspace = None
        if reg_loss:
            self.reg_loss = torch.zeros((1,), dtype=torch.float32, device=device)
            self.workspace = torch.empty(_load().pcnn_momentum_workspace_size(self.total_chunks), dtype=torch.uint8,
                                         device=device)

    def apply(self, lr, momentum, weight_reg, gamma=0.1, stepsize=0, stream=None):
        """One update of every tensor of the plan, in place, on `stream`
        (default: the current one): one library call, two launches, no sync,
        capturable.  The learning rate of this update is lr * gamma^(step_dev
        // stepsize) (stepsize 0: lr); afterwards step_dev is one higher,
        lr_used holds that rate and reg_loss weight_reg / 2 times the sum of
        squares of the regularised tensors before the update."""
        ws = self.workspace
        rc = _load().pcnn_momentum_sgd(_lib.ptr(self.table), _lib.ptr(self.chunk_start), self.T, self.total_chunks,
                                       float(lr), float(gamma), int(stepsize), float(momentum), float(weight_reg),
                                       _lib.ptr(self.step_dev), _lib.ptr(self.reg_loss), _lib.ptr(self.lr_used),
                                       _lib.ptr(ws), ws.numel() if ws is not None else 0, _lib.stream_ptr(stream))
        _lib.check(rc, "momentum_sgd")


def momentum_sgd_plan(params, grads, bufs, regularize=None, reg_loss=True, step_dev=None):
    """Validate the triples (params[i], grads[i], bufs[i]) and build the device
    table of one fused update over all of them (include/posecnn_train.h).

    Each tensor is a contiguous float32 device tensor; the three of a triple
    have the same number of elements; all are on one device; no two of the
    3 T tensors share memory (params and bufs are written in place, grads are
    only read).  A row block of a matrix is a contiguous slab and is fine.  A
    tensor that starts at an odd element offset of its storage takes the
    kernel's scalar path.  regularize: one bool per triple (None: all) -- the
    tensors whose gradient takes the L2 term weight_reg * w.  reg_loss=False:
    the L2 loss value is not computed.  step_dev: an existing (1,) int64
    device counter to continue from (default: a new one at 0).  Raises
    ValueError naming the argument; reads attributes only (no sync), and the
    table reaches the device by an asynchronous copy from pinned memory on the
    current stream."""
    who = "momentum_sgd_plan"
    params, grads, bufs = list(params), list(grads), list(bufs)
    T = len(params)
    if len(grads) != T or len(bufs) != T:
        raise ValueError(f"{who}: {T} params, {len(grads)} grads and {len(bufs)} bufs")
    flags = _flags(regularize, T, who)
    f32 = torch.float32
    spans = []
    device = step_dev.device if step_dev is not None else None
    for i in range(T):
        for label, t in (("params", params[i]), ("grads", grads[i]), ("bufs", bufs[i])):
            name = f"{who}: {label}[{i}]"
            _lib.require(t, f32, name=name)
            if t.numel() != params[i].numel():
                raise ValueError(f"{name}: {t.numel()} elements where params[{i}] has {params[i].numel()}")
            if device is None:
                device = t.device
            elif t.device != device:
                raise ValueError(f"{name}: on {t.device}, the set is on {device}")
            if t.numel():
                spans.append((t.data_ptr(), t.data_ptr() + 4 * t.numel(), name))
    spans.sort()
    for (_, end, a), (begin, _, b) in zip(spans, spans[1:]):
        if begin < end:
            raise ValueError(f"{b} overlaps {a[len(who) + 2:]}: the tensors of one update must not share memory")
    if step_dev is not None:
        _lib.require_counter(step_dev, f"{who}: step_dev", torch.int64)
    if device is None:
        _lib.require_gpu()
        device = torch.device("cuda", torch.cuda.current_device())
    return MomentumPlan(params, grads, bufs, flags, device, step_dev, reg_loss)


class MomentumSGD(torch.optim.Optimizer):
    """momentum_sgd_plan as a torch optimizer: one fused library call per
    parameter group and step.  Group keys: lr, momentum, weight_reg, gamma,
    stepsize (the staircase: lr * gamma^(steps // stepsize); 0: constant) and
    regularize (True, False, or one bool per parameter of the group).

    step() leaves parameters whose .grad is None out of that step's table and
    rebuilds the table (an asynchronous copy from pinned memory, no sync) when
    a parameter's, gradient's or buffer's address moved -- zero_grad(
    set_to_none=True) reallocates the gradients.  The step count of a group
    lives on the device (plans[g].step_dev), next to reg_loss and lr_used of
    the last step; state_dict() reads the counts back and carries them with
    the momentum buffers."""

    def __init__(self, params, lr=0.001, momentum=0.9, weight_reg=1e-4, gamma=0.1, stepsize=0, regularize=True):
        if lr < 0 or not 0 <= momentum < 1 or weight_reg < 0 or gamma <= 0 or stepsize < 0:
            raise ValueError("MomentumSGD: lr >= 0, 0 <= momentum < 1, weight_reg >= 0, gamma > 0, stepsize >= 0")
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_reg=weight_reg, gamma=gamma, stepsize=stepsize,
                                      regularize=regularize))
        self.plans = [None] * len(self.param_groups)
        self._counters = [None] * len(self.param_groups)

    def add_param_group(self, group):
        super().add_param_group(group)
        if hasattr(self, "plans"):
            self.plans.append(None)
            self._counters.append(None)

    def _plan(self, gi, group):
        who = "MomentumSGD"
        flags = _flags(group["regularize"], len(group["params"]), who)
        live = [(p, f) for p, f in zip(group["params"], flags) if p.grad is not None]
        params = [p.detach() for p, _ in live]
        grads = [p.grad.detach() for p, _ in live]
        bufs = []
        for p, _ in live:
            st = self.state[p]
            if "momentum_buffer" not in st:
                st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            bufs.append(st["momentum_buffer"])
        key = tuple(t.data_ptr() for trio in zip(params, grads, bufs) for t in trio)
        plan = self.plans[gi]
        if plan is None or plan.key != key or plan.flags != [f for _, f in live]:
            if self._counters[gi] is None:
                dev = params[0].device if params else torch.device("cuda", torch.cuda.current_device())
                self._counters[gi] = torch.full((1,), int(group.get("step", 0)), dtype=torch.int64, device=dev)
            plan = self.plans[gi] = momentum_sgd_plan(params, grads, bufs, [f for _, f in live],
                                                      step_dev=self._counters[gi])
        return plan

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            self._plan(gi, group).apply(group["lr"], group["momentum"], group["weight_reg"], group["gamma"],
                                        group["stepsize"])
        return loss

    def state_dict(self):
        for gi, group in enumerate(self.param_groups):
            if self._counters[gi] is not None:
                group["step"] = int(self._counters[gi].item())  # a checkpoint reads the device
            else:
                group.setdefault("step", 0)
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        # the loaded buffers are new tensors and the counts are the groups' "step": new plans on the next step
        self.plans = [None] * len(self.param_groups)
        self._counters = [None] * len(self.param_groups)
