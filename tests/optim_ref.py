"""The fused momentum-SGD update (include/posecnn_train.h, csrc/momentum.hip)
restated in numpy: the float32 operation order of one element, the float64
staircase of the learning rate, and the reduction of the L2 loss value in the
kernel's own shape (per-thread serial sums, wave butterflies, ascending wave
sums).  A test helper, not a test."""
import numpy as np

F = np.float32
CHUNK = 4096            # pcnn_momentum_chunk(): 256 threads x 4 quads x 4 elements
THREADS, QUADS = 256, 4
FINISH_THREADS = 1024
WAVE = 64


def lr_at(n, lr0, gamma, stepsize):
    """(float)(lr0 gamma^(n // stepsize)): float64, n // stepsize multiplications left to right, rounded once."""
    x, g = np.float64(F(lr0)), np.float64(F(gamma))
    for _ in range(int(n) // int(stepsize) if stepsize > 0 else 0):
        x = x * g
    return F(x)


def update(w, g, m, lr, momentum, weight_reg, regularize=True):
    """One update of float32 arrays; returns (w', m').  Every operation is rounded to float32 on its own."""
    w, g, m = (np.asarray(a, F) for a in (w, g, m))
    lr, momentum, weight_reg = F(lr), F(momentum), F(weight_reg)
    g2 = g + weight_reg * w if regularize else g
    m2 = momentum * m + g2
    u = lr * m2
    return w - u, m2


def update64(w, g, m, lr, momentum, weight_reg, regularize=True):
    """The same update in float64 (the yardstick of the float32 order's error)."""
    w, g, m = (np.asarray(a, np.float64) for a in (w, g, m))
    g2 = g + weight_reg * w if regularize else g
    m2 = momentum * m + g2
    return w - lr * m2, m2


def _butterfly(v):
    """v (..., 64): every lane adds its partner's value for the offsets 32, 16, ..., 1; lane 0's result."""
    lanes = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ o]
    return v[..., 0]


def chunk_partials(w):
    """The float32 partial sum of w^2 of every chunk of one tensor, in the
    kernel's shape: thread t owns the elements 4 (t + 256 j) + k and adds
    their squares to 0 in the order j = 0..3 (outer), k = 0..3; a wave adds
    as a butterfly; the four waves as (s0 + s1) + (s2 + s3)."""
    w = np.asarray(w, F).ravel()
    n_chunks = (w.size + CHUNK - 1) // CHUNK
    pad = np.zeros(n_chunks * CHUNK, F)
    pad[:w.size] = w
    sq = (pad * pad).reshape(n_chunks, QUADS, THREADS, 4)
    acc = np.zeros((n_chunks, THREADS), F)
    for j in range(QUADS):
        for k in range(4):
            acc = acc + sq[:, j, :, k]   # (the padding adds +0: the sum is unchanged)
    s = _butterfly(acc.reshape(n_chunks, THREADS // WAVE, WAVE))
    assert s.dtype == F
    return (s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])


def reg_loss(weights, flags, weight_reg):
    """weight_reg / 2 times the sum of squares of the flagged tensors (in table
    order), reduced as the two kernels do: the chunks' float32 partials (0 for
    an unflagged tensor's chunks), then in float64 thread t of 1024 adds the
    chunks t, t + 1024, ... in ascending order, a wave adds as a butterfly,
    the 16 wave sums are added in ascending order; one rounding to float32."""
    parts = [chunk_partials(w) if f else np.zeros((np.asarray(w).size + CHUNK - 1) // CHUNK, F)
             for w, f in zip(weights, flags)]
    p = np.concatenate(parts + [np.zeros(0, F)]).astype(np.float64)
    rows = (p.size + FINISH_THREADS - 1) // FINISH_THREADS
    pad = np.zeros(max(rows, 1) * FINISH_THREADS, np.float64)
    pad[:p.size] = p
    acc = np.zeros(FINISH_THREADS, np.float64)
    for r in pad.reshape(-1, FINISH_THREADS):
        acc = acc + r
    waves = _butterfly(acc.reshape(FINISH_THREADS // WAVE, WAVE))
    total = waves[0]
    for s in waves[1:]:
        total = total + s
    return F((np.float64(F(weight_reg)) * 0.5) * total)


def reg_loss64(weights, flags, weight_reg):
    return float(weight_reg) * 0.5 * sum(float((np.asarray(w, np.float64) ** 2).sum())
                                         for w, f in zip(weights, flags) if f)


def apply(weights, grads, moms, flags, n, lr0, momentum, weight_reg, gamma=0.1, stepsize=0):
    """One pcnn_momentum_sgd call at step count n on lists of float32 arrays:
    returns (new weights, new momenta, reg_loss, lr used); the count is then n + 1."""
    lr = lr_at(n, lr0, gamma, stepsize)
    loss = reg_loss(weights, flags, weight_reg)
    out = [update(w, g, m, lr, momentum, weight_reg, f) for w, g, m, f in zip(weights, grads, moms, flags)]
    return [o[0] for o in out], [o[1] for o in out], loss, lr
