"""The upscore layers on the GPU against tests/upscore_ref.py.

The two forward ops have a pinned order of float32 operations and are compared
bit for bit.  The backward sums have the device's own (fixed) order: on integer
inputs (gradients in [-4,4], dyadic weights) every partial sum is exact in
float32 in any order, so they must equal the float64 reference exactly -- the
test that catches a dropped or doubled pixel; on normal inputs they must lie
within the worst-case bound of float32 summation in any order
(upscore_ref.sum_bound).  Every output is prefilled with NaN and every
workspace with 0xFF before each call.
"""
import functools

import numpy as np
import pytest
import torch

import upscore_ref as ref

pytestmark = pytest.mark.gpu

#           (B, h, w, Ch, s)
GENERIC = [(2, 3, 5, 22, 8),    # Ch not a multiple of 4, borders
           (1, 1, 1, 4, 8),     # every output has one tap
           (1, 2, 3, 128, 2),
           (1, 4, 4, 1, 16),
           (2, 7, 9, 64, 8),
           (1, 5, 3, 66, 4),
           # beyond the issue's table, for the paths the kernels take at other sizes:
           (1, 2, 9, 128, 8),   # two column tiles per row, forward and backward
           (1, 2, 2, 200, 16),  # the backward's channels in two chunks (192 + 8)
           (1, 1, 2, 2050, 2)]  # the forward's channels in two chunks (2048 + 2), three column tiles
#           (B, h, w, C, s)
COMPACT = [(2, 3, 5, 22, 8),
           (1, 1, 1, 1, 8),
           (1, 6, 4, 4, 2),
           (1, 2, 3, 21, 16),
           (2, 9, 7, 22, 8),
           (1, 15, 20, 22, 8)]  # several workgroups
PATTERNS = ["random", "blocky", "one_class", "missing_class"]


def dev(a):
    return torch.tensor(np.asarray(a), device="cuda")


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return host(t).view(np.int32)


def nan_like(shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def labels(B, H, W, C, pattern, rng):
    """Label map (B,H,W) int32 with -1, C, C+5 and -100 planted in it."""
    if pattern == "random":
        lab = rng.integers(0, C, size=(B, H, W))
    elif pattern == "blocky":   # rectangles of one class on background 0
        lab = np.zeros((B, H, W), np.int64)
        for _ in range(6 * B):
            b, y, x = rng.integers(0, B), rng.integers(0, H), rng.integers(0, W)
            lab[b, y:y + rng.integers(1, H // 2 + 2), x:x + rng.integers(1, W // 2 + 2)] = rng.integers(0, C)
    elif pattern == "one_class":
        lab = np.full((B, H, W), C - 1, np.int64)
    else:                       # class `gone` has no pixel (C = 1: no live pixel at all)
        gone = C // 2
        lab = rng.integers(0, C, size=(B, H, W))
        lab[lab == gone] = gone + 1 if gone + 1 < C else -1
    flat = lab.reshape(-1)
    flat[rng.choice(flat.size, 4, replace=False)] = [-1, C, C + 5, -100]
    return lab.astype(np.int32)


# ---------------------------------------------------------------- the generic pair

@functools.lru_cache(maxsize=None)
def generic_case(shape, integers=False):
    """Host inputs, read-only: x, bias, d_y and a forward output y to mask with."""
    B, h, w, Ch, s = shape
    rng = np.random.default_rng(100 * sum(shape) + integers)
    if integers:
        x = rng.integers(-8, 9, size=(B, h, w, Ch)).astype(np.float32)
        bias = rng.integers(-4, 5, size=Ch).astype(np.float32)
        d_y = rng.integers(-4, 5, size=(B, s * h, s * w, Ch)).astype(np.float32)
    else:
        x = rng.standard_normal((B, h, w, Ch)).astype(np.float32)
        bias = rng.standard_normal(Ch).astype(np.float32)
        d_y = rng.standard_normal((B, s * h, s * w, Ch)).astype(np.float32)
    y = ref.upscore_fwd_ref(x, s, bias=bias, relu=True)
    for a in (x, bias, d_y, y):
        a.setflags(write=False)
    return x, bias, d_y, y


def run_fwd(x, shape, bias=None, relu=False, stream=None):
    from posecnn_amd import _lib
    B, h, w, Ch, s = shape
    st = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(st):
        y = nan_like((B, s * h, s * w, Ch))
        rc = _lib.load().pcnn_upscore_fwd(_lib.ptr(x), B, h, w, Ch, s, _lib.ptr(bias), int(relu), _lib.ptr(y),
                                          _lib.stream_ptr(st))
    assert rc == 0, rc
    return y


def run_bwd(d_y, y, shape, want_bias=True, stream=None):
    """(d_x, guard): d_bias is the middle row of the NaN guard (3, Ch), or not passed at all."""
    from posecnn_amd import _lib
    B, h, w, Ch, s = shape
    lib = _lib.load()
    st = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(st):
        d_x = nan_like((B, h, w, Ch))
        guard = nan_like((3, Ch))
        ws = _lib.workspace(lib.pcnn_upscore_bwd_workspace_size(B, h, w, Ch, s), d_y.device, "upscore_bwd_test", st)
        ws.fill_(0xFF)
        if want_bias:
            rc = lib.pcnn_upscore_bwd(_lib.ptr(d_y), _lib.ptr(y), B, h, w, Ch, s, _lib.ptr(d_x), _lib.ptr(guard[1]),
                                      _lib.ptr(ws), ws.numel(), _lib.stream_ptr(st))
        else:
            rc = lib.pcnn_upscore_bwd(_lib.ptr(d_y), _lib.ptr(y), B, h, w, Ch, s, _lib.ptr(d_x), None, None, 0,
                                      _lib.stream_ptr(st))
    assert rc == 0, rc
    return d_x, guard


@pytest.mark.parametrize("shape", GENERIC)
def test_forward_bit_for_bit(hip, shape):
    x, bias, _, y_relu = generic_case(shape)
    s = shape[4]
    xd, bd = dev(x), dev(bias)
    np.testing.assert_array_equal(bits(run_fwd(xd, shape)), ref.upscore_fwd_ref(x, s).view(np.int32))
    np.testing.assert_array_equal(bits(run_fwd(xd, shape, bd)), ref.upscore_fwd_ref(x, s, bias=bias).view(np.int32))
    np.testing.assert_array_equal(bits(run_fwd(xd, shape, bd, True)), y_relu.view(np.int32))
    np.testing.assert_array_equal(bits(run_fwd(xd, shape, None, True)),
                                  ref.upscore_fwd_ref(x, s, relu=True).view(np.int32))
    if x.size >= 64:
        assert (y_relu == 0).any() and (y_relu > 0).any()
    # zero padding, not clamping: a constant input is darker at the border
    ones = host(run_fwd(torch.ones_like(xd), shape))
    assert ones.max() == 1.0 or shape[1] == 1 or shape[2] == 1
    assert ones[0, 0, 0, 0] == ((s + 1) / (2.0 * s)) ** 2


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("shape", GENERIC)
def test_backward_on_integers_is_exact(hip, shape, masked):
    _, _, d_y, y = generic_case(shape, integers=True)
    y = y if masked else None
    r = ref.upscore_bwd_ref(d_y, shape[4], y=y)
    d_x, guard = run_bwd(dev(d_y), None if y is None else dev(y), shape)
    np.testing.assert_array_equal(host(d_x), r["d_x"])
    np.testing.assert_array_equal(host(guard[1]), r["d_bias"])
    assert torch.isnan(guard[0]).all() and torch.isnan(guard[2]).all()
    assert r["d_x"].any()
    if masked and d_y.size >= 4096:
        assert (y > 0).any() and (y == 0).any()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("shape", GENERIC)
def test_backward_within_the_worst_case_bound(hip, shape, masked):
    _, _, d_y, y = generic_case(shape)
    y = y if masked else None
    r = ref.upscore_bwd_ref(d_y, shape[4], y=y)
    d_x, guard = run_bwd(dev(d_y), None if y is None else dev(y), shape)
    got_x, got_b = host(d_x), host(guard[1])
    assert np.isfinite(got_x).all() and np.isfinite(got_b).all()
    ex, eb = np.abs(got_x - r["d_x"]), np.abs(got_b - r["d_bias"])
    bx = ref.sum_bound(r["n_x"][None, :, :, None], r["abs_x"])
    bb = ref.sum_bound(r["n_b"], r["abs_b"])
    print(f"{shape} masked={masked}: d_x max err / bound {np.max(ex / np.maximum(bx, 1e-300)):.3f}, "
          f"d_bias {np.max(eb / np.maximum(bb, 1e-300)):.3f}")
    assert (ex <= bx).all() and (eb <= bb).all()


@pytest.mark.parametrize("shape", [GENERIC[0], GENERIC[2], GENERIC[4]])
def test_backward_without_bias_and_on_a_second_stream(hip, shape):
    _, _, d_y, y = generic_case(shape)
    gd, yd = dev(d_y), dev(y)
    d_x, guard = run_bwd(gd, yd, shape)
    alone, untouched = run_bwd(gd, yd, shape, want_bias=False)   # no d_bias, no workspace
    np.testing.assert_array_equal(bits(alone), bits(d_x))
    assert torch.isnan(untouched).all()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    d_x2, guard2 = run_bwd(gd, yd, shape, stream=side)
    y2 = run_fwd(dev(generic_case(shape)[0]), shape, dev(generic_case(shape)[1]), True, stream=side)
    side.synchronize()
    np.testing.assert_array_equal(bits(d_x2), bits(d_x))
    np.testing.assert_array_equal(bits(guard2[1]), bits(guard[1]))
    np.testing.assert_array_equal(bits(y2), y.view(np.int32))


# ---------------------------------------------------------------- the class-compact pair

@functools.lru_cache(maxsize=None)
def compact_case(shape, pattern, integers=False):
    """Host inputs, read-only: z, bias, label, g."""
    B, h, w, C, s = shape
    rng = np.random.default_rng(1000 * sum(shape) + 10 * PATTERNS.index(pattern) + integers)
    label = labels(B, s * h, s * w, C, pattern, rng)
    z = rng.standard_normal((B, h, w, 3 * C)).astype(np.float32)
    bias = rng.standard_normal(3 * C).astype(np.float32)
    if integers:
        g = rng.integers(-4, 5, size=(B, s * h, s * w, 3)).astype(np.float32)
    else:
        g = rng.standard_normal((B, s * h, s * w, 3)).astype(np.float32)
    for a in (z, bias, label, g):
        a.setflags(write=False)
    return z, bias, label, g


def run_compact_fwd(z, bias, label, shape, stream=None):
    from posecnn_amd import _lib
    B, h, w, C, s = shape
    st = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(st):
        v3 = nan_like((B, s * h, s * w, 3))
        rc = _lib.load().pcnn_upscore_compact_fwd(_lib.ptr(z), _lib.ptr(bias), _lib.ptr(label), B, h, w, C, s,
                                                  _lib.ptr(v3), _lib.stream_ptr(st))
    assert rc == 0, rc
    return v3


def run_compact_bwd(label, g, shape, want=("z", "bias"), stream=None):
    """(d_z or None, guard): d_bias is the middle row of the NaN guard (3, 3C) when asked for."""
    from posecnn_amd import _lib
    B, h, w, C, s = shape
    lib = _lib.load()
    st = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(st):
        d_z = nan_like((B, h, w, 3 * C)) if "z" in want else None
        guard = nan_like((3, 3 * C))
        ws = _lib.workspace(lib.pcnn_upscore_compact_bwd_workspace_size(B, h, w, C, s), g.device,
                            "upscore_compact_bwd_test", st)
        ws.fill_(0xFF)
        with_bias = "bias" in want
        rc = lib.pcnn_upscore_compact_bwd(_lib.ptr(label), _lib.ptr(g), B, h, w, C, s, _lib.ptr(d_z),
                                          _lib.ptr(guard[1]) if with_bias else None,
                                          _lib.ptr(ws) if with_bias else None, ws.numel() if with_bias else 0,
                                          _lib.stream_ptr(st))
    assert rc == 0, rc
    return d_z, guard


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", COMPACT)
def test_compact_forward_bit_for_bit(hip, shape, pattern):
    z, bias, label, _ = compact_case(shape, pattern)
    B, h, w, C, s = shape
    zd, bd, ld = dev(z), dev(bias), dev(label)
    v3 = run_compact_fwd(zd, bd, ld, shape)
    np.testing.assert_array_equal(bits(v3), ref.upscore_compact_fwd_ref(z, bias, label, s).view(np.int32))
    dense = run_fwd(zd, (B, h, w, 3 * C, s), bd)   # op 1, gathered on the host
    np.testing.assert_array_equal(bits(v3), ref.gather_class(host(dense), label).view(np.int32))
    assert (host(v3)[~ref.live(label, C)] == 0).all()


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", COMPACT)
def test_compact_backward_on_integers_is_exact(hip, shape, pattern):
    _, _, label, g = compact_case(shape, pattern, integers=True)
    B, h, w, C, s = shape
    r = ref.upscore_compact_bwd_ref(label, g, C, s)
    d_z, guard = run_compact_bwd(dev(label), dev(g), shape)
    np.testing.assert_array_equal(host(d_z), r["d_z"])
    np.testing.assert_array_equal(host(guard[1]), r["d_bias"])
    assert torch.isnan(guard[0]).all() and torch.isnan(guard[2]).all()
    if pattern == "missing_class":
        gone = C // 2
        assert r["n_b"][3 * gone] == 0 and (host(d_z)[..., 3 * gone:3 * gone + 3] == 0).all()
    if C > 1 or pattern != "missing_class":
        assert r["d_z"].any() and r["d_bias"].any()


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", COMPACT)
def test_compact_backward_within_the_worst_case_bound(hip, shape, pattern):
    _, _, label, g = compact_case(shape, pattern)
    B, h, w, C, s = shape
    r = ref.upscore_compact_bwd_ref(label, g, C, s)
    d_z, guard = run_compact_bwd(dev(label), dev(g), shape)
    got_z, got_b = host(d_z), host(guard[1])
    assert np.isfinite(got_z).all() and np.isfinite(got_b).all()
    ez, eb = np.abs(got_z - r["d_z"]), np.abs(got_b - r["d_bias"])
    bz, bb = ref.sum_bound(r["n_z"], r["abs_z"]), ref.sum_bound(r["n_b"], r["abs_b"])
    print(f"{shape} {pattern}: d_z max err / bound {np.max(ez / np.maximum(bz, 1e-300)):.3f}, "
          f"d_bias {np.max(eb / np.maximum(bb, 1e-300)):.3f}")
    assert (ez <= bz).all() and (eb <= bb).all()


@pytest.mark.parametrize("shape", [COMPACT[0], COMPACT[3], COMPACT[5]])
def test_compact_outputs_alone_and_on_a_second_stream(hip, shape):
    z, bias, label, g = compact_case(shape, "blocky")
    ld, gd = dev(label), dev(g)
    d_z, guard = run_compact_bwd(ld, gd, shape)
    z_alone, untouched = run_compact_bwd(ld, gd, shape, want=("z",))
    np.testing.assert_array_equal(bits(z_alone), bits(d_z))
    assert torch.isnan(untouched).all()
    none, guard_alone = run_compact_bwd(ld, gd, shape, want=("bias",))
    assert none is None
    np.testing.assert_array_equal(bits(guard_alone), bits(guard))   # NaN rows around the same d_bias
    side = torch.cuda.Stream()
    zd, bd = dev(z), dev(bias)
    v3 = run_compact_fwd(zd, bd, ld, shape)
    torch.cuda.synchronize()
    d_z2, guard2 = run_compact_bwd(ld, gd, shape, stream=side)
    v32 = run_compact_fwd(zd, bd, ld, shape, stream=side)
    side.synchronize()
    np.testing.assert_array_equal(bits(d_z2), bits(d_z))
    np.testing.assert_array_equal(bits(guard2), bits(guard))
    np.testing.assert_array_equal(bits(v32), bits(v3))


def test_argument_validation(hip):
    """Rejected before any launch: 1 = PCNN_EINVAL, 3 = PCNN_ECAPACITY; the queries answer 0."""
    from posecnn_amd import _lib
    t = torch.zeros(4096, device="cuda")
    p, lab = _lib.ptr(t), _lib.ptr(torch.zeros(4096, dtype=torch.int32, device="cuda"))
    st = _lib.stream_ptr()
    assert hip.pcnn_upscore_fwd(p, 1, 2, 2, 4, 3, None, 0, p, st) == 1          # stride
    assert hip.pcnn_upscore_fwd(p, 1, 2, 2, 4, 32, None, 0, p, st) == 1
    assert hip.pcnn_upscore_fwd(None, 1, 2, 2, 4, 8, None, 0, p, st) == 1       # NULL input
    assert hip.pcnn_upscore_fwd(p, 1, 2, 2, 4, 8, None, 0, None, st) == 1
    assert hip.pcnn_upscore_fwd(p, 0, 2, 2, 4, 8, None, 0, p, st) == 1          # dimensions
    assert hip.pcnn_upscore_fwd(p, 1, 2, -2, 4, 8, None, 0, p, st) == 1
    assert hip.pcnn_upscore_fwd(p, 64, 256, 256, 8, 16, None, 0, p, st) == 1    # 2^33 outputs
    assert hip.pcnn_upscore_fwd(p, 1, 1 << 15, 1 << 15, 1, 2, None, 0, p, st) == 1   # B*H*W*3 = 3 * 2^32
    assert hip.pcnn_upscore_bwd(p, None, 1, 2, 2, 4, 5, p, None, None, 0, st) == 1
    assert hip.pcnn_upscore_bwd(p, None, 1, 2, 2, 4, 8, None, None, None, 0, st) == 1
    assert hip.pcnn_upscore_bwd(p, None, 1, 2, 2, 4, 8, p, p, None, 0, st) == 1      # d_bias needs the workspace
    assert hip.pcnn_upscore_bwd(p, None, 1, 2, 2, 4, 8, p, p, p, 4, st) == 3
    assert hip.pcnn_upscore_compact_fwd(p, None, lab, 1, 2, 2, 2, 8, p, st) == 1     # bias is required
    assert hip.pcnn_upscore_compact_fwd(p, p, lab, 1, 2, 2, 0, 8, p, st) == 1
    assert hip.pcnn_upscore_compact_fwd(p, p, lab, 1, 2, 2, 2, 6, p, st) == 1
    assert hip.pcnn_upscore_compact_bwd(lab, p, 1, 2, 2, 2, 8, None, None, None, 0, st) == 1   # no output
    assert hip.pcnn_upscore_compact_bwd(None, p, 1, 2, 2, 2, 8, p, None, None, 0, st) == 1
    assert hip.pcnn_upscore_compact_bwd(lab, p, 1, 2, 2, 2, 8, p, p, p, 4, st) == 3
    assert hip.pcnn_upscore_compact_bwd(lab, p, 1, 2, 2, 2, 7, p, None, None, 0, st) == 1
    assert hip.pcnn_upscore_bwd_workspace_size(1, 2, 2, 4, 3) == 0
    assert hip.pcnn_upscore_bwd_workspace_size(0, 2, 2, 4, 8) == 0
    assert hip.pcnn_upscore_bwd_workspace_size(64, 256, 256, 8, 16) == 0
    assert hip.pcnn_upscore_compact_bwd_workspace_size(1, 2, 2, 0, 8) == 0
    assert hip.pcnn_upscore_compact_bwd_workspace_size(1, 2, 2, 2, 12) == 0
    assert hip.pcnn_upscore_bwd_workspace_size(2, 3, 5, 22, 8) > 0
    assert hip.pcnn_upscore_compact_bwd_workspace_size(1, 15, 20, 22, 8) >= 10 * 66 * 4   # several partials
    torch.cuda.synchronize()
    assert (t == 0).all()


def test_wrappers(hip):
    from posecnn_amd import upscore as up
    shape = GENERIC[0]
    B, h, w, Ch, s = shape
    x, bias, d_y, y = generic_case(shape)
    xd, bd, gd, yd = dev(x), dev(bias), dev(d_y), dev(y)
    out = up.upscore(xd, s, bias=bd, relu=True)
    assert out.shape == (B, s * h, s * w, Ch)
    np.testing.assert_array_equal(bits(out), y.view(np.int32))
    into = nan_like((B, s * h, s * w, Ch))
    assert up.upscore(xd.double(), s, bias=bd.double(), relu=True, out=into) is into   # float64 in: its float32 copy
    np.testing.assert_array_equal(bits(into), y.view(np.int32))
    d_x, guard = run_bwd(gd, yd, shape)
    wx, wb = up.upscore_bwd(gd.double(), s, y=yd, want_bias=True)
    np.testing.assert_array_equal(bits(wx), bits(d_x))
    np.testing.assert_array_equal(bits(wb), bits(guard[1]))
    np.testing.assert_array_equal(bits(up.upscore_bwd(gd, s, y=yd)), bits(d_x))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    on_side = up.upscore(xd, s, bias=bd, relu=True, stream=side)
    side.synchronize()
    np.testing.assert_array_equal(bits(on_side), y.view(np.int32))
    with pytest.raises(ValueError):
        up.upscore(xd, 3)
    with pytest.raises(ValueError):
        up.upscore(xd, s, bias=bd[:-1])
    with pytest.raises(ValueError):
        up.upscore(xd[0], s)
    with pytest.raises(ValueError):
        up.upscore(xd, s, out=into[:, :-1])
    with pytest.raises(ValueError):
        up.upscore_bwd(gd[:, :-1], s)
    with pytest.raises(ValueError):
        up.upscore_bwd(gd, s, y=yd[..., :-1])
    cshape = COMPACT[0]
    B, h, w, C, s = cshape
    z, cb, label, g = compact_case(cshape, "blocky")
    zd, cbd, ld, g3 = dev(z), dev(cb), dev(label), dev(g)
    v3 = run_compact_fwd(zd, cbd, ld, cshape)
    np.testing.assert_array_equal(bits(up.upscore_compact(zd.double(), cbd, ld.long(), s)), bits(v3))   # int64 labels
    d_z, cguard = run_compact_bwd(ld, g3, cshape)
    both = up.upscore_compact_bwd(ld.long(), g3.double(), C, s)
    assert sorted(both) == ["bias", "z"] and both["z"].shape == (B, h, w, 3 * C) and both["bias"].shape == (3 * C,)
    np.testing.assert_array_equal(bits(both["z"]), bits(d_z))
    np.testing.assert_array_equal(bits(both["bias"]), bits(cguard[1]))
    only = up.upscore_compact_bwd(ld, g3, C, s, want=("bias",))
    assert list(only) == ["bias"]
    np.testing.assert_array_equal(bits(only["bias"]), bits(cguard[1]))
    with pytest.raises(ValueError):
        up.upscore_compact(zd, cbd, ld, 5)
    with pytest.raises(ValueError):
        up.upscore_compact(zd, cbd, ld[:, :-1], s)      # label shape does not match z and the stride
    with pytest.raises(ValueError):
        up.upscore_compact(zd, cbd, ld, 4)
    with pytest.raises(ValueError):
        up.upscore_compact(zd, cbd[:-1], ld, s)
    with pytest.raises(ValueError):
        up.upscore_compact(zd[..., :-1], cbd, ld, s)    # channels not 3C
    with pytest.raises(ValueError):
        up.upscore_compact_bwd(ld, g3[..., :2], C, s)
    with pytest.raises(ValueError):
        up.upscore_compact_bwd(ld, g3, C, s, want=())
    with pytest.raises(ValueError):
        up.upscore_compact_bwd(ld, g3, C, s, want=("label",))


def test_graph_capture_and_replay(hip):
    from posecnn_amd import _lib
    shape, cshape = GENERIC[0], COMPACT[0]
    B, h, w, Ch, s = shape
    C = cshape[3]
    x, bias, d_y, y = generic_case(shape)
    z, cb, label, g = compact_case(cshape, "blocky")
    xd, bd, gd = dev(x), dev(bias), dev(d_y)
    zd, cbd, ld, g3 = dev(z), dev(cb), dev(label), dev(g)
    want_dx, want_guard = run_bwd(gd, dev(y), shape)
    want_v3 = run_compact_fwd(zd, cbd, ld, cshape)
    want_dz, want_cguard = run_compact_bwd(ld, g3, cshape)
    out = {"y": torch.empty((B, s * h, s * w, Ch), device="cuda"), "d_x": torch.empty((B, h, w, Ch), device="cuda"),
           "d_b": torch.empty((Ch,), device="cuda"), "v3": torch.empty((B, s * h, s * w, 3), device="cuda"),
           "d_z": torch.empty((B, h, w, 3 * C), device="cuda"), "d_cb": torch.empty((3 * C,), device="cuda")}
    ws = torch.empty(hip.pcnn_upscore_bwd_workspace_size(*shape), dtype=torch.uint8, device="cuda")
    cws = torch.empty(hip.pcnn_upscore_compact_bwd_workspace_size(*cshape), dtype=torch.uint8, device="cuda")

    def call():
        st = _lib.stream_ptr()
        assert hip.pcnn_upscore_fwd(_lib.ptr(xd), B, h, w, Ch, s, _lib.ptr(bd), 1, _lib.ptr(out["y"]), st) == 0
        assert hip.pcnn_upscore_bwd(_lib.ptr(gd), _lib.ptr(out["y"]), B, h, w, Ch, s, _lib.ptr(out["d_x"]),
                                    _lib.ptr(out["d_b"]), _lib.ptr(ws), ws.numel(), st) == 0
        assert hip.pcnn_upscore_compact_fwd(_lib.ptr(zd), _lib.ptr(cbd), _lib.ptr(ld), *cshape[:3], C, s,
                                            _lib.ptr(out["v3"]), st) == 0
        assert hip.pcnn_upscore_compact_bwd(_lib.ptr(ld), _lib.ptr(g3), *cshape[:3], C, s, _lib.ptr(out["d_z"]),
                                            _lib.ptr(out["d_cb"]), _lib.ptr(cws), cws.numel(), st) == 0
    call()   # eager first: code objects loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for t in out.values():
        t.fill_(float("nan"))
    ws.fill_(0xFF)
    cws.fill_(0xFF)
    graph.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(out["y"]), y.view(np.int32))
    np.testing.assert_array_equal(bits(out["d_x"]), bits(want_dx))
    np.testing.assert_array_equal(bits(out["d_b"]), bits(want_guard[1]))
    np.testing.assert_array_equal(bits(out["v3"]), bits(want_v3))
    np.testing.assert_array_equal(bits(out["d_z"]), bits(want_dz))
    np.testing.assert_array_equal(bits(out["d_cb"]), bits(want_cguard[1]))


# ---------------------------------------------------------------- the modules

HEAD = (2, 3, 5, 128, 22, 8)   # (B, h, w, K, C, s)


def tap_counts(h, w, s):
    """(H, W): the number of low-res pixels an output taps."""
    return np.outer((ref.matrix(h, s) > 0).sum(axis=1), (ref.matrix(w, s) > 0).sum(axis=1))


def check(name, got, want, n, abs_sum, e_ref):
    """got within the worst-case bound of `n` float32 terms of magnitude sum
    `abs_sum` of the float64 value; the ratio to E_ref is printed only."""
    got = host(got).astype(np.float64)
    assert got.shape == want.shape, name
    assert np.isfinite(got).all(), name
    err = np.abs(got - want)
    bound = ref.sum_bound(n, abs_sum)
    print(f"{name}: max err {err.max():.3e}, max err / bound {np.max(err / np.maximum(bound, 1e-300)):.4f}, "
          f"max err / E_ref {err.max() / max(e_ref, 1e-300):.2f} (E_ref {e_ref:.3e})")
    assert (err <= bound).all(), name


def test_upscore_module(hip):
    from posecnn_amd.pth import Upscore
    shape = GENERIC[5]
    B, h, w, Ch, s = shape
    x, _, d_y, _ = generic_case(shape)
    for relu in (False, True):
        xd = dev(x).requires_grad_(True)
        out = Upscore(s, relu=relu)(xd)
        y = ref.upscore_fwd_ref(x, s, relu=relu)
        np.testing.assert_array_equal(bits(out), y.view(np.int32))
        out.backward(dev(d_y))
        want, _ = run_bwd(dev(d_y), dev(y) if relu else None, shape, want_bias=False)
        np.testing.assert_array_equal(bits(xd.grad), bits(want))
    with pytest.raises(ValueError):
        Upscore(3)


def test_vertex_head_compact(hip):
    """Output and gradients against the reference's order in float64: the
    upscore of x, then the 1x1 conv at the pixel's class.  The head computes
    the conv first (z = x W, torch.matmul) and the upscore of z: the same
    elementary terms tap weight * x * W (forward), tap weight * g * W (d_x) and
    tap weight * x * g (d_weight), summed in another order, so each result lies
    within (n + 1) 2^-24 sum |terms| of the float64 value for its n terms."""
    from posecnn_amd import losses
    from posecnn_amd.pth import VertexHeadCompact, VertexLoss, VertexPredCompact
    B, h, w, K, C, s = HEAD
    H, W = s * h, s * w
    rng = np.random.default_rng(11)
    label = labels(B, H, W, C, "blocky", rng)
    x = rng.standard_normal((B, h, w, K)).astype(np.float32)
    wt = (rng.standard_normal((K, 3 * C)) * 0.1).astype(np.float32)
    bias = rng.standard_normal(3 * C).astype(np.float32)
    vertex3 = rng.standard_normal((B, H, W, 3)).astype(np.float32)
    donor = VertexPredCompact(K, C)
    with torch.no_grad():
        donor.weight.copy_(torch.tensor(wt))
        donor.bias.copy_(torch.tensor(bias))
    mod = VertexHeadCompact(K, C, stride=s)
    mod.load_state_dict(donor.state_dict())   # the same names and shapes
    mod = mod.cuda()
    np.testing.assert_array_equal(host(mod.weight), wt)
    xd, ld, v3 = dev(x).requires_grad_(True), dev(label), dev(vertex3)
    pred = mod(xd, ld)
    assert pred.shape == (B, H, W, 3)
    VertexLoss(sigma=1.0, w_inside=10.0, num_classes=C)(pred, ld, v3).backward()
    _, d3 = losses.vertex_loss_compact(pred.detach(), ld, v3, C, 10.0, 1.0, want_grad=True)
    g3 = host(d3)
    assert np.abs(g3).max() > 0
    # the reference's order
    x64, w64 = x.astype(np.float64), wt.astype(np.float64)
    up64 = ref.upscore_fwd_ref(x64, s, mode="f64")
    up_abs = ref.upscore_fwd_ref(np.abs(x64), s, mode="f64")
    lv = ref.live(label, C)
    taps_px = tap_counts(h, w, s)[None]
    pred64 = ref.gather_class(up64 @ w64 + bias, label)
    pred_abs = ref.gather_class(up_abs @ np.abs(w64) + np.abs(bias), label)
    up32 = ref.upscore_fwd_ref(x, s)
    e_pred = np.abs(ref.gather_class(up32 @ wt + bias, label) - pred64).max()
    check("pred", pred, pred64, (taps_px * K + 1)[..., None], pred_abs, e_pred)
    assert (host(pred)[~lv] == 0).all()
    G = ref.scatter_class(g3, label, C)
    rb = ref.upscore_bwd_ref(G @ w64.T, s)
    n_live = ref.upscore_compact_bwd_ref(label, g3, C, s)["n_z"].reshape(B, h, w, C, 3)[..., 0].sum(axis=-1)
    dx_abs = ref.upscore_bwd_ref(np.abs(G) @ np.abs(w64).T, s)["d_x"]
    G32 = G.astype(np.float32)
    e_dx = np.abs(ref.upscore_bwd_ref((G32 @ wt.T).astype(np.float64), s)["d_x"] - rb["d_x"]).max()
    check("d_x_low", xd.grad, rb["d_x"], (3 * n_live)[..., None], dx_abs, e_dx)
    dw64 = up64.reshape(-1, K).T @ G.reshape(-1, 3 * C)
    dw_abs = up_abs.reshape(-1, K).T @ np.abs(G).reshape(-1, 3 * C)
    n_w = np.array([(taps_px * (label == c)).sum() for c in range(C)])
    e_dw = np.abs((up32.reshape(-1, K).T @ G32.reshape(-1, 3 * C)).astype(np.float64) - dw64).max()
    check("d_weight", mod.weight.grad, dw64, np.repeat(n_w, 3)[None, :], dw_abs, e_dw)
    n_c = np.array([(label == c).sum() for c in range(C)])
    e_db = np.abs(G32.reshape(-1, 3 * C).sum(axis=0, dtype=np.float32) - G.sum(axis=(0, 1, 2))).max()
    check("d_bias", mod.bias.grad, G.sum(axis=(0, 1, 2)), np.repeat(n_c, 3), np.abs(G).sum(axis=(0, 1, 2)), e_db)
    assert mod.weight.grad.abs().max().item() > 0 and mod.bias.grad.abs().max().item() > 0
    # only the gradients autograd needs: frozen parameters, a feature map that needs none
    mod2 = VertexHeadCompact(K, C, stride=s).cuda()
    mod2.load_state_dict(mod.state_dict())
    mod2.weight.requires_grad_(False)
    pred2 = mod2(dev(x), ld)
    np.testing.assert_array_equal(bits(pred2), bits(pred))
    VertexLoss(sigma=1.0, w_inside=10.0, num_classes=C)(pred2, ld, v3).backward()
    assert mod2.weight.grad is None
    np.testing.assert_array_equal(bits(mod2.bias.grad), bits(mod.bias.grad))
    with pytest.raises(ValueError):
        mod(xd[..., :-1], ld)
    with pytest.raises(ValueError):
        mod(xd, ld[:, :-1])


def test_score_head(hip):
    """relu(upscore(x W) + b) and its gradients under SegmentationLoss against
    the reference's order in float64, relu(upscore(x) W + b); the gradients'
    ReLU mask is the device output's (the output itself is checked first)."""
    from posecnn_amd import losses
    from posecnn_amd.pth import ScoreHead, SegmentationLoss
    B, h, w, K, C, s = HEAD
    H, W = s * h, s * w
    rng = np.random.default_rng(12)
    gt = np.clip(labels(B, H, W, C, "blocky", rng), 0, C - 1)
    x = rng.standard_normal((B, h, w, K)).astype(np.float32)
    wt = (rng.standard_normal((K, C)) * 0.1).astype(np.float32)
    bias = rng.standard_normal(C).astype(np.float32)
    mod = ScoreHead(K, C, stride=s).cuda()
    assert mod.weight.shape == (K, C) and mod.bias.shape == (C,)
    with torch.no_grad():
        mod.weight.copy_(dev(wt))
        mod.bias.copy_(dev(bias))
    xd, gtd = dev(x).requires_grad_(True), dev(gt)
    score = mod(xd)
    assert score.shape == (B, H, W, C)
    loss, label_2d = SegmentationLoss(1.0)(score, gtd)
    loss.backward()
    _, out = losses.seg_loss(score.detach(), gtd, 1.0, want=("d_score",))
    x64, w64 = x.astype(np.float64), wt.astype(np.float64)
    up64 = ref.upscore_fwd_ref(x64, s, mode="f64")
    up_abs = ref.upscore_fwd_ref(np.abs(x64), s, mode="f64")
    up32 = ref.upscore_fwd_ref(x, s)
    taps_px = tap_counts(h, w, s)[None]
    score64 = np.maximum(up64 @ w64 + bias, 0.0)
    e_score = np.abs(np.maximum(up32 @ wt + bias, 0) - score64).max()
    check("score", score, score64, (taps_px * K + 1)[..., None], up_abs @ np.abs(w64) + np.abs(bias), e_score)
    got = host(score)
    assert (got == 0).any() and (got > 0).any() and (got >= 0).all()
    G = np.where(got > 0, host(out["d_score"]).astype(np.float64), 0.0)
    assert np.abs(G).max() > 0
    G32 = G.astype(np.float32)
    rb = ref.upscore_bwd_ref(G @ w64.T, s)
    dx_abs = ref.upscore_bwd_ref(np.abs(G) @ np.abs(w64).T, s)["d_x"]
    e_dx = np.abs(ref.upscore_bwd_ref((G32 @ wt.T).astype(np.float64), s)["d_x"] - rb["d_x"]).max()
    check("d_x_low", xd.grad, rb["d_x"], (C * ref.term_counts(h, w, s))[None, :, :, None], dx_abs, e_dx)
    dw64 = up64.reshape(-1, K).T @ G.reshape(-1, C)
    e_dw = np.abs((up32.reshape(-1, K).T @ G32.reshape(-1, C)).astype(np.float64) - dw64).max()
    check("d_weight", mod.weight.grad, dw64, B * taps_px.sum(), up_abs.reshape(-1, K).T @ np.abs(G).reshape(-1, C),
          e_dw)
    e_db = np.abs(G32.reshape(-1, C).sum(axis=0, dtype=np.float32) - G.sum(axis=(0, 1, 2))).max()
    check("d_bias", mod.bias.grad, G.sum(axis=(0, 1, 2)), B * H * W, np.abs(G).sum(axis=(0, 1, 2)), e_db)
    # frozen parameters get no gradient
    mod2 = ScoreHead(K, C, stride=s).cuda()
    mod2.load_state_dict(mod.state_dict())
    for p in mod2.parameters():
        p.requires_grad_(False)
    x2 = dev(x).requires_grad_(True)
    score2 = mod2(x2)
    np.testing.assert_array_equal(bits(score2), bits(score))
    SegmentationLoss(1.0)(score2, gtd)[0].backward()
    assert mod2.weight.grad is None and mod2.bias.grad is None
    np.testing.assert_array_equal(bits(x2.grad), bits(xd.grad))
