"""The backward of the class-compact vertex_pred layer on the GPU against
tests/vertex_pred_ref.py.

d_feat has a pinned order of float32 operations and is compared as floats,
element for element.  The sums d_weights and d_bias have the device's own
(fixed) order: on integer inputs every partial sum is an integer below 2^24, so
float32 addition is exact in any order and they must equal the reference
exactly -- the test that catches a dropped, doubled or misrouted pixel; on
random normal inputs they must lie within the worst-case bound of float32
summation in any order (vertex_pred_ref.sum_bounds) of the float64 reference.
Every output is prefilled with NaN before each call.
"""
import functools

import numpy as np
import pytest
import torch

import vertex_pred_ref as ref

pytestmark = pytest.mark.gpu

#          (B, H, W, K, C)
SHAPES = [(2, 24, 32, 128, 22),   # the real K and C
          (1, 9, 13, 16, 4),      # ragged pixel count
          (1, 5, 7, 4, 1),        # smallest K and C
          (1, 3, 5, 252, 21),     # K not a multiple of 64, LDS image at its limit
          (3, 33, 65, 128, 22),   # odd pixel counts
          (2, 120, 160, 16, 4)]   # several first-stage partials
PATTERNS = ["random", "blocky", "one_class", "missing_class"]
ALL = ("feat", "weights", "bias")


def dev(a):
    return torch.tensor(np.asarray(a), device="cuda")   # a copy: the cached host arrays are read-only


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return host(t).view(np.int32)


def labels(shape, pattern, rng):
    """Label map (B,H,W) int32 with -1, C, C+5 and -100 planted in it."""
    B, H, W, K, C = shape
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


@functools.lru_cache(maxsize=None)
def case(shape, pattern, integers=False, sparse=False):
    """Host inputs and references, built once and read-only: (feat, w, label, g, r32, r64)."""
    B, H, W, K, C = shape
    rng = np.random.default_rng(1000 * sum(shape) + 10 * PATTERNS.index(pattern) + 2 * integers + sparse)
    label = labels(shape, pattern, rng)
    if integers:
        feat = rng.integers(-8, 9, size=(B, H, W, K)).astype(np.float32)
        w = rng.integers(-4, 5, size=(K, 3 * C)).astype(np.float32)
        g = rng.integers(-4, 5, size=(B, H, W, 3)).astype(np.float32)
    else:
        feat = rng.standard_normal((B, H, W, K)).astype(np.float32)
        w = rng.standard_normal((K, 3 * C)).astype(np.float32)
        g = rng.standard_normal((B, H, W, 3)).astype(np.float32)
    if sparse:   # the training pattern: a gradient on one class's pixels only
        on = np.bincount(label[(label >= 0) & (label < C)], minlength=C).argmax()
        g[label != on] = 0
        assert (label == on).any() and (label != on).any()
    r32 = ref.vertex_pred_bwd_ref(feat, w, label, g, mode="f32")
    r64 = ref.vertex_pred_bwd_ref(feat, w, label, g, mode="f64")
    for a in (feat, w, label, g):
        a.setflags(write=False)
    return feat, w, label, g, r32, r64


def run(feat, w, label, g, want=ALL, stream=None):
    """The op on NaN-prefilled outputs, through the C entry point: {name: tensor}."""
    from posecnn_amd import _lib
    B, H, W, K = feat.shape
    C = w.shape[1] // 3
    shapes = {"feat": (B, H, W, K), "weights": (K, 3 * C), "bias": (3 * C,)}
    lib = _lib.load()
    st = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(st):
        out = {n: torch.full(shapes[n], float("nan"), dtype=torch.float32, device="cuda") for n in want}
        ws = _lib.workspace(lib.pcnn_vertex_pred_compact_bwd_workspace_size(B, H, W, K, C), feat.device,
                            "vertex_pred_bwd_test", st)
        ws.fill_(0xFF)   # recycled memory: NaN bit patterns in the partials
        rc = lib.pcnn_vertex_pred_compact_bwd(_lib.ptr(feat), _lib.ptr(w), _lib.ptr(label), _lib.ptr(g), B, H, W, K, C,
                                              *[_lib.ptr(out.get(n)) for n in ALL], _lib.ptr(ws), ws.numel(),
                                              _lib.stream_ptr(st))
    assert rc == 0, rc
    return out


@functools.lru_cache(maxsize=None)
def device_case(shape, pattern, integers=False, sparse=False):
    feat, w, label, g, _, _ = case(shape, pattern, integers, sparse)
    return run(dev(feat), dev(w), dev(label), dev(g))


def check_against_reference(out, r32, r64, what):
    np.testing.assert_array_equal(host(out["feat"]), r32["d_feat"], err_msg=f"{what} d_feat")
    bw, bb = ref.sum_bounds(r64)
    ew = np.abs(host(out["weights"]).astype(np.float64) - r64["d_weights"])
    eb = np.abs(host(out["bias"]).astype(np.float64) - r64["d_bias"])
    print(f"{what}: d_weights max err {ew.max():.3e}, max err / bound {np.max(ew / np.maximum(bw, 1e-300)):.3f}; "
          f"d_bias max err {eb.max():.3e}, max err / bound {np.max(eb / np.maximum(bb, 1e-300)):.3f}")
    assert np.isfinite(host(out["weights"])).all() and np.isfinite(host(out["bias"])).all()
    assert (ew <= bw).all(), f"{what} d_weights"
    assert (eb <= bb).all(), f"{what} d_bias"


def test_partial_counts(hip):
    assert hip.pcnn_vertex_pred_compact_bwd_partials(2, 120, 160, 16, 4) >= 3
    assert hip.pcnn_vertex_pred_compact_bwd_partials(1, 5, 7, 4, 1) == 1


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", SHAPES)
def test_random_inputs_against_the_reference(hip, shape, pattern):
    _, _, label, _, r32, r64 = case(shape, pattern)
    C = shape[4]
    if pattern == "missing_class":
        assert r64["n"][C // 2] == 0
    if pattern == "one_class":
        assert r64["n"][C - 1] == label.size - 4 and r64["n"].sum() == label.size - 4
    check_against_reference(device_case(shape, pattern), r32, r64, f"{shape} {pattern}")


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", SHAPES)
def test_integer_inputs_sum_exactly(hip, shape, pattern):
    _, _, _, _, r32, r64 = case(shape, pattern, integers=True)
    out = device_case(shape, pattern, integers=True)
    np.testing.assert_array_equal(host(out["weights"]), r64["d_weights"])
    np.testing.assert_array_equal(host(out["bias"]), r64["d_bias"])
    np.testing.assert_array_equal(host(out["feat"]), r64["d_feat"])
    np.testing.assert_array_equal(host(out["feat"]), r32["d_feat"])
    if shape[4] > 1 or pattern != "missing_class":
        assert r64["d_weights"].any() and r64["d_bias"].any()


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3], SHAPES[5]])
def test_sparse_gradient(hip, shape):
    for integers in (False, True):
        _, _, label, g, r32, r64 = case(shape, "blocky", integers, sparse=True)
        assert (g.reshape(-1, 3)[label.reshape(-1) >= 0].any(axis=1)).mean() < 1   # pixels the sums skip
        out = device_case(shape, "blocky", integers, sparse=True)
        if integers:
            np.testing.assert_array_equal(host(out["weights"]), r64["d_weights"])
            np.testing.assert_array_equal(host(out["bias"]), r64["d_bias"])
            np.testing.assert_array_equal(host(out["feat"]), r64["d_feat"])
        else:
            check_against_reference(out, r32, r64, f"{shape} sparse")


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[4], SHAPES[5]])
def test_two_calls_give_the_same_bits(hip, shape):
    feat, w, label, g, _, _ = case(shape, "random")
    first = device_case(shape, "random")
    side = torch.cuda.Stream()
    args = [dev(x) for x in (feat, w, label, g)]
    torch.cuda.synchronize()
    second = run(*args, stream=side)
    side.synchronize()
    for n in ALL:
        np.testing.assert_array_equal(bits(second[n]), bits(first[n]), err_msg=n)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1], SHAPES[3]])
def test_each_output_alone(hip, shape):
    from posecnn_amd.vertex_pred import vertex_pred_compact_bwd
    feat, w, label, g, _, _ = case(shape, "blocky")
    every = device_case(shape, "blocky")
    f, wd, lb, gd = dev(feat), dev(w), dev(label), dev(g)
    for n in ALL:
        alone = run(f, wd, lb, gd, want=(n,))
        assert list(alone) == [n]
        np.testing.assert_array_equal(bits(alone[n]), bits(every[n]), err_msg=n)
        viaw = vertex_pred_compact_bwd(f, wd, lb, gd, want=(n,))
        assert list(viaw) == [n]
        np.testing.assert_array_equal(bits(viaw[n]), bits(every[n]), err_msg=n)
    two = run(f, wd, lb, gd, want=("weights", "bias"))
    for n in two:
        np.testing.assert_array_equal(bits(two[n]), bits(every[n]), err_msg=n)


def test_null_inputs_of_unrequested_outputs(hip):
    """feat may be NULL without d_weights, weights without d_feat; an output
    passed as NULL is not written (its neighbour buffers keep their NaNs)."""
    from posecnn_amd import _lib
    shape = SHAPES[1]
    B, H, W, K, C = shape
    feat, w, label, g, _, _ = case(shape, "random")
    every = device_case(shape, "random")
    f, wd, lb, gd = dev(feat), dev(w), dev(label), dev(g)
    ws = _lib.workspace(hip.pcnn_vertex_pred_compact_bwd_workspace_size(*shape), f.device, "vertex_pred_bwd_test")
    guard = torch.full((3, 3 * C), float("nan"), dtype=torch.float32, device="cuda")   # d_bias in the middle row
    rc = hip.pcnn_vertex_pred_compact_bwd(None, None, _lib.ptr(lb), _lib.ptr(gd), *shape, None, None,
                                          _lib.ptr(guard[1]), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    assert rc == 0
    np.testing.assert_array_equal(bits(guard[1]), bits(every["bias"]))
    assert torch.isnan(guard[0]).all() and torch.isnan(guard[2]).all()
    d_feat = torch.full((B, H, W, K), float("nan"), dtype=torch.float32, device="cuda")
    rc = hip.pcnn_vertex_pred_compact_bwd(None, _lib.ptr(wd), _lib.ptr(lb), _lib.ptr(gd), *shape, _lib.ptr(d_feat),
                                          None, None, None, 0, _lib.stream_ptr())
    assert rc == 0
    np.testing.assert_array_equal(bits(d_feat), bits(every["feat"]))
    d_w = torch.full((K, 3 * C), float("nan"), dtype=torch.float32, device="cuda")
    rc = hip.pcnn_vertex_pred_compact_bwd(_lib.ptr(f), None, _lib.ptr(lb), _lib.ptr(gd), *shape, None, _lib.ptr(d_w),
                                          None, _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    assert rc == 0
    np.testing.assert_array_equal(bits(d_w), bits(every["weights"]))


def test_wrapper_shapes_and_validation(hip):
    from posecnn_amd.vertex_pred import vertex_pred_compact_bwd
    shape = SHAPES[1]
    B, H, W, K, C = shape
    feat, w, label, g, _, _ = case(shape, "random")
    every = device_case(shape, "random")
    f, wd, lb, gd = dev(feat), dev(w), dev(label), dev(g)
    out = vertex_pred_compact_bwd(f, wd, lb, gd)
    assert sorted(out) == sorted(ALL)
    assert out["feat"].shape == (B, H, W, K) and out["weights"].shape == (K, 3 * C) and out["bias"].shape == (3 * C,)
    for n in ALL:
        np.testing.assert_array_equal(bits(out[n]), bits(every[n]), err_msg=n)
    # the reference's (1,1,K,3C) kernel; float64 / int64 inputs: the results of their float32 / int32 copies
    out4 = vertex_pred_compact_bwd(f.double(), wd.reshape(1, 1, K, 3 * C), lb.long(), gd.double())
    assert out4["weights"].shape == (1, 1, K, 3 * C)
    for n in ALL:
        np.testing.assert_array_equal(bits(out4[n]).reshape(-1), bits(every[n]).reshape(-1), err_msg=n)
    with pytest.raises(ValueError):
        vertex_pred_compact_bwd(f, wd, lb, gd, want=("label",))
    with pytest.raises(ValueError):
        vertex_pred_compact_bwd(f, wd, lb, gd, want=())
    with pytest.raises(ValueError):
        vertex_pred_compact_bwd(f, wd, lb[:, :-1], gd)
    with pytest.raises(ValueError):
        vertex_pred_compact_bwd(f, wd, lb, gd[..., :2])
    with pytest.raises(ValueError):
        vertex_pred_compact_bwd(f, wd[:, :-1], lb, gd)
    with pytest.raises(ValueError):
        vertex_pred_compact_bwd(f[..., :6].contiguous(), wd[:6].contiguous(), lb, gd)   # K % 4


def test_graph_capture_and_replay(hip):
    from posecnn_amd import _lib
    shape = SHAPES[0]
    B, H, W, K, C = shape
    feat, w, label, g, _, _ = case(shape, "blocky")
    every = device_case(shape, "blocky")
    f, wd, lb, gd = dev(feat), dev(w), dev(label), dev(g)
    out = {"feat": torch.empty((B, H, W, K), device="cuda"), "weights": torch.empty((K, 3 * C), device="cuda"),
           "bias": torch.empty((3 * C,), device="cuda")}
    ws = torch.empty(hip.pcnn_vertex_pred_compact_bwd_workspace_size(*shape), dtype=torch.uint8, device="cuda")

    def call():
        rc = hip.pcnn_vertex_pred_compact_bwd(_lib.ptr(f), _lib.ptr(wd), _lib.ptr(lb), _lib.ptr(gd), *shape,
                                              *[_lib.ptr(out[n]) for n in ALL], _lib.ptr(ws), ws.numel(),
                                              _lib.stream_ptr())
        assert rc == 0
    call()   # eager first: code objects loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for t in out.values():
        t.fill_(float("nan"))
    ws.fill_(0xFF)
    graph.replay()
    torch.cuda.synchronize()
    for n in ALL:
        np.testing.assert_array_equal(bits(out[n]), bits(every[n]), err_msg=n)


def test_module_end_to_end(hip):
    """VertexPredCompact + VertexLoss on scene-style ground truth: background 0,
    rectangles of object classes, a vote target per pixel."""
    from posecnn_amd import losses
    from posecnn_amd.pth import VertexLoss, VertexPredCompact
    from posecnn_amd.vertex_pred import vertex_pred_compact, vertex_pred_compact_bwd
    shape = SHAPES[0]
    B, H, W, K, C = shape
    rng = np.random.default_rng(77)
    label = labels(shape, "blocky", rng)
    vertex3 = rng.standard_normal((B, H, W, 3)).astype(np.float32)
    feat = rng.standard_normal((B, H, W, K)).astype(np.float32)
    mod = VertexPredCompact(K, C).cuda()
    assert mod.weight.shape == (K, 3 * C) and mod.bias.shape == (3 * C,)
    with torch.no_grad():
        mod.weight.copy_(dev(rng.standard_normal((K, 3 * C)).astype(np.float32) * 0.1))
        mod.bias.copy_(dev(rng.standard_normal(3 * C).astype(np.float32)))
    f = dev(feat).requires_grad_(True)
    lb, v3 = dev(label), dev(vertex3)
    pred = mod(f, lb)
    want_pred = vertex_pred_compact(f.detach(), mod.weight.detach(), mod.bias.detach(), lb)
    assert pred.shape == (B, H, W, 3) and torch.equal(pred.detach(), want_pred)
    crit = VertexLoss(sigma=1.0, w_inside=10.0, num_classes=C)
    loss = crit(pred, lb, v3)
    (3 * loss).backward()
    _, d3 = losses.vertex_loss_compact(want_pred, lb, v3, C, 10.0, 1.0, want_grad=True, grad_scale=3.0)
    assert d3.abs().max().item() > 0 and (d3 == 0).all(dim=-1).any()
    direct = vertex_pred_compact_bwd(f.detach(), mod.weight.detach(), lb, d3)
    for name, got in (("feat", f.grad), ("weights", mod.weight.grad), ("bias", mod.bias.grad)):
        assert got is not None and got.shape == direct[name].shape
        np.testing.assert_array_equal(bits(got), bits(direct[name]), err_msg=name)
    assert mod.weight.grad.abs().max().item() > 0 and mod.bias.grad.abs().max().item() > 0
    # only the gradients autograd needs: frozen parameters, a feature map that needs none
    mod2 = VertexPredCompact(K, C).cuda()
    mod2.load_state_dict(mod.state_dict())
    mod2.weight.requires_grad_(False)
    crit(mod2(dev(feat), lb), lb, v3).backward()
    assert mod2.weight.grad is None
    _, d1 = losses.vertex_loss_compact(want_pred, lb, v3, C, 10.0, 1.0, want_grad=True)
    np.testing.assert_array_equal(bits(mod2.bias.grad),
                                  bits(vertex_pred_compact_bwd(dev(feat), mod.weight.detach(), lb, d1)["bias"]))
