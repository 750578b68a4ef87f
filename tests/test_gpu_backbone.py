"""The backbone's forward on the device (csrc/backbone.hip,
posecnn_amd/backbone.py, pth.VGG16Convs) against tests/backbone_ref.py: the
MFMA conv bit for bit on exact integer operands and under the float32
summation bound on floats, conv1_1 and the max-pool bit for bit, determinism,
the whole stack as the composition of the public ops (buffers, graph capture),
the module, and the argument contract."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import abi_guard
import backbone_cases as bc
import backbone_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
U24 = 2.0 ** -24
HEADER = os.path.join(abi_guard.ROOT, "include", "posecnn_backbone.h")
EINVAL, ECAPACITY = 1, 3   # PCNN_EINVAL, PCNN_ECAPACITY (posecnn_hip.h)


def dev(a):
    return torch.from_numpy(np.array(a, copy=True)).to(DEV)   # (a copy: the cached cases are read-only)


def host(t):
    return t.detach().cpu().numpy()


def same_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=what)


@functools.lru_cache(maxsize=None)
def exact_reference(cls, shape, relu):
    x, w, b = bc.exact_case(cls, shape)
    want, _ = ref.conv3x3_f64(x, w, b, relu)
    out = want.astype(np.float32)
    assert (out.astype(np.float64) == want).all()
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def float_reference(shape):
    x, w, b = bc.float_case(shape)
    return ref.conv3x3_f64(x, w, b, True)


# ---- 1. the MFMA conv on exact integer operands: no tolerance ----
@pytest.mark.parametrize("shape", bc.MFMA_SHAPES, ids=bc.ident)
@pytest.mark.parametrize("cls", ("dense4", "x19", "w19", "mm10"))
def test_mfma_conv_is_exact_on_integers(hip, cls, shape):
    from posecnn_amd import backbone
    x, w, b = (dev(a) for a in bc.exact_case(cls, shape))
    for relu in (True, False):
        got = host(backbone.conv3x3(x, w, b, relu=relu))
        same_bits(got, exact_reference(cls, shape, relu), f"{cls} {shape} relu={relu}")
    # no bias
    want, _ = ref.conv3x3_f64(*bc.exact_case(cls, shape)[:2], None, False)
    same_bits(host(backbone.conv3x3(x, w, None, relu=False)), want.astype(np.float32), f"{cls} {shape} no bias")


@pytest.mark.parametrize("shape", bc.MFMA_SHAPES, ids=bc.ident)
def test_padding_is_zero_not_a_neighbour(hip, shape):
    """A constant non-zero map: a fragment read from the wrong row or image in
    place of zero padding changes border outputs only."""
    from posecnn_amd import backbone
    B, H, W, Cin, Cout = shape
    x, w, b = (dev(a) for a in bc.exact_case("const", shape))
    got = host(backbone.conv3x3(x, w, b, relu=False))
    want = exact_reference("const", shape, False)
    bad = (got.view(np.uint32) != want.view(np.uint32)).any(axis=3)
    border = ref.border_mask(B, H, W)
    assert not bad[~border].any(), f"{int(bad[~border].sum())} interior pixels differ: not a padding fault"
    assert not bad[border].any(), (f"{int(bad[border].sum())} of {int(border.sum())} BORDER pixels differ and no "
                                   f"interior one: padding was read from a neighbouring row or image; first at "
                                   f"(b, y, x) = {tuple(np.argwhere(bad)[0])}")


# ---- 2. conv1_1, bit for bit ----
@pytest.mark.parametrize("shape", bc.DIRECT_SHAPES, ids=bc.ident)
@pytest.mark.parametrize("relu", (True, False))
def test_conv1_1_is_bit_exact(hip, shape, relu):
    from posecnn_amd import backbone
    x, w, b = bc.float_case(shape)
    got = host(backbone.conv3x3(dev(x), dev(w), dev(b), relu=relu))
    same_bits(got, ref.conv3x3_direct_f32(x, w, b, relu), f"{shape} relu={relu}")
    same_bits(host(backbone.conv3x3(dev(x), dev(w), None, relu=relu)), ref.conv3x3_direct_f32(x, w, None, relu),
              f"{shape} no bias")


# ---- 3. the max-pool, bit for bit ----
@pytest.mark.parametrize("shape", bc.POOL_SHAPES, ids=bc.ident)
def test_max_pool_is_bit_exact(hip, shape):
    from posecnn_amd import backbone
    x = bc.negative_map(shape)
    got = host(backbone.max_pool2x2(dev(x)))
    same_bits(got, ref.max_pool2x2(x), str(shape))
    assert (got < 0).all(), "a zero from padding won a window"


# ---- 4. floats ----
@pytest.mark.parametrize("shape", bc.FLOAT_SHAPES, ids=bc.ident)
def test_mfma_conv_on_floats(hip, shape):
    """Per output at most (9 Cin + 16) 2^-24 (sum |x||w| + |b|): the worst case
    of float32 summation over the contraction, the bound
    test_gpu_neck.py::test_whole_layer_on_floats holds the precision-2 GEMM
    to.  ReLU is 1-Lipschitz: the same bound holds behind it."""
    from posecnn_amd import backbone
    x, w, b = bc.float_case(shape)
    want, mag = float_reference(shape)
    got = host(backbone.conv3x3(dev(x), dev(w), dev(b), relu=True)).astype(np.float64)
    err = np.abs(got - want)
    bound = (9 * shape[3] + 16) * U24 * mag
    worst = float((err / np.maximum(bound, 1e-300)).max(initial=0))
    print(f"{shape}: max error {err.max(initial=0):.3e}, at most {worst:.4f} of its bound")
    assert (err <= bound).all(), worst


# ---- 5. determinism ----
@pytest.mark.parametrize("shape", (bc.SPLIT_SHAPE, bc.MFMA_SHAPES[1]), ids=bc.ident)
def test_two_calls_give_the_same_bits(hip, shape):
    from posecnn_amd import backbone
    B, H, W, Cin, Cout = shape
    if shape == bc.SPLIT_SHAPE:
        assert backbone._load().pcnn_conv3x3_workspace_size(B, H, W, Cin, Cout, 2) > 0, "the planner no longer splits"
    x, w, b = (dev(a) for a in bc.float_case(shape))
    first = host(backbone.conv3x3(x, w, b))
    for _ in range(3):
        same_bits(host(backbone.conv3x3(x, w, b)), first, str(shape))


# ---- 6. the whole stack ----
@functools.lru_cache(maxsize=None)
def device_params():
    return {n: (dev(w), dev(b)) for n, (w, b) in bc.stack_params().items()}


@pytest.mark.parametrize("shape", bc.STACK_SHAPES, ids=bc.ident)
def test_stack_is_the_composition_of_the_ops(hip, shape):
    from posecnn_amd import backbone
    B, H, W = shape
    params, x = device_params(), dev(bc.blob(shape))
    names = [layer[0] for layer in backbone.LAYERS]
    c4, c5, kept = backbone.vgg16_convs(x, params, keep=tuple(names))
    shapes = ref.vgg16_shapes(backbone.LAYERS, B, H, W)
    cur = x
    for layer in backbone.LAYERS:
        cur = backbone.conv3x3(cur, *params[layer[0]]) if len(layer) == 3 else backbone.max_pool2x2(cur)
        assert tuple(kept[layer[0]].shape) == shapes[layer[0]], layer[0]
        same_bits(host(kept[layer[0]]), host(cur), layer[0])
    same_bits(host(c4), host(kept["conv4_3"]))
    same_bits(host(c5), host(kept["conv5_3"]))
    assert np.isfinite(host(c5)).all() and host(c5).any(), "the stack's output died"
    # through the ping-pong buffers: the same bits
    p4, p5 = backbone.vgg16_convs(x, params)
    same_bits(host(p4), host(c4), "conv4_3 through the buffers")
    same_bits(host(p5), host(c5), "conv5_3 through the buffers")
    # the second call at a shape allocates nothing but what it returns
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    q4, q5 = backbone.vgg16_convs(x, params)
    torch.cuda.synchronize()
    returned = sum(t.untyped_storage().nbytes() for t in (q4, q5))
    grown = torch.cuda.memory_allocated() - before
    assert grown <= returned + 2 * 512, (grown, returned)   # (the allocator rounds a block up to 512 B)
    same_bits(host(q5), host(c5))


def test_stack_replays_from_a_graph(hip):
    from posecnn_amd import backbone
    shape = bc.STACK_SHAPES[1]
    params, x = device_params(), dev(bc.blob(shape))
    e4, e5 = backbone.vgg16_convs(x, params)
    e4, e5 = host(e4), host(e5)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        backbone.vgg16_convs(x, params)   # sizes this stream's workspace outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):   # single stream, linear
        g4, g5 = backbone.vgg16_convs(x, params)
    g4.fill_(-1.0)
    g5.fill_(-1.0)
    g.replay()
    torch.cuda.synchronize()
    same_bits(host(g4), e4, "conv4_3 replayed")
    same_bits(host(g5), e5, "conv5_3 replayed")


# ---- 7. the module ----
def test_module(hip):
    from posecnn_amd import backbone, pth
    m = pth.VGG16Convs(seed=3)
    named = dict(m.named_parameters())
    assert len(named) == 26
    for name, cin, cout in backbone.CONVS:
        w, b = named[f"{name}.weights"], named[f"{name}.biases"]
        assert tuple(w.shape) == (3, 3, cin, cout) and tuple(b.shape) == (cout,)
        assert not w.requires_grad and not b.requires_grad
        assert float(w.abs().max()) <= 0.002 and float(w.std()) > 0.0005 and not b.any()
    raw = bc.stack_params()
    m.load_reference(**raw)
    for name, (w, b) in raw.items():
        same_bits(named[f"{name}.weights"].numpy(), w, name)
        same_bits(named[f"{name}.biases"].numpy(), b, name)
    with pytest.raises(ValueError):
        m.load_reference(conv9_9=raw["conv1_1"])
    with pytest.raises(ValueError):
        m.load_reference(conv1_1=raw["conv1_2"])
    m = m.to(DEV)
    shape = bc.STACK_SHAPES[0]
    x = dev(bc.blob(shape))
    c4, c5 = m(x)
    w4, w5 = backbone.vgg16_convs(x, device_params())
    same_bits(host(c4), host(w4), "conv4_3")
    same_bits(host(c5), host(w5), "conv5_3")
    # no silent zero gradients
    with pytest.raises(NotImplementedError, match="backward"):
        m(x.clone().requires_grad_(True))
    m.conv3_2.weights.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="conv3_2.weights"):
        m(x)
    m.conv3_2.weights.requires_grad_(False)
    m(x)


def test_module_feeds_the_neck_and_heads(hip):
    from posecnn_amd import pth
    B, H, W, C = 1, 32, 32, 3
    torch.manual_seed(0)
    net = pth.VGG16Convs().to(DEV).eval()
    net.load_reference(**bc.stack_params())
    neck = pth.EmbeddingNeck(in_channels=512, num_units=64, vertex_units=128).to(DEV).eval()
    score = pth.ScoreHead(64, C).to(DEV).eval()
    vertex = pth.VertexHeadCompact(128, C).to(DEV).eval()
    with torch.no_grad():
        c4, c5 = net(dev(bc.blob((B, H, W))))
        assert tuple(c4.shape) == (B, 4, 4, 512) and tuple(c5.shape) == (B, 2, 2, 512)
        a_s, a_v = neck(c4, c5)
        assert tuple(a_s.shape) == (B, 4, 4, 64) and tuple(a_v.shape) == (B, 4, 4, 128)
        s = score(a_s)
        label = torch.zeros((B, H, W), dtype=torch.int32, device=DEV)
        v = vertex(a_v, label)
    assert tuple(s.shape) == (B, H, W, C) and tuple(v.shape) == (B, H, W, 3)
    for t in (c4, c5, a_s, a_v, s, v):
        assert torch.isfinite(t).all()


# ---- 8. refusals ----
def test_c_abi_refusals(hip):
    from posecnn_amd import backbone
    lib = backbone._load()
    assert lib.pcnn_backbone_abi_version() == 1
    B, H, W, Cin, Cout = bc.SPLIT_SHAPE
    x = torch.zeros((B, H, W, Cin), device=DEV)
    w = torch.zeros((3, 3, Cin, Cout), device=DEV)
    b = torch.zeros(Cout, device=DEV)
    y = torch.full((B, H, W, Cout), 7.0, device=DEV)
    need = lib.pcnn_conv3x3_workspace_size(B, H, W, Cin, Cout, 2)
    assert need > 0
    ws = torch.zeros(need + 64, dtype=torch.uint8, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def conv(**kw):
        a = dict(x=x.data_ptr(), w=w.data_ptr(), b=b.data_ptr(), B=B, H=H, W=W, Cin=Cin, Cout=Cout, act=1, prec=2,
                 y=y.data_ptr(), ws=ws.data_ptr(), ws_bytes=need)
        a.update(kw)
        return lib.pcnn_conv3x3_fwd(a["x"], a["w"], a["b"], a["B"], a["H"], a["W"], a["Cin"], a["Cout"], a["act"],
                                    a["prec"], a["y"], a["ws"], a["ws_bytes"], st)

    bad = {
        "precision 0": dict(prec=0), "precision 1": dict(prec=1), "precision 3": dict(prec=3),
        "act 2": dict(act=2), "B 0": dict(B=0), "H 0": dict(H=0), "W -1": dict(W=-1), "Cin 0": dict(Cin=0),
        "Cout 0": dict(Cout=0), "Cin 8": dict(Cin=8), "Cin 24": dict(Cin=24), "Cout 6": dict(Cout=6),
        "input of 2^31 bytes": dict(B=1 << 20, H=1, W=1, Cin=512, Cout=4),
        "output of 2^31 bytes": dict(B=1 << 20, H=1, W=1, Cin=16, Cout=512),
        "NULL x": dict(x=None), "NULL weights": dict(w=None), "NULL y": dict(y=None),
        "misaligned x": dict(x=x.data_ptr() + 4), "misaligned weights": dict(w=w.data_ptr() + 8),
        "misaligned y": dict(y=y.data_ptr() + 4), "x == y": dict(y=x.data_ptr()),
    }
    for what, kw in bad.items():
        assert conv(**kw) == EINVAL, what
        dims = {k: kw.get(k, v) for k, v in dict(B=B, H=H, W=W, Cin=Cin, Cout=Cout).items()}
        if not any(k in kw for k in ("x", "w", "y", "act")):
            assert lib.pcnn_conv3x3_workspace_size(dims["B"], dims["H"], dims["W"], dims["Cin"], dims["Cout"],
                                                   kw.get("prec", 2)) == 0, what
    assert conv(ws_bytes=need - 1) == ECAPACITY
    assert conv(ws_bytes=0, ws=None) == ECAPACITY
    assert conv(b=None) == 0    # a NULL bias is allowed
    torch.cuda.synchronize()
    assert not y.any()          # ... and that call ran (zeros in, zeros out)
    y.fill_(7.0)

    def pool(**kw):
        a = dict(x=x.data_ptr(), B=B, H=H, W=W, C=Cin, y=y.data_ptr())
        a.update(kw)
        return lib.pcnn_maxpool2x2_fwd(a["x"], a["B"], a["H"], a["W"], a["C"], a["y"], st)

    for what, kw in {"B 0": dict(B=0), "H 0": dict(H=0), "W 0": dict(W=0), "C 0": dict(C=0), "C 6": dict(C=6),
                     "2^31 bytes": dict(B=1 << 20, H=1, W=1, C=512), "NULL x": dict(x=None), "NULL y": dict(y=None),
                     "misaligned x": dict(x=x.data_ptr() + 4), "misaligned y": dict(y=y.data_ptr() + 8),
                     "x == y": dict(y=x.data_ptr())}.items():
        assert pool(**kw) == EINVAL, what
    torch.cuda.synchronize()
    assert (y == 7.0).all(), "a refused call wrote its output"


def test_wrappers_refuse_before_any_launch(hip):
    from posecnn_amd import _lib, backbone
    real = backbone._load()
    x = torch.zeros((1, 4, 4, 16), device=DEV)
    w = torch.zeros((3, 3, 16, 8), device=DEV)
    b = torch.zeros(8, device=DEV)
    params = device_params()
    blob = torch.zeros((1, 4, 4, 3), device=DEV)
    bad_conv = {
        "a CPU map": dict(x=x.cpu()), "float64": dict(x=x.double()), "a strided map": dict(x=x.transpose(1, 2)),
        "3-D": dict(x=x[0]), "8 channels": dict(x=torch.zeros((1, 4, 4, 8), device=DEV)),
        "OIHW weights": dict(weights=w.permute(3, 2, 0, 1).contiguous()), "strided weights": dict(weights=w.permute(1, 0, 2, 3)),
        "6 output channels": dict(weights=torch.zeros((3, 3, 16, 6), device=DEV), bias=torch.zeros(6, device=DEV)),
        "a short bias": dict(bias=b[:4]), "a CPU bias": dict(bias=b.cpu()),
        "out of the wrong shape": dict(out=torch.zeros((1, 4, 4, 4), device=DEV)), "out == x": dict(out=x, weights=torch.zeros((3, 3, 16, 16), device=DEV), bias=None),
    }
    bad_pool = {"a CPU map": dict(x=x.cpu()), "6 channels": dict(x=torch.zeros((1, 4, 4, 6), device=DEV)),
                "int32": dict(x=x.int()), "out of the floor shape": dict(x=torch.zeros((1, 5, 5, 4), device=DEV),
                                                                         out=torch.zeros((1, 2, 2, 4), device=DEV))}
    guard = abi_guard.GuardedLib(real, header=HEADER)
    _lib._lib = guard
    try:
        for what, kw in bad_conv.items():
            with pytest.raises((ValueError, TypeError)):
                backbone.conv3x3(**dict(dict(x=x, weights=w, bias=b), **kw))
        for what, kw in bad_pool.items():
            with pytest.raises((ValueError, TypeError)):
                backbone.max_pool2x2(**dict(dict(x=x), **kw))
        with pytest.raises(ValueError):
            backbone.vgg16_convs(torch.zeros((1, 4, 4, 4), device=DEV), params)
        with pytest.raises(ValueError):
            backbone.vgg16_convs(blob, {k: v for k, v in params.items() if k != "conv4_2"})
        with pytest.raises(ValueError):
            backbone.vgg16_convs(blob, dict(params, conv2_1=params["conv2_2"]))
        with pytest.raises(ValueError):
            backbone.vgg16_convs(blob, params, keep=("conv6_1",))
        assert guard.launches == 0, guard.calls
        backbone.conv3x3(x, w, b)               # the guard sees the good calls
        backbone.max_pool2x2(x)
        assert guard.launches == 2
    finally:
        _lib._lib = real
