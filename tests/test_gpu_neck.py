"""The embedding neck on the device (csrc/neck.hip, posecnn_amd/neck.py,
pth.EmbeddingNeck) against tests/neck_ref.py: the two fused passes bit for bit
where the order is pinned, under the worst-case float32 summation bound and
exactly on integers where it is the device's own; the whole layer as its
composition, exactly on integers and under a derived bound on floats; the
module under autograd; the argument contract."""
import functools

import numpy as np
import pytest
import torch

import abi_guard
import neck_cases as nc
import neck_ref as ref
import upscore_ref as up

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEEP = 0.5
U24 = 2.0 ** -24
GRADS = ("x4", "x5", "W4", "b4", "W5", "b5")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def same_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=what)


@functools.lru_cache(maxsize=None)
def device_case(kind, shape):
    c = nc.float_case(shape) if kind == "float" else nc.integer_case(shape)
    return {n: dev(v) for n, v in c.items()}


@functools.lru_cache(maxsize=None)
def keeps(shape, step):
    B, h, w, K, U, V = shape
    return ref.keep_maps(B * h * w, U, V, nc.SEED, step, nc.STREAM_IDS, KEEP)


def step_counter(step):
    return torch.tensor([step], dtype=torch.int64, device=DEV)


# ---- 1. the forward pass, bit for bit ----
@pytest.mark.parametrize("shape", nc.SHAPES, ids=nc.IDS)
def test_forward_pass_is_bit_exact(hip, shape):
    from posecnn_amd import neck
    B, h, w, K, U, V = shape
    c, t = nc.float_case(shape), device_case("float", shape)
    s, v, ks, kv = neck.neck_fwd(t["z4"], t["z5"], t["b4"], t["b5"], U)
    assert ks is None and kv is None and s.shape == (B, h, w, U) and v.shape == (B, h, w, V)
    rs, rv = ref.neck_fwd_ref(c["z4"], c["z5"], c["b4"], c["b5"], U)
    same_bits(host(s), rs, "add_score, keep_prob 1")
    same_bits(host(v), rv, "add_score_vertex, keep_prob 1")
    counter = step_counter(0)
    seen = []
    for step in (0, 1):
        s, v, ks, kv = neck.neck_fwd(t["z4"], t["z5"], t["b4"], t["b5"], U, keep_prob=KEEP,
                                     drop_gen=(nc.SEED, counter, nc.STREAM_IDS))
        counter += 1   # on the device: the next call reads it there
        want = keeps(shape, step)
        assert ks.dtype == torch.uint8 and ks.shape == (B * h * w, U) and kv.shape == (B * h * w, V)
        np.testing.assert_array_equal(host(ks), want[0], err_msg=f"keep_score, step {step}")
        np.testing.assert_array_equal(host(kv), want[1], err_msg=f"keep_vertex, step {step}")
        rs, rv = ref.neck_fwd_ref(c["z4"], c["z5"], c["b4"], c["b5"], U, KEEP, want)
        same_bits(host(s), rs, f"add_score, step {step}")
        same_bits(host(v), rv, f"add_score_vertex, step {step}")
        seen.append(np.concatenate([host(ks), host(kv)], axis=1))
    assert (seen[0] != seen[1]).any()


# ---- 2. the backward pass ----
@pytest.mark.parametrize("shape", nc.SHAPES, ids=nc.IDS)
@pytest.mark.parametrize("keep_prob", [1.0, KEEP])
def test_backward_pass(hip, shape, keep_prob):
    from posecnn_amd import neck
    B, h, w, K, U, V = shape
    c, t = nc.float_case(shape), device_case("float", shape)
    keep = keeps(shape, 0)
    dk = [None, None] if keep_prob == 1.0 else [dev(k) for k in keep]
    run = lambda tt: neck.neck_bwd(tt["d_s"], tt["d_v"], dk[0], dk[1], tt["z4"], tt["z5"], tt["b4"],  # noqa: E731
                                   tt["b5"], U, keep_prob=keep_prob)
    dz4, dz5, db4, db5 = (host(x) for x in run(t))
    args = (c["d_s"], c["d_v"], keep, c["z4"], c["z5"], c["b4"], c["b5"], U, keep_prob)
    r32, r64 = ref.neck_bwd_ref(*args, mode="f32"), ref.neck_bwd_ref(*args, mode="f64")
    same_bits(dz4, r32["dz4"], "dz4")
    same_bits(dz5, r32["dz5"], "dz5 (the pinned window order)")
    # against float64 under the worst-case bound of float32 summation for the term counts (g is exact: the
    # division by 0.5 or 1 does not round): dz5 has n_dz5 <= 16 products; db4 sums M4 exact terms; db5 sums M5
    # values that each carry dz5's (16 + 1) roundings
    err = np.abs(dz5 - r64["dz5"])
    assert (err <= up.sum_bound(r64["n_dz5"][None, :, :, None], r64["abs_dz5"])).all(), err.max()
    err = np.abs(db4 - r64["db4"])
    assert (err <= up.sum_bound(r64["n_db4"], r64["abs_db4"])).all(), (err.max(), r64["abs_db4"].max())
    err = np.abs(db5 - r64["db5"])
    assert (err <= up.sum_bound(r64["n_db5"] + 16, r64["abs_db5"])).all(), (err.max(), r64["abs_db5"].max())
    # the same bits on a second run
    again = run(t)
    same_bits(host(again[2]), db4, "db4, second run")
    same_bits(host(again[3]), db5, "db5, second run")
    same_bits(host(again[1]), dz5, "dz5, second run")
    # exactly, on integers
    ci, ti = nc.integer_case(shape), device_case("integer", shape)
    got = [host(x) for x in run(ti)]
    want = ref.neck_bwd_ref(ci["d_s"], ci["d_v"], keep, ci["z4"], ci["z5"], ci["b4"], ci["b5"], U, keep_prob,
                            mode="f64")
    for g, n in zip(got, ("dz4", "dz5", "db4", "db5")):
        np.testing.assert_array_equal(g, want[n], err_msg=f"{n} on integers")


# ---- 3. the layer is its composition ----
@pytest.mark.parametrize("shape,precision", [(s, 2) for s in nc.SHAPES] + [(nc.REAL, 0), (nc.REAL, 1)],
                         ids=[f"{i}-p2" for i in nc.IDS] + ["real-p0", "real-p1"])
def test_layer_is_gemm_then_the_fused_pass(hip, shape, precision):
    from posecnn_amd import neck, pose_head
    B, h, w, K, U, V = shape
    N, M4 = U + V, B * h * w
    c, t = nc.float_case(shape), device_case("float", shape)
    z4 = torch.empty((M4, N), device=DEV)
    z5 = torch.empty((M4 // 4, N), device=DEV)
    pose_head.gemm(t["x4"].view(M4, K), t["W4"], z4, precision=precision)
    pose_head.gemm(t["x5"].view(M4 // 4, K), t["W5"], z5, precision=precision)
    hz4, hz5 = host(z4).reshape(B, h, w, N), host(z5).reshape(B, h // 2, w // 2, N)
    for keep_prob in (1.0, KEEP):
        s, v, ctx = neck.embedding(t["x4"], t["x5"], t["W4"], t["b4"], t["W5"], t["b5"], U, keep_prob=keep_prob,
                                   drop_gen=(nc.SEED, step_counter(0), None), precision=precision)
        rs, rv = ref.neck_fwd_ref(hz4, hz5, c["b4"], c["b5"], U, keep_prob, keeps(shape, 0))
        same_bits(host(s), rs, f"add_score, keep_prob {keep_prob}")
        same_bits(host(v), rv, f"add_score_vertex, keep_prob {keep_prob}")
        same_bits(host(ctx["z4"]), hz4, "z4")
        assert (ctx["keep_score"] is None) == (keep_prob == 1.0)


# ---- 4. the whole layer, exactly, on integers ----
@pytest.mark.parametrize("shape", nc.SHAPES, ids=nc.IDS)
def test_whole_layer_is_exact_on_integers(hip, shape):
    from posecnn_amd import neck
    B, h, w, K, U, V = shape
    c, t = nc.integer_case(shape), device_case("integer", shape)
    keep = keeps(shape, 0)
    s, v, ctx = neck.embedding(t["x4"], t["x5"], t["W4"], t["b4"], t["W5"], t["b5"], U, keep_prob=KEEP,
                               drop_gen=(nc.SEED, step_counter(0), nc.STREAM_IDS))
    d = neck.embedding_bwd(ctx, t["d_s"], t["d_v"])
    r = ref.layer_f64(c["x4"], c["x5"], c["W4"], c["b4"], c["W5"], c["b5"], U, KEEP, keep, d=(c["d_s"], c["d_v"]))
    np.testing.assert_array_equal(host(s), r["add_score"])
    np.testing.assert_array_equal(host(v), r["add_score_vertex"])
    assert set(d) == set(GRADS)
    for n in GRADS:
        assert d[n].shape == t[n].shape and d[n].dtype == torch.float32, n
        np.testing.assert_array_equal(host(d[n]), r[n], err_msg=n)
    # only what `want` names
    some = neck.embedding_bwd(ctx, t["d_s"], t["d_v"], want=("W5", "b4"))
    assert set(some) == {"W5", "b4"}
    np.testing.assert_array_equal(host(some["W5"]), r["W5"])
    np.testing.assert_array_equal(host(some["b4"]), r["b4"])


# ---- 5. the whole layer on floats ----
@functools.lru_cache(maxsize=None)
def float_layer_reference(shape, keep_prob):
    """(the float64 layer, the same expression on absolute values under the true ReLU masks)."""
    c = nc.float_case(shape)
    U = shape[4]
    args = [c[n] for n in ("x4", "x5", "W4", "b4", "W5", "b5")]
    r = ref.layer_f64(*args, U, keep_prob, keeps(shape, 0), d=(c["d_s"], c["d_v"]))
    mag = ref.layer_f64(*[np.abs(a) for a in args], U, keep_prob, keeps(shape, 0),
                        d=(np.abs(c["d_s"]), np.abs(c["d_v"])), masks=r["masks"])
    return r, mag


def contraction_lengths(shape):
    B, h, w, K, U, V = shape
    M4 = B * h * w
    return dict(add_score=K, add_score_vertex=K, x4=U + V, x5=U + V, W4=M4, b4=M4, W5=M4 // 4, b5=M4 // 4)


@pytest.mark.parametrize("shape", nc.SHAPES, ids=nc.IDS)
@pytest.mark.parametrize("keep_prob", [1.0, KEEP])
def test_whole_layer_on_floats(hip, shape, keep_prob):
    """Per element at most (L + 16) 2^-24 times the expression on absolute
    values, L the contraction length: the worst case of float32 summation,
    which the precision-2 GEMM is documented to be faithful to.  The ReLU
    masks of the device and of float64 agree as long as no pre-activation is
    within that bound of zero, which the operands are checked for."""
    from posecnn_amd import neck
    B, h, w, K, U, V = shape
    c, t = nc.float_case(shape), device_case("float", shape)
    r, mag = float_layer_reference(shape, keep_prob)
    for pre, room in nc.mask_room(c, shape):   # float_case draws its operands so
        assert (pre > room).all(), "a pre-activation too close to 0 for a well-posed mask"
    s, v, ctx = neck.embedding(t["x4"], t["x5"], t["W4"], t["b4"], t["W5"], t["b5"], U, keep_prob=keep_prob,
                               drop_gen=(nc.SEED, step_counter(0), nc.STREAM_IDS))
    got = dict(neck.embedding_bwd(ctx, t["d_s"], t["d_v"]), add_score=s, add_score_vertex=v)
    L = contraction_lengths(shape)
    for n, g in got.items():
        err = np.abs(host(g).astype(np.float64) - r[n])
        bound = (L[n] + 16) * U24 * mag[n]
        worst = float((err / np.maximum(bound, 1e-300)).max(initial=0))
        print(f"{n}: max error {err.max(initial=0):.3e}, at most {worst:.3f} of its bound")
        assert (err <= bound).all(), (n, worst)


# ---- 6. the module ----
def make_module(shape, **kw):
    from posecnn_amd import pth
    B, h, w, K, U, V = shape
    torch.manual_seed(0)
    return pth.EmbeddingNeck(in_channels=K, num_units=U, vertex_units=V, **kw).to(DEV)


def test_module_backward_is_embedding_bwd(hip):
    from posecnn_amd import neck
    shape = nc.SHAPES[0]
    B, h, w, K, U, V = shape
    t = device_case("float", shape)
    m = make_module(shape, keep_prob=KEEP, seed=nc.SEED)
    assert m.weight4.shape == (K, U + V) and m.bias5.shape == (U + V,) and m.step.dtype == torch.int64
    w4 = m.weight4.detach()
    assert float(w4.abs().max()) <= 0.002 and float(w4.std()) > 0.0005 and not m.bias4.any()
    assert not torch.equal(m.weight4, m.weight5)
    with torch.no_grad():   # order-1 parameters, so that every gradient is far from 0
        for p, n in ((m.weight4, "W4"), (m.bias4, "b4"), (m.weight5, "W5"), (m.bias5, "b5")):
            p.copy_(t[n])
    m.advance()
    m.advance()
    x4, x5 = t["x4"].clone().requires_grad_(), t["x5"].clone().requires_grad_()
    s, v = m(x4, x5)
    ((s * t["d_s"]).sum() + (v * t["d_v"]).sum()).backward()
    rs, rv, ctx = neck.embedding(t["x4"], t["x5"], t["W4"], t["b4"], t["W5"], t["b5"], U, keep_prob=KEEP,
                                 drop_gen=(nc.SEED, step_counter(2), nc.STREAM_IDS))
    d = neck.embedding_bwd(ctx, t["d_s"], t["d_v"])
    same_bits(host(s), host(rs), "add_score")
    same_bits(host(v), host(rv), "add_score_vertex")
    np.testing.assert_array_equal(host(ctx["keep_score"]), keeps(shape, 2)[0])
    for n, leaf in (("x4", x4), ("x5", x5), ("W4", m.weight4), ("b4", m.bias4), ("W5", m.weight5), ("b5", m.bias5)):
        same_bits(host(leaf.grad), host(d[n]), n)


def test_module_load_reference_equals_the_per_branch_composition(hip):
    """The four reference variables, loaded, against the layers one branch at a
    time through the ops that were there before the neck (gemm with bias and
    activation, upscore, a torch add): both sides are within test 5's bound of
    the exact value, so within twice it of each other."""
    from posecnn_amd import pose_head, upscore
    shape = nc.SHAPES[0]
    B, h, w, K, U, V = shape
    N, M4 = U + V, B * h * w
    c, t = nc.float_case(shape), device_case("float", shape)
    m = make_module(shape).eval()
    split = lambda W, b: ((W[:, :U].reshape(1, 1, K, U), b[:U]), (W[:, U:].copy(), b[U:]))  # noqa: E731
    (s4, v4), (s5, v5) = split(c["W4"], c["b4"]), split(c["W5"], c["b5"])
    m.load_reference(score_conv4=s4, score_conv5=s5, score_conv4_vertex=v4, score_conv5_vertex=v5)
    same_bits(host(m.weight4), c["W4"], "weight4")
    same_bits(host(m.bias5), c["b5"], "bias5")
    with torch.no_grad():
        got = m(t["x4"], t["x5"])
    _, mag = float_layer_reference(shape, 1.0)
    for out, (W4b, b4b), (W5b, b5b), act, name in ((got[0], s4, s5, 1, "add_score"),
                                                   (got[1], v4, v5, 0, "add_score_vertex")):
        n = b4b.shape[0]
        y4 = torch.empty((M4, n), device=DEV)
        y5 = torch.empty((M4 // 4, n), device=DEV)
        pose_head.gemm(t["x4"].view(M4, K), dev(W4b.reshape(K, n)), y4, bias=dev(b4b), act=act)
        pose_head.gemm(t["x5"].view(M4 // 4, K), dev(W5b.reshape(K, n)), y5, bias=dev(b5b), act=act)
        want = y4.view(B, h, w, n) + upscore.upscore(y5.view(B, h // 2, w // 2, n), 2)
        err = np.abs(host(out).astype(np.float64) - host(want))
        assert (err <= 2 * (K + 16) * U24 * mag[name]).all(), (name, err.max())


def test_module_eval_draws_nothing_and_training_draws_per_step(hip):
    from posecnn_amd import neck
    shape = nc.SHAPES[0]
    B, h, w, K, U, V = shape
    t = device_case("float", shape)
    m = make_module(shape, keep_prob=KEEP, seed=7)
    with torch.no_grad():
        m.weight4.copy_(t["W4"]), m.weight5.copy_(t["W5"]), m.bias4.copy_(t["b4"]), m.bias5.copy_(t["b5"])
        m.eval()
        e0 = m(t["x4"], t["x5"])
        m.advance()
        e1 = m(t["x4"], t["x5"])
        plain = neck.embedding(t["x4"], t["x5"], t["W4"], t["b4"], t["W5"], t["b5"], U)
        for a, b, p in zip(e0, e1, plain[:2]):
            same_bits(host(a), host(p), "eval() is keep_prob 1")
            same_bits(host(a), host(b), "eval() does not depend on the step")
        assert plain[2]["keep_score"] is None
        m.train()
        a = m(t["x4"], t["x5"])
        again = m(t["x4"], t["x5"])
        m.advance()
        b = m(t["x4"], t["x5"])
    assert int(m.step) == 2
    same_bits(host(a[0]), host(again[0]), "the same step draws the same mask")
    za, zb = host(a[1]) == 0, host(b[1]) == 0
    assert 0.35 < za.mean() < 0.65 and (za != zb).any()
    kept = ~host(a[0] == 0)
    np.testing.assert_array_equal(host(a[0])[kept], (host(e0[0]) / np.float32(KEEP))[kept])


def test_module_feeds_both_heads_end_to_end(hip):
    from posecnn_amd import pth
    shape = nc.SHAPES[0]
    B, h, w, K, U, V = shape
    C = 5
    t = device_case("float", shape)
    torch.manual_seed(1)
    m = make_module(shape, keep_prob=KEEP)
    score_head = pth.ScoreHead(U, C, stride=8).to(DEV)
    vertex_head = pth.VertexHeadCompact(V, C, stride=8).to(DEV)
    with torch.no_grad():
        m.weight4.copy_(t["W4"]), m.weight5.copy_(t["W5"]), m.bias4.copy_(t["b4"]), m.bias5.copy_(t["b5"])
        for head in (score_head, vertex_head):
            head.weight.mul_(1000.0)
    label = torch.randint(0, C, (B, 8 * h, 8 * w), device=DEV, dtype=torch.int32)
    add_score, add_score_vertex = m(t["x4"], t["x5"])
    score = score_head(add_score)
    vertex3 = vertex_head(add_score_vertex, label)
    assert score.shape == (B, 8 * h, 8 * w, C) and vertex3.shape == (B, 8 * h, 8 * w, 3)
    (score.sum() + (vertex3 * vertex3).sum()).backward()
    for name, p in list(m.named_parameters()) + [("score.weight", score_head.weight),
                                                 ("vertex.weight", vertex_head.weight)]:
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, name
    assert sorted(n for n, _ in m.named_parameters()) == ["bias4", "bias5", "weight4", "weight5"]


# ---- 7. the contract ----
def test_contract_refusals_come_before_any_launch(hip):
    from posecnn_amd import neck
    shape = nc.SHAPES[0]
    B, h, w, K, U, V = shape
    t = device_case("float", shape)
    ok = dict(x4=t["x4"], x5=t["x5"], W4=t["W4"], b4=t["b4"], W5=t["W5"], b5=t["b5"], num_units=U, keep_prob=KEEP,
              drop_gen=(nc.SEED, step_counter(0), nc.STREAM_IDS))
    wide = torch.zeros((B, h, w, 2 * K), device=DEV)
    bad = {
        "float64 x4": dict(x4=t["x4"].double()),
        "float64 W5": dict(W5=t["W5"].double()),
        "strided x4": dict(x4=wide[..., ::2]),
        "strided W4": dict(W4=torch.zeros((K, 2 * (U + V)), device=DEV)[:, ::2]),
        "odd h": dict(x4=t["x4"][:, :5].contiguous()),
        "odd w": dict(x4=t["x4"][:, :, :9].contiguous()),
        "U % 4": dict(num_units=U + 2),
        "x5 extents": dict(x5=t["x5"][:, :, :4].contiguous()),
        "x5 channels": dict(x5=t["x5"][..., :K - 4].contiguous()),
        "b4 length": dict(b4=t["b4"][:-4].contiguous()),
        "int32 step counter": dict(drop_gen=(nc.SEED, torch.zeros(1, dtype=torch.int32, device=DEV), nc.STREAM_IDS)),
        "host step counter": dict(drop_gen=(nc.SEED, torch.zeros(1, dtype=torch.int64), nc.STREAM_IDS)),
        "keep_prob 0": dict(keep_prob=0.0),
    }
    neck._load()
    with abi_guard.installed() as guard:   # counts the GEMM launches: the layer's first
        for what, kw in bad.items():
            with pytest.raises(ValueError):
                neck.embedding(**dict(ok, **kw))
            assert guard.launches == 0 and not guard.calls, what
        neck.embedding(**ok)
        assert guard.calls["pcnn_gemm"] == 2
    z = dict(z4=t["z4"], z5=t["z5"], b4=t["b4"], b5=t["b5"], relu_cols=U)
    for what, kw in {"float64 z4": dict(z4=t["z4"].double()), "strided z5": dict(z5=t["z5"].transpose(1, 2)),
                     "odd h": dict(z4=t["z4"][:, :5].contiguous()), "U % 4": dict(relu_cols=U + 1),
                     "z5 extents": dict(z5=t["z5"][:, :2].contiguous())}.items():
        with pytest.raises(ValueError):
            neck.neck_fwd(**dict(z, **kw))
    s, v, ks, kv = neck.neck_fwd(**z, keep_prob=KEEP, drop_gen=(nc.SEED, step_counter(0), None))
    with pytest.raises(ValueError):   # a float keep map
        neck.neck_bwd(t["d_s"], t["d_v"], ks.float(), kv, t["z4"], t["z5"], t["b4"], t["b5"], U, keep_prob=KEEP)
    with pytest.raises(ValueError):   # a gradient of the wrong width
        neck.neck_bwd(t["d_v"], t["d_v"], ks, kv, t["z4"], t["z5"], t["b4"], t["b5"], U, keep_prob=KEEP)
    with pytest.raises(ValueError):
        neck.embedding_bwd({}, t["d_s"], t["d_v"], want=("x4", "nothing"))
