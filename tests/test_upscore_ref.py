"""tests/upscore_ref.py against independent statements of the same layer, on
the CPU: torch's depthwise conv_transpose2d with the bilinear filter, the
closed form of the weights, the adjoint identity, and per-pixel loops for the
class-compact forms."""
import numpy as np
import pytest
import torch

import upscore_ref as ref


def bilinear_filter(s):
    """The 2s-tap hat 1 - |t/s - (2s-1)/(2s)| of the reference's deconv filter."""
    t = np.arange(2 * s, dtype=np.float64)
    return 1.0 - np.abs(t / s - (2 * s - 1) / (2.0 * s))


@pytest.mark.parametrize("s", ref.STRIDES)
@pytest.mark.parametrize("hw", [(1, 1), (1, 4), (3, 5), (4, 2)])
def test_f64_mode_is_the_depthwise_transposed_conv(s, hw):
    h, w = hw
    rng = np.random.default_rng(10 * s + h)
    x = rng.standard_normal((2, h, w, 3))
    f = bilinear_filter(s)
    k = torch.tensor(np.outer(f, f)).expand(3, 1, 2 * s, 2 * s).contiguous()
    want = torch.nn.functional.conv_transpose2d(torch.tensor(x).permute(0, 3, 1, 2), k, stride=s, padding=s // 2,
                                                groups=3).permute(0, 2, 3, 1).numpy()
    got = ref.upscore_fwd_ref(x, s, mode="f64")
    assert got.shape == (2, s * h, s * w, 3) == want.shape
    assert np.abs(got - want).max() <= 1e-12
    # the pinned float32 order on float32 inputs: within four roundings of it
    x32 = x.astype(np.float32)
    got32 = ref.upscore_fwd_ref(x32, s, mode="f32")
    assert got32.dtype == np.float32
    err = np.abs(got32 - ref.upscore_fwd_ref(x32, s, mode="f64"))
    assert (err <= ref.sum_bound(4, ref.upscore_fwd_ref(np.abs(x32), s, mode="f64"))).all()


@pytest.mark.parametrize("s", ref.STRIDES)
def test_weights_equal_the_closed_form(s):
    for n in (1, 2, 5):
        m = ref.matrix(n, s)
        y, i = np.arange(s * n)[:, None], np.arange(n)[None, :]
        hat = np.maximum(0.0, 1.0 - np.abs(y - (s * i + (s - 1) / 2.0)) / s)   # centre of low-res pixel i
        np.testing.assert_array_equal(m, hat)
        assert ((m > 0).sum(axis=1) <= 2).all() and ((m > 0).sum(axis=0) <= 2 * s).all()
        assert (m.astype(np.float32) == m).all()   # dyadic: exact in float32
        interior = m[s // 2:s * n - s // 2]
        if len(interior):
            np.testing.assert_array_equal(interior.sum(axis=1), 1.0)
        i0, i1, w0, w1, p0, p1 = ref.taps(n, s)
        assert (i0 == i1 - 1).all() and (p0 | p1).all()
        np.testing.assert_array_equal(w0 + w1, 1.0)


@pytest.mark.parametrize("s", ref.STRIDES)
def test_adjoint_identity_is_exact_on_integers(s):
    rng = np.random.default_rng(s)
    h, w, Ch = 3, 2, 5
    x = rng.integers(-4, 5, size=(2, h, w, Ch)).astype(np.float64)
    g = rng.integers(-4, 5, size=(2, s * h, s * w, Ch)).astype(np.float64)
    r = ref.upscore_bwd_ref(g, s)
    assert (ref.upscore_fwd_ref(x, s, mode="f64") * g).sum() == (x * r["d_x"]).sum()
    np.testing.assert_array_equal(r["d_bias"], g.sum(axis=(0, 1, 2)))
    # float32 mode on the same integers: no rounding anywhere
    np.testing.assert_array_equal(ref.upscore_fwd_ref(x.astype(np.float32), s, mode="f32"),
                                  ref.upscore_fwd_ref(x, s, mode="f64"))
    assert r["n_x"].max() <= (2 * s) ** 2
    assert r["n_x"].sum() == (ref.matrix(h, s) > 0).sum() * (ref.matrix(w, s) > 0).sum()
    # with a ReLU mask
    y = rng.standard_normal(g.shape)
    rm = ref.upscore_bwd_ref(g, s, y=y)
    np.testing.assert_array_equal(rm["d_x"], ref.upscore_bwd_ref(np.where(y > 0, g, 0.0), s)["d_x"])


def test_bias_and_relu_epilogue():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((1, 2, 3, 4)).astype(np.float32)
    b = rng.standard_normal(4).astype(np.float32)
    plain = ref.upscore_fwd_ref(x, 4)
    np.testing.assert_array_equal(ref.upscore_fwd_ref(x, 4, bias=b), plain + b)
    full = ref.upscore_fwd_ref(x, 4, bias=b, relu=True)
    np.testing.assert_array_equal(full, np.maximum(plain + b, 0))
    assert (full == 0).any() and (full > 0).any()


@pytest.mark.parametrize("s", [2, 8])
def test_compact_forms_are_the_dense_forms_by_class(s):
    rng = np.random.default_rng(5 + s)
    B, h, w, C = 2, 2, 3, 4
    H, W = s * h, s * w
    z = rng.standard_normal((B, h, w, 3 * C))
    bias = rng.standard_normal(3 * C)
    label = rng.integers(0, C, size=(B, H, W))
    label.reshape(-1)[rng.choice(label.size, 4, replace=False)] = [-1, C, C + 5, -100]
    g = rng.integers(-4, 5, size=(B, H, W, 3)).astype(np.float64)
    mr, mc = ref.matrix(h, s), ref.matrix(w, s)
    fwd = np.zeros((B, H, W, 3))
    d_z = np.zeros((B, h, w, 3 * C))
    d_b = np.zeros(3 * C)
    n_z = np.zeros((B, h, w, 3 * C))
    for b in range(B):
        for y in range(H):
            for x in range(W):
                l = label[b, y, x]
                if not 0 <= l < C:
                    continue
                ch = slice(3 * l, 3 * l + 3)
                wgt = np.outer(mr[y], mc[x])   # (h, w)
                fwd[b, y, x] = np.tensordot(wgt, z[b, :, :, ch], axes=2) + bias[ch]
                d_z[b, :, :, ch] += wgt[:, :, None] * g[b, y, x]
                n_z[b, :, :, ch] += (wgt > 0)[:, :, None]
                d_b[ch] += g[b, y, x]
    got = ref.upscore_compact_fwd_ref(z, bias, label, s, mode="f64")
    assert np.abs(got - fwd).max() <= 1e-12
    assert (got[~ref.live(label, C)] == 0).all()
    r = ref.upscore_compact_bwd_ref(label, g, C, s)
    np.testing.assert_array_equal(r["d_z"], d_z)   # integers times dyadic weights: exact
    np.testing.assert_array_equal(r["d_bias"], d_b)
    np.testing.assert_array_equal(r["n_z"], n_z)
    # gather and scatter are adjoint
    dense = rng.standard_normal((B, H, W, 3 * C))
    assert np.isclose((ref.gather_class(dense, label) * g).sum(), (dense * ref.scatter_class(g, label, C)).sum())
    # the float32 compact forward is the float32 dense forward at those channels
    z32, b32 = z.astype(np.float32), bias.astype(np.float32)
    np.testing.assert_array_equal(ref.upscore_compact_fwd_ref(z32, b32, label, s),
                                  ref.gather_class(ref.upscore_fwd_ref(z32, s, bias=b32), label))
