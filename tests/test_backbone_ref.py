"""The backbone's numpy restatement and test operands, checked on the CPU:
tests/backbone_ref.py against torch's own conv2d / max_pool2d in float64, the
exact operand classes of tests/backbone_cases.py against the plane-product
model of tests/gemm_exact_cases.py, and the layer table of
posecnn_amd/backbone.py against the reference's."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import backbone_cases as bc
import backbone_ref as ref
import gemm_exact_cases as gx

REF_SHAPES = ((2, 5, 7, 16, 20), (1, 1, 1, 16, 4), (1, 1, 9, 16, 4), (2, 5, 7, 3, 64), (1, 4, 6, 3, 8),
              (1, 1, 1, 3, 4))


def torch_conv(x, w, bias, relu):
    xt = torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2)           # NHWC -> NCHW
    wt = torch.from_numpy(w.astype(np.float64)).permute(3, 2, 0, 1)           # HWIO -> OIHW
    bt = None if bias is None else torch.from_numpy(bias.astype(np.float64))
    y = F.conv2d(xt, wt, bt, stride=1, padding=1)
    if relu:
        y = F.relu(y)
    return y.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("shape", REF_SHAPES, ids=bc.ident)
@pytest.mark.parametrize("relu", (True, False))
def test_conv_restatements_match_torch(shape, relu):
    x, w, b = bc.float_case(shape)
    want = torch_conv(x, w, b, relu)
    got, mag = ref.conv3x3_f64(x, w, b, relu)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12 * max(1.0, float(mag.max())))
    assert (mag >= np.abs(got) - 1e-12).all()
    # without a bias
    np.testing.assert_allclose(ref.conv3x3_f64(x, w, None, relu)[0], torch_conv(x, w, None, relu), rtol=0,
                               atol=1e-12 * max(1.0, float(mag.max())))
    if shape[3] == 3:   # the float32 order: within float32 summation error of float64
        d = ref.conv3x3_direct_f32(x, w, b, relu)
        assert d.dtype == np.float32
        assert (np.abs(d - want) <= (27 + 2) * 2.0 ** -24 * mag).all()


def test_im2col_is_the_implicit_matrix():
    shape = (2, 5, 7, 16, 20)
    x, w, b = bc.float_case(shape)
    A = ref.im2col(x)
    assert A.shape == (2 * 5 * 7, 9 * 16)
    got = (A.astype(np.float64) @ w.reshape(9 * 16, 20).astype(np.float64)).reshape(2, 5, 7, 20)
    np.testing.assert_allclose(got, ref.conv3x3_f64(x, w, None, relu=False)[0], rtol=0, atol=1e-12)


@pytest.mark.parametrize("shape", bc.POOL_SHAPES + ((1, 1, 6, 4), (2, 7, 1, 4), (1, 3, 3, 8)), ids=bc.ident)
def test_pool_restatement_matches_torch(shape):
    x = bc.negative_map(shape)
    want = F.max_pool2d(torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2), 2, 2, ceil_mode=True)
    got = ref.max_pool2x2(x)
    assert got.dtype == np.float32 and got.shape == (shape[0], (shape[1] + 1) // 2, (shape[2] + 1) // 2, shape[3])
    np.testing.assert_array_equal(got.astype(np.float64), want.permute(0, 2, 3, 1).numpy())
    assert (got < 0).all()


@pytest.mark.parametrize("shape", bc.MFMA_SHAPES, ids=bc.ident)
@pytest.mark.parametrize("cls", sorted(bc.CLASSES))
def test_exact_classes_stay_exact(cls, shape):
    """Every kept plane product and every partial sum is an integer below
    2^24 (bias included), nothing is dropped, and the class lights the plane
    products it is named for -- where the shape has room for them."""
    x, w, b = bc.exact_case(cls, shape)
    Cin, Cout = shape[3], shape[4]
    for a in (x, w, b):
        assert (a == np.round(a)).all()
    p = gx.kept_products(ref.im2col(x), w.reshape(9 * Cin, Cout), "x6")
    assert p.dropped == 0.0
    assert p.abs_sum + float(np.abs(b).max()) < bc.LIMIT, p.abs_sum
    want, _ = ref.conv3x3_f64(x, w, None, relu=False)
    np.testing.assert_array_equal(p.model.reshape(want.shape), want)
    if cls == "x19":
        assert (np.count_nonzero(w.reshape(9 * Cin, Cout), axis=0) <= bc.SPARSE_NNZ).all()
    if cls == "w19":
        assert (np.count_nonzero(ref.im2col(x), axis=1) <= 9).all()
    if shape[0] * shape[1] * shape[2] >= 16:   # a one-pixel map need not reach every plane
        for name in bc.CLASSES[cls]:
            assert p.active[name], (cls, name)


def test_classes_light_all_six_products():
    lit = set()
    for cls in ("dense4", "x19", "w19", "mm10"):
        lit |= set(bc.CLASSES[cls])
    shape = bc.MFMA_SHAPES[1]
    active = set()
    for cls in ("dense4", "x19", "w19", "mm10"):
        x, w, _ = bc.exact_case(cls, shape)
        p = gx.kept_products(ref.im2col(x), w.reshape(9 * shape[3], shape[4]), "x6")
        active |= {n for n, on in p.active.items() if on}
    assert active == set(bc.ALL_KEPT)
    assert lit <= active


def test_layer_table_is_the_reference():
    from posecnn_amd import backbone
    convs = [("conv1_1", 3, 64), ("conv1_2", 64, 64), ("conv2_1", 64, 128), ("conv2_2", 128, 128),
             ("conv3_1", 128, 256), ("conv3_2", 256, 256), ("conv3_3", 256, 256), ("conv4_1", 256, 512),
             ("conv4_2", 512, 512), ("conv4_3", 512, 512), ("conv5_1", 512, 512), ("conv5_2", 512, 512),
             ("conv5_3", 512, 512)]
    assert list(backbone.CONVS) == convs and len(backbone.CONVS) == 13
    names = [layer[0] for layer in backbone.LAYERS]
    pools = {"pool1": "conv1_2", "pool2": "conv2_2", "pool3": "conv3_3", "pool4": "conv4_3"}
    assert [n for n in names if n.startswith("pool")] == list(pools)
    for pool, before in pools.items():
        assert names[names.index(pool) - 1] == before
    assert names[-1] == "conv5_3"
    shapes = ref.vgg16_shapes(backbone.LAYERS, 8, 480, 640)
    assert shapes["conv4_3"] == (8, 60, 80, 512) and shapes["conv5_3"] == (8, 30, 40, 512)
    assert ref.vgg16_shapes(backbone.LAYERS, 1, 17, 23)["conv5_3"] == (1, 2, 2, 512)
    # about 94 GMAC per 640 x 480 frame
    macs = sum(shapes[n][1] * shapes[n][2] * 9 * cin * cout for n, cin, cout in backbone.CONVS)
    assert 90e9 < macs < 98e9


def test_header_and_bindings_agree():
    """posecnn_backbone.h declares exactly the symbols backbone.SIGS binds, with as many parameters."""
    import os
    import abi_guard
    from posecnn_amd import backbone
    header = os.path.join(abi_guard.ROOT, "include", "posecnn_backbone.h")
    protos = abi_guard.prototypes(header)
    assert set(protos) == set(backbone.SIGS)
    for name, params in protos.items():
        assert len(params) == len(backbone.SIGS[name][1]), name
