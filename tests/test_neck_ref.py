"""CPU checks of the numpy restatement of the embedding neck
(tests/neck_ref.py): the float64 layer and its backward against a torch-CPU
composition (1x1 conv2d, ReLU on the score columns, conv_transpose2d with the
bilinear filter, add, mask) and its autograd; the float32 order against the
float64 mode; the integer operands' magnitudes; and include/posecnn_neck.h
against posecnn_amd/neck.py's signature table, the built library's exports and
the entry points' host-side refusals."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import abi_guard
import neck_cases as nc
import neck_ref as ref
import upscore_ref as up

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NECK_HEADER = os.path.join(ROOT, "include", "posecnn_neck.h")
KEEP = 0.5


def torch_layer(c, shape, keep, keep_prob):
    """The layer as a float64 torch-CPU graph, per branch as the reference
    builds it; returns (add_score, add_score_vertex, leaves)."""
    B, h, w, K, U, V = shape
    leaves = {n: torch.tensor(c[n], dtype=torch.float64, requires_grad=True) for n in ("x4", "x5", "W4", "b4", "W5",
                                                                                       "b5")}
    t = np.arange(4, dtype=np.float64)
    hat = torch.tensor(1.0 - np.abs(t / 2 - 0.75))   # the reference's make_deconv_filter at 4x4: 1/4 3/4 3/4 1/4
    outs = []
    for lo, hi, relu, km in ((0, U, True, keep[0]), (U, U + V, False, keep[1])):
        n = hi - lo
        if n == 0:
            outs.append(torch.zeros((B, h, w, 0), dtype=torch.float64))
            continue
        conv = lambda x, W, b: torch.nn.functional.conv2d(  # noqa: E731
            x.permute(0, 3, 1, 2), W[:, lo:hi].t().reshape(n, K, 1, 1), b[lo:hi])
        s4 = conv(leaves["x4"], leaves["W4"], leaves["b4"])
        s5 = conv(leaves["x5"], leaves["W5"], leaves["b5"])
        if relu:
            s4, s5 = torch.relu(s4), torch.relu(s5)
        kern = torch.outer(hat, hat).expand(n, 1, 4, 4).contiguous()
        a = s4 + torch.nn.functional.conv_transpose2d(s5, kern, stride=2, padding=1, groups=n)
        a = a.permute(0, 2, 3, 1)
        if keep_prob != 1.0:
            a = (a / keep_prob) * torch.tensor(km.reshape(B, h, w, n), dtype=torch.float64)
        outs.append(a)
    return outs[0], outs[1], leaves


@pytest.mark.parametrize("shape", nc.SHAPES[:2] + nc.SHAPES[3:], ids=nc.IDS[:2] + nc.IDS[3:])
@pytest.mark.parametrize("keep_prob", [1.0, KEEP])
def test_f64_layer_is_the_torch_composition_and_its_autograd(shape, keep_prob):
    B, h, w, K, U, V = shape
    c = nc.float_case(shape)
    keep = ref.keep_maps(B * h * w, U, V, nc.SEED, 3, nc.STREAM_IDS, KEEP)
    s, v, leaves = torch_layer(c, shape, keep, keep_prob)
    r = ref.layer_f64(c["x4"], c["x5"], c["W4"], c["b4"], c["W5"], c["b5"], U, keep_prob, keep, d=(c["d_s"], c["d_v"]))
    assert r["add_score"].shape == (B, h, w, U) and r["add_score_vertex"].shape == (B, h, w, V)
    np.testing.assert_allclose(r["add_score"], s.detach().numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(r["add_score_vertex"], v.detach().numpy(), rtol=0, atol=1e-12)
    loss = (s * torch.tensor(c["d_s"], dtype=torch.float64)).sum() + \
           (v * torch.tensor(c["d_v"], dtype=torch.float64)).sum()
    loss.backward()
    for n in ("x4", "x5", "W4", "b4", "W5", "b5"):
        np.testing.assert_allclose(r[n], leaves[n].grad.numpy(), rtol=0, atol=1e-10, err_msg=n)


@pytest.mark.parametrize("shape", nc.SHAPES, ids=nc.IDS)
def test_two_passes_equal_the_layer_and_f32_tracks_f64(shape):
    """neck_fwd_ref / neck_bwd_ref on z = x W are the layer; the pinned float32
    order stays within the rounding of its few operations of the float64 mode."""
    B, h, w, K, U, V = shape
    c = nc.float_case(shape)
    keep = ref.keep_maps(B * h * w, U, V, nc.SEED, 0, nc.STREAM_IDS, KEEP)
    lay = ref.layer_f64(c["x4"], c["x5"], c["W4"], c["b4"], c["W5"], c["b5"], U, KEEP, keep, d=(c["d_s"], c["d_v"]))
    s, v = ref.neck_fwd_ref(lay["z4"], lay["z5"], c["b4"], c["b5"], U, KEEP, keep, mode="f64")
    np.testing.assert_array_equal(s, lay["add_score"])
    np.testing.assert_array_equal(v, lay["add_score_vertex"])
    b = ref.neck_bwd_ref(c["d_s"], c["d_v"], keep, lay["z4"], lay["z5"], c["b4"], c["b5"], U, KEEP, mode="f64")
    np.testing.assert_array_equal(b["dz4"], lay["dz4"])
    np.testing.assert_allclose(b["dz5"], lay["dz5"], rtol=0, atol=1e-13)
    np.testing.assert_allclose(b["db5"], lay["b5"], rtol=0, atol=1e-11)
    assert b["n_dz5"].shape == (h // 2, w // 2) and b["n_dz5"].min() == 9   # a corner's window: 3 x 3 inside
    assert b["n_dz5"].max() == (16 if min(h, w) >= 6 else 12 if max(h, w) >= 6 else 9)
    # float32 on float32 operands: z + b, four products, three sums, the add, (the division by 0.5 is exact)
    z4, z5 = c["z4"], c["z5"]
    s32, v32 = ref.neck_fwd_ref(z4, z5, c["b4"], c["b5"], U, KEEP, keep, mode="f32")
    s64, v64 = ref.neck_fwd_ref(z4, z5, c["b4"], c["b5"], U, KEEP, keep, mode="f64")
    # the magnitudes: absolute operands and no ReLU column, so all N columns come back as the second map
    _, mag = ref.neck_fwd_ref(np.abs(z4), np.abs(z5), np.abs(c["b4"]), np.abs(c["b5"]), 0, KEEP, keep, mode="f64")
    assert s32.dtype == np.float32 and v32.dtype == np.float32
    assert (np.abs(s32 - s64) <= up.sum_bound(8, mag[..., :U])).all()
    assert (np.abs(v32 - v64) <= up.sum_bound(8, mag[..., U:])).all()
    b32 = ref.neck_bwd_ref(c["d_s"], c["d_v"], keep, z4, z5, c["b4"], c["b5"], U, KEEP, mode="f32")
    b64 = ref.neck_bwd_ref(c["d_s"], c["d_v"], keep, z4, z5, c["b4"], c["b5"], U, KEEP, mode="f64")
    np.testing.assert_array_equal(b32["dz4"], b64["dz4"])
    assert (np.abs(b32["dz5"] - b64["dz5"]) <= up.sum_bound(b64["n_dz5"][None, :, :, None], b64["abs_dz5"])).all()


@pytest.mark.parametrize("shape", nc.SHAPES, ids=nc.IDS)
def test_integer_operands_stay_exact_in_float32(shape):
    """Every magnitude of the integer cases stays below 2^20 and every value is a
    multiple of 1/16: any float32 summation order is exact (the device tests
    compare with == on these operands)."""
    B, h, w, K, U, V = shape
    c = nc.integer_case(shape)
    keep = ref.keep_maps(B * h * w, U, V, nc.SEED, 0, nc.STREAM_IDS, KEEP)
    args = [c[n] for n in ("x4", "x5", "W4", "b4", "W5", "b5")]
    r = ref.layer_f64(*args, U, KEEP, keep, d=(c["d_s"], c["d_v"]))
    mag = ref.layer_f64(*[np.abs(a) for a in args], U, KEEP, keep, d=(np.abs(c["d_s"]), np.abs(c["d_v"])),
                        masks=r["masks"])
    for n in ("add_score", "add_score_vertex", "z4", "z5", "dz4", "dz5", "x4", "x5", "W4", "b4", "W5", "b5"):
        assert np.abs(mag[n]).max(initial=0) < 2 ** 20, n
        assert (np.abs(r[n]) <= mag[n]).all(), n
        assert (r[n] * 16 == np.round(r[n] * 16)).all(), n
        assert (r[n].astype(np.float32) == r[n]).all(), n
    # the two passes alone, on integer z: the float32 order gives the float64 values
    s32, v32 = ref.neck_fwd_ref(c["z4"], c["z5"], c["b4"], c["b5"], U, KEEP, keep, mode="f32")
    s64, v64 = ref.neck_fwd_ref(c["z4"], c["z5"], c["b4"], c["b5"], U, KEEP, keep, mode="f64")
    np.testing.assert_array_equal(s32, s64)
    np.testing.assert_array_equal(v32, v64)
    b32 = ref.neck_bwd_ref(c["d_s"], c["d_v"], keep, c["z4"], c["z5"], c["b4"], c["b5"], U, KEEP, mode="f32")
    b64 = ref.neck_bwd_ref(c["d_s"], c["d_v"], keep, c["z4"], c["z5"], c["b4"], c["b5"], U, KEEP, mode="f64")
    for n in ("dz4", "dz5", "db4", "db5"):
        np.testing.assert_array_equal(b32[n], b64[n], err_msg=n)


def test_keep_maps_are_dense_masks_per_branch():
    ks, kv = ref.keep_maps(30, 12, 20, nc.SEED, 1, (1, 2), KEEP)
    assert ks.shape == (30, 12) and kv.shape == (30, 20) and ks.dtype == np.uint8
    assert set(np.unique(ks)) == {0, 1} and 0.3 < ks.mean() < 0.7 and 0.3 < kv.mean() < 0.7
    ks0, _ = ref.keep_maps(30, 12, 20, nc.SEED, 0, (1, 2), KEEP)
    assert (ks0 != ks).any()
    _, kv_as_s = ref.keep_maps(30, 12, 12, nc.SEED, 1, (1, 1), KEEP)
    np.testing.assert_array_equal(kv_as_s, ks)   # the stream id, not the branch, picks the stream


# ---- the header, the build and the library ----
def test_new_source_and_header_are_built():
    from posecnn_amd import build
    assert "neck.hip" in build.SOURCES and "neck.hip" not in build.NO_SLP
    assert os.path.abspath(NECK_HEADER) in [os.path.abspath(h) for h in build.HEADERS]


def test_header_parses_and_matches_the_signature_table():
    from posecnn_amd import _lib, evaluate, neck, optim
    from posecnn_amd.synthesize import image
    protos = abi_guard.prototypes(header=NECK_HEADER)
    assert set(protos) == set(neck.SIGS)
    for other in (_lib._SIGS, optim.SIGS, evaluate.SIGS, image.SIGS):
        assert not set(neck.SIGS) & set(other)
    assert not set(neck.SIGS) & set(abi_guard.prototypes())   # not in include/posecnn_hip.h either
    ints = {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t, "long": ctypes.c_long,
            "uint64_t": ctypes.c_uint64}
    for name, params in protos.items():
        res, args = neck.SIGS[name]
        assert len(args) == len(params), name
        for p, a in zip(params, args):
            assert a is (ctypes.c_void_p if p.is_pointer else ints[p.c_type]), (name, p.name)
            assert not p.is_pointer or p.elem_type in abi_guard.ELEM, (name, p.name)
    decl = open(NECK_HEADER).read()
    assert "size_t pcnn_neck_bwd_workspace_size" in decl and "int pcnn_neck_fwd" in decl
    assert '#include "posecnn_hip.h"' in decl


def test_library_exports_every_declared_function():
    from posecnn_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in out.stdout.splitlines() if line.strip()}
    missing = set(abi_guard.declarations(NECK_HEADER)) - exported
    assert not missing, missing


@pytest.fixture(scope="module")
def lib():
    from posecnn_amd import neck
    return neck._load()


def test_versions_and_queries(lib):
    assert lib.pcnn_neck_abi_version() == 1
    assert lib.pcnn_abi_version() == 8 and lib.pcnn_train_abi_version() == 1 and lib.pcnn_eval_abi_version() == 1
    need = lib.pcnn_neck_bwd_workspace_size(8, 60, 80, 64, 128)
    assert need >= 2 * 192 * 4 and need % 256 == 0
    assert lib.pcnn_neck_bwd_workspace_size(8, 60, 80, 64, 128) > lib.pcnn_neck_bwd_workspace_size(1, 60, 80, 64, 128)
    for bad in ((0, 4, 4, 4, 4), (1, 3, 4, 4, 4), (1, 4, 5, 4, 4), (1, 4, 4, 6, 4), (1, 4, 4, 4, 2), (1, 4, 4, 0, 0),
                (1, 4, 4, -4, 8), (2048, 1024, 1024, 4, 0)):
        assert lib.pcnn_neck_bwd_workspace_size(*bad) == 0, bad


def test_host_side_refusals_need_no_gpu(lib):
    """Each of these is refused by the argument check, before any HIP call; the
    pointers are never dereferenced."""
    fake = ctypes.c_void_p(0x1000)
    ok = dict(z4=fake, z5=fake, b4=fake, b5=fake, B=1, h=4, w=4, U=4, V=4, keep_prob=0.5, seed=1, step_dev=fake,
              sid_s=1, sid_v=2, add_score=fake, add_score_vertex=fake, keep_score=fake, keep_vertex=fake, stream=None)

    def fwd(**kw):
        return lib.pcnn_neck_fwd(*dict(ok, **kw).values())

    for name in ("z4", "z5", "b4", "b5", "add_score", "add_score_vertex", "keep_score", "keep_vertex"):
        assert fwd(**{name: None}) == 1, name
        assert fwd(**{name: ctypes.c_void_p(0x1002)}) == 1, name
    assert fwd(h=3) == 1 and fwd(w=5) == 1 and fwd(B=0) == 1 and fwd(h=0) == 1
    assert fwd(U=6) == 1 and fwd(V=2) == 1 and fwd(U=0, V=0) == 1 and fwd(U=-4, V=8) == 1
    assert fwd(keep_prob=0.0) == 1 and fwd(keep_prob=1.5) == 1 and fwd(keep_prob=float("nan")) == 1
    assert fwd(sid_s=-1) == 1 and fwd(sid_v=-1) == 1
    assert fwd(B=2048, h=1024, w=1024, U=4, V=0) == 1   # 2^33 elements
    assert fwd(B=128, h=1024, w=1024, U=8, V=8) == 1    # exactly 2^31

    need = lib.pcnn_neck_bwd_workspace_size(1, 4, 4, 4, 4)
    ok_b = dict(d_s=fake, d_v=fake, keep_score=fake, keep_vertex=fake, z4=fake, z5=fake, b4=fake, b5=fake, B=1, h=4,
                w=4, U=4, V=4, keep_prob=0.5, dz4=fake, dz5=fake, db4=fake, db5=fake, workspace=fake,
                workspace_bytes=need, stream=None)

    def bwd(**kw):
        return lib.pcnn_neck_bwd(*dict(ok_b, **kw).values())

    for name in ("d_s", "d_v", "keep_score", "keep_vertex", "z4", "z5", "b4", "b5", "dz4", "dz5", "db4", "db5",
                 "workspace"):
        assert bwd(**{name: None}) == 1, name
    assert bwd(h=3) == 1 and bwd(w=5) == 1 and bwd(U=6) == 1 and bwd(V=2) == 1
    assert bwd(keep_prob=0.0) == 1 and bwd(keep_prob=2.0) == 1
    assert bwd(dz4=ctypes.c_void_p(0x1004)) == 1
    assert bwd(workspace_bytes=need - 1) == 3   # PCNN_ECAPACITY
    assert lib.pcnn_strerror(1) == b"invalid argument"


def test_python_wrappers_refuse_host_tensors():
    """No CPU path: the wrappers take device tensors only."""
    from posecnn_amd import neck
    c = nc.float_case(nc.SHAPES[3])
    t = {n: torch.from_numpy(v) for n, v in c.items()}
    with pytest.raises(ValueError):
        neck.embedding(t["x4"], t["x5"], t["W4"], t["b4"], t["W5"], t["b5"], 16)
    with pytest.raises(ValueError):
        neck.neck_fwd(t["z4"], t["z5"], t["b4"], t["b5"], 16)
