"""Every path of the RoI-pool kernels against the oracle, bit for bit.

tests/test_gpu_ops.py pools 7x7 on shapes that all run the backward's 1x4
tile with at most 64 sorted rows per image.  Here each test names the path it
is for, asserts through pcnn_roi_pool_bwd_form that its shape runs the kernel
form it means to (tests/roi_pool_cases.py), asserts that its inputs have the
property it is named for, and then compares with the oracle.  The kernels and
the oracle sum in the same order, so every comparison is assert_array_equal.
"""
import functools

import numpy as np
import pytest
import torch

import roi_pool_cases as cases
from posecnn_amd import _lib
from posecnn_amd.roi_pooling_layer import roi_pooling_op as rp

pytestmark = pytest.mark.gpu
D = torch.device("cuda")
PLATEAU = 3.5  # above almost every N(0, 1) sample: a bin over two plateau pixels is a first-max tie


def T(a):
    return torch.from_numpy(np.array(a, order="C")).to(D)  # a copy: the shared cases are read-only


def N(t):
    return t.cpu().numpy()


def _rois(rng, counts, H, W, scale_img):
    """Rows as _rois of test_gpu_ops.py (boxes past the map edges, widths
    1..200 px), counts[b] of them in image b, sorted by image."""
    R = int(sum(counts))
    x1 = rng.uniform(-20, W * scale_img - 10, R)
    y1 = rng.uniform(-20, H * scale_img - 10, R)
    w = rng.uniform(1, 200, R)
    h = rng.uniform(1, 200, R)
    b = np.repeat(np.arange(len(counts)), counts)
    cls = rng.integers(0, 8, R)
    return np.stack([b, cls, x1, y1, x1 + w, y1 + h, np.zeros(R)], 1).astype(np.float32)


def _data(rng, s):
    data = rng.normal(size=(s.B, s.H, s.W, s.C)).astype(np.float32)
    data[:, 2:6, 3:9] = PLATEAU
    return data


def _box(rois, scale):
    """Rounded feature-map box of each row (sw, sh, ew, eh), round half away from zero."""
    v = rois[:, 2:6].astype(np.float32) * np.float32(scale)
    return (np.sign(v) * np.floor(np.abs(v) + np.float32(0.5))).astype(np.int64).T


def _arbitrary(rng, oa, n_flat):
    """30 % of the argmax replaced by arbitrary values, as test_roi_pool_bwd_overlap does."""
    bad = oa.copy()
    sel = rng.random(bad.shape) < 0.3
    bad[sel] = rng.integers(-1, n_flat, int(sel.sum()))
    return bad


def _plateau_pixels(s, rois, scale):
    """(R, PH, PW) plateau pixels inside each bin, by the op's own fp32 bin bounds."""
    sw, sh, ew, eh = _box(rois, scale)

    def span(start, end, P, size, p0, p1):
        bin_ = (np.maximum(end - start + 1, 1).astype(np.float32) / np.float32(P))[:, None]
        p = np.arange(P, dtype=np.float32)[None]
        lo = np.clip(np.floor(p * bin_).astype(np.int64) + start[:, None], 0, size)
        hi = np.clip(np.ceil((p + np.float32(1)) * bin_).astype(np.int64) + start[:, None], 0, size)
        return np.clip(np.minimum(hi, p1) - np.maximum(lo, p0), 0, None)

    return span(sh, eh, s.PH, s.H, 2, 6)[:, :, None] * span(sw, ew, s.PW, s.W, 3, 9)[:, None, :]


def _check_inputs(s, rois, scale, ot, oa, od, share=0.05):
    """Some empty bins, some first-max ties on the plateau, a share of non-zero gradients."""
    assert (oa < 0).any() and (oa >= 0).any()
    # a bin over two or more plateau pixels that the plateau value won is a first-max tie
    ties = (ot == PLATEAU) & (_plateau_pixels(s, rois, scale) >= 2)[..., None]
    assert ties.sum() > 50 and (oa[ties] >= 0).all()
    assert (od != 0).mean() > share


def _form(hip, name):
    s = cases.SHAPES[name]
    assert cases.form_of(hip, s) == s.form, name
    return s


def _fwd(data, rois, s, scale, **kw):
    top, arg = rp.roi_pool(T(data), T(rois), s.PH, s.PW, scale, 0, **kw)
    return N(top), N(arg)


def _bwd(data_shape, rois, arg, g, s, scale, **kw):
    like = torch.empty(data_shape, device=D)
    arg = arg if torch.is_tensor(arg) else T(arg)
    return N(rp.roi_pool_grad(like, T(rois), arg, T(g), s.PH, s.PW, scale, 0, **kw))


# ---------------------------------------------------------------- a. the 2x4 tile

SCALE_A = 1.0 / 8
LIVE_A = 73  # device row count: image 0 keeps 73 rows (a second round of 9), image 1 none


@functools.lru_cache(maxsize=None)
def _case_a():
    from oracle import oracle as orc
    s = cases.SHAPES["tile2x4"]
    rng = np.random.default_rng(45)
    data = _data(rng, s)
    rois = _rois(rng, (90, 60), s.H, s.W, 8)
    ot, oa = orc.roi_pool_fwd(data, rois, s.PH, s.PW, SCALE_A)
    g = rng.normal(size=ot.shape).astype(np.float32)
    od = orc.roi_pool_bwd(g, oa, data.shape, rois, s.PH, s.PW, SCALE_A)
    for a in (data, rois, ot, oa, g, od):
        a.setflags(write=False)
    return s, data, rois, ot, oa, g, od


def test_tile_2x4_inputs(hip, orc):
    s, data, rois, ot, oa, g, od = _case_a()
    assert s.H % 2 == 1 and s.W % 4 == 3  # a one-row last tile, a three-column last tile
    assert (np.bincount(rois[:, 0].astype(int)) == (90, 60)).all()  # image 0: a second round of 64
    _check_inputs(s, rois, SCALE_A, ot, oa, od)
    # the ragged last tile row and columns receive gradient
    assert (od[:, s.H - 1] != 0).any() and (od[:, :, s.W - 3:] != 0).any()


def test_tile_2x4_forward(hip, orc):
    s, data, rois, ot, oa, g, od = _case_a()
    _form(hip, "tile2x4")
    top, arg = _fwd(data, rois, s, SCALE_A)
    np.testing.assert_array_equal(top, ot)
    np.testing.assert_array_equal(arg, oa)


def test_tile_2x4_forward_device_count(hip, orc):
    """73 of 150 rows: one row past the first block of 8 x 9 rows of the XCD run mapping."""
    s, data, rois, ot, oa, g, od = _case_a()
    n = torch.tensor([LIVE_A], dtype=torch.int32, device=D)
    top = torch.full(ot.shape, 7.0, device=D)
    arg = torch.full(oa.shape, -7, dtype=torch.int32, device=D)
    rp.roi_pool(T(data), T(rois), s.PH, s.PW, SCALE_A, 0, num_rois=n, out=(top, arg))
    np.testing.assert_array_equal(N(top[:LIVE_A]), ot[:LIVE_A])
    np.testing.assert_array_equal(N(arg[:LIVE_A]), oa[:LIVE_A])
    assert (top[LIVE_A:] == 7.0).all() and (arg[LIVE_A:] == -7).all()


def test_tile_2x4_backward_int32(hip, orc):
    """The int32-argmax 2x4 instantiation, ragged tiles, two rounds of 64 rows."""
    s, data, rois, ot, oa, g, od = _case_a()
    _form(hip, "tile2x4")
    np.testing.assert_array_equal(_bwd(data.shape, rois, oa, g, s, SCALE_A), od)


def test_tile_2x4_backward_device_count(hip, orc):
    """73 live rows, all in image 0: its second round holds 9 rows and image 1 has none."""
    s, data, rois, ot, oa, g, od = _case_a()
    _form(hip, "tile2x4")
    assert (rois[:LIVE_A, 0] == 0).all()
    n = torch.tensor([LIVE_A], dtype=torch.int32, device=D)
    want = orc.roi_pool_bwd(g[:LIVE_A], oa[:LIVE_A], data.shape, rois[:LIVE_A], s.PH, s.PW, SCALE_A)
    assert (want[0] != 0).any() and not want[1].any()
    np.testing.assert_array_equal(_bwd(data.shape, rois, oa, g, s, SCALE_A, num_rois=n), want)


def test_tile_2x4_backward_arbitrary_argmax(hip, orc):
    """The backward follows the reference's membership tests, not the forward's argmax."""
    s, data, rois, ot, oa, g, od = _case_a()
    _form(hip, "tile2x4")
    bad = _arbitrary(np.random.default_rng(46), oa, s.H * s.W * s.C)
    want = orc.roi_pool_bwd(g, bad, data.shape, rois, s.PH, s.PW, SCALE_A)
    assert (want != od).any()
    np.testing.assert_array_equal(_bwd(data.shape, rois, bad, g, s, SCALE_A), want)


def test_tile_2x4_backward_pixel_argmax(hip, orc):
    """The oracle's argmax as uint16 pixel indices (0xFFFF for -1) in an int16 tensor."""
    s, data, rois, ot, oa, g, od = _case_a()
    _form(hip, "tile2x4_px")
    px = np.where(oa < 0, 0xFFFF, oa // s.C).astype(np.uint16)
    assert (px == 0xFFFF).any() and (px != 0xFFFF).any()
    np.testing.assert_array_equal(_bwd(data.shape, rois, T(px.view(np.int16)), g, s, SCALE_A), od)


# ---------------------------------------------------------------- b, d. rows per image, row order

SCALE_B = 1.0 / 16


@functools.lru_cache(maxsize=None)
def _case_b():
    """100 rows in image 0, 40 in image 1; rows 40..69 are jittered copies of
    one box, so the tiles under it list more than 16 consecutive rows."""
    from oracle import oracle as orc
    s = cases.SHAPES["rounds"]
    rng = np.random.default_rng(30)
    data = _data(rng, s)
    rois = _rois(rng, (100, 40), s.H, s.W, 16)
    for k in range(40, 70):
        jx, jy = rng.uniform(-12, 12, 2)
        rois[k, 2:6] = [150 + jx, 100 + jy, 420 + jx, 330 + jy]
    ot, oa = orc.roi_pool_fwd(data, rois, s.PH, s.PW, SCALE_B)
    g = rng.normal(size=ot.shape).astype(np.float32)
    od = orc.roi_pool_bwd(g, oa, data.shape, rois, s.PH, s.PW, SCALE_B)
    for a in (data, rois, ot, oa, g, od):
        a.setflags(write=False)
    return s, data, rois, ot, oa, g, od


def test_rounds_of_64_rows(hip, orc):
    s, data, rois, ot, oa, g, od = _case_b()
    _form(hip, "rounds")
    assert (np.bincount(rois[:, 0].astype(int)) == (100, 40)).all()
    sw, sh, ew, eh = _box(rois[40:70], SCALE_B)
    # the 30 consecutive jittered boxes share map pixels: one tile lists them all
    assert sw.max() + 4 <= ew.min() and sh.max() < eh.min() and sw.max() >= 0 and ew.min() < s.W
    _check_inputs(s, rois, SCALE_B, ot, oa, od)
    top, arg = _fwd(data, rois, s, SCALE_B)
    np.testing.assert_array_equal(top, ot)
    np.testing.assert_array_equal(arg, oa)
    np.testing.assert_array_equal(_bwd(data.shape, rois, oa, g, s, SCALE_B), od)
    bad = _arbitrary(np.random.default_rng(31), oa, s.H * s.W * s.C)
    want = orc.roi_pool_bwd(g, bad, data.shape, rois, s.PH, s.PW, SCALE_B)
    np.testing.assert_array_equal(_bwd(data.shape, rois, bad, g, s, SCALE_B), want)


def test_rows_in_any_order(hip, orc):
    """The rows of the case above shuffled across images, with three rows whose
    batch index is outside [0, B): those pool to 0 / -1 and add no gradient."""
    _, data, rois0, _, _, _, _ = _case_b()
    s = _form(hip, "any_order")
    rng = np.random.default_rng(32)
    rois = np.concatenate([rois0, rois0[[5, 50, 120]]])
    rois[140:, 0] = [-1, s.B, s.B + 5]
    rois = rois[rng.permutation(len(rois))]
    b = rois[:, 0].astype(int)
    ok = (b >= 0) & (b < s.B)
    assert len(rois) == s.R and (~ok).sum() == 3 and set(b[~ok]) == {-1, s.B, s.B + 5}
    r0, r1 = np.flatnonzero(b == 0), np.flatnonzero(b == 1)
    assert len(r0) == 100 and len(r1) == 40 and (np.diff(b[ok]) < 0).sum() > 20  # not sorted
    lo, hi = max(r0[0], r1[0]), min(r0[-1], r1[-1])  # both images' row ranges cover [lo, hi]
    assert hi - lo > 128 and (~ok)[lo:hi].sum() == 3
    ot, oa = orc.roi_pool_fwd(data, rois[ok], s.PH, s.PW, SCALE_B)  # the oracle rejects bad indices
    want_t = np.zeros((s.R,) + ot.shape[1:], np.float32)
    want_a = np.full((s.R,) + oa.shape[1:], -1, np.int32)
    want_t[ok], want_a[ok] = ot, oa
    top, arg = _fwd(data, rois, s, SCALE_B)
    np.testing.assert_array_equal(top, want_t)
    np.testing.assert_array_equal(arg, want_a)
    g = rng.normal(size=want_t.shape).astype(np.float32)
    od = orc.roi_pool_bwd(g[ok], oa, data.shape, rois[ok], s.PH, s.PW, SCALE_B)
    _check_inputs(s, rois[ok], SCALE_B, ot, oa, od)
    np.testing.assert_array_equal(_bwd(data.shape, rois, want_a, g, s, SCALE_B), od)
    # a bad row's gradient must not land anywhere even if its argmax names map elements
    full = want_a.copy()
    full[~ok] = rng.integers(0, s.H * s.W * s.C, full[~ok].shape)
    np.testing.assert_array_equal(_bwd(data.shape, rois, full, g, s, SCALE_B), od)


# ---------------------------------------------------------------- c. pooled sizes

SCALE_C = 1.0 / 4
ONE_PIXEL = (9, 14)  # (h, w) of the one-pixel box, inside image 0


def _rois_c(rng, s):
    """40 rows: 32 in image 0, 8 in image 1.  Row 3 covers the whole map, row 5
    lies past it (empty bins at every pooled size); rows 16..31 (one aligned
    group of 16) are the same one-pixel box, whose pixel lies in every bin, so
    one tile lists 16 * PH * PW entries in one round."""
    rois = _rois(rng, (32, 8), s.H, s.W, 4)
    rois[3, 2:6] = [0, 0, s.W * 4 - 1, s.H * 4 - 1]
    rois[5, 2:6] = [s.W * 4 + 40, s.H * 4 + 30, s.W * 4 + 90, s.H * 4 + 70]
    rois[16:32, 2:6] = [ONE_PIXEL[1] * 4, ONE_PIXEL[0] * 4, ONE_PIXEL[1] * 4, ONE_PIXEL[0] * 4]
    return rois


@pytest.mark.parametrize("PH,PW", sorted(cases.POOLED))
def test_pooled_sizes(hip, orc, PH, PW):
    s = _form(hip, f"pooled_{PH}x{PW}")
    rng = np.random.default_rng(100 * PH + PW)
    data = _data(rng, s)
    rois = _rois_c(rng, s)
    assert len(rois) == s.R
    ot, oa = orc.roi_pool_fwd(data, rois, PH, PW, SCALE_C)
    pix = ONE_PIXEL[0] * s.W + ONE_PIXEL[1]
    # every bin of the 16 one-pixel rows holds exactly that pixel
    np.testing.assert_array_equal(oa[16:32], np.broadcast_to(pix * s.C + np.arange(s.C), oa[16:32].shape))
    sw, sh, ew, eh = _box(rois[3:4], SCALE_C)
    assert sw[0] == 0 and sh[0] == 0 and ew[0] >= s.W - 1 and eh[0] >= s.H - 1
    g = rng.normal(size=ot.shape).astype(np.float32)
    od = orc.roi_pool_bwd(g, oa, data.shape, rois, PH, PW, SCALE_C)
    # 1x1 pooling sends each row's gradient to one pixel per channel: at most R / (B * H * W) = 7 %
    _check_inputs(s, rois, SCALE_C, ot, oa, od, share=0.02)
    top, arg = _fwd(data, rois, s, SCALE_C)
    np.testing.assert_array_equal(top, ot)
    np.testing.assert_array_equal(arg, oa)
    np.testing.assert_array_equal(_bwd(data.shape, rois, oa, g, s, SCALE_C), od)
    bad = _arbitrary(rng, oa, s.H * s.W * s.C)
    bad[16:32] = oa[16:32]  # keep the full entry list matched
    want = orc.roi_pool_bwd(g, bad, data.shape, rois, PH, PW, SCALE_C)
    np.testing.assert_array_equal(_bwd(data.shape, rois, bad, g, s, SCALE_C), want)


# ---------------------------------------------------------------- e. batch_base

def test_batch_base(hip, orc):
    """Rows carry the global image index b + 5 and the call passes batch_base 5:
    equal to batch_base 0 on local indices and to the oracle; a neighbouring
    rank's row (global index 4) pools to 0 / -1 and adds no gradient."""
    s5, s4 = _form(hip, "base5"), _form(hip, "base4")
    _form(hip, "base5_px"), _form(hip, "base4_px")
    rng = np.random.default_rng(5)
    d5, d4 = _data(rng, s5), _data(rng, s4)
    local = _rois(rng, (17, 14), 480, 640, 1)
    local[11, 0] = -1  # the neighbour's row
    local[2, 2:6], local[20, 2:6] = [20, 10, 180, 120], [30, 20, 150, 110]  # over the plateau of both maps
    glob = local.copy()
    glob[:, 0] += 5
    assert len(local) == s5.R and glob[11, 0] == 4 and (np.delete(glob[:, 0], 11) >= 5).all()
    ok = local[:, 0] >= 0
    R, g = s5.R, rng.normal(size=(s5.R, 7, 7, s5.C)).astype(np.float32)
    want = {}
    for key, d, s, sc in (("5", d5, s5, 1.0 / 16), ("4", d4, s4, 1.0 / 8)):
        ot, oa = orc.roi_pool_fwd(d, local[ok], 7, 7, sc)
        t, a = np.zeros((R,) + ot.shape[1:], np.float32), np.full((R,) + oa.shape[1:], -1, np.int32)
        t[ok], a[ok] = ot, oa
        od = orc.roi_pool_bwd(g[ok], oa, d.shape, local[ok], 7, 7, sc)
        _check_inputs(s, local[ok], sc, ot, oa, od)
        want[key] = (t, a, od)
    for rois, base in ((glob, 5), (local, 0)):
        for key, d, s, sc in (("5", d5, s5, 1.0 / 16), ("4", d4, s4, 1.0 / 8)):
            t, a, od = want[key]
            top, arg = _fwd(d, rois, s, sc, batch_base=base)
            np.testing.assert_array_equal(top, t)
            np.testing.assert_array_equal(arg, a)
            np.testing.assert_array_equal(_bwd(d.shape, rois, a, g, s, sc, batch_base=base), od)
        for px in (False, True):
            top, a5, a4 = rp.roi_pool_pair(T(d5), 1.0 / 16, T(d4), 1.0 / 8, T(rois), 7, 7, batch_base=base,
                                           pixel_argmax=px)
            np.testing.assert_array_equal(N(top), want["5"][0] + want["4"][0])
            for key, arg, d, s, sc in (("5", a5, d5, s5, 1.0 / 16), ("4", a4, d4, s4, 1.0 / 8)):
                t, a, od = want[key]
                if px:
                    assert arg.dtype == torch.int16
                    np.testing.assert_array_equal(N(arg).view(np.uint16), np.where(a < 0, 0xFFFF, a // s.C))
                else:
                    np.testing.assert_array_equal(N(arg), a)
                np.testing.assert_array_equal(_bwd(d.shape, rois, arg, g, s, sc, batch_base=base), od)


# ---------------------------------------------------------------- f. fallbacks

@functools.lru_cache(maxsize=None)
def _case_f(C, PH=7, PW=7):
    from oracle import oracle as orc
    s = cases.SHAPES["rows5"]._replace(C=C, PH=PH, PW=PW)
    rng = np.random.default_rng(600 + C)
    data = _data(rng, s)
    rois = _rois(rng, (23, 17), s.H, s.W, 4)
    ot, oa = orc.roi_pool_fwd(data, rois, PH, PW, SCALE_C)
    g = rng.normal(size=ot.shape).astype(np.float32)
    od = orc.roi_pool_bwd(g, oa, data.shape, rois, PH, PW, SCALE_C)
    _check_inputs(s, rois, SCALE_C, ot, oa, od)
    for a in (data, rois, ot, oa, g, od):
        a.setflags(write=False)
    return data, rois, ot, oa, g, od


def test_five_column_rows(hip, orc):
    """[b, x1, y1, x2, y2] rows on the NHWC vector forward and the entry-list backward."""
    s = _form(hip, "rows5")
    data, rois, ot, oa, g, od = _case_f(s.C)
    rois5 = np.ascontiguousarray(rois[:, [0, 2, 3, 4, 5]])
    assert s.C % 4 == 0 and rois5.shape == (s.R, 5)
    top, arg = _fwd(data, rois5, s, SCALE_C)
    np.testing.assert_array_equal(top, ot)
    np.testing.assert_array_equal(arg, oa)
    np.testing.assert_array_equal(_bwd(data.shape, rois5, oa, g, s, SCALE_C), od)


@pytest.mark.parametrize("name", ["acc66", "acc3"])
def test_generic_forward_accumulate(hip, orc, name):
    """C % 4 != 0: the generic forward; accumulate adds the pooled value to top in one fp32 add."""
    s = _form(hip, name)
    data, rois, ot, oa, g, od = _case_f(s.C)
    assert s.C % 4 != 0
    base = np.random.default_rng(66).normal(size=ot.shape).astype(np.float32)
    top, arg = T(base), torch.full(oa.shape, -7, dtype=torch.int32, device=D)
    rp.roi_pool(T(data), T(rois), s.PH, s.PW, SCALE_C, 0, out=(top, arg), accumulate=True)
    np.testing.assert_array_equal(N(top), base + ot)
    np.testing.assert_array_equal(N(arg), oa)
    np.testing.assert_array_equal(_bwd(data.shape, rois, oa, g, s, SCALE_C), od)


def test_nchw_layout(hip, orc):
    """layout 1 with 7-column rows at a pooled size other than 7x7: data (B, C, H, W),
    outputs (R, C, PH, PW), argmax (c * H + h) * W + w."""
    s = _form(hip, "nchw")
    data, rois, ot, oa, g, od = _case_f(s.C, s.PH, s.PW)
    assert (s.PH, s.PW) != (7, 7) and rois.shape[1] == 7
    c = np.arange(s.C)
    want_a = np.where(oa < 0, -1, c * (s.H * s.W) + oa // s.C).astype(np.int32)
    assert (oa[oa >= 0] % s.C == np.broadcast_to(c, oa.shape)[oa >= 0]).all()
    nchw = T(data.transpose(0, 3, 1, 2))
    top, arg = rp.roi_pool(nchw, T(rois), s.PH, s.PW, SCALE_C, 0, layout=1)
    assert tuple(top.shape) == (s.R, s.C, s.PH, s.PW)
    np.testing.assert_array_equal(N(top), ot.transpose(0, 3, 1, 2))
    np.testing.assert_array_equal(N(arg), want_a.transpose(0, 3, 1, 2))
    dd = rp.roi_pool_grad(nchw, T(rois), arg, T(g.transpose(0, 3, 1, 2)), s.PH, s.PW, SCALE_C, 0, layout=1)
    np.testing.assert_array_equal(N(dd), od.transpose(0, 3, 1, 2))


def _off4(a, dtype=torch.float32):
    """`a` as a contiguous view 4 bytes into a larger buffer: no longer 8- or 16-byte aligned."""
    buf = torch.empty(a.size + 1, dtype=dtype, device=D)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:].view(a.shape)
    v.copy_(T(a))
    assert v.is_contiguous() and v.data_ptr() % 8 == 4
    return v


@pytest.mark.parametrize("which", ["data", "top", "argmax", "all"])
def test_misaligned_forward(hip, orc, which):
    """Each pointer the 16-byte forward checks, misaligned alone and together."""
    s = _form(hip, "misaligned")
    data, rois, ot, oa, g, od = _case_f(s.C)
    mis = lambda k: which in (k, "all")
    d = _off4(data) if mis("data") else T(data)
    top = _off4(np.full(ot.shape, 7.0, np.float32)) if mis("top") else torch.full(ot.shape, 7.0, device=D)
    arg = (_off4(np.full(oa.shape, -7, np.int32), torch.int32) if mis("argmax")
           else torch.full(oa.shape, -7, dtype=torch.int32, device=D))
    rp.roi_pool(d, T(rois), s.PH, s.PW, SCALE_C, 0, out=(top, arg))
    np.testing.assert_array_equal(N(top), ot)
    np.testing.assert_array_equal(N(arg), oa)


@pytest.mark.parametrize("which", ["grad", "argmax", "bottom", "all"])
def test_misaligned_backward(hip, orc, which):
    """Each pointer the entry-list backward checks, misaligned alone and together:
    the shape reports the entry list, the call takes the generic kernel."""
    s = _form(hip, "misaligned")
    data, rois, ot, oa, g, od = _case_f(s.C)
    mis = lambda k: which in (k, "all")
    gt = _off4(g) if mis("grad") else T(g)
    arg = _off4(oa, torch.int32) if mis("argmax") else T(oa)
    out = (_off4(np.full(data.shape, 7.0, np.float32)) if mis("bottom") else torch.full(data.shape, 7.0, device=D))
    dd = rp.roi_pool_grad(torch.empty(data.shape, device=D), T(rois), arg, gt, s.PH, s.PW, SCALE_C, 0, out=out)
    assert dd.data_ptr() == out.data_ptr()
    np.testing.assert_array_equal(N(dd), od)


# ---------------------------------------------------------------- g. no rows

def _prefilled(shape, dtype=torch.float32, value=7):
    return torch.full(shape, value, dtype=dtype, device=D)


def _zero_bits(t):
    return bool((t.view(torch.int32) == 0).all())


@pytest.mark.parametrize("name", ["empty", "empty_generic"])
def test_no_rows_device_count(hip, orc, name):
    """A device row count of 0 over a non-empty buffer."""
    s = _form(hip, name)
    rng = np.random.default_rng(70)
    data = _data(rng, s)
    rois = _rois(rng, (12, 8), s.H, s.W, 4)
    n = torch.zeros(1, dtype=torch.int32, device=D)
    shape = (20, s.PH, s.PW, s.C)
    top, arg = _prefilled(shape), _prefilled(shape, torch.int32, -7)
    rp.roi_pool(T(data), T(rois), s.PH, s.PW, SCALE_C, 0, num_rois=n, out=(top, arg))
    assert (top == 7).all() and (arg == -7).all()
    if s.C % 4 == 0:
        for dt in (torch.int32, torch.int16):
            top, a, b = _prefilled(shape), _prefilled(shape, dt, -7), _prefilled(shape, dt, -7)
            rp.roi_pool_pair(T(data), SCALE_C, T(data), SCALE_C, T(rois), s.PH, s.PW, num_rois=n, out=(top, a, b))
            assert (top == 7).all() and (a == -7).all() and (b == -7).all()
    g = rng.normal(size=shape).astype(np.float32)
    arg = rng.integers(0, s.H * s.W * s.C, shape).astype(np.int32)
    dd = rp.roi_pool_grad(T(data), T(rois), T(arg), T(g), s.PH, s.PW, SCALE_C, 0, num_rois=n,
                          out=_prefilled(data.shape))
    assert _zero_bits(dd)


@pytest.mark.parametrize("name", ["empty", "empty_generic"])
def test_no_rows_capacity_zero(hip, orc, name):
    """R_cap = 0 at the library call (buffers non-empty, so every pointer is real)
    and through the op layer with zero-row tensors."""
    s = _form(hip, name)
    rng = np.random.default_rng(71)
    data, rois = T(_data(rng, s)), T(_rois(rng, (12, 8), s.H, s.W, 4))
    shape = (20, s.PH, s.PW, s.C)
    top, arg = _prefilled(shape), _prefilled(shape, torch.int32, -7)
    st = _lib.stream_ptr()
    for fn in (hip.pcnn_roi_pool_fwd, hip.pcnn_roi_pool_fwd_accumulate):
        rc = fn(_lib.ptr(data), s.B, s.H, s.W, s.C, 0, _lib.ptr(rois), 0, 7, 0, None, SCALE_C, s.PH, s.PW, 0,
                _lib.ptr(top), _lib.ptr(arg), st)
        assert rc == 0
    assert (top == 7).all() and (arg == -7).all()
    g = T(rng.normal(size=shape).astype(np.float32))
    a = T(rng.integers(0, s.H * s.W * s.C, shape).astype(np.int32))
    dd = _prefilled(tuple(data.shape))
    ws = _lib.workspace(hip.pcnn_roi_pool_bwd_workspace_size(s.B, 0), D, "roi_bwd")
    rc = hip.pcnn_roi_pool_bwd(_lib.ptr(g), _lib.ptr(a), s.B, s.H, s.W, s.C, 0, _lib.ptr(rois), 0, 7, 0, None, SCALE_C,
                               s.PH, s.PW, 0, _lib.ptr(dd), _lib.ptr(ws), ws.numel(), st)
    assert rc == 0 and _zero_bits(dd)
    # the op layer: zero-row tensors (which have no device pointer)
    none = torch.empty((0, 7), device=D)
    top0, arg0 = rp.roi_pool(data, none, s.PH, s.PW, SCALE_C, 0)
    assert tuple(top0.shape) == (0, s.PH, s.PW, s.C) and arg0.dtype == torch.int32
    rp.roi_pool(data, none, s.PH, s.PW, SCALE_C, 0, out=(top, arg))
    assert (top == 7).all() and (arg == -7).all()
    for dt in (torch.int32, torch.int16) if s.C % 2 == 0 else (torch.int32,):
        dd = rp.roi_pool_grad(data, none, torch.empty((0, s.PH, s.PW, s.C), dtype=dt, device=D),
                              torch.empty((0, s.PH, s.PW, s.C), device=D), s.PH, s.PW, SCALE_C, 0,
                              out=_prefilled(tuple(data.shape)))
        assert _zero_bits(dd)
    if s.C % 4 == 0:
        t, a5, a4 = rp.roi_pool_pair(data, SCALE_C, data, SCALE_C, none, s.PH, s.PW)
        assert t.numel() == 0 and a5.numel() == 0 and a4.numel() == 0
