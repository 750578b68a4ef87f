"""Shapes of tests/test_gpu_roi_pool_paths.py and the RoI-pool backward form
(pcnn_roi_pool_bwd_form, csrc/roi_plan.h) each of them is there to run.  The
GPU module asserts the form before it runs a shape and tests/test_roi_plan.py
asserts the same table on a CPU host, so a retune of the tile threshold that
moves a shape to another kernel fails a test instead of emptying one."""
from collections import namedtuple

GENERIC, ENT_1X4, ENT_2X4 = 0, 1, 2

# B, H, W, C of the feature map; pooled size; RoI rows (R_cap); pixel-index argmax;
# layout (0 NHWC, 1 NCHW); the form the backward must report
Shape = namedtuple("Shape", "B H W C PH PW R px layout form")


def _s(B, H, W, C, PH, PW, R, form, px=0, layout=0):
    return Shape(B, H, W, C, PH, PW, R, px, layout, form)


# c: pooled sizes.  The entry list has room for 49 bins per RoI: 8x8 and 16x8
# are past it, 2x14 is past the 8 bin columns of the column mask.
POOLED = {(1, 1): ENT_1X4, (3, 5): ENT_1X4, (6, 6): ENT_1X4, (7, 7): ENT_1X4, (8, 8): GENERIC, (16, 8): GENERIC,
          (2, 14): GENERIC}

SHAPES = {
    # a: 2 * 23 * 23 * 8 = 8464 >= 8192 workgroups of 2x4 tiles; odd H, W % 4 == 3
    "tile2x4": _s(2, 45, 91, 1024, 7, 7, 150, ENT_2X4),
    "tile2x4_px": _s(2, 45, 91, 1024, 7, 7, 150, ENT_2X4, px=1),
    # b, d: more than 64 rows per image on 1x4 tiles
    "rounds": _s(2, 30, 40, 64, 7, 7, 140, ENT_1X4),
    "any_order": _s(2, 30, 40, 64, 7, 7, 143, ENT_1X4),
    # e: both maps of the pool pair
    "base5": _s(2, 30, 40, 64, 7, 7, 31, ENT_1X4),
    "base4": _s(2, 60, 80, 64, 7, 7, 31, ENT_1X4),
    "base5_px": _s(2, 30, 40, 64, 7, 7, 31, ENT_1X4, px=1),
    "base4_px": _s(2, 60, 80, 64, 7, 7, 31, ENT_1X4, px=1),
    # f: the fallbacks (the form assumes aligned buffers: "misaligned" reports the
    # entry list and runs the generic kernel)
    "rows5": _s(2, 13, 21, 64, 7, 7, 40, ENT_1X4),
    "acc66": _s(2, 13, 21, 66, 7, 7, 40, ENT_1X4),
    "acc3": _s(2, 13, 21, 3, 7, 7, 40, GENERIC),
    "nchw": _s(2, 13, 21, 64, 3, 5, 40, GENERIC, layout=1),
    "misaligned": _s(2, 13, 21, 64, 7, 7, 40, ENT_1X4),
    # g: no rows
    "empty": _s(2, 13, 21, 64, 7, 7, 0, ENT_1X4),
    "empty_generic": _s(2, 13, 21, 3, 7, 7, 0, GENERIC),
}
for (_ph, _pw), _form in POOLED.items():
    SHAPES[f"pooled_{_ph}x{_pw}"] = _s(2, 13, 21, 64, _ph, _pw, 40, _form)


def form_of(lib, s, pool_channel=0):
    return lib.pcnn_roi_pool_bwd_form(s.B, s.H, s.W, s.C, s.layout, pool_channel, s.PH, s.PW, s.R, s.px)
