"""The RoI-pool backward's choice of kernel (csrc/roi_plan.h, exported as
pcnn_roi_pool_bwd_form) -- CPU only.  0 = generic, 1 = entry list on 1x4
tiles, 2 = entry list on 2x4 tiles, negative = rejected.  The expected forms
follow from the dispatch as it stood before it was factored out (2x4 tiles
unless they give fewer than 8192 workgroups; NHWC, all channels, even C), plus
the list's capacity: 16 RoIs of at most 49 bins per round."""
import pytest

import roi_pool_cases as cases
from roi_pool_cases import ENT_1X4, ENT_2X4, GENERIC


@pytest.fixture(scope="module")
def lib():
    from posecnn_amd import _lib, build
    if build.needs_build():
        build.build()
    return _lib.load()


def form(lib, B, H, W, C, PH=7, PW=7, R=1152, layout=0, pool_channel=0, px=0):
    return lib.pcnn_roi_pool_bwd_form(B, H, W, C, layout, pool_channel, PH, PW, R, px)


def test_step_shapes(lib):
    """The pose step's two maps, in both argmax encodings."""
    for px in (0, 1):
        assert form(lib, 8, 30, 40, 512, px=px) == ENT_1X4  # conv5_3: 8 * 15 * 10 * 4 = 4800 workgroups of 2x4
        assert form(lib, 8, 60, 80, 512, px=px) == ENT_2X4  # conv4_3: 19200


def test_threshold_between_the_tiles(lib):
    """2x4 tiles from 8192 workgroups on: B * ceil(H/2) * ceil(W/4) * ceil(C/128)."""
    assert form(lib, 1, 64, 128, 1024) == ENT_2X4  # 32 * 32 * 8 = 8192
    assert form(lib, 1, 64, 124, 1024) == ENT_1X4  # 32 * 31 * 8 = 7936
    assert form(lib, 1, 63, 125, 898) == ENT_2X4   # ragged edges round up: 32 * 32 * 8


def test_generic_shapes(lib):
    assert form(lib, 8, 60, 80, 512, layout=1) == GENERIC       # NCHW
    assert form(lib, 8, 60, 80, 512, pool_channel=1) == GENERIC
    assert form(lib, 8, 60, 80, 511) == GENERIC                 # odd C: two channels per lane
    assert form(lib, 8, 60, 80, 510) == ENT_2X4
    # offsets past 32 bits: H * W * C >= 2^30 elements, or R * PH * PW * C >= 2^29
    assert form(lib, 1, 1024, 1024, 1024) == GENERIC
    assert form(lib, 8, 60, 80, 512, R=21400) == GENERIC        # 21400 * 49 * 512 >= 2^29
    assert form(lib, 8, 60, 80, 512, R=21399) == ENT_2X4


def test_entry_list_capacity(lib):
    """A round lists 16 RoIs in 16 * 49 entries, and a RoI one pixel wide puts
    its pixel into every bin: pooled sizes above 49 bins run the generic
    kernel; so do those whose row / column masks pass 32 bits."""
    for shape in ((8, 30, 40, 512), (8, 60, 80, 512)):
        ent = form(lib, *shape)
        assert form(lib, *shape, PH=7, PW=7) == ent
        assert form(lib, *shape, PH=6, PW=8) == ent      # 48 bins
        assert form(lib, *shape, PH=49, PW=1) == GENERIC  # 49 bins, but 49 bin rows are past the row mask
        assert form(lib, *shape, PH=5, PW=10) == GENERIC  # 10 * 4 column bits
        assert form(lib, *shape, PH=8, PW=8) == GENERIC   # 64 bins
        assert form(lib, *shape, PH=10, PW=5) == GENERIC  # 50 bins
        assert form(lib, *shape, PH=16, PW=8) == GENERIC
    assert form(lib, 8, 30, 40, 512, PH=24, PW=2) == ENT_1X4  # 48 bins, 24 row bits on 1x4 tiles
    assert form(lib, 8, 60, 80, 512, PH=24, PW=2) == GENERIC  # 48 row bits on 2x4 tiles


def test_pixel_argmax_is_rejected_off_the_entry_list(lib):
    """Only the entry-list kernel reads the uint16 pixel-index argmax."""
    assert form(lib, 8, 60, 80, 511, px=1) < 0            # odd C
    assert form(lib, 8, 60, 80, 512, PH=8, PW=8, px=1) < 0  # past the list's capacity
    assert form(lib, 1, 256, 256, 64, px=1) < 0           # H * W = 0x10000: 0xFFFF marks an empty bin
    assert form(lib, 1, 255, 257, 64, px=1) < 0           # H * W = 0xFFFF
    assert form(lib, 1, 254, 258, 64, px=1) == ENT_2X4    # 0xFFFC pixels


def test_invalid_arguments_are_rejected(lib):
    assert form(lib, 0, 60, 80, 512) < 0
    assert form(lib, 8, 60, 80, 512, PH=0) < 0
    assert form(lib, 8, 60, 80, 512, layout=2) < 0
    assert form(lib, 8, 60, 80, 512, R=-1) < 0
    assert form(lib, 8, 60, 80, 512, R=0) == ENT_2X4
    assert form(lib, 1, 2048, 2048, 512) < 0              # H * W * C >= 2^31


def test_extreme_arguments(lib):
    """The plan's arithmetic holds at the ends of int."""
    big = 2 ** 31 - 1
    assert form(lib, 1, big, 1, 1) == GENERIC
    assert form(lib, 1, 1, big, 1) == GENERIC
    assert form(lib, big, 1, 1, 2) == ENT_2X4
    assert form(lib, 8, 60, 80, 512, R=big) == GENERIC
    assert form(lib, 8, 60, 80, 512, PH=big, PW=big) == GENERIC
    assert form(lib, 1, 1, 1, 2 ** 30, R=big) == GENERIC


@pytest.mark.parametrize("name", sorted(cases.SHAPES))
def test_shapes_of_the_gpu_module(lib, name):
    s = cases.SHAPES[name]
    assert cases.form_of(lib, s) == s.form
