"""rsx_scale_validate's refusals in their documented order (include/rsx.h section 6), through the
host build of the core and, where the library is built, through the C-ABI's own export: no GPU
needed, validation touches no device."""
import ctypes as C

import numpy as np
import pytest

from rawspeed_amd import abi, build, capi

OK, INVALID_ARG, UNSUPPORTED = abi.RSX_OK, 1, 7


def _host(desc, img):
    L = C.CDLL(build.build_scale_host()[0])
    L.rsx_scale_host_validate.argtypes = [C.c_void_p, C.c_void_p]
    return L.rsx_scale_host_validate(None if desc is None else C.byref(desc),
                                     None if img is None else C.byref(img))


@pytest.fixture(params=["host", "abi"])
def validate(request):
    return _host if request.param == "host" else capi.scale_validate


def image(w=40, h=8, cpp=1, pitch=None, ss=2):
    return abi.Image(0, w * cpp * ss if pitch is None else pitch, w, h, cpp, 1)


def desc(crop=(0, 0, 40, 8), **kw):
    kw.setdefault("black_level", 10)
    kw.setdefault("white_point", 1000)
    return abi.scale_desc(crop, **kw)


def test_a_plain_call_passes(validate):
    d, keep = desc()
    assert validate(d, image()) == OK
    d, keep = desc(areas=[(0, 2, False), (36, 4, True)])
    assert validate(d, image()) == OK


def test_nulls(validate):
    d, keep = desc()
    assert validate(None, image()) == INVALID_ARG
    assert validate(d, None) == INVALID_ARG
    d.n_areas = 1  # (areas NULL)
    assert validate(d, image()) == INVALID_ARG


def test_bad_image_and_pitch(validate):
    d, keep = desc()
    assert validate(d, image(cpp=0)) == INVALID_ARG
    assert validate(d, image(w=0)) == INVALID_ARG
    assert validate(d, image(pitch=78)) == INVALID_ARG  # below dim_x samples
    assert validate(d, image(pitch=81)) == INVALID_ARG  # no multiple of 2
    f, keep2 = desc(is_f32=True)
    assert validate(f, image(ss=4, pitch=162)) == INVALID_ARG  # no multiple of 4
    assert validate(f, image(ss=4)) == OK


def test_crop_outside_the_image(validate):
    for crop in ((-1, 0, 10, 4), (0, -1, 10, 4), (0, 0, -1, 4), (1, 0, 40, 8), (0, 1, 40, 8),
                 (41, 0, 0, 0)):
        d, keep = desc(crop)
        assert validate(d, image()) == INVALID_ARG, crop
    d, keep = desc((40, 8, 0, 0))
    assert validate(d, image()) == OK


def test_order_pitch_before_crop_before_size(validate):
    d, keep = desc((0, 0, 41, 8))
    assert validate(d, image(pitch=81)) == INVALID_ARG
    big = image(w=65537, h=8)
    d, keep = desc((0, 0, 65538, 8))
    assert validate(d, big) == INVALID_ARG  # the crop is checked in front of the size
    d, keep = desc((0, 0, 65537, 8))
    assert validate(d, big) == UNSUPPORTED
    d, keep = desc((0, 0, 8, 65537))
    assert validate(d, image(w=8, h=65537)) == UNSUPPORTED
    d, keep = desc((0, 0, 8, 65536))
    assert validate(d, image(w=8, h=65536)) == OK
    d, keep = desc((0, 0, 8, 8))
    assert validate(d, image(w=8, cpp=5)) == UNSUPPORTED


def test_f32_refusals(validate):
    d, keep = abi.scale_desc((0, 0, 40, 8), black_level=10, white_point=None, is_f32=True)
    assert validate(d, image(ss=4)) == UNSUPPORTED
    d, keep = desc(is_f32=True, areas=[(0, 2, False)])
    assert validate(d, image(ss=4)) == UNSUPPORTED
    # the size is refused in front of them, the crop in front of the size
    d, keep = abi.scale_desc((0, 0, 41, 8), black_level=10, white_point=None, is_f32=True)
    assert validate(d, image(ss=4)) == INVALID_ARG


def test_area_past_the_image(validate):
    for area in ((7, 2, False), (8, 3, False), (38, 4, True), (0x80000000, 2, True), (0, 0x80000000, False)):
        d, keep = desc(areas=[(0, 2, False), area])
        assert validate(d, image()) == INVALID_ARG, area
    # the size is rounded down to even first; an area that ends on the edge passes
    for area in ((7, 1, False), (6, 3, False), (36, 5, True), (40, 1, True)):
        d, keep = desc(areas=[area])
        assert validate(d, image()) == OK, area
    # the areas are not looked at where calculateBlackAreas does not run
    d, keep = desc(areas=[(7, 2, False)], black_separate=(1, 2, 3, 4))
    assert validate(d, image()) == OK
    d, keep = desc((3, 1, 0, 2), areas=[(7, 2, False)])
    assert validate(d, image()) == OK


def test_what_only_the_image_decides_passes_validation(validate):
    d, keep = abi.scale_desc((0, 0, 40, 8), black_level=2000, white_point=1000)
    assert validate(d, image()) == OK  # (refused by the call, from the levels)
    d, keep = abi.scale_desc((0, 0, 8, 65536), black_level=0, white_point=2, host_sse2=False)
    assert validate(d, image(w=8, h=65536)) == OK  # (the row seed: refused by the call)
