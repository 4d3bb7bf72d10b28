"""rsx_image_hash_validate (include/rsx.h section 4g): every verdict, in the header's order, from
the library and from the host build of the core; and what a plan adds for a job's offsets is
checked where a device is (tests/test_gpu_image_hash.py).  No GPU."""
import ctypes as C

import pytest

import image_hash_files as F
from rawspeed_amd import abi, capi


def _img(dim_x=8, dim_y=4, cpp=1, pitch=None, sb=2):
    return abi.Image(None, dim_x * cpp * sb if pitch is None else pitch, dim_x, dim_y, cpp, 0)


def _both(img, sb):
    a = capi.image_hash_validate(img, sb)
    b = F.host().rsx_image_hash_host_validate(None if img is None else C.byref(img), sb)
    assert a == b
    return a


def test_accepts():
    for sb in (2, 4):
        for cpp in (1, 3):
            assert _both(_img(cpp=cpp, sb=sb), sb) == F.OK
            assert _both(_img(cpp=cpp, sb=sb, pitch=8 * cpp * sb + sb), sb) == F.OK
    assert _both(_img(1, 1), 2) == F.OK
    # the largest row and the most rows
    assert _both(_img((1 << 27) - 1, 1), 2) == F.OK
    assert _both(_img((1 << 26) - 1, 1, sb=4), 4) == F.OK
    assert _both(_img(1, (1 << 24) - 1), 2) == F.OK


def test_null_image():
    assert _both(None, 2) == F.INVALID_ARG
    assert _both(None, 3) == F.INVALID_ARG


@pytest.mark.parametrize("sb", (-2, 0, 1, 3, 8, 16))
def test_sample_bytes(sb):
    assert _both(_img(), sb) == F.INVALID_ARG
    # ... in front of the dimensions' and the limits' verdicts
    assert _both(_img(0, 0, 0), sb) == F.INVALID_ARG
    assert _both(_img(1, 1 << 24), sb) == F.INVALID_ARG


@pytest.mark.parametrize("dims", [(0, 4, 1), (8, 0, 1), (8, 4, 0), (-1, 4, 1), (8, -3, 1),
                                  (8, 4, -1), (-(1 << 31), 4, 1)])
def test_dimensions(dims):
    x, y, c = dims
    assert _both(abi.Image(None, 1 << 20, x, y, c, 0), 2) == F.INVALID_ARG


def test_pitch():
    assert _both(_img(pitch=14), 2) == F.INVALID_ARG      # below row_bytes
    assert _both(_img(pitch=17), 2) == F.INVALID_ARG      # not a multiple of 2
    assert _both(_img(pitch=18), 2) == F.OK
    assert _both(_img(pitch=34, sb=4), 4) == F.INVALID_ARG  # a multiple of 2, not of 4
    assert _both(_img(pitch=36, sb=4), 4) == F.OK
    assert _both(_img(pitch=0), 2) == F.INVALID_ARG
    # the product is taken in 64 bits: no pitch reaches it
    big = (1 << 31) - 1
    assert _both(abi.Image(None, 0xFFFFFFFC, big, 1, big, 0), 4) == F.INVALID_ARG
    # ... in front of the limits' verdict: too many rows AND a short pitch
    assert _both(_img(8, 1 << 24, pitch=14), 2) == F.INVALID_ARG
    assert _both(abi.Image(None, (1 << 28) - 2, 1 << 27, 1, 1, 0), 2) == F.INVALID_ARG


def test_limits():
    assert _both(_img(1 << 27, 1), 2) == F.UNSUPPORTED          # row_bytes = 2^28
    assert _both(_img(1 << 26, 1, sb=4), 4) == F.UNSUPPORTED
    assert _both(_img(1 << 25, 1, cpp=4), 2) == F.UNSUPPORTED
    assert _both(abi.Image(None, 0xFFFFFFFE, (1 << 31) - 1, 1, 1, 0), 2) == F.UNSUPPORTED
    assert _both(_img(1, 1 << 24), 2) == F.UNSUPPORTED          # dim_y = 2^24
    assert _both(_img(1, (1 << 31) - 1), 2) == F.UNSUPPORTED


def test_the_call_refuses_null_arguments_without_a_device():
    r = abi.ImageHashResult()
    img = _img()
    lib = capi.lib()
    assert lib.rsx_image_hash(None, C.byref(img), 2, None, C.byref(r)) == F.INVALID_ARG
    assert lib.rsx_image_hash(None, None, 2, None, C.byref(r)) == F.INVALID_ARG
    plan = C.c_void_p()
    job = abi.image_hash_job(0, 0, 64, 2, 8, 4, 1, 16)
    assert lib.rsx_image_hash_plan_create(None, 1, C.byref(job), C.byref(plan)) == F.INVALID_ARG
