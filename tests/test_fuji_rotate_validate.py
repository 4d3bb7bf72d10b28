"""rsx_raf_rotate_validate and rsx_raf_rotate_geometry (include/rsx.h section 3y): every row of
the validation order, and which of two faults wins.  The host build of the core header must give
the same verdicts.  No GPU needed: neither function touches the device."""
import ctypes as C

import numpy as np
import pytest

import fuji_rotate_files as F
from rawspeed_amd import abi, capi

OK, INV, UNS = F.OK, F.INVALID_ARG, F.UNSUPPORTED


def _img(dim_x, dim_y, pitch=None, cpp=1, data=None):
    return abi.Image(data, 2 * dim_x if pitch is None else pitch, dim_x, dim_y, cpp, 1)


def _good(W=8, H=6, alt=0, cx=1, cy=2):
    R = F.rotated_size(W, H, alt)[0]
    return abi.fuji_rotate_desc((cx, cy), (W, H), alt), _img(W + cx, H + cy), _img(R, R - 1)


def _both(d, s, t):
    a = capi.fuji_rotate_validate(d, s, t)
    ref = lambda x: None if x is None else C.byref(x)  # noqa: E731
    b = F.host_lib().rsx_fuji_rotate_host_validate(ref(d), ref(s), ref(t))
    assert a == b, "the library and the host build of the core disagree"
    return a


def test_a_good_descriptor_passes_under_both_layouts():
    assert _both(*_good()) == OK
    assert _both(*_good(alt=1)) == OK
    assert capi.fuji_rotate_geometry(_good()[0]) == (OK, 11, 10, 7)
    assert capi.fuji_rotate_geometry(_good(alt=1)[0]) == (OK, 10, 9, 3)


def test_null_arguments():
    d, s, t = _good()
    assert _both(None, s, t) == INV
    assert _both(d, None, t) == INV
    assert _both(d, s, None) == INV
    assert capi.fuji_rotate_geometry(None)[0] == INV


def test_cpp():
    d, s, t = _good()
    s.cpp = 3
    assert _both(d, s, t) == INV
    d, s, t = _good()
    t.cpp = 2
    assert _both(d, s, t) == INV


@pytest.mark.parametrize("field", ["dim_x", "dim_y"])
@pytest.mark.parametrize("which", [1, 2])
@pytest.mark.parametrize("value", [0, -1])
def test_dimensions(field, which, value):
    args = list(_good())
    setattr(args[which], field, value)
    assert _both(*args) == INV


@pytest.mark.parametrize("which", [1, 2])
def test_pitch_too_small_or_odd(which):
    for delta in (-2, 1):
        args = list(_good())
        args[which].pitch_bytes += delta
        assert _both(*args) == INV
    args = list(_good())
    args[which].pitch_bytes += 2
    assert _both(*args) == OK


def test_sizes_and_crops():
    for W, H in [(0, 6), (8, 0), (-1, 6), (8, -2)]:
        d, s, t = _good()
        d.size_x, d.size_y = W, H
        assert _both(d, s, t) == INV
        assert capi.fuji_rotate_geometry(d)[0] == INV
    for cx, cy in [(-1, 0), (0, -1)]:
        d, s, t = _good()
        d.crop_x, d.crop_y = cx, cy
        assert _both(d, s, t) == INV
        assert capi.fuji_rotate_geometry(d)[0] == INV


def test_crop_plus_size_beyond_the_source():
    d, s, t = _good()
    s.dim_x -= 1
    s.pitch_bytes += 2
    assert _both(d, s, t) == INV
    d, s, t = _good()
    s.dim_y -= 1
    assert _both(d, s, t) == INV
    d, s, t = _good()
    d.crop_x = 0x7FFFFFFF  # (no overflow in crop + size)
    assert _both(d, s, t) == INV


def test_rotated_size_limits():
    # R < 2: 1 x 1 under the alt layout has R = 1 (and under the normal one as well)
    for alt in (0, 1):
        d = abi.fuji_rotate_desc((0, 0), (1, 1), alt)
        assert _both(d, _img(1, 1), _img(1, 1)) == INV
        assert capi.fuji_rotate_geometry(d)[0] == INV
    # R = 65535 passes, 65536 does not
    d = abi.fuji_rotate_desc((0, 0), (65533, 4), 0)
    assert capi.fuji_rotate_geometry(d) == (OK, 65535, 65534, 65532)
    d = abi.fuji_rotate_desc((0, 0), (65534, 4), 0)
    assert capi.fuji_rotate_geometry(d)[0] == INV
    assert _both(d, _img(65534, 4), _img(65535, 65534)) == INV
    d = abi.fuji_rotate_desc((0, 0), (2, 65535), 1)
    assert capi.fuji_rotate_geometry(d)[0] == INV


def test_destination_size():
    for dx, dy in [(1, 0), (0, 1), (-1, 0), (0, -1), (1, 1)]:
        d, s, t = _good()
        t.dim_x += dx
        t.dim_y += dy
        t.pitch_bytes = 2 * t.dim_x
        assert _both(d, s, t) == INV


def test_overlapping_images():
    d, s, t = _good()  # source 9 x 8 (pitch 18), destination 11 x 10 (pitch 22)
    buf = np.zeros(18 * 8 + 22 * 10, np.uint8)
    s.data, t.data = buf.ctypes.data, buf.ctypes.data + 18 * 8
    assert _both(d, s, t) == OK  # back to back
    t.data = buf.ctypes.data + 18 * 8 - 2
    assert _both(d, s, t) == INV
    t.data = buf.ctypes.data
    assert _both(d, s, t) == INV
    s.data, t.data = buf.ctypes.data + 22 * 10, buf.ctypes.data  # the other way round
    assert _both(d, s, t) == OK
    s.data -= 2
    assert _both(d, s, t) == INV


def test_layouts_the_reference_does_not_survive():
    d, s, t = _good(W=8, H=7)
    assert _both(d, s, t) == INV  # the reference throws "Trying to write out of bounds"
    assert capi.fuji_rotate_geometry(d)[0] == INV
    d, s, t = _good(W=7, H=6, alt=1)
    assert _both(d, s, t) == UNS  # the reference writes row -1
    assert capi.fuji_rotate_geometry(d)[0] == UNS


def test_precedence():
    # a NULL together with a bad size
    d, s, t = _good()
    d.size_x = 0
    assert _both(d, None, t) == INV
    # odd W alt (UNSUPPORTED) together with a wrong dst size, a bad pitch, a crop past the source,
    # overlapping images: INVALID_ARG comes first every time
    d, s, t = _good(W=7, H=6, alt=1)
    t.dim_y += 1
    assert _both(d, s, t) == INV
    d, s, t = _good(W=7, H=6, alt=1)
    s.pitch_bytes += 1
    assert _both(d, s, t) == INV
    d, s, t = _good(W=7, H=6, alt=1)
    d.crop_x += 1
    assert _both(d, s, t) == INV
    d, s, t = _good(W=7, H=6, alt=1)
    buf = np.zeros(4096, np.uint8)
    s.data = t.data = buf.ctypes.data
    assert _both(d, s, t) == INV
    # ... and UNSUPPORTED only when everything else is in order
    d, s, t = _good(W=7, H=6, alt=1)
    assert _both(d, s, t) == UNS
    # cpp before the dimensions, the dimensions before the pitch
    d, s, t = _good(W=7, H=6, alt=1)
    s.cpp, s.dim_x = 2, 0
    assert _both(d, s, t) == INV
    # the geometry call: a size below 1 before the layout
    d = abi.fuji_rotate_desc((0, 0), (7, 0), 1)
    assert capi.fuji_rotate_geometry(d)[0] == INV
    # R out of range before the layout: 2 x 65535 alt has R = 65536, 65535 x 2 alt has odd W
    d = abi.fuji_rotate_desc((0, 0), (65535, 65535), 1)
    assert capi.fuji_rotate_geometry(d)[0] == INV


def test_model_refusals_agree_with_the_geometry_call():
    for alt in (0, 1):
        for W in range(0, 12):
            for H in range(0, 12):
                d = abi.fuji_rotate_desc((0, 0), (W, H), alt)
                st, dx, dy, pos = capi.fuji_rotate_geometry(d)
                assert st == F.refusal(W, H, alt), (W, H, alt)
                if st == OK:
                    R, p = F.rotated_size(W, H, alt)
                    assert (dx, dy, pos) == (R, R - 1, p)
