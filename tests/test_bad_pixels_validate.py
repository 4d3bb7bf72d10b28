"""rsx_bad_pixels_validate (include/rsx.h section 5): every verdict in its order, through the
product library's validate (no GPU needed) and through the host build of the same core, whose
fix must leave a refused image untouched; and the empty case."""
import ctypes as C

import numpy as np
import pytest

import bad_pixels_files as B
from rawspeed_amd import abi, build, capi

OK, INVALID, UNSUPPORTED = abi.RSX_OK, abi.RSX_ERR_INVALID_ARG, abi.RSX_ERR_UNSUPPORTED
W, H = 40, 6


@pytest.fixture(scope="module")
def host():
    lib_path, _ = build.build_bad_pixels_host()
    L = C.CDLL(lib_path)
    L.rsx_bad_pixels_host_validate.argtypes = [C.c_void_p, C.c_void_p]
    L.rsx_bad_pixels_host_fix.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def _both(host, desc, view):
    d = None if desc is None else C.byref(desc)
    v = None if view is None else C.byref(view)
    a = capi.bad_pixels_validate(desc, view)
    b = host.rsx_bad_pixels_host_validate(d, v)
    assert a == b
    return a


def _image(w=W, h=H, cpp=1, pitch=None, bpc=2):
    pitch = pitch if pitch is not None else w * cpp * bpc
    buf = np.full(max(pitch, 1) * max(h, 1) + 64, 0x33, np.uint8)
    return buf, abi.Image(buf.ctypes.data, pitch, w, h, cpp, 1)


def _desc(positions=(B.pos(3, 2),), **kw):
    return abi.bad_pixels_desc(positions, (W, H), **kw)


def test_nulls(host):
    d, keep, _ = _desc()
    _, v = _image()
    assert _both(host, None, v) == INVALID
    assert _both(host, d, None) == INVALID
    d.positions = None  # (a count without a list)
    assert _both(host, d, v) == INVALID


@pytest.mark.parametrize("kw", [dict(cpp=0), dict(w=0), dict(h=0), dict(w=-3), dict(pitch=2 * W - 2),
                                dict(pitch=2 * W + 1)])
def test_image_arguments(host, kw):
    d, keep, _ = _desc()
    _, v = _image(**kw)
    assert _both(host, d, v) == INVALID


def test_f32_pitch_is_in_four_byte_samples(host):
    d, keep, _ = _desc(is_f32=True)
    assert _both(host, d, _image(pitch=4 * W + 2)[1]) == INVALID
    assert _both(host, d, _image(pitch=4 * W - 4)[1]) == INVALID
    assert _both(host, d, _image(pitch=4 * W + 4)[1]) == OK


def test_cpp_above_one_is_unsupported_after_the_argument_checks(host):
    d, keep, _ = _desc()
    assert _both(host, d, _image(cpp=3)[1]) == UNSUPPORTED
    # ... and in front of the map and the positions
    bad, keep2, _ = _desc(positions=(B.pos(W, 0),), map_pitch=48)
    assert _both(host, bad, _image(cpp=3)[1]) == UNSUPPORTED
    # a pitch too small for three components is the earlier verdict
    assert _both(host, d, _image(cpp=3, pitch=2 * W)[1]) == INVALID


def test_dimensions_past_16_bits(host):
    d, keep, _ = abi.bad_pixels_desc((), (65537, 1), want_map=False)
    assert _both(host, d, abi.Image(1, 2 * 65537, 65537, 1, 1, 1)) == UNSUPPORTED


def test_map_pitch(host):
    _, v = _image()
    for pitch in (15, 32, 5):
        d, keep, _ = _desc(map_pitch=pitch)
        assert _both(host, d, v) == INVALID
    d, keep, _ = _desc(want_map=False, map_pitch=0)
    assert _both(host, d, v) == OK
    d, keep, _ = _desc(want_map=False, map_pitch=16)
    assert _both(host, d, v) == OK
    # in front of the positions
    d, keep, _ = _desc(positions=(B.pos(W, 0),), map_pitch=32)
    assert _both(host, d, v) == INVALID
    assert abi.bad_pixels_map_pitch(W) == 16 and abi.bad_pixels_map_pitch(129) == 32


@pytest.mark.parametrize("p", [B.pos(W, 0), B.pos(0, H), B.pos(65535, 65535), B.pos(W - 1, H)])
def test_positions_outside(host, p):
    _, v = _image()
    d, keep, _ = _desc(positions=(B.pos(1, 1), p))
    assert _both(host, d, v) == INVALID


@pytest.mark.parametrize("x,y", [(W, 0), (W + 7, H - 1), (127, 3)])
def test_map_bits_outside(host, x, y):
    _, v = _image()
    m = np.zeros((H, 16), np.uint8)
    m[y, x >> 3] |= 1 << (x & 7)
    d, keep, _ = _desc(positions=(), map_in=m)
    assert _both(host, d, v) == INVALID
    m[:] = 0
    m[H - 1, (W - 1) >> 3] |= 1 << ((W - 1) & 7)
    d, keep, _ = _desc(positions=(), map_in=m)
    assert _both(host, d, v) == OK


def test_a_refused_call_leaves_image_and_map_untouched(host):
    for positions, kw, view_kw in (((B.pos(W, 0),), {}, {}), ((B.pos(3, 2),), dict(map_pitch=32), {}),
                                   ((B.pos(3, 2),), {}, dict(cpp=3))):
        buf, v = _image(**view_kw)
        d, keep, map_out = _desc(positions=positions, **kw)
        r = abi.BadPixelsResult()
        st = host.rsx_bad_pixels_host_fix(C.byref(d), C.byref(v), C.byref(r))
        assert st in (INVALID, UNSUPPORTED)
        assert (buf == 0x33).all() and (map_out == 0xA5).all()
        assert (r.n_bad, r.n_fixed, r.map_made) == (0, 0, 0)


def test_the_empty_case(host):
    buf, v = _image()
    d, keep, map_out = _desc(positions=())
    assert _both(host, d, v) == OK
    r = abi.BadPixelsResult(7, 7, 7, 7)
    assert host.rsx_bad_pixels_host_fix(C.byref(d), C.byref(v), C.byref(r)) == OK
    assert (r.n_bad, r.n_fixed, r.map_made) == (0, 0, 0)
    assert (buf == 0x33).all() and (map_out == 0xA5).all()
    # an empty map handed in IS a map: made, nothing fixed
    d, keep, map_out = _desc(positions=(), map_in=np.zeros((H, 16), np.uint8))
    assert host.rsx_bad_pixels_host_fix(C.byref(d), C.byref(v), C.byref(r)) == OK
    assert (r.n_bad, r.n_fixed, r.map_made) == (0, 0, 1)
    assert (buf == 0x33).all() and (map_out == 0).all()
