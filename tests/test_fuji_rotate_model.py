"""The model of the SuperCCD rotation (tests/fuji_rotate_files.py, transcribed from
decoders/RafDecoder.cpp:228-270) against hand-worked answers, its own inverse, and the host build
of the core header (librsx_fuji_rotate_host.so).  The reference cannot be run for this path here:
the model, the host build and the hand-worked answers are the yardstick of the device tests.

Two properties of the reference's loop are established here for every W, H <= 40:
  * its "Trying to write out of bounds" fires exactly for the normal layout with odd H, where
    (y = H - 1, x = 0) lands on row R - 1 = dim.y; everywhere else every write is in bounds;
  * with alt_layout and odd W, (y = 0, x = W - 1) lands on row -1, which its signed `h < dim.y`
    does not catch.
Both shapes are refused by the C-ABI (INVALID_ARG like every ThrowRDE, and UNSUPPORTED)."""
import ctypes as C

import numpy as np
import pytest

import fuji_rotate_files as F

N = 40


def test_hand_worked_2x2_normal():
    s = np.array([[11, 12], [21, 22]], np.uint16)  # s[y][x]
    assert F.rotated_size(2, 2, 0) == (3, 1)
    want = [[0, 12, 22], [11, 21, 0]]
    for fn in (F.rotate_literal, F.rotate_scatter, F.rotate_gather):
        assert fn(s, 0, 0, 2, 2, 0).tolist() == want, fn.__name__


def test_hand_worked_2x2_alt():
    s = np.array([[11, 12], [21, 22]], np.uint16)
    assert F.rotated_size(2, 2, 1) == (3, 0)
    want = [[11, 12, 0], [0, 21, 22]]
    for fn in (F.rotate_literal, F.rotate_scatter, F.rotate_gather):
        assert fn(s, 0, 0, 2, 2, 1).tolist() == want, fn.__name__


def test_forward_equals_inverse_and_the_map_is_injective_and_in_bounds():
    ran = 0
    for alt in (0, 1):
        for W in range(1, N + 1):
            for H in range(1, N + 1):
                if F.refusal(W, H, alt) != F.OK:
                    continue
                R = F.rotated_size(W, H, alt)[0]
                y, x = np.mgrid[0:H, 0:W]
                h, w = F.forward(W, H, alt, x, y)
                assert h.min() >= 0 and h.max() <= R - 2, (W, H, alt)
                assert w.min() >= 0 and w.max() <= R - 1, (W, H, alt)
                assert len(set(zip(h.ravel().tolist(), w.ravel().tolist()))) == W * H
                xi, yi = F.inverse(W, alt, h, w)
                assert (xi == x).all() and (yi == y).all(), (W, H, alt)
                src = F.source(W + 3, H + 5, seed=W * 64 + H)
                a = F.rotate_scatter(src, 3, 5, W, H, alt)
                assert np.array_equal(a, F.rotate_gather(src, 3, 5, W, H, alt)), (W, H, alt)
                assert np.count_nonzero(a) == W * H
                ran += 1
    assert ran == N * (N // 2) * 2 - 0  # even H under normal, even W under alt


def test_the_literal_loop_equals_the_vectorised_model():
    for W, H, alt in [(2, 2, 0), (7, 6, 0), (9, 16, 0), (1, 2, 0), (8, 8, 1), (2, 1, 1), (6, 7, 1)]:
        src = F.source(W + 1, H + 2)
        assert np.array_equal(F.rotate_literal(src, 1, 2, W, H, alt),
                              F.rotate_scatter(src, 1, 2, W, H, alt))


def test_the_reference_throws_exactly_for_the_normal_layout_with_odd_height():
    for W in range(1, 13):
        for H in range(1, 13):
            src = F.source(W, H)
            if H % 2:
                with pytest.raises(F.OutOfBounds) as e:
                    F.rotate_literal(src, 0, 0, W, H, 0)
                x, y, h, w = e.value.args[0]
                R = F.rotated_size(W, H, 0)[0]
                assert h == R - 1 and w < R
                if W + H // 2 >= 2:
                    assert F.refusal(W, H, 0) == F.INVALID_ARG
            else:
                F.rotate_literal(src, 0, 0, W, H, 0)
    assert F.forward(5, 7, 0, 0, 6) == (5 - 1 + 3, 3)  # (y = H - 1, x = 0) -> row R - 1 = 7


def test_alt_layout_with_odd_width_reaches_row_minus_one():
    for W in (1, 3, 5, 9, 31):
        for H in (1, 2, 7):
            assert F.forward(W, H, 1, W - 1, 0)[0] == -1, (W, H)
            assert F.refusal(W, H, 1) in (F.UNSUPPORTED, F.INVALID_ARG)
    with pytest.raises(IndexError):
        F.rotate_literal(F.source(3, 4), 0, 0, 3, 4, 1)
    assert F.refusal(3, 4, 1) == F.UNSUPPORTED


def test_host_maps_equal_the_model():
    L = F.host_lib()
    a, b = C.c_int32(), C.c_int32()
    for alt in (0, 1):
        for W, H in [(2, 2), (8, 6), (40, 38), (4352, 1446), (4000, 3000)]:
            for x, y in [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, H // 3)]:
                L.rsx_fuji_rotate_host_forward(W, H, alt, x, y, C.byref(a), C.byref(b))
                assert (a.value, b.value) == F.forward(W, H, alt, x, y)
                h, w = a.value, b.value
                L.rsx_fuji_rotate_host_inverse(W, alt, h, w, C.byref(a), C.byref(b))
                assert (a.value, b.value) == (x, y)
            for h, w in [(0, 0), (0, 5), (7, 0), (3, 1)]:  # (points nothing lands on included)
                L.rsx_fuji_rotate_host_inverse(W, alt, h, w, C.byref(a), C.byref(b))
                assert (a.value, b.value) == F.inverse(W, alt, h, w)


@pytest.mark.parametrize("W,H,alt", F.cases())
def test_host_library_equals_the_model_on_the_device_case_list(W, H, alt):
    want_st = F.refusal(W, H, alt)
    for cx, cy in F.CROPS:
        src = F.source(W + cx + 2, H + cy + 1, seed=W + H)
        for which in ("scatter", "gather"):
            st, rows = F.host_rotate(which, src, cx, cy, W, H, alt)
            assert st == want_st, (which, cx, cy)
            if st == F.OK:
                assert np.array_equal(rows, F.rotate_scatter(src, cx, cy, W, H, alt)), (which, cx, cy)


def test_host_library_camera_sized_frames():
    for W, H, alt in [(4000, 3000, 0), (4352, 1446, 1)]:
        src = F.source(W + 8, H + 4)
        st, rows = F.host_rotate("gather", src, 4, 2, W, H, alt)
        assert st == F.OK
        assert np.array_equal(rows, F.rotate_scatter(src, 4, 2, W, H, alt))
