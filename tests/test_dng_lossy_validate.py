"""rsx_dng_lossy_validate (include/rsx.h section 4f): every check of the chain that needs no pixel,
over the case table and at the chain's own rules, against the composed model of
tests/dng_lossy_files.py.  No GPU needed: validation touches no device."""
import ctypes as C

import numpy as np
import pytest

import dng_lossy_files as F
import dng_post_files as P
from rawspeed_amd import abi, capi

OK, INVALID_ARG, IO, UNSUPPORTED = F.OK, F.INVALID_ARG, F.IO, F.UNSUPPORTED


def image(c):
    s = c.shape
    return abi.Image(0, 2 * s.dim_x * s.cpp + 6, s.dim_x, s.dim_y, s.cpp, int(s.cfa))


def check_list(r, info):
    assert (r.list_status, r.list_reason, r.n_applied, r.crop()) == \
        (info["list_status"], info["reason"], info["n_applied"], tuple(info["crop"]))


def run(c):
    d, keep = F.desc(c, abi)
    st, r, bad = capi.dng_lossy_validate(d, image(c), c.bad_cap)
    want, info1, info2, fixed = F.validate(c)
    assert st == want, c.name
    if info1 is not None:
        check_list(r.list1, info1)
    if info2 is not None:
        check_list(r.list2, info2)
    else:
        assert r.list2.n_opcodes == 0 and r.list2.n_bad == 0
    assert r.stages == 0 and r.scale.variant == 0 and r.fixed.n_bad == 0
    if want == OK:
        assert bad == fixed, c.name
    return st, r, bad


@pytest.mark.parametrize("name", [c.name for c in F.cases()])
def test_case_table(name):
    st, r, bad = run(F.case(name))
    assert st == OK


def test_nulls_and_f32():
    c = F.case("maptable_sse2_dither")
    d, keep = F.desc(c, abi)
    assert capi.dng_lossy_validate(None, image(c))[0] == INVALID_ARG
    assert capi.dng_lossy_validate(d, None)[0] == INVALID_ARG
    assert capi.lib().rsx_dng_lossy_validate(C.byref(d), C.byref(image(c)), None, None, 4) == INVALID_ARG
    d.stage1.is_f32 = 1
    assert capi.dng_lossy_validate(d, image(c))[0] == INVALID_ARG
    d.stage1.is_f32 = 0
    d.scale.is_f32 = 1
    assert capi.dng_lossy_validate(d, image(c))[0] == INVALID_ARG
    d.scale.is_f32 = 0
    assert capi.dng_lossy_validate(d, image(c))[0] == OK


def test_without_list2_the_scale_descriptor_is_ignored():
    c = F.case("post_rgb")
    d, keep = F.desc(c, abi)
    d.scale.crop_x = -5  # (rsx_scale_validate would refuse it)
    d.opcodes2_bytes = 3  # (opcodes2 NULL)
    st, r, bad = capi.dng_lossy_validate(d, image(c))
    assert st == OK and r.list2.n_opcodes == 0


def test_scale_crop_must_be_what_list1_left():
    c = F.case("trim_scalecol_plain_dither")
    st, r, _ = run(c)
    assert st == OK and r.list1.crop() == (5, 2, 87, 139)
    for crop in ((0, 0, 96, 144), (5, 2, 87, 138), (4, 2, 87, 139)):
        wrong = F.Case("x", c.shape.name, c.list1, c.table, None, c.list2, c.black, c.white,
                       sse2=False, scale_crop=crop)
        assert run(wrong)[0] == INVALID_ARG, crop
    # a list 1 that stops in front of its TrimBounds leaves the image's crop
    t = np.arange(256, dtype=np.uint16)
    stopped = F.Case("x", c.shape.name, P.opcode_list([P.op_bad_constant(1), P.op_trim((2, 5, 141, 92))]),
                     c.table, None, P.opcode_list([P.op_table((0, 0, 144, 96), t)]), 256, 16383)
    st, r, _ = run(stopped)
    assert st == OK and r.list1.n_applied == 0 and r.list1.crop() == (0, 0, 96, 144)
    assert r.list1.list_reason == P.REASON_SETUP_CPP


def test_an_empty_list2_fails_the_file():
    c = F.case("maptable_sse2_dither")
    empty = F.Case("x", c.shape.name, None, c.table, None, b"", 256, 16383)
    assert run(empty)[0] == IO
    # ... unlike list 1, where an entry of 0 bytes is none
    none1 = F.Case("x", c.shape.name, b"", c.table, None, c.list2, 256, 16383)
    assert run(none1)[0] == OK
    # a count of 0 is a list, and an empty one
    zero = F.Case("x", c.shape.name, None, c.table, None, P.opcode_list([]), 256, 16383)
    st, r, _ = run(zero)
    assert st == OK and r.list2.n_opcodes == 0
    short = F.Case("x", c.shape.name, None, c.table, None, b"\0\0", 256, 16383)
    assert run(short)[0] == IO
    cut = F.Case("x", c.shape.name, None, c.table, None, c.list2[:-3], 256, 16383)
    assert run(cut)[0] == IO


def test_a_list1_that_fails_the_file_comes_first():
    c = F.case("maptable_sse2_dither")
    both = F.Case("x", c.shape.name, b"\0\0", c.table, None, b"", 256, 16383, scale_crop=(1, 1, 2, 2))
    assert run(both)[0] == IO


def test_list2_fails_while_it_is_constructed():
    st, r, _ = run(F.case("list2_fails_constructed"))
    assert st == OK
    assert (r.list2.list_status, r.list2.list_reason, r.list2.n_applied) == \
        (INVALID_ARG, P.REASON_ROI, 0)


def test_list2_stops_at_a_setup():
    st, r, _ = run(F.case("list2_stops_at_setup"))
    assert st == OK
    assert (r.list2.list_status, r.list2.list_reason, r.list2.n_opcodes, r.list2.n_applied) == \
        (INVALID_ARG, P.REASON_SETUP_CPP, 3, 1)


def test_list2_rois_are_held_against_list1s_crop():
    c = F.case("trim_scalecol_plain_dither")
    t = np.arange(256, dtype=np.uint16)
    inside = F.Case("x", c.shape.name, c.list1, c.table, None,
                    P.opcode_list([P.op_table((0, 0, 139, 87), t)]), 256, 16383)
    st, r, _ = run(inside)
    assert st == OK and r.list2.list_status == OK and r.list2.crop() == (5, 2, 87, 139)
    outside = F.Case("x", c.shape.name, c.list1, c.table, None,
                     P.opcode_list([P.op_table((0, 0, 140, 87), t)]), 256, 16383)
    st, r, _ = run(outside)
    assert st == OK and (r.list2.list_status, r.list2.list_reason) == (INVALID_ARG, P.REASON_ROI)
    # a TrimBounds of list 2 goes on from list 1's
    trim = F.Case("x", c.shape.name, c.list1, c.table, None,
                  P.opcode_list([P.op_trim((1, 1, 100, 50))]), 256, 16383)
    st, r, _ = run(trim)
    assert st == OK and r.list2.crop() == (6, 3, 49, 99)


def test_a_scale_descriptor_rsx_scale_validate_refuses():
    c = F.case("black_area")
    past = F.Case("x", c.shape.name, None, c.table, None, c.list2, 0, 65535, areas=[(98, 4, False)])
    assert run(past)[0] == INVALID_ARG
    d, keep = F.desc(c, abi)
    d.scale.n_areas = 3  # (areas holds two)
    d.scale.areas = None
    assert capi.dng_lossy_validate(d, image(c))[0] == INVALID_ARG


def test_fix_with_cpp3_and_a_list_of_positions():
    c = F.case("maptable_sse2_dither")
    pts = P.opcode_list([P.op_bad_list([(1, 2)])])
    in2 = F.Case("x", c.shape.name, None, c.table, None, pts, 256, 16383, fix=True)
    assert run(in2)[0] == UNSUPPORTED
    in1 = F.Case("x", c.shape.name, pts, c.table, None, None, fix=True)
    assert run(in1)[0] == UNSUPPORTED
    # without the fix the positions are handed out; a constant refuses such an image itself
    st, r, bad = run(F.Case("x", c.shape.name, None, c.table, None, pts, 256, 16383))
    assert st == OK and bad == [1 << 16 | 2]
    const = F.Case("x", c.shape.name, None, c.table, None, P.opcode_list([P.op_bad_constant(5)]), 256,
                   16383, fix=True)
    st, r, bad = run(const)
    assert st == OK and r.list2.list_reason == P.REASON_SETUP_CPP and bad == []


def test_merged_order_of_the_positions():
    """list 2's FixBadPixelsList entries, then list 1's; inside a list the later opcode in front"""
    c = F.case("const2_fix")
    l1 = P.opcode_list([P.op_bad_list([(1, 1), (2, 2)]), P.op_bad_constant(9), P.op_bad_list([(3, 3)])])
    l2 = P.opcode_list([P.op_bad_list([(4, 4)], [(5, 5, 6, 7)]), P.op_bad_list([(8, 8)])])
    both = F.Case("x", c.shape.name, l1, c.table, None, l2, 256, 14600, fix=True)
    st, r, bad = run(both)
    p = lambda y, x: y << 16 | x  # noqa: E731
    assert st == OK
    assert bad == [p(8, 8), p(4, 4), p(5, 5), p(5, 6), p(3, 3), p(1, 1), p(2, 2)]
    assert (r.list1.n_bad, r.list2.n_bad) == (3, 4)
    # a capacity below their number
    small = F.Case("x", c.shape.name, l1, c.table, None, l2, 256, 14600, fix=True, bad_cap=6)
    st, r, bad = run(small)
    assert st == UNSUPPORTED and (r.list1.n_bad, r.list2.n_bad) == (3, 4)
