"""rsx_dng_post_validate (include/rsx.h section 4d): every refusal, in the header's order, through
the core library's entry point (no device) and through the host build of the same core, where
"the image is untouched" is checked on every status but RSX_OK."""
import ctypes as C
import struct

import numpy as np
import pytest

import dng_post_files as K
from oracle_lib import HostImage
from rawspeed_amd import abi, build, capi
from test_dng_post_model import host_apply

OK, INVALID, IO, UNSUPPORTED = abi.RSX_OK, K.INVALID_ARG, K.IO, K.UNSUPPORTED
T256 = list(range(0, 65536, 256))
FULL = (0, 0, 20, 70)


@pytest.fixture(scope="module")
def host():
    lib_path, _ = build.build_dng_post_host()
    L = C.CDLL(lib_path)
    for f in (L.rsx_dng_post_host_apply, L.rsx_dng_post_host_validate):
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    return L


def _view(w=70, h=20, cpp=1, pitch=None, bpc=2):
    return HostImage(w, h, cpp=cpp, pitch=pitch, bpc=bpc)


def _validate(opcodes=None, table=None, crop=(0, 0, 70, 20), img=None, is_f32=False, bad_cap=1 << 16, **kw):
    img = img or _view(bpc=4 if is_f32 else 2)
    d, keep = abi.dng_post_desc(opcodes, table, crop, is_f32, **kw)
    return capi.dng_post_validate(d, img.view(), bad_cap)


def test_arguments_in_header_order():
    img = _view()
    d, keep = abi.dng_post_desc(None, None, (0, 0, 70, 20))
    assert capi.dng_post_validate(None, img.view())[0] == INVALID
    assert capi.dng_post_validate(d, None)[0] == INVALID
    for cpp in (0, 5):
        v = img.view()
        v.cpp = cpp
        assert capi.dng_post_validate(d, v)[0] == INVALID
    for dims in ((0, 20), (70, 0), (-1, 20)):
        v = img.view()
        v.dim_x, v.dim_y = dims
        assert capi.dng_post_validate(d, v)[0] == INVALID
    for pitch in (138, 141):  # (short; not a multiple of the sample size)
        v = img.view()
        v.pitch_bytes = pitch
        assert capi.dng_post_validate(d, v)[0] == INVALID
    for crop in ((0, 0, 0, 20), (0, 0, 70, 0), (-1, 0, 70, 20), (1, 0, 70, 20), (0, 1, 70, 20), (0, 0, 71, 20)):
        assert _validate(crop=crop)[0] == INVALID, crop
    assert _validate(opcodes_bytes=8)[0] == INVALID      # (NULL list with a size)
    assert _validate(table_count=3)[0] == INVALID        # (NULL table with a count)
    assert _validate(table=[1] * 65536, table_count=65537)[0] == INVALID
    assert _validate(table=[1] * 65536)[0] == OK


def test_unsupported_before_the_list_is_read():
    truncated = K.opcode_list([K.op_table(FULL, T256)])[:-1]
    # a table on an F32 image, whatever the list says
    assert _validate(truncated, [1, 2], is_f32=True)[0] == UNSUPPORTED
    assert _validate(truncated, None, is_f32=True)[0] == IO
    # the bound the seeds' high half needs: dim_x + 13 dim_y < 2^20
    v = _view().view()
    v.dim_x, v.dim_y, v.pitch_bytes = 65536, 75620, 2 * 65536
    d, keep = abi.dng_post_desc(None, None, (0, 0, 70, 20))
    assert capi.dng_post_validate(d, v)[0] == UNSUPPORTED
    v.dim_y = 75610
    assert capi.dng_post_validate(d, v)[0] == OK


def _list_cases():
    """(name, list, status, reason, n_applied)"""
    L, R = K.opcode_list, K
    ok_table = K.op_table(FULL, T256)
    pix = lambda code, body: K.raw(code, struct.pack(">8I", 0, 0, 20, 70, 0, 1, 1, 1) + body)  # noqa: E731
    return [
        # IOException: the file fails
        ("no_count", b"\0\0\0", IO, 0, 0),
        ("count_past_the_list", L([ok_table], count=2), IO, 0, 0),
        ("header_cut", struct.pack(">I", 1) + b"\0" * 10, IO, 0, 0),
        ("second_header_cut", L([ok_table], count=2) + b"\0" * 15, IO, 0, 0),
        ("size_past_the_list", L([K.raw(7, b"", size=9)]), IO, 0, 0),
        ("roi_cut", L([K.raw(6, b"\0" * 15)]), IO, 0, 0),
        ("planes_cut", L([K.raw(7, struct.pack(">5I", 0, 0, 20, 70, 0))]), IO, 0, 0),
        ("pitch_cut", L([K.raw(7, struct.pack(">7I", 0, 0, 20, 70, 0, 1, 1))]), IO, 0, 0),
        ("table_count_cut", L([pix(7, b"")]), IO, 0, 0),
        ("table_values_cut", L([pix(7, struct.pack(">IH", 2, 5))]), IO, 0, 0),
        ("poly_check", L([pix(8, struct.pack(">Id", 1, 0.5))]), IO, 0, 0),
        ("poly_check_comes_before_the_degree", L([pix(8, struct.pack(">I", 11) + b"\0" * 80)]), IO, 0, 0),
        ("delta_check", L([pix(10, struct.pack(">I", 20) + b"\0" * 79)]), IO, 0, 0),
        ("delta_check_comes_before_the_count", L([pix(10, struct.pack(">I", 21) + b"\0" * 80)]), IO, 0, 0),
        ("bad_constant_cut", L([K.raw(4, b"\0" * 7)]), IO, 0, 0),
        ("bad_list_points_cut", L([K.op_bad_list([(1, 1)], n_points=2)]), IO, 0, 0),
        ("bad_list_rects_cut", L([K.op_bad_list([], [(0, 0, 1, 1)], n_rects=2)]), IO, 0, 0),
        ("bad_list_count_overflow", L([K.op_bad_list(n_points=0x20000000)]), IO, 0, 0),
        ("io_behind_a_refusal_still_fails", L([K.raw(14), ok_table], count=3), IO, 0, 0),
        # RawDecoderException while the list is constructed: nothing applied
        ("roi_bottom", L([ok_table, K.op_table((0, 0, 21, 70), T256)]), OK, R.REASON_ROI, 0),
        ("roi_right", L([K.op_table((0, 0, 20, 71), T256)]), OK, R.REASON_ROI, 0),
        ("roi_reversed", L([K.op_table((5, 0, 4, 70), T256)]), OK, R.REASON_ROI, 0),
        ("roi_negative", L([K.op_trim((0xFFFFFFFF, 0, 20, 70))]), OK, R.REASON_ROI, 0),
        ("roi_refusal_needs_no_more_bytes", L([K.raw(7, struct.pack(">4I", 0, 0, 21, 70))]), OK, R.REASON_ROI, 0),
        ("planes_zero", L([K.op_table(FULL, T256, planes=(0, 0))]), OK, R.REASON_PLANES, 0),
        ("planes_past_cpp", L([K.op_table(FULL, T256, planes=(1, 1))]), OK, R.REASON_PLANES, 0),
        ("pitch_zero", L([K.op_table(FULL, T256, pitch=(0, 1))]), OK, R.REASON_PITCH, 0),
        ("pitch_above_roi", L([K.op_table((0, 0, 3, 70), T256, pitch=(4, 1))]), OK, R.REASON_PITCH, 0),
        ("pitch_on_empty_roi", L([K.op_table((3, 0, 3, 70), T256)]), OK, R.REASON_PITCH, 0),
        ("table_size_zero", L([pix(7, struct.pack(">I", 0))]), OK, R.REASON_TABLE_SIZE, 0),
        ("table_size_above", L([pix(7, struct.pack(">I", 65537))]), OK, R.REASON_TABLE_SIZE, 0),
        ("poly_degree", L([K.op_poly(FULL, [0.0] * 10)]), OK, R.REASON_POLY_DEGREE, 0),
        ("delta_count", L([K.op_delta(11, FULL, [0.0] * 69)]), OK, R.REASON_DELTA_COUNT, 0),
        ("delta_count_pitch", L([K.op_delta(11, FULL, [0.0] * 35, pitch=(1, 3))]), OK, R.REASON_DELTA_COUNT, 0),
        ("delta_inf", L([K.op_delta(12, FULL, [1.0] * 19 + [float("inf")])]), OK, R.REASON_DELTA_NOT_FINITE, 0),
        ("bad_point", L([K.op_bad_list([(0, 70)])]), OK, R.REASON_BAD_POINT, 0),
        ("bad_rect", L([K.op_bad_list([], [(0, 0, 21, 1)])]), OK, R.REASON_ROI, 0),
        ("code_0", L([K.raw(0)]), OK, R.REASON_UNKNOWN_OPCODE, 0),
        ("code_14", L([ok_table, K.raw(14)]), OK, R.REASON_UNKNOWN_OPCODE, 0),
        ("warp_required", L([K.raw(1)]), OK, R.REASON_UNSUPPORTED_OPCODE, 0),
        ("gainmap_required", L([K.raw(9, b"\0" * 4)]), OK, R.REASON_UNSUPPORTED_OPCODE, 0),
        ("gainmap_optional_with_bytes", L([K.raw(9, b"\0" * 4, flags=1)]), OK, R.REASON_INCONSISTENT_LENGTH, 0),
        ("bytes_left", L([K.raw(6, struct.pack(">5I", 0, 0, 20, 70, 0))]), OK, R.REASON_INCONSISTENT_LENGTH, 0),
        # ... from setup() or apply(): what stands in front stays applied
        ("offset_range", L([ok_table, K.op_delta(10, FULL, [0.0] * 19 + [-1.5])]), OK, R.REASON_SETUP_DELTA_RANGE, 1),
        ("scale_range", L([ok_table, ok_table, K.op_delta(13, FULL, [0.0] * 69 + [32.01])]), OK,
         R.REASON_SETUP_DELTA_RANGE, 2),
        ("trim_empty", L([ok_table, K.op_trim((4, 4, 4, 9)), K.op_bad_constant(1)]), OK, R.REASON_TRIM_EMPTY, 1),
        # fine
        ("optional_empty_opcodes", L([K.raw(c, flags=1) for c in (1, 2, 3, 9)] + [ok_table]), OK, 0, 5),
        ("whole_roi_trim", L([K.op_trim(FULL), ok_table]), OK, 0, 2),
    ]


@pytest.mark.parametrize("case", _list_cases(), ids=lambda c: c[0])
def test_list_verdicts(host, case):
    name, opcodes, status, reason, n_applied = case
    rng = np.random.default_rng(len(name))
    st, r, bad = _validate(opcodes, T256)
    assert st == status
    if st == OK:
        assert (r.list_reason, r.n_applied) == (reason, n_applied)
        assert r.list_status == (INVALID if reason else OK)
    # the model agrees, and the host core leaves a failed file's image alone (host_apply checks)
    img = rng.integers(0, 65536, size=(20, 70)).astype(np.uint16)
    want = K.apply(img, 1, (0, 0, 70, 20), opcodes, T256)
    assert want[0] == status
    got = host_apply(host, img, 1, (0, 0, 70, 20), opcodes, T256)
    assert got[0] == status and got[1].tobytes() == want[1].tobytes()
    if status == OK:
        assert (got[2].list_reason, got[2].n_applied) == (want[2]["reason"], want[2]["n_applied"]) == (reason, n_applied)
    else:
        assert np.array_equal(got[1], img)


def test_setup_refusals_that_depend_on_the_image(host):
    ok_table = K.op_table((0, 0, 9, 14), T256)
    delta = K.op_delta(10, (0, 0, 9, 14), [0.25] * 9)
    # F32: a table or FixBadPixelsConstant stops the list, offsets beyond the uint16 limits do not
    for ops, reason, n in (([delta, ok_table], K.REASON_SETUP_NOT_U16, 1),
                           ([K.op_bad_constant(1), delta], K.REASON_SETUP_NOT_U16, 0),
                           ([K.op_delta(10, (0, 0, 9, 14), [7.0] * 9), delta], 0, 2)):
        st, r, _ = _validate(K.opcode_list(ops), None, (0, 0, 14, 9), _view(14, 9, bpc=4), True)
        assert (st, r.list_reason, r.n_applied) == (OK, reason, n)
    # cpp 3: FixBadPixelsConstant
    st, r, _ = _validate(K.opcode_list([K.op_table((0, 0, 9, 14), T256, planes=(2, 1)), K.op_bad_constant(1)]),
                         None, (0, 0, 14, 9), _view(14, 9, cpp=3))
    assert (st, r.list_reason, r.n_applied) == (OK, K.REASON_SETUP_CPP, 1)


def test_caps():
    ok_table = K.op_table(FULL, T256)
    offs = K.op_delta(10, FULL, [0.0] * 20)
    assert _validate(K.opcode_list([offs] * 16))[0] == OK
    assert _validate(K.opcode_list([offs] * 17))[0] == UNSUPPORTED
    # only the applied part counts: the seventeenth stands behind a setup refusal
    st, r, _ = _validate(K.opcode_list([offs] * 16 + [K.op_delta(10, FULL, [2.0] * 20), offs]))
    assert (st, r.n_applied, r.list_reason) == (OK, 16, K.REASON_SETUP_DELTA_RANGE)
    assert _validate(K.opcode_list([ok_table] * 16 + [K.raw(14)]))[0] == OK       # (a refused list holds no table)
    assert _validate(K.opcode_list([ok_table] * 17 + [K.raw(14)]))[0] == UNSUPPORTED


def test_crop_and_host_side_positions():
    ops = [K.op_bad_list([(1, 2)]), K.op_trim((2, 4, 12, 44)), K.op_bad_constant(7),
           K.op_bad_list([(3, 3)], [(0, 0, 1, 2)]), K.op_trim((1, 1, 9, 30))]
    st, r, bad = _validate(K.opcode_list(ops), None, crop=(3, 1, 60, 18))
    assert (st, r.list_status, r.n_opcodes, r.n_applied) == (OK, OK, 5, 5)
    assert r.crop() == (3 + 4 + 1, 1 + 2 + 1, 29, 8)
    assert bad == [3 << 16 | 3, 0, 1, 1 << 16 | 2] and r.n_bad == 4
    st, r, bad = _validate(K.opcode_list(ops), None, crop=(3, 1, 60, 18), bad_cap=3)
    assert st == UNSUPPORTED and r.n_bad == 4 and bad is None
