"""rsx_fpwrite_pack_validate: every verdict in its documented order (rsx_unpack_f32_validate's, then
the writer's own) against the Python restatement of tests/fpwrite_files.py, from the library and
from the host build of the core; where the reader's checks apply the reader agrees.  The integer
writer keeps refusing the widths of F32 images.  No GPU needed."""
import ctypes as C

import pytest

import fpwrite_files as F
from rawspeed_amd import abi, capi


def _img(dim_x=12, dim_y=6, cpp=1, pitch=None):
    return abi.Image(None, 4 * dim_x * cpp if pitch is None else pitch, dim_x, dim_y, cpp, 0)


def _cases():
    """(name, desc fields, image, out_cap): one verdict each, and pairs that fix the order"""
    ok = dict(crop_x=1, crop_y=1, crop_w=8, crop_h=4, pitch=16, bps=16, order=abi.ORDER_MSB)
    out = []

    def add(name, img=None, cap=None, **kw):
        f = dict(ok, **kw)
        d = F.pack_desc(f["crop_x"], f["crop_y"], f["crop_w"], f["crop_h"], f["pitch"], f["bps"],
                        f["order"])
        need = F.round_up4(max(f["crop_h"], 0) * max(f["pitch"], 0))
        out.append((name, d, img or _img(), need if cap is None else cap))

    add("ok16")
    add("ok24", bps=24, pitch=24, order=abi.ORDER_LSB)
    add("ok32", bps=32, pitch=35)
    add("ok32_any_order", bps=32, pitch=32, order=abi.ORDER_MSB32)
    add("ok_cpp3", img=_img(cpp=3), crop_w=3, pitch=18)
    add("stream_past_32_bits", crop_h=1 << 16, pitch=1 << 16)
    add("stream_past_32_bits_before_empty", crop_h=-1, pitch=1 << 20)
    add("empty_w", crop_w=0)
    add("empty_h", crop_h=0)
    add("pitch_0", pitch=0)
    add("order_jpeg", order=abi.ORDER_MSB32 + 1)
    add("order_negative", order=-1)
    add("cpp_0", img=_img(cpp=0))
    add("cpp_4", img=_img(cpp=4))
    add("bps_0", bps=0)
    add("bps_33", bps=33, pitch=64)
    add("bits_not_bytes", bps=12, crop_w=3, pitch=16)
    add("pitch_short", pitch=15)
    add("crop_x_negative", crop_x=-1)
    add("crop_y_negative", crop_y=-1)
    add("crop_y_past", crop_y=7)
    add("crop_x_past", crop_x=5)
    add("bps_8", bps=8, pitch=8)
    add("bps_12", bps=12, pitch=12)
    add("order_msb16", order=abi.ORDER_MSB16)
    add("order_msb32_24", bps=24, pitch=24, order=abi.ORDER_MSB32)
    add("two_bytes", crop_w=1, crop_h=1, pitch=2)
    add("two_bytes_32_has_no_streamer", bps=32, crop_w=1, crop_h=1, pitch=4)
    add("four_bytes", crop_w=2, crop_h=1, pitch=4)
    add("rows_past_image", crop_y=3)
    add("rows_to_the_edge", crop_y=2)
    add("image_pitch_odd", img=_img(pitch=50))
    add("image_pitch_short", img=_img(pitch=32))
    add("image_pitch_exact", img=_img(pitch=36))
    add("image_pitch_short_32_cpp", img=_img(cpp=2, pitch=68), bps=32, pitch=64)
    add("image_pitch_exact_32_cpp", img=_img(cpp=2, pitch=72), bps=32, pitch=64)
    add("image_dim_y_negative", img=abi.Image(None, 48, 12, -6, 1, 0))
    add("image_dim_x_negative", img=abi.Image(None, 48, -12, 6, 1, 0))
    add("image_dim_y_0", img=abi.Image(None, 48, 12, 0, 1, 0), crop_y=0)
    add("cap_one_short", cap=63)
    add("cap_tail", pitch=17, cap=67)  # roundUp(68, 4) is 68
    add("cap_tail_ok", pitch=17, cap=68)
    # order: the reader's verdict comes before the writer's
    add("bps_before_rows", bps=12, crop_y=3)
    add("io_before_cap", crop_w=1, crop_h=1, pitch=2, cap=0)
    return out


CASES = _cases()
# the status of every case that is not RSX_ERR_INVALID_ARG, written down
EXPECT = dict({n: F.OK for n in ("ok16", "ok24", "ok32", "ok32_any_order", "ok_cpp3", "four_bytes",
                                 "two_bytes_32_has_no_streamer", "rows_to_the_edge",
                                 "image_pitch_exact", "image_pitch_exact_32_cpp", "cap_tail_ok")},
              **{n: F.IO for n in ("stream_past_32_bits", "stream_past_32_bits_before_empty",
                                   "two_bytes", "io_before_cap")})


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_verdict(case):
    name, d, img, cap = case
    want = F.validate_model(d, img, cap)
    assert capi.fpwrite_pack_validate(d, img, cap) == want, name
    assert F.host().rsx_fpwrite_host_pack_validate(C.byref(d), C.byref(img), cap) == want, name
    assert want == EXPECT.get(name, F.INVALID_ARG), name
    # a stream the writer accepts is one the reader accepts
    if want == F.OK:
        assert capi.lib().rsx_unpack_f32_validate(C.byref(d), C.byref(img), cap) == F.OK


def test_the_list_reaches_every_status():
    got = {F.validate_model(d, img, cap) for _, d, img, cap in CASES}
    assert got == {F.OK, F.INVALID_ARG, F.IO}


def test_null_arguments():
    _, d, img, cap = CASES[0]
    assert capi.fpwrite_pack_validate(None, img, cap) == F.INVALID_ARG
    assert capi.fpwrite_pack_validate(d, None, cap) == F.INVALID_ARG


def test_the_readers_verdicts_come_first():
    """wherever the reader refuses a descriptor for a stream of the writer's size, the writer gives
    the same status"""
    for name, d, img, cap in CASES:
        need = F.round_up4(max(d.crop_h, 0) * max(d.input_pitch_bytes, 0))
        rd = capi.lib().rsx_unpack_f32_validate(C.byref(d), C.byref(img), max(need, 1 << 33))
        if rd != F.OK:
            assert capi.fpwrite_pack_validate(d, img, cap) == rd, name


def test_the_integer_writer_still_refuses_the_widths_of_f32_images():
    img = abi.Image(None, 64, 8, 4, 1, 1)
    for bps in range(17, 33):
        d = abi.UnpackDesc(0, 0, 8, 4, 8 * bps // 8 + 4, bps, abi.ORDER_MSB)
        assert capi.encode_pack_validate(d, img, 1 << 20) == abi.RSX_ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------
# deflate tiles
# ---------------------------------------------------------------------------------------------
def _dimg(dim_x=40, dim_y=30, cpp=1, pitch=None):
    return abi.Image(None, 4 * dim_x * cpp if pitch is None else pitch, dim_x, dim_y, cpp, 0)


DEFLATE_CASES = [
    ("ok", 16, 3, (8, 8, 4, 4, 8, 8), _dimg(), F.OK),
    ("ok_ragged", 24, 34894, (16, 16, 32, 20, 8, 10), _dimg(), F.OK),
    ("ok_cpp4", 32, 34895, (16, 4, 144, 0, 16, 4), _dimg(cpp=4), F.OK),
    ("bps_8", 8, 3, (8, 8, 0, 0, 8, 8), _dimg(), F.INVALID_ARG),
    ("bps_before_predictor", 12, 2, (8, 8, 0, 0, 8, 8), _dimg(), F.INVALID_ARG),
    ("predictor_2", 16, 2, (8, 8, 0, 0, 8, 8), _dimg(), F.INVALID_ARG),
    ("cpp_0", 16, 3, (8, 8, 0, 0, 8, 8), _dimg(cpp=0), F.INVALID_ARG),
    ("cpp_5", 16, 3, (8, 8, 0, 0, 8, 8), _dimg(cpp=5), F.INVALID_ARG),
    ("dim_x_0", 16, 3, (8, 8, 0, 0, 8, 8), _dimg(dim_x=0, pitch=160), F.INVALID_ARG),
    ("dim_y_negative", 16, 3, (8, 8, 0, 0, 8, 8), _dimg(dim_y=-3), F.INVALID_ARG),
    ("pitch_odd", 16, 3, (8, 8, 0, 0, 8, 8), _dimg(pitch=162), F.INVALID_ARG),
    ("tile_w_0", 16, 3, (0, 8, 0, 0, 8, 8), _dimg(), F.INVALID_ARG),
    ("height_0", 16, 3, (8, 8, 0, 0, 8, 0), _dimg(), F.INVALID_ARG),
    ("width_past_tile", 16, 3, (8, 8, 0, 0, 9, 8), _dimg(), F.INVALID_ARG),
    ("height_past_tile", 16, 3, (8, 8, 0, 0, 8, 9), _dimg(), F.INVALID_ARG),
    ("window_past_right", 16, 3, (8, 8, 33, 0, 8, 8), _dimg(), F.INVALID_ARG),
    ("window_to_the_edge", 16, 3, (8, 8, 32, 22, 8, 8), _dimg(), F.OK),
    ("window_past_bottom", 16, 3, (8, 8, 0, 23, 8, 8), _dimg(), F.INVALID_ARG),
    ("pitch_short", 16, 3, (8, 8, 0, 0, 8, 8), _dimg(pitch=156), F.INVALID_ARG),
    ("tile_too_large", 32, 3, (1 << 13, 1 << 13, 0, 0, 8, 8), _dimg(), F.UNSUPPORTED),
    ("tile_largest", 16, 3, (1 << 13, (1 << 14) - 1, 0, 0, 8, 8), _dimg(), F.OK),
    ("window_before_size", 32, 3, (1 << 13, 1 << 13, 40, 0, 8, 8), _dimg(), F.INVALID_ARG),
]


@pytest.mark.parametrize("case", DEFLATE_CASES, ids=lambda c: c[0])
def test_deflate_verdict(case):
    name, bps, pred, geom, img, want = case
    assert F.deflate_validate_model(bps, pred, geom, img) == want
    d, t = abi.DngDeflateDesc(bps, pred), F.deflate_tile(geom)
    assert capi.fpwrite_deflate_validate(d, t, img) == want
    bound = capi.fpwrite_deflate_bound(d, t, img)
    assert F.dfl().rsx_fpwrite_host_deflate_bound(C.byref(d), C.byref(t), C.byref(img)) == bound
    n = bps // 8 * geom[0] * geom[1]
    assert bound == (F.bound_model(n) if want == F.OK else 0)
    # where the reader has a verdict of its own it is the same one (its size limit is 2^32)
    rd = capi.dng_deflate_validate(bps, pred, geom, 64, img)
    assert rd == (F.OK if want == F.UNSUPPORTED else want)


def test_deflate_null_arguments():
    d, t, img = abi.DngDeflateDesc(16, 3), F.deflate_tile((8, 8, 0, 0, 8, 8)), _dimg()
    for args in ((None, t, img), (d, None, img), (d, t, None)):
        assert capi.fpwrite_deflate_validate(*args) == F.INVALID_ARG
        assert capi.fpwrite_deflate_bound(*args) == 0
