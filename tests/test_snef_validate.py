"""rsx_nikon_snef_validate: every rejection include/rsx.h section 3m lists, in the reference's
order (DecodeSNefUncompressed, NefDecoder.cpp:389-394, then DecodeNikonSNef, :666-711), and the
accepted corners.  Host code only: no GPU needed."""
import numpy as np
import pytest

import snef_files as S
from rawspeed_amd import abi, capi

OK, INV, IO = abi.RSX_OK, abi.RSX_ERR_INVALID_ARG, abi.RSX_ERR_IO
TABLE = np.zeros(8192, np.uint16)
WB = (512, 683)


def _img(w, h, cpp=3, pitch=None):
    return abi.Image(None, 6 * w if pitch is None else pitch, w, h, cpp, 0)


def _v(w, h, cpp=3, pitch=None, wb=WB, table=TABLE, n=None):
    return capi.nikon_snef_validate(wb, table, _img(w, h, cpp, pitch), 3 * w * h if n is None else n)


def test_accepted_corners():
    assert _v(6, 1) == OK
    assert _v(S.MAX_W, S.MAX_H) == OK
    assert _v(6, S.MAX_H) == OK and _v(S.MAX_W, 1) == OK
    assert _v(8, 2, pitch=6 * 8 + 10) == OK           # pitch padding
    assert _v(8, 2, n=3 * 8 * 2 + 5) == OK            # bytes behind the image
    for wb in ((S.INV_WB_MIN, S.INV_WB_MAX), (S.INV_WB_MAX, S.INV_WB_MIN)):
        assert _v(8, 2, wb=wb) == OK


def test_null_descriptor_and_null_table():
    assert capi.nikon_snef_validate(None, None, _img(8, 2), 48) == INV
    assert _v(8, 2, table=None) == INV
    assert capi.lib().rsx_nikon_snef_validate(None, None, 0) == INV  # (no image either)


@pytest.mark.parametrize("w,h,cpp,pitch", [
    (8, 2, 1, None), (8, 2, 2, None), (8, 2, 4, None),       # cpp
    (0, 2, 3, None), (8, 0, 3, None), (-2, 2, 3, 64), (8, -1, 3, None),
    (7, 2, 3, None), (9, 2, 3, None), (S.MAX_W + 1, 2, 3, None),
    (S.MAX_W + 2, 2, 3, None), (8, S.MAX_H + 1, 3, None),
    (8, 2, 3, 6 * 8 - 2), (8, 2, 3, 0),                      # pitch below 6 w
])
def test_geometry_is_an_invalid_argument(w, h, cpp, pitch):
    assert _v(w, h, cpp, pitch, n=1 << 30) == INV


def test_narrow_images_are_an_io_error():
    """dim.x < 6 is ThrowIOE (:666-667), behind the dimension checks and in front of the white
    balance and the input size"""
    for w in (2, 4):
        assert _v(w, 3) == IO
        assert _v(w, 3, wb=(1, 1)) == IO and _v(w, 3, n=0) == IO
    assert _v(4, 3, cpp=1) == INV and _v(3, 3) == INV and _v(4, S.MAX_H + 1) == INV
    assert _v(4, 3, table=None) == INV


@pytest.mark.parametrize("wb", [(S.INV_WB_MIN - 1, 512), (512, S.INV_WB_MIN - 1), (S.INV_WB_MAX + 1, 512),
                                (512, S.INV_WB_MAX + 1), (0, 512), (512, -5), (1 << 30, 512)])
def test_white_balance_outside_the_reference_s_range(wb):
    assert _v(8, 2, wb=wb) == INV
    assert _v(8, 2, wb=wb, n=0) == INV  # in front of the input size


def test_short_input_is_an_io_error():
    assert _v(8, 2, n=47) == IO and _v(8, 2, n=0) == IO
    assert _v(S.MAX_W, S.MAX_H, n=3 * S.MAX_W * S.MAX_H - 1) == IO
