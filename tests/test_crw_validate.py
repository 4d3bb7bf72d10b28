"""rsx_crw_validate (the library's and the host build's) against the model's validate, which is
the reference's constructor in its order (tests/crw_files.py, VALIDATION; the cases a file can
express are in tests/golden/crw_ref.json), then the pitch and the reader's 8 bytes."""
import ctypes as C

import pytest

import crw_files as F
from rawspeed_amd import abi, capi


def _both(table, lowbits, img, in_bytes, low_bytes):
    a = capi.crw_validate(table, lowbits, img, in_bytes, low_bytes)
    d = None if table is None else abi.crw_desc(table, lowbits)
    b = F.host_lib().rsx_crw_host_validate(None if d is None else C.byref(d),
                                           None if img is None else C.byref(img), in_bytes,
                                           low_bytes)
    assert a == b
    return a


@pytest.mark.parametrize("case", F.VALIDATION, ids=[v[0] for v in F.VALIDATION])
def test_validation_case(case):
    name, w, h, table, low_short, cpp, pitch, want = case
    img = abi.Image(None, 2 * w if pitch is None else pitch, w, h, cpp, 1)
    low_bytes = max(0, w * h // 4) - low_short
    assert _both(table, True, img, 64, max(0, low_bytes)) == want
    assert want == F.validate(w, h, table, True, low_bytes, 64, cpp, pitch)
    if name == "low_one_short":  # (without low bits nothing is asked of them)
        assert _both(table, False, img, 64, 0) == F.OK


def test_null_arguments_and_the_order_of_the_checks():
    img = abi.Image(None, 128, 64, 4, 1, 1)
    assert _both(None, False, img, 64, 0) == F.ERR_INVALID_ARG
    assert _both(0, False, None, 64, 0) == F.ERR_INVALID_ARG
    # the reader's 8 bytes come last: a bad table with 7 bytes is the table's refusal
    assert _both(0, False, img, 7, 0) == F.ERR_IO
    assert _both(0, False, img, 8, 0) == F.OK
    assert _both(3, False, img, 7, 0) == F.ERR_INVALID_ARG
    assert _both(0, True, img, 7, 63) == F.ERR_INVALID_ARG
    assert _both(0, True, img, 7, 64) == F.ERR_IO
    bad = abi.Image(None, 126, 64, 4, 1, 1)
    assert _both(0, False, bad, 7, 0) == F.ERR_INVALID_ARG
