"""rsx_sony_arw2_validate at the edges of SonyArw2Decompressor's constructor
(SonyArw2Decompressor.cpp:40-54: cpp 1, dim > 0, dim_x % 32 == 0, dim_x <= 9600,
dim_y <= 6376, then input.peekStream(w * h)) and of the table descriptor.  Where a case can
be reached through a whole ARW2 file, the unmodified reference's outcome is checked too.
No GPU needed."""
import numpy as np
import pytest

import arw2_files as A
from oracle_lib import Ref
from rawspeed_amd import abi, build, capi

OK, INV, IO = abi.RSX_OK, abi.RSX_ERR_INVALID_ARG, abi.RSX_ERR_IO
TABLE = A.table_dither(A.decode_curve(A.REALISTIC_CURVE))


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.build_core()
    return capi.lib()


def _view(w, h, cpp=1):
    return abi.Image(None, max(2 * w, 2), w, h, cpp, 1)


@pytest.mark.parametrize("w,h,want", [
    (0, 2, INV), (31, 2, INV), (32, 2, OK), (48, 2, INV), (9600, 2, OK), (9632, 2, INV),
    (32, 6376, OK), (32, 6377, INV), (32, 0, INV), (-32, 2, INV)])
def test_dimensions(w, h, want):
    n = max(w, 0) * max(h, 0)
    assert capi.sony_arw2_validate(abi.ARW2_TABLE_NONE, None, _view(w, h), n) == want
    assert capi.sony_arw2_validate(abi.ARW2_TABLE_DITHER, TABLE, _view(w, h), n) == want


def test_component_count():
    assert capi.sony_arw2_validate(abi.ARW2_TABLE_NONE, None, _view(64, 2, 2), 128) == INV
    assert capi.sony_arw2_validate(abi.ARW2_TABLE_NONE, None, _view(64, 2, 1), 128) == OK


def test_input_size():
    v = _view(64, 4)
    assert capi.sony_arw2_validate(abi.ARW2_TABLE_NONE, None, v, 64 * 4 - 1) == IO
    assert capi.sony_arw2_validate(abi.ARW2_TABLE_NONE, None, v, 64 * 4) == OK
    assert capi.sony_arw2_validate(abi.ARW2_TABLE_NONE, None, v, 64 * 4 + 7) == OK
    assert capi.sony_arw2_validate(abi.ARW2_TABLE_NONE, None, v, 0) == IO
    # the dimension checks come first (the constructor's order)
    assert capi.sony_arw2_validate(abi.ARW2_TABLE_NONE, None, _view(33, 4), 0) == INV


def test_pitch_too_small():
    v = abi.Image(None, 2 * 64 - 2, 64, 2, 1, 1)
    assert capi.sony_arw2_validate(abi.ARW2_TABLE_NONE, None, v, 128) == INV


def test_table_misuse():
    v = _view(64, 2)
    assert capi.sony_arw2_validate(None, None, v, 128) == INV  # NULL desc
    for mode in (-1, 3, 7):
        assert capi.sony_arw2_validate(mode, TABLE, v, 128) == INV
    assert capi.sony_arw2_validate(abi.ARW2_TABLE_PLAIN, None, v, 128) == INV
    assert capi.sony_arw2_validate(abi.ARW2_TABLE_DITHER, None, v, 128) == INV
    assert capi.sony_arw2_validate(abi.ARW2_TABLE_PLAIN, TABLE[:4096], v, 128) == OK
    assert capi.sony_arw2_validate(abi.ARW2_TABLE_DITHER, TABLE, v, 128) == OK
    # NONE ignores a table
    assert capi.sony_arw2_validate(abi.ARW2_TABLE_NONE, TABLE, v, 128) == OK
    assert lib_validate_null_image() == INV


def lib_validate_null_image():
    d, keep = abi.sony_arw2_desc(abi.ARW2_TABLE_NONE)
    return capi.lib().rsx_sony_arw2_validate(capi.C.byref(d), None, 128)


@pytest.mark.ref
@pytest.mark.skipif(not Ref.available(), reason="oracle/_ref not built")
@pytest.mark.parametrize("w,h,ok", [(32, 2, True), (9600, 2, True), (9632, 2, False),
                                    (48, 2, False), (32, 6376, True), (32, 6378, False)])
def test_reference_agrees_on_dimensions(w, h, ok):
    """Whole files through ArwDecoder (which also wants an even height, ArwDecoder.cpp:225)."""
    rng = np.random.default_rng([w, h])
    data = A.random_stream(rng, w, h)  # (every w here is a multiple of 16)
    st, dec = Ref().decode_file(A.arw2_file(w, h, data))
    assert (st == 0) == ok, (st, Ref().last_error())
    want = OK if ok else INV
    assert capi.sony_arw2_validate(abi.ARW2_TABLE_NONE, None, _view(w, h), w * h) == want


@pytest.mark.ref
@pytest.mark.skipif(not Ref.available(), reason="oracle/_ref not built")
def test_reference_agrees_on_input_size():
    """w * h - 1 bytes: the constructor's peekStream throws (an IOException, which
    RawDecoder::decodeRaw rethrows as a RawDecoderException: INVALID_ARG for the whole file,
    RSX_ERR_IO for the constructor alone); w * h + 7 bytes: the rest is not read."""
    ref = Ref()
    rng = np.random.default_rng(3)
    w, h = 64, 4
    data = A.random_stream(rng, w, h)
    blob = A.arw2_file(w, h, data)
    st, dec = ref.decode_file(blob[:-1])
    assert st != 0 and "getSubView" in ref.last_error(), (st, ref.last_error())
    assert capi.sony_arw2_validate(abi.ARW2_TABLE_NONE, None, _view(w, h), w * h - 1) == IO
    st, dec = ref.decode_file(A.arw2_file(w, h, data, gap=7), uncorrected=True)
    assert st == 0
    _, img, _ = A.model_decode(data, w, h)
    assert np.array_equal(dec.u16()[:h, :w], img)
    assert capi.sony_arw2_validate(abi.ARW2_TABLE_NONE, None, _view(w, h), w * h + 7) == OK
