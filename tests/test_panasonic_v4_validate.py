"""rsx_panasonic_v4_validate at the edges of PanasonicV4Decompressor's constructor
(PanasonicV4Decompressor.cpp:49-86), in its order: cpp 1, positive area and dim_x % 14 == 0,
section_split_offset <= 0x4000, bufSize <= UINT32_MAX -- ThrowRDE, RSX_ERR_INVALID_ARG -- then
input.peekStream(bufSize) -- an IOException, RSX_ERR_IO.  Behind them a split no caller passes
(neither 0 nor 0x1FF8) is RSX_ERR_UNSUPPORTED.  The entry points of section 3j keep refusing
version 4.  Where oracle/_ref is built, the unmodified reference's whole-file outcome is checked
for the same geometry.  No GPU needed."""
import numpy as np
import pytest

import rw2_v4_files as V
from oracle_lib import Ref
from rawspeed_amd import abi, build, capi

OK, INV, IO, UNS = abi.RSX_OK, abi.RSX_ERR_INVALID_ARG, abi.RSX_ERR_IO, abi.RSX_ERR_UNSUPPORTED
needs_ref = pytest.mark.skipif(not Ref.available(), reason="oracle/_ref not built")


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.build_core()
    return capi.lib()


def _view(w, h, cpp=1, pitch=None):
    return abi.Image(None, max(2 * w, 2) if pitch is None else pitch, w, h, cpp, 1)


def _validate(split, view, in_bytes, zero_is_bad=1):
    return capi.panasonic_v4_validate(split, zero_is_bad, view, in_bytes)


@pytest.mark.parametrize("split", V.SPLITS)
def test_accepts_and_the_constructor_s_order(split):
    w, h = 4 * 14, 6
    need = V.consumed(split, w, h)
    assert abi.panasonic_v4_consumed(split, w, h) == need
    for flag in (0, 1):
        assert _validate(split, _view(w, h), need, flag) == OK
    # 1. the component count
    assert _validate(split, _view(w, h, cpp=2), need) == INV
    assert _validate(split, _view(w, h, cpp=3), need) == INV
    # 2. the dimensions
    for bw, bh in ((0, h), (w, 0), (-w, h), (w, -h), (w + 1, h), (w - 1, h), (13, h), (7, 2)):
        assert _validate(split, _view(bw, bh), 1 << 30) == INV, (bw, bh)
    assert _validate(split, _view(14, 1), V.consumed(split, 14, 1)) == OK
    # (they come before the split, the size and the input: none of those changes the answer)
    assert _validate(split, _view(w + 1, h), 0) == INV
    assert _validate(0x4001, _view(w + 1, h), 0) == INV
    assert _validate(1, _view(w, h, cpp=2), 0) == INV
    # the image's own row must hold its pixels
    assert _validate(split, _view(w, h, pitch=2 * w - 2), need) == INV
    assert _validate(split, _view(w, h, pitch=2 * w + 6), need) == OK


def test_the_split():
    """<= 0x4000 for the constructor; of those only 0 and 0x1FF8 have a caller and a test"""
    w, h = 14 * 100, 30  # 3000 packets
    v = _view(w, h)
    whole = 3 * 0x4000
    assert V.consumed(0, w, h) == 48000 and V.consumed(V.SPLIT, w, h) == whole
    assert _validate(0, v, 48000) == OK and _validate(0x1FF8, v, whole) == OK
    for split in (1, 8, 0x1FF7, 0x1FF9, 0x2000, 0x3FFF, 0x4000):
        assert _validate(split, v, whole) == UNS, split
        # the constructor's own checks come first: the input (whole blocks for any split but 0)
        assert _validate(split, v, whole - 1) == IO, split
        assert _validate(split, _view(w + 1, h), whole) == INV, split
    for split in (0x4001, 0x8000, 0xFFFFFFFF):
        assert _validate(split, v, whole) == INV, split
        assert _validate(split, v, 0) == INV, split  # ... in front of the input's size


@pytest.mark.parametrize("split", V.SPLITS)
@pytest.mark.parametrize("packets_w,h", [(1, 1), (3, 5), (128, 8), (128, 9), (1024, 3)])
def test_input_size_boundary(split, packets_w, h):
    """one byte short fails with the IOException's status, exact passes, extra passes (bytes
    behind are not read)"""
    w = 14 * packets_w
    need = V.consumed(split, w, h)
    packets = packets_w * h
    assert need == (16 * packets if split == 0 else -(-packets // 1024) * 0x4000)
    v = _view(w, h)
    assert _validate(split, v, need - 1) == IO
    assert _validate(split, v, need) == OK
    assert _validate(split, v, need + 1) == OK
    assert _validate(split, v, need + 0x4000 + 5) == OK
    assert _validate(split, v, 0) == IO
    if split:
        # the last block is demanded whole, however few packets of it hold pixels
        assert _validate(split, v, 16 * packets) == (OK if need == 16 * packets else IO)


def test_buffer_size_must_fit_32_bits():
    """"Raw dimensions require input buffer larger than supported" is a ThrowRDE"""
    huge = 1 << 40
    assert 65534 % 14 == 0
    assert _validate(0, _view(65534, 65535), huge) == INV
    assert _validate(V.SPLIT, _view(65534, 65535), huge) == INV
    w = 14 * 1024  # 0x4000 bytes a row
    h_fit = 0xFFFFFFFF // 0x4000
    for split in V.SPLITS:
        assert V.consumed(split, w, h_fit) <= 0xFFFFFFFF < V.consumed(split, w, h_fit + 1)
        assert _validate(split, _view(w, h_fit), huge) == OK
        assert _validate(split, _view(w, h_fit + 1), huge) == INV
        assert _validate(split, _view(w, h_fit + 1), 0) == INV  # (in front of the input's size)
        assert _validate(split, _view(w, h_fit), 0xFFFFFFFF - 0x4000) == IO
    # rounding up to whole blocks is what passes the limit here: 16 packets fit, the blocks do not
    w, h = 14 * 1023, 262400
    assert w * h // 14 * 16 <= 0xFFFFFFFF < V.consumed(V.SPLIT, w, h)
    assert _validate(0, _view(w, h), huge) == OK and _validate(V.SPLIT, _view(w, h), huge) == INV


def test_null_desc_and_null_image():
    v = _view(14, 2)
    assert capi.panasonic_v4_validate(None, 1, v, 1 << 20) == INV
    assert capi.panasonic_v4_validate(0, 1, None, 1 << 20) == INV
    assert capi.panasonic_v4_validate(None, 1, None, 1 << 20) == INV
    assert capi.panasonic_v4_validate(0, 1, v, 1 << 20) == OK


def test_the_entry_points_of_3j_still_refuse_version_4():
    v = _view(14 * 9 * 10, 2)  # (a width every layout of 3j accepts)
    for bps in (12, 14):
        assert capi.panasonic_validate(4, bps, v, 1 << 20) == INV


@pytest.mark.ref
@needs_ref
@pytest.mark.parametrize("split", V.SPLITS)
@pytest.mark.parametrize("dw,short,want", [(0, 0, OK), (0, 1, IO), (0, 17, IO), (1, 0, INV), (-1, 0, INV)])
def test_reference_agrees(split, dw, short, want):
    """The same geometry as a whole file through the unmodified reference: it accepts and refuses
    the same files.  The dimensions are a ThrowRDE (RSX_ERR_INVALID_ARG).  peekStream's
    IOException does not leave the decoder as one: RawDecoder::decodeRaw catches it and throws a
    RawDecoderException ("image file may be truncated"), so through a file the reference's status
    is RSX_ERR_INVALID_ARG there too, where the constructor alone -- and rsx_panasonic_v4_validate
    -- says RSX_ERR_IO."""
    ref = Ref()
    w, h = 5 * 14 + dw, 3
    rng = np.random.default_rng([4, split, dw + 1, short])
    data = rng.integers(0, 256, size=V.consumed(split, 5 * 14, h) - short, dtype=np.uint8)
    st, _ = ref.decode_file(V.v4_file(split, w, h, data))
    assert st == (OK if want == OK else INV), (st, ref.last_error())
    if want == IO:
        assert "may be truncated" in ref.last_error()
    elif want == INV:
        assert "Unexpected image dimensions" in ref.last_error()
    assert _validate(split, _view(w, h), data.size) == want
