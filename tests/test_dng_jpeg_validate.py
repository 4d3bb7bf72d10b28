"""rsx_dng_jpeg_validate (include/rsx.h section 4e): every refusal of the header parse with its
status, the colour-space rule of default_decompress_parms on all five marker and id combinations,
and the fields of rsx_dng_jpeg_info -- through librsx.so (the entry point needs no device), the
host build of the same core, and the numpy model.  The streams are the committed fixtures with
their markers patched (tests/dng_jpeg_files.py)."""
import ctypes as C

import pytest

import dng_jpeg_files as J
from rawspeed_amd import abi, build, capi


def _img(cpp, dim=(64, 64), pitch=None):
    return abi.Image(None, pitch if pitch is not None else 2 * cpp * dim[0] + 2, dim[0], dim[1], cpp, 0)


def _validate(stream, cpp, off=(0, 0), img=None):
    """the three implementations must agree; -> (status, info of librsx.so)"""
    img = img or _img(cpp)
    st, info = capi.dng_jpeg_validate(stream, off, img)
    L = C.CDLL(build.build_jpeg_host()[0])
    tiles, keep = abi.dng_jpeg_tiles([stream], [off])
    hinfo = abi.DngJpegInfo()
    assert L.rsx_jpeg_host_validate(tiles, C.byref(img), C.byref(hinfo)) == st
    if st == J.OK:
        assert bytes(hinfo) == bytes(info)
    return st, info


def _sof(stream):
    return next(m for m, _, _ in J.markers(stream) if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC))


BASE = J.case("420_17x17")["stream"]
GREY = J.case("grey_8x8")["stream"]


def _with_marker_code(stream, old, new):
    at = next(a for m, a, _ in J.markers(stream) if m == old)
    return stream[:at + 1] + bytes([new]) + stream[at + 2:]


def test_fixtures_validate_with_their_geometry():
    for c in J.cases():
        st, info = _validate(c["stream"], c["cpp"], img=_img(c["cpp"], (100, 100)))
        assert st == J.OK, c["name"]
        assert (info.width, info.height, info.components) == (c["width"], c["height"], c["cpp"])
        assert J.model_validate(c["stream"], c["cpp"])[0] == J.OK
    _, info = _validate(J.case("420_47x71")["stream"], 3)
    assert (info.h_samp, info.v_samp, info.colour_space, info.n_segments) == (2, 2, J.YCBCR, 1)
    _, info = _validate(J.case("422_47x71")["stream"], 3)
    assert (info.h_samp, info.v_samp) == (2, 1)
    _, info = _validate(J.case("restart3_420_64x96")["stream"], 3, img=_img(3, (100, 100)))
    assert (info.restart_interval, info.n_segments) == (3, 8)
    _, info = _validate(J.case("restart1_grey_80x8")["stream"], 1, img=_img(1, (100, 100)))
    assert (info.restart_interval, info.n_segments, info.colour_space) == (1, 10, J.GREY)


@pytest.mark.parametrize("name,stream,cpp,want", [
    ("progressive SOF2", _with_marker_code(BASE, 0xC0, 0xC2), 3, J.UNSUPPORTED),
    ("lossless SOF3", _with_marker_code(BASE, 0xC0, 0xC3), 3, J.UNSUPPORTED),
    ("arithmetic SOF9", _with_marker_code(BASE, 0xC0, 0xC9), 3, J.UNSUPPORTED),
    ("extended SOF1 is accepted", _with_marker_code(BASE, 0xC0, 0xC1), 3, J.OK),
    ("12 bits", J.patched(BASE, 0xC0, 0, 12), 3, J.UNSUPPORTED),
    ("16 bits", J.patched(BASE, 0xC0, 0, 16), 3, J.IO),
    ("4:1:1", J.patched(BASE, 0xC0, 7, 0x41), 3, J.UNSUPPORTED),
    ("4:4:0", J.patched(BASE, 0xC0, 7, 0x12), 3, J.UNSUPPORTED),
    ("chroma 2 x 1", J.patched(BASE, 0xC0, 10, 0x21), 3, J.UNSUPPORTED),
    ("a sampling factor of 5", J.patched(BASE, 0xC0, 7, 0x51), 3, J.IO),
    ("zero width", J.patched(J.patched(BASE, 0xC0, 3, 0), 0xC0, 4, 0), 3, J.IO),
    ("zero height", J.patched(J.patched(BASE, 0xC0, 1, 0), 0xC0, 2, 0), 3, J.IO),
    ("a quantiser that is not there", J.patched(BASE, 0xC0, 8, 3), 3, J.IO),
    ("a DC table that is not there", J.patched(BASE, 0xDA, 2, 0x30), 3, J.IO),
    ("an AC table that is not there", J.patched(BASE, 0xDA, 4, 0x12), 3, J.IO),
    ("an unknown component in SOS", J.patched(BASE, 0xDA, 3, 9), 3, J.IO),
    ("the scan's order is not the frame's",
     J.patched(J.patched(BASE, 0xDA, 3, 3), 0xDA, 5, 2), 3, J.UNSUPPORTED),
    ("spectral selection", J.patched(BASE, 0xDA, 8, 5), 3, J.UNSUPPORTED),
    ("successive approximation", J.patched(BASE, 0xDA, 9, 0x10), 3, J.UNSUPPORTED),
    ("a DQT index of 4", J.patched(BASE, 0xDB, 0, 4), 3, J.IO),
    ("a DHT index of 4", J.patched(BASE, 0xC4, 0, 0x04), 3, J.IO),
    ("a DHT class of 2", J.patched(BASE, 0xC4, 0, 0x20), 3, J.IO),
    ("DHT counts that are no prefix code", J.patched(BASE, 0xC4, 1, 3), 3, J.IO),
    ("no SOI", b"\x00" + BASE[1:], 3, J.IO),
    ("a segment past the end", BASE[:40], 3, J.IO),
    ("nothing behind SOI", BASE[:2], 3, J.IO),
    ("EOI in front of SOS", BASE[:2] + b"\xff\xd9" + BASE[2:], 3, J.IO),
    ("cpp 1 for three components", BASE, 1, J.INVALID_ARG),
    ("cpp 3 for one component", GREY, 3, J.INVALID_ARG),
], ids=lambda v: v if isinstance(v, str) else None)
def test_refusals(name, stream, cpp, want):
    st, _ = _validate(stream, cpp)
    assert st == want, (name, st)
    assert J.model_validate(stream, cpp)[0] == want, "the model"


def _two_scans(stream):
    """the first scan holds one component only (a non-interleaved file starts like this)"""
    m, at, n = J.markers(stream)[-1]
    sos = bytes([0xFF, 0xDA, 0, 8, 1]) + stream[at + 5:at + 7] + stream[at + n - 3:at + n]
    return stream[:at] + sos + stream[at + n:]


def _four_components(stream):
    at, n = next((a, n) for m, a, n in J.markers(stream) if m == 0xC0)
    sof = bytearray(stream[at:at + n]) + bytes([4, 0x11, 1])
    sof[3] = n - 2 + 3
    sof[9] = 4
    return stream[:at] + bytes(sof) + stream[at + n:]


def test_two_scans_and_four_components():
    assert _validate(_two_scans(BASE), 3)[0] == J.UNSUPPORTED
    assert J.model_validate(_two_scans(BASE), 3)[0] == J.UNSUPPORTED
    assert _validate(_four_components(BASE), 3)[0] == J.UNSUPPORTED
    assert _validate(_four_components(BASE), 4)[0] == J.UNSUPPORTED
    assert J.model_validate(_four_components(BASE), 4)[0] == J.UNSUPPORTED


def test_the_colour_space_rule():
    s444 = J.case("444_17x9")["stream"]
    bare = J.without_marker(s444, 0xE0)  # ids 1, 2, 3, neither JFIF nor Adobe
    rgb_ids = J.with_ids(bare, b"RGB")
    combos = [
        ("JFIF", s444, J.YCBCR),
        ("JFIF wins over an Adobe marker", J.with_segment(s444, 0xEE, J.adobe_app14(0)), J.YCBCR),
        ("JFIF wins over the ids", J.with_ids(s444, b"RGB"), J.YCBCR),
        ("Adobe, transform 0", J.with_segment(bare, 0xEE, J.adobe_app14(0)), J.RGB),
        ("Adobe, transform 1", J.with_segment(rgb_ids, 0xEE, J.adobe_app14(1)), J.YCBCR),
        ("Adobe, transform 2", J.with_segment(bare, 0xEE, J.adobe_app14(2)), J.YCBCR),
        ("no marker, ids 1 2 3", bare, J.YCBCR),
        ("no marker, ids R G B", rgb_ids, J.RGB),
        ("no marker, other ids", J.with_ids(bare, (10, 11, 12)), J.YCBCR),
    ]
    for name, stream, want in combos:
        st, info = _validate(stream, 3)
        assert (st, info.colour_space) == (J.OK, want), name
        mst, H = J.model_validate(stream, 3)
        assert (mst, H["colour"]) == (J.OK, want), name
    # the recorded RGB stream is Adobe with transform 0; subsampled RGB is left to the CPU
    assert _validate(J.case("rgb_40x56")["stream"], 3)[1].colour_space == J.RGB
    sub = J.with_ids(J.without_marker(BASE, 0xE0), b"RGB")
    assert _validate(sub, 3)[0] == J.UNSUPPORTED


def test_argument_checks_come_first():
    broken = b"\x00" + BASE[1:]
    for img in (_img(3, (0, 8)), _img(3, (8, 0)), _img(0), _img(3, pitch=2 * 3 * 64 + 1),
                _img(3, pitch=2 * 3 * 64 - 2)):
        assert _validate(broken, 3, img=img)[0] == J.INVALID_ARG
    assert _validate(broken, 3, off=(64, 0))[0] == J.INVALID_ARG
    assert _validate(broken, 3, off=(0, 64))[0] == J.INVALID_ARG
    assert _validate(BASE, 3, off=(63, 63))[0] == J.OK
    assert capi.lib().rsx_dng_jpeg_validate(None, C.byref(_img(3)), None) == J.INVALID_ARG
    tiles, keep = abi.dng_jpeg_tiles([BASE], [(0, 0)])
    assert capi.lib().rsx_dng_jpeg_validate(tiles, None, None) == J.INVALID_ARG
    assert capi.lib().rsx_dng_jpeg_validate(tiles, C.byref(_img(3)), None) == J.OK
