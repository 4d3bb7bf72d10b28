"""rsx_fuji_parse and rsx_fuji_validate (include/rsx.h section 3u), through the product library
and through the host build of the same core: the container parse with every read past the end,
and one case per refusal of the constructor's checks, in the reference's order."""
import ctypes as C
import struct

import pytest

import fuji_files as F
from rawspeed_amd import abi, capi


def _host_parse(data):
    return F.host_parse(data)


def _host_validate(d, view):
    return F.host_lib().rsx_fuji_host_validate(None if d is None else C.byref(d),
                                               None if view is None else C.byref(view))


PARSERS = [capi.fuji_parse, _host_parse]
VALIDATORS = [capi.fuji_validate, _host_validate]


def _view(w, h, cpp=1, pitch=None):
    return abi.Image(None, 2 * w * cpp if pitch is None else pitch, w, h, cpp, 1)


@pytest.mark.parametrize("parse", PARSERS)
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 16])
def test_parse_layout(parse, n):
    """the sizes, the padding rule raw_offset & 0xC, the strips one after another"""
    h = F.header(16, 14, 768 * n, 6)
    strips = [bytes([s + 1]) * (5 + 3 * s) for s in range(n)]
    data = F.container(h, strips)
    pad = 0x10 - ((4 * n) & 0xC) if (4 * n) & 0xC else 0
    st, d = parse(data)
    assert st == F.OK and d.n_strips == n
    for k, v in h.items():
        assert getattr(d, k) == v, k
    pos = 16 + 4 * n + pad
    for s in range(n):
        assert (d.strip_offset[s], d.strip_bytes[s]) == (pos, len(strips[s]))
        pos += len(strips[s])
    assert pos == len(data)
    assert F.parse(data) == (F.OK, h, [(d.strip_offset[s], d.strip_bytes[s]) for s in range(n)])
    # every read past the end: the header, the sizes, the padding, each strip
    for cut in (0, 15, 16, 16 + 4 * n - 1, 16 + 4 * n + pad - 1, len(data) - 1,
                len(data) - len(strips[-1])):
        if cut == 16 + 4 * n + pad - 1 and not pad:
            continue
        assert parse(data[:cut])[0] == F.ERR_IO == F.parse(data[:cut])[0], cut


@pytest.mark.parametrize("parse", PARSERS)
def test_parse_leaves_a_refused_header_to_validate(parse):
    h = F.header(16, 14, 768, 6, blocks_in_row=200)
    st, d = parse(F.container(h, [], sizes=[]))
    assert st == F.OK and d.n_strips == 0 and d.blocks_in_row == 200
    assert capi.fuji_validate(d, _view(768, 6)) == F.ERR_INVALID_ARG


# FujiHeader::operator bool, :919-937, clause by clause
BAD_HEADERS = [
    dict(signature=0x4954), dict(version=2), dict(raw_height=0x3006, total_lines=0x801),
    dict(raw_height=0, total_lines=0), dict(raw_height=7), dict(raw_width=0x3018),
    dict(raw_width=0x2E8), dict(raw_width=780), dict(raw_rounded_width=0x3300),
    dict(block_size=0x200), dict(raw_rounded_width=0), dict(raw_rounded_width=1000),
    dict(raw_rounded_width=3072, blocks_in_row=4), dict(blocks_in_row=17), dict(blocks_in_row=0),
    dict(blocks_in_row=2), dict(total_lines=0x801), dict(total_lines=0), dict(total_lines=3),
    dict(raw_bits=10), dict(raw_type=1),
]


@pytest.mark.parametrize("validate", VALIDATORS)
def test_validate_refusals_in_the_reference_order(validate):
    good = F.header(16, 14, 1560, 12)
    assert F.header_ok(good)
    d = abi.fuji_desc(good, [(64, 100), (164, 100), (264, 100)])
    v = _view(1560, 12)
    assert validate(d, v) == F.OK
    assert validate(None, v) == F.ERR_INVALID_ARG and validate(d, None) == F.ERR_INVALID_ARG
    # 1. the component count, in front of everything else
    bad_all = abi.fuji_desc(dict(good, signature=0, raw_bits=12), [])
    assert validate(bad_all, _view(1, 1, cpp=3)) == F.ERR_INVALID_ARG
    # 2. the header, clause by clause, in front of the dimensions and the depth
    for over in BAD_HEADERS:
        h = dict(good, **over)
        assert not F.header_ok(h), over
        assert validate(abi.fuji_desc(h, [(64, 100)] * 3), v) == F.ERR_INVALID_ARG, over
    # 3. the dimensions in front of the 12-bit refusal
    twelve = abi.fuji_desc(dict(good, raw_bits=12), [(64, 100)] * 3)
    assert validate(twelve, _view(1560, 6)) == F.ERR_INVALID_ARG
    assert validate(twelve, _view(1536, 12)) == F.ERR_INVALID_ARG
    assert validate(d, _view(1560, 12, pitch=2 * 1560 - 2)) == F.ERR_INVALID_ARG
    # 4. 12 bits: the reference throws
    assert validate(twelve, v) == F.ERR_UNSUPPORTED
    # 5. a descriptor whose strips do not match the header
    assert validate(abi.fuji_desc(good, [(64, 100)] * 2), v) == F.ERR_INVALID_ARG
    # both types and depths pass
    for raw_type, raw_bits in F.TYPES:
        assert validate(abi.fuji_desc(F.header(raw_type, raw_bits, 768, 6), [(32, 9)]),
                        _view(768, 6)) == F.OK


def test_header_bytes_are_big_endian():
    h = F.header(0, 16, 6240, 4160)
    data = F.container(h, [b"abcd"] * 9)
    assert data[:2] == b"\x49\x53" and struct.unpack(">H", data[9:11])[0] == 6240
    st, d = capi.fuji_parse(data)
    assert st == F.OK and (d.raw_width, d.raw_height, d.blocks_in_row, d.total_lines) == \
        (6240, 4160, 9, 693)
