"""The numpy model of the writers (tests/encode_files.py) against three independent witnesses: the
bytes recorded from the reference's BitVacuumer* and PrefixCodeVectorEncoder
(tests/golden/encode_ref.json, scripts/record_encode_ref.cpp), the test writers of
rawspeed_amd/csrc/synth/rsx_synth.c, and the oracle's readers, which must give the image back."""
import hashlib

import numpy as np
import pytest

from rawspeed_amd import abi, synth

import encode_files as F
from oracle_lib import HostImage

EOI = np.array([0xFF, 0xD9] + [0] * 16, dtype=np.uint8)


@pytest.fixture(scope="module")
def golden():
    return F.load_golden()


def _same(data, rec):
    """bytes against a record: hex for the small cases, length + md5 for the larger ones"""
    if "hex" in rec:
        return bytes(data).hex() == rec["hex"]
    return len(data) == rec["length"] and hashlib.md5(bytes(data)).hexdigest() == rec["md5"]


def test_pack_model_equals_the_reference_vacuumers(golden):
    n = 0
    for name, order, bps, cols, rows, pad in F.pack_cases():
        if rows != 1:
            continue
        px = F.pack_case_rows(name, bps, cols, rows)
        got = F.model_pack(px, bps, order, cols * bps // 8)
        assert _same(got, golden["pack"][name]), name
        n += 1
    assert n == len(golden["pack"]) and n >= 4 * 7 * 3


def test_ljpeg_model_equals_the_reference_encoder_in_vacuumer_mode(golden):
    """One recorded case differs by rule: with fixDNGBug16 the reference's encoder writes the 16
    low bits of -32769 (7FFF) behind the code of -32768, where include/rsx.h section 7b and
    rsx_synth.c write 16 zero bits; the reader skips them either way.  The record of those cases
    holds the reference's bytes; the model's differ from them in exactly those 16-bit fields."""
    n = 0
    for name, tab, fix16, diffs in F.difference_lists():
        st, got, bits = F.model_ljpeg_diffs(diffs, [F.TABLES[tab]], fix16, F.TAIL_VACUUMER)
        assert st == F.OK
        rec = golden["ljpeg"][name]
        if fix16 and -32768 in diffs:
            st, ref_like, _ = F.model_ljpeg_diffs(diffs, [F.TABLES[tab]], fix16, F.TAIL_VACUUMER,
                                                  skip_bits=0x7FFF)
            assert _same(ref_like, rec), name
            assert len(got) <= len(ref_like)
        else:
            assert _same(got, rec), name
        assert bits == rec["symbol_bits"], name
        n += 1
    assert n == len(golden["ljpeg"])


@pytest.mark.parametrize("order", F.ORDERS)
def test_pack_model_equals_synth_pack_rows(order):
    word = {abi.ORDER_MSB16: 2, abi.ORDER_MSB32: 4}.get(order, 1)
    n = 0
    for name, o, bps, cols, rows, pad in F.pack_cases():
        pitch = cols * bps // 8 + pad
        if o != order or rows * pitch % word != 0:
            continue  # (rsx_synth_pack_rows writes whole words only)
        px = F.pack_case_rows(name, bps, cols, rows, oversized=True)
        want = synth.pack_rows(px, bps, order, pitch)
        got = F.model_pack(px & ((1 << bps) - 1), bps, order, pitch)
        assert np.array_equal(got[:rows * pitch], want), name
        assert not got[rows * pitch:].any()
        n += 1
    assert n >= 7


LJPEG_SHAPES = [  # rows, frame_w, n_comp, rpi (0: none), tables per component, fix16, kind
    (1, 1, 1, 0, ("full17",), False, "uniform16"),
    (5, 7, 1, 0, ("nikon14",), False, "noise14"),
    (6, 5, 2, 1, ("full17", "deep16"), False, "uniform16"),
    (7, 4, 3, 3, ("deep16", "full17", "deep16"), True, "uniform16"),
    (9, 3, 4, 4, ("full17",) * 4, True, "uniform16"),
    (4, 33, 2, 2, ("nikon14", "nikon14"), False, "noise14"),
]


def _shape_case(i):
    rows, fw, nc, rpi, tabs, fix16, kind = LJPEG_SHAPES[i]
    tile = F.ljpeg_tile("shape%d" % i, rows, fw * nc, kind)
    if fix16:
        tile[rows // 2, nc:] = tile[rows // 2, :-nc] ^ 0x8000  # -32768 present
    init = [1 << 13, 0, 65535, 777][:nc]
    return tile, nc, init, [F.TABLES[t] for t in tabs], rpi, fix16


@pytest.mark.parametrize("i", range(len(LJPEG_SHAPES)))
def test_ljpeg_model_equals_synth_in_jpeg_mode(i):
    tile, nc, init, tabs, rpi, fix16 = _shape_case(i)
    st, got, bits = F.model_ljpeg(tile, nc, init, tabs, rpi or tile.shape[0], fix16, F.TAIL_JPEG)
    want, want_bits = synth.ljpeg_encode_scan(tile, nc, init, tabs, rpi, fix16)
    assert st == F.OK and bytes(want) == got and bits == want_bits


@pytest.mark.parametrize("tail", (F.TAIL_JPEG, F.TAIL_VACUUMER))
@pytest.mark.parametrize("i", range(len(LJPEG_SHAPES)))
def test_ljpeg_model_decodes_through_the_oracle(oracle, i, tail):
    tile, nc, init, tabs, rpi, fix16 = _shape_case(i)
    rows, n = tile.shape
    st, data, _ = F.model_ljpeg(tile, nc, init, tabs, rpi or rows, fix16, tail)
    assert st == F.OK
    img = F.Img(np.zeros((rows + 2, n + 3), np.uint16))
    d = F.ljpeg_desc((1, 2, n, rows), img, nc, tabs, list(range(nc)), init, rpi or None, fix16)
    got = HostImage(n + 3, rows + 2)
    st, consumed = oracle.ljpeg(d, np.concatenate([np.frombuffer(data, np.uint8), EOI]), got)
    assert st == F.OK and consumed <= len(data)
    assert np.array_equal(got.pixels()[2:, 1:1 + n], tile)


def test_pack_model_decodes_through_the_oracle(oracle):
    n = 0
    for name, order, bps, cols, rows, pad in F.pack_cases():
        pitch = cols * bps // 8 + pad
        if rows * pitch % F.chunk_bytes(order) != 0:
            # the reader takes crop_h * pitch bytes: of a last MSB16 / MSB32 chunk cut short it
            # sees the bytes that lie inside them, which are not the stream's next ones
            continue
        n += 1
        px = F.pack_case_rows(name, bps, cols, rows)
        data = F.model_pack(px, bps, order, pitch)
        d = F.pack_desc(1, cols, rows, pitch, bps, order)
        got = HostImage(cols, rows + 1)
        assert oracle.unpack(d, data, got) == F.OK, name
        assert np.array_equal(got.pixels()[1:], px), name
    assert n >= 4 * 7
