"""The validations of the writers in the product library (no GPU needed): every branch in its order,
the reader's checks the same as rsx_unpack_validate and rsx_ljpeg_validate make them, the container
against the test writer's header, and the bound against the worst data there is."""
import ctypes as C

import numpy as np

from rawspeed_amd import abi, capi, synth

import encode_files as F


def test_pack_validate_is_the_readers_then_the_writers():
    lib = capi.lib()
    rng = np.random.default_rng(F.seed_of("pack_validate"))
    img = F.Img(np.zeros((6, 40), np.uint16))
    v = img.view()
    seen = set()
    for _ in range(4000):
        d = abi.UnpackDesc(int(rng.integers(-1, 3)), int(rng.integers(-1, 8)),
                           int(rng.choice([-1, 0, 8, 16, 40, 41])), int(rng.integers(-1, 8)),
                           int(rng.choice([-1, 0, 1, 3, 14, 28, 70, 80, 1 << 30])),
                           int(rng.choice([0, 1, 7, 8, 12, 14, 16])), int(rng.integers(-1, 6)))
        # the reader's input is the stream the writer makes: exactly the bytes the reader asks for
        stream = (d.crop_h & 0xFFFFFFFF) * (d.input_pitch_bytes & 0xFFFFFFFF)
        got = capi.encode_pack_validate(d, v, 1 << 62)
        want = lib.rsx_unpack_validate(C.byref(d), C.byref(v), stream)
        if want != F.OK:
            assert got == want, list(bytes(d))
        elif d.crop_y + d.crop_h > img.dim_y:
            assert got == F.INVALID_ARG
        else:
            assert got == F.OK
            need = F.round_up4(stream)
            assert capi.encode_pack_validate(d, v, need - 1) == F.INVALID_ARG
            assert capi.encode_pack_validate(d, v, need) == F.OK
        seen.add((want, got))
    assert {(F.OK, F.OK), (F.OK, F.INVALID_ARG), (F.IO, F.IO), (F.INVALID_ARG, F.INVALID_ARG)} <= seen
    d = F.pack_desc(0, 16, 4, 64, 32, abi.ORDER_MSB)
    assert capi.encode_pack_validate(d, v, 1 << 20) == F.UNSUPPORTED  # F32 widths
    d = F.pack_desc(0, 16, 4, 28, 14, abi.ORDER_MSB)
    assert capi.encode_pack_validate(None, v, 1 << 20) == F.INVALID_ARG
    assert capi.encode_pack_validate(d, None, 1 << 20) == F.INVALID_ARG
    odd = abi.Image(None, img.pitch + 1, img.dim_x, img.dim_y, 1, 1)
    assert capi.encode_pack_validate(d, odd, 1 << 20) == F.INVALID_ARG


def _desc(img, **kw):
    d = F.ljpeg_desc((0, 0, 12, 4), img, 2, [F.FULL17], [0, 0], [0, 0], None)
    for k, val in kw.items():
        setattr(d, k, val)
    return d


def test_ljpeg_validate_order():
    lib = capi.lib()
    img = F.Img(np.zeros((4, 12), np.uint16))
    v = img.view()

    def both(**kw):
        d = _desc(img, **kw)
        return capi.encode_ljpeg_validate(d, v), lib.rsx_ljpeg_validate(C.byref(d), C.byref(v), 0)
    assert both() == (F.OK, F.OK)
    # 1. what the reader says comes first, whatever the subset would say
    for kw in (dict(tile_w=0), dict(tile_x=-1), dict(tile_h=5), dict(frame_w=0),
               dict(mcu_w=5, n_comp=5), dict(n_comp=3), dict(rows_per_restart_interval=0),
               dict(frame_w=5), dict(n_tables=0), dict(mcu_w=2, mcu_h=2, n_comp=4, n_tables=9)):
        got, want = both(**kw)
        assert want != F.OK and got == want, kw
    # 2. the subset
    for kw in (dict(mcu_w=2, mcu_h=2, n_comp=4, frame_h=2), dict(frame_w=7), dict(frame_h=5),
               dict(tile_w=11, frame_w=6)):
        got, want = both(**kw)
        assert (got, want) == (F.UNSUPPORTED, F.OK), kw
    assert both(rows_per_restart_interval=1000) == (F.OK, F.OK)  # >= tile_h: no markers
    assert capi.encode_ljpeg_validate(None, v) == F.INVALID_ARG
    assert capi.encode_ljpeg_validate(_desc(img), None) == F.INVALID_ARG
    # the bound: 8 bytes a sample, 2 a marker, 8; 0 for what the validation refuses
    assert capi.encode_ljpeg_bound(_desc(img), v) == 8 * 48 + 8
    assert capi.encode_ljpeg_bound(_desc(img, rows_per_restart_interval=1), v) == 8 * 48 + 6 + 8
    assert capi.encode_ljpeg_bound(_desc(img, rows_per_restart_interval=3), v) == 8 * 48 + 2 + 8
    assert capi.encode_ljpeg_bound(_desc(img, frame_w=7), v) == 0
    assert F.host().rsx_encode_host_ljpeg_bound(C.byref(_desc(img)), C.byref(v)) == 8 * 48 + 8


def test_container_is_the_test_writers_header():
    img = F.Img(np.zeros((9, 24), np.uint16))
    v = img.view()
    for nc, rpi, tabs, index in ((1, None, [F.NIKON14], [0]), (2, 4, [F.FULL17, F.DEEP16], [0, 1]),
                                 (4, 1, [F.FULL17, F.NIKON14], [1, 0, 0, 1])):
        d = F.ljpeg_desc((0, 0, 24, 9), img, nc, tabs, index, [0] * nc, rpi)
        st, hdr = capi.encode_ljpeg_container(d, v, 14, 1234)
        assert st == F.OK
        keep = synth._table_ptrs(tabs)
        want = np.empty(1024, np.uint8)
        cs = (C.c_int * nc)(*index)
        n = synth.lib().rsx_synth_ljpeg_header(want.ctypes.data, 14, 24 // nc, 9, nc, cs, len(tabs),
                                               keep[2], keep[3], keep[4],
                                               rpi * (24 // nc) if rpi else 0, None, None)
        assert bytes(hdr) == bytes(want[:n])
        assert capi.encode_ljpeg_container(d, v, 14, 0, cap=len(hdr) - 1)[0] == F.INVALID_ARG
    # the largest layout there is: four components, four tables of 162 values (duplicates are
    # allowed by the reader's validation), a restart interval
    big = ([0, 0, 0, 0, 0, 0, 0, 162] + [0] * 8, [k % 17 for k in range(162)])
    d = F.ljpeg_desc((0, 0, 24, 9), img, 4, [big] * 4, [0, 1, 2, 3], [0] * 4, 2)
    assert capi.encode_ljpeg_validate(d, v) == F.OK
    st, hdr = capi.encode_ljpeg_container(d, v, 14, 0, cap=778)
    assert st == F.OK and len(hdr) == 2 + 22 + 4 * 183 + 6 + 16 == 778
    keep = synth._table_ptrs([big] * 4)
    want = np.empty(1024, np.uint8)
    n = synth.lib().rsx_synth_ljpeg_header(want.ctypes.data, 14, 6, 9, 4, (C.c_int * 4)(0, 1, 2, 3),
                                           4, keep[2], keep[3], keep[4], 2 * 6, None, None)
    assert bytes(hdr) == bytes(want[:n])
    assert capi.encode_ljpeg_container(d, v, 14, 0, cap=777)[0] == F.INVALID_ARG
    assert capi.encode_ljpeg_container(d, v, 17)[0] == F.INVALID_ARG
    d.frame_w = 7
    assert capi.encode_ljpeg_container(d, v, 14)[0] == F.UNSUPPORTED


def test_container_and_bytes_are_a_tile_the_oracle_takes(oracle):
    """the header names the scan's layout; the scan behind it decodes to the tile"""
    from oracle_lib import HostImage
    tile = F.ljpeg_tile("container", 5, 12, "noise14")
    img = F.Img(tile)
    d = F.ljpeg_desc((0, 0, 12, 5), img, 2, [F.NIKON14], [0, 0], [8192, 8192], 2)
    st, out, r, _ = F.host_ljpeg(d, img, F.TAIL_JPEG)
    st2, hdr = capi.encode_ljpeg_container(d, img.view(), 14, r.bytes)
    assert st == st2 == F.OK and bytes(hdr[:4]) == b"\xff\xd8\xff\xc3" and bytes(hdr[-3:]) == b"\x01\x00\x00"
    blob = np.concatenate([hdr, out[:r.bytes], np.array([0xFF, 0xD9] + [0] * 16, np.uint8)])
    got = HostImage(12, 5)
    st, consumed = oracle.ljpeg(d, blob[len(hdr):], got)
    assert st == F.OK and consumed <= r.bytes and np.array_equal(got.pixels(), tile)


def test_the_bound_holds_on_the_worst_data():
    """every symbol 32 bits (-32768 under fix16 with a 16-bit code), and every byte FF (31-bit
    symbols of ones under a code of sixteen ones), with a marker after every row"""
    wide = np.tile(np.array([[0x8000, 0]], np.uint16), (3, 20))
    wide[1] ^= 0x8000  # the first of a row against the row above
    st, data, bits = F.model_ljpeg(wide, 1, [0], [F.ALL_ONES], 3, True, F.TAIL_JPEG)
    assert bits == 32 * wide.size and len(data) == 5 * wide.size  # FF 00 FE 00 00 a symbol
    for tile, tab, fix16 in ((wide, F.ALL_ONES, True), (F.ff_tile(3, 40), F.ALL_ONES, False)):
        for rpi in (1, 3):
            init = [0]
            for tail in (F.TAIL_JPEG, F.TAIL_VACUUMER):
                st, data, bits = F.model_ljpeg(tile, 1, init, [tab], rpi, fix16, tail)
                bound = 8 * tile.size + 2 * (-(-3 // rpi) - 1) + 8
                assert st == F.OK and len(data) <= bound
                img = F.Img(tile)
                d = F.ljpeg_desc((0, 0, 40, 3), img, 1, [tab], [0], init, rpi, fix16)
                assert capi.encode_ljpeg_bound(d, img.view()) == bound
                hst, out, r, _ = F.host_ljpeg(d, img, tail)
                assert hst == F.OK and bytes(out[:r.bytes]) == data
    st, data, bits = F.model_ljpeg(F.ff_tile(3, 40), 1, [0], [F.ALL_ONES], 3, False, F.TAIL_JPEG)
    assert bits == 31 * 120 and data == b"\xff\x00" * (31 * 120 // 8)
