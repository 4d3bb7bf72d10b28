"""The host build of the writers' core (rawspeed_amd/librsx_encode_host.so, rsx_encode_core.h)
against the numpy model of tests/encode_files.py, byte for byte over the whole case list, and the
statuses of include/rsx.h section 7 in their order.  Every output buffer carries a guard behind
its capacity and is compared whole."""
import ctypes as C

import numpy as np
import pytest

from rawspeed_amd import abi

import encode_files as F
from test_encode_model import LJPEG_SHAPES, _shape_case

GUARD = 0x5A


def _check_pack(name, order, bps, cols, rows, pad, crop_y=0, oversized=False):
    pitch = cols * bps // 8 + pad
    px = F.pack_case_rows(name, bps, cols, rows + crop_y, oversized)
    img = F.Img(px, pad=6)
    st, out, written, stream = F.host_pack(F.pack_desc(crop_y, cols, rows, pitch, bps, order), img)
    want = F.model_pack(px[crop_y:] & ((1 << bps) - 1), bps, order, pitch)
    assert st == F.OK and (written, stream) == (len(want), rows * pitch), name
    assert np.array_equal(out[:written], want), name
    assert (out[written:] == GUARD).all(), name


def test_pack_equals_the_model_over_the_case_list():
    for name, order, bps, cols, rows, pad in F.pack_cases():
        _check_pack(name, order, bps, cols, rows, pad)
        _check_pack(name + "_crop", order, bps, cols, rows, pad, crop_y=2, oversized=True)


@pytest.mark.parametrize("order", F.ORDERS)
def test_pack_past_one_lane_and_one_workgroup(order):
    block = F.pack_block_bytes()
    for bps, cols in ((14, 8 * 3), (12, block * 8 // 12 + 2), (16, block // 2 + 1), (1, 72)):
        _check_pack("wide_%d_%d" % (bps, cols), order, bps, cols, 3, 3, crop_y=1, oversized=True)


def test_pack_statuses_in_order():
    img = F.Img(np.zeros((4, 16), np.uint16))
    D = F.pack_desc

    def st(d, cap=1 << 20, im=img):
        return F.host_pack(d, im, cap)[0]
    assert st(D(0, 16, 4, 28, 14, abi.ORDER_MSB)) == F.OK
    # the size check comes first, whatever else is wrong
    assert st(abi.UnpackDesc(0, 0, 0, 1 << 17, 1 << 17, 99, 9)) == F.IO
    assert st(D(0, 0, 4, 28, 14, 9)) == F.INVALID_ARG            # empty tile before the order
    assert st(D(0, 16, 4, 28, 14, abi.ORDER_JPEG)) == F.INVALID_ARG
    assert st(D(0, 16, 4, 64, 32, abi.ORDER_MSB)) == F.UNSUPPORTED  # an F32 width
    assert st(D(0, 16, 4, 64, 17, abi.ORDER_MSB)) == F.UNSUPPORTED
    assert st(D(0, 16, 4, 64, 0, abi.ORDER_MSB)) == F.INVALID_ARG
    assert st(D(0, 15, 4, 28, 14, abi.ORDER_MSB)) == F.INVALID_ARG  # bits not whole bytes
    assert st(D(0, 16, 4, 27, 14, abi.ORDER_MSB)) == F.INVALID_ARG  # pitch below the row
    assert st(D(5, 16, 4, 28, 14, abi.ORDER_MSB)) == F.INVALID_ARG  # crop_y past the image
    assert st(D(0, 16, 4, 28, 14, abi.ORDER_MSB, crop_x=1)) == F.INVALID_ARG
    assert st(D(0, 2, 1, 3, 12, abi.ORDER_MSB)) == F.IO              # a stream below 4 bytes
    assert st(D(1, 16, 4, 28, 14, abi.ORDER_MSB)) == F.INVALID_ARG  # the writer's: rows that exist
    assert st(D(0, 16, 4, 29, 14, abi.ORDER_MSB), cap=115) == F.INVALID_ARG  # roundUp(116, 4)
    assert st(D(0, 16, 4, 29, 14, abi.ORDER_MSB), cap=116) == F.OK
    # a refused call writes nothing
    s, out, written, stream = F.host_pack(D(0, 16, 4, 29, 14, abi.ORDER_MSB), img, 115)
    assert (out == GUARD).all() and (written, stream) == (0, 0)


def _host_case(i, tail, tile_at=(0, 0), cap=None):
    tile, nc, init, tabs, rpi, fix16 = _shape_case(i)
    rows, n = tile.shape
    x, y = tile_at
    px = np.full((rows + y + 1, n + x + 2), 0x1234, np.uint16)
    px[y:y + rows, x:x + n] = tile
    img = F.Img(px, pad=4)
    d = F.ljpeg_desc((x, y, n, rows), img, nc, tabs, list(range(nc)), init, rpi or None, fix16)
    return tile, nc, init, tabs, rpi or rows, fix16, F.host_ljpeg(d, img, tail, cap)


@pytest.mark.parametrize("tail", (F.TAIL_JPEG, F.TAIL_VACUUMER))
@pytest.mark.parametrize("i", range(len(LJPEG_SHAPES)))
def test_ljpeg_equals_the_model(i, tail):
    for at in ((0, 0), (3, 2)):
        tile, nc, init, tabs, rpi, fix16, (st, out, r, hist) = _host_case(i, tail, at)
        mst, want, bits = F.model_ljpeg(tile, nc, init, tabs, rpi, fix16, tail)
        assert st == mst == F.OK == r.status
        assert (r.bytes, r.symbol_bits) == (len(want), bits)
        assert bytes(out[:r.bytes]) == want and (out[r.bytes:] == GUARD).all()
        assert np.array_equal(hist, F.model_histogram(tile, nc, init, rpi))


def test_ljpeg_equals_the_model_on_the_difference_lists():
    """the recorder's lists as one-row tiles of one component (init_pred 0)"""
    for name, tab, fix16, diffs in F.difference_lists():
        px = (np.cumsum(np.asarray(diffs, np.int64)) & 0xFFFF).astype(np.uint16)[None, :]
        img = F.Img(px)
        d = F.ljpeg_desc((0, 0, px.shape[1], 1), img, 1, [F.TABLES[tab]], [0], [0], None, fix16)
        for tail in (F.TAIL_JPEG, F.TAIL_VACUUMER):
            st, out, r, _ = F.host_ljpeg(d, img, tail)
            mst, want, bits = F.model_ljpeg_diffs(diffs, [F.TABLES[tab]], fix16, tail)
            assert st == mst == F.OK and bytes(out[:r.bytes]) == want, name
            assert r.symbol_bits == bits and (out[r.bytes:] == GUARD).all(), name


def test_ljpeg_data_dependent_statuses():
    # a category the table lacks: 16-bit noise under the Nikon tree
    tile = F.ljpeg_tile("missing", 3, 8, "uniform16")
    img = F.Img(tile)
    d = F.ljpeg_desc((0, 0, 8, 3), img, 2, [F.NIKON14], [0, 0], [0, 0], None)
    st, out, r, _ = F.host_ljpeg(d, img, F.TAIL_JPEG)
    assert st == F.BAD_HUFFMAN_CODE == r.status and (r.bytes, r.symbol_bits) == (0, 0)
    assert (out[-16:] == GUARD).all()
    # out_cap one byte short
    d = F.ljpeg_desc((0, 0, 8, 3), img, 2, [F.FULL17], [0, 0], [0, 0], 1)
    st, out, r, _ = F.host_ljpeg(d, img, F.TAIL_JPEG)
    assert st == F.OK
    n = int(r.bytes)
    st, out, r, _ = F.host_ljpeg(d, img, F.TAIL_JPEG, n - 1)
    assert st == F.INPUT_OVERFLOW == r.status and r.bytes == 0 and (out[n - 1:] == GUARD).all()
    st, out, r, _ = F.host_ljpeg(d, img, F.TAIL_JPEG, n)
    assert st == F.OK and r.bytes == n


def test_ljpeg_subset_statuses():
    img = F.Img(np.zeros((4, 12), np.uint16))
    v = img.view()

    def st(**kw):
        d = F.ljpeg_desc((0, 0, 12, 4), img, 2, [F.FULL17], [0, 0], [0, 0], None)
        for k, val in kw.items():
            setattr(d, k, val)
        return F.host().rsx_encode_host_ljpeg_subset(C.byref(d), C.byref(v))
    assert st() == F.OK
    assert st(mcu_w=2, mcu_h=2, n_comp=4) == F.UNSUPPORTED
    assert st(frame_w=7) == F.UNSUPPORTED   # a wider frame
    assert st(frame_h=5) == F.UNSUPPORTED   # a taller frame
    assert st(n_comp=3, mcu_w=3, frame_w=4) == F.OK
    assert st(tile_w=11, frame_w=6) == F.UNSUPPORTED  # a trailing partial MCU
