"""The writers on the device (rsx_encode_*, rawspeed_amd/csrc/rsx_encode_pack.hip and
rsx_encode_ljpeg.hip) through the C-ABI, held byte for byte against the host build of their core
(tests/encode_files.py, which tests/test_encode_host.py pins to the numpy model and
tests/test_encode_model.py to the reference's recorded bytes).  Every output buffer starts as a
guard pattern and is compared whole, the bytes in front of a plan job's out_offset included.
Random inputs are seeded from their names; random data runs under tables of all 17 categories, so
the only cases that end with a non-OK status are the two built to."""
import ctypes as C

import numpy as np
import pytest
import torch

import encode_files as F
from oracle_lib import HostImage
from rawspeed_amd import abi

pytestmark = pytest.mark.gpu

GUARD = 0x5A
EOI = np.array([0xFF, 0xD9] + [0] * 16, dtype=np.uint8)
TAILS = (F.TAIL_JPEG, F.TAIL_VACUUMER)


@pytest.fixture(scope="module")
def gpu():
    import gpu_util
    return gpu_util.ctx()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(n):
    return torch.full((n,), GUARD, dtype=torch.uint8, device="cuda")


# ---------------------------------------------------------------------------------------------
# pack
# ---------------------------------------------------------------------------------------------
def _check_pack(gpu, name, order, bps, cols, rows, pad, crop_y=1, lead=0):
    """host pointers and device pointers (the output `lead` bytes into its buffer) against the
    host build; then rsx_unpack_u16 on the result gives the masked image"""
    pitch = cols * bps // 8 + pad
    px = F.pack_case_rows(name, bps, cols, rows + crop_y, oversized=True)
    img = F.Img(px, pad=6)
    d = F.pack_desc(crop_y, cols, rows, pitch, bps, order)
    st, want, written, stream = F.host_pack(d, img)
    assert st == F.OK and stream == rows * pitch
    # host pointers
    out = np.full(len(want), GUARD, np.uint8)
    got = gpu.encode_pack_u16(d, img.view(), out.ctypes.data, written)
    assert got == (F.OK, written, stream), name
    assert np.array_equal(out, want), name
    # device pointers
    dimg, dout = _dev(img.buf), _guarded(lead + len(want))
    got = gpu.encode_pack_u16(d, img.view(dimg.data_ptr()), dout.data_ptr() + lead, written)
    assert got == (F.OK, written, stream), name
    back = dout.cpu().numpy()
    assert (back[:lead] == GUARD).all() and np.array_equal(back[lead:], want), name
    if stream % F.chunk_bytes(order) == 0:
        u = F.pack_desc(0, cols, rows, pitch, bps, order)
        dec = HostImage(cols, rows)
        assert gpu.unpack_u16(u, want[:written], dec.view()) == F.OK
        assert np.array_equal(dec.pixels(), px[crop_y:] & ((1 << bps) - 1)), name


@pytest.mark.parametrize("order", F.ORDERS)
def test_pack_case_list(gpu, order):
    for name, o, bps, cols, rows, pad in F.pack_cases():
        if o == order:
            _check_pack(gpu, name, order, bps, cols, rows, pad, lead=1 if rows > 1 else 0)


@pytest.mark.parametrize("order", F.ORDERS)
def test_pack_widths_of_words_and_past_one_workgroup(gpu, order):
    for words in (1, 2, 3, 5):  # output words of a row of 16-bit samples
        _check_pack(gpu, "words%d" % words, order, 16, 2 * words, 1, 0)
        _check_pack(gpu, "words%d_rows" % words, order, 16, 2 * words, 3, 4 if words & 1 else 0)
    block = F.pack_block_bytes()
    # one sample more than one workgroup's lanes cover, at 8 and at 12 bits
    _check_pack(gpu, "block8", order, 8, block + 1, 2, 3)
    _check_pack(gpu, "block12", order, 12, block * 8 // 12 + 2, 2, 0, lead=3)
    _check_pack(gpu, "block14", order, 14, (2 * block * 8 // 14 + 8) // 8 * 8, 3, 1)


def test_pack_plan_of_mixed_jobs(gpu):
    """jobs of every order in one launch, odd output offsets, one job refused: the whole output
    buffer against the host build's bytes in a guard pattern"""
    imgs, jobs, wants = [], [], []
    img_off, out_off = 0, 3
    for k, (order, bps, cols, rows, pad) in enumerate(
            [(abi.ORDER_MSB, 14, 72, 5, 2), (abi.ORDER_LSB, 12, 6, 1, 0),
             (abi.ORDER_MSB32, 10, 2000, 3, 7), (abi.ORDER_MSB16, 7, 8, 9, 1),
             (abi.ORDER_LSB, 16, 33, 2, 0)]):
        pitch = cols * bps // 8 + pad
        img = F.Img(F.pack_case_rows("plan%d" % k, bps, cols, rows + 2, True), pad=2 * (k % 3))
        d = F.pack_desc(2, cols, rows, pitch, bps, order)
        st, want, written, _ = F.host_pack(d, img)
        assert st == F.OK
        bad = k == 3
        if bad:
            d = F.pack_desc(3, cols, rows, pitch, bps, order)  # a row past the image
        jobs.append(abi.encode_pack_job(d, img_off, out_off, written, img.dim_x, img.dim_y, 1,
                                        img.pitch))
        wants.append((out_off, None if bad else want[:written]))
        imgs.append((img_off, img.buf))
        img_off += (len(img.buf) + 15) // 16 * 16
        out_off += written + 5
    src = np.zeros(img_off, np.uint8)
    for off, buf in imgs:
        src[off:off + len(buf)] = buf
    want = np.full(out_off + 16, GUARD, np.uint8)
    for off, w in wants:
        if w is not None:
            want[off:off + len(w)] = w
    dsrc, dout = _dev(src), _guarded(len(want))
    plan = gpu.encode_pack_plan(jobs)
    plan.run(dsrc.data_ptr(), dout.data_ptr())
    rc, st, cons = plan.results()
    assert rc == F.INVALID_ARG and st == [0, 0, 0, F.INVALID_ARG, 0]
    assert cons == [0 if w is None else len(w) for _, w in wants]
    assert np.array_equal(dout.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------
# lossless JPEG
# ---------------------------------------------------------------------------------------------
def _place(tile, at=(0, 0), pad=4):
    rows, n = tile.shape
    x, y = at
    px = np.full((rows + y + (1 if y else 0), n + x + (2 if x else 0)), 0x1234, np.uint16)
    px[y:y + rows, x:x + n] = tile
    return F.Img(px, pad=pad)


def _check_ljpeg(gpu, oracle, tile, nc, tabs, index, init, rpi, fix16, tail, at=(0, 0)):
    """host pointers and device pointers against the host build; then rsx_ljpeg_decode gives the
    tile back and consumes what the oracle consumes"""
    rows, n = tile.shape
    img = _place(tile, at)
    d = F.ljpeg_desc((at[0], at[1], n, rows), img, nc, tabs, index, init, rpi, fix16)
    st, want, r, _ = F.host_ljpeg(d, img, tail)
    assert st == F.OK
    cap = len(want) - 16
    out = np.full(len(want), GUARD, np.uint8)
    st, g = gpu.encode_ljpeg(d, img.view(), tail, out.ctypes.data, cap)
    assert (st, g.status, g.bytes, g.symbol_bits) == (F.OK, F.OK, r.bytes, r.symbol_bits)
    assert np.array_equal(out, want)
    dimg, dout = _dev(img.buf), _guarded(len(want) + 1)
    st, g = gpu.encode_ljpeg(d, img.view(dimg.data_ptr()), tail, dout.data_ptr() + 1, cap)
    assert (st, g.status, g.bytes, g.symbol_bits) == (F.OK, F.OK, r.bytes, r.symbol_bits)
    back = dout.cpu().numpy()
    assert back[0] == GUARD and np.array_equal(back[1:], want)
    data = np.concatenate([want[:r.bytes], EOI])
    dec, ref = HostImage(img.dim_x, img.dim_y), HostImage(img.dim_x, img.dim_y)
    got = gpu.ljpeg_decode(d, data, dec.view())
    assert got == oracle.ljpeg(d, data, ref) and got[0] == F.OK and got[1] <= r.bytes
    assert np.array_equal(dec.pixels()[at[1]:at[1] + rows, at[0]:at[0] + n], tile)
    return r


@pytest.mark.parametrize("tail", TAILS)
@pytest.mark.parametrize("nc", (1, 2, 3, 4))
def test_ljpeg_components_tables_and_small_tiles(gpu, oracle, nc, tail):
    per_comp = [F.FULL17, F.DEEP16, F.FULL17, F.DEEP16][:nc]
    init = [1 << 13, 0, 65535, 777][:nc]
    for mcus_w, rows in ((1, 1), (2, 1), (1, 3), (7, 7)):
        name = "small_%d_%d_%d" % (nc, mcus_w, rows)
        tile = F.ljpeg_tile(name, rows, mcus_w * nc, "uniform16")
        for rpi in (None, 1, 3):
            _check_ljpeg(gpu, oracle, tile, nc, [F.FULL17], [0] * nc, init, rpi, False, tail)
            _check_ljpeg(gpu, oracle, tile, nc, per_comp, list(range(nc)), init, rpi, False, tail,
                         at=(3, 2))


@pytest.mark.parametrize("tail", TAILS)
def test_ljpeg_workgroup_edges(gpu, oracle, tail):
    """a job of exactly one, of one-plus-one-sample and of three-plus-one-sample workgroups' worth;
    a tile inside a larger image; intervals that do not divide the height"""
    run = F.ljpeg_run()
    for n in (run, run + 1, 3 * run + 1):
        tile = F.ljpeg_tile("edge%d" % n, 1, n, "uniform16")
        _check_ljpeg(gpu, oracle, tile, 1, [F.FULL17], [0], [0x8000], None, False, tail)
    tile = F.ljpeg_tile("edge_rows", 7, (run + 2) // 2 * 2, "uniform16")
    _check_ljpeg(gpu, oracle, tile, 2, [F.DEEP16, F.FULL17], [0, 1], [5, 6], 3, False, tail, at=(4, 1))
    _check_ljpeg(gpu, oracle, tile, 2, [F.DEEP16], [0, 0], [5, 6], 1, False, tail)
    sensor = F.ljpeg_tile("edge_sensor", 9, 3 * run // 2, "noise14")
    _check_ljpeg(gpu, oracle, sensor, 2, [F.NIKON14], [0, 0], [8192, 8192], 4, False, tail)


@pytest.mark.parametrize("tail", TAILS)
def test_ljpeg_ff_runs_and_widest_symbols(gpu, oracle, tail):
    run = F.ljpeg_run()
    # every stream byte FF: 31-bit symbols, so a workgroup's range ends inside a byte, on a byte
    # and on a word in turn, and FFs straddle the words two workgroups share
    for rows, n in ((1, 8), (1, 33), (2, run + 5), (3, 2 * run)):
        r = _check_ljpeg(gpu, oracle, F.ff_tile(rows, n), 1, [F.ALL_ONES], [0], [0], None, False, tail)
        assert r.bytes >= 2 * (31 * rows * n // 8)
    for k in (7, 8, 9, 12):
        _check_ljpeg(gpu, oracle, F.ff_tile(2, run + 3, k), 1, [F.ALL_ONES], [0], [0], 1, False, tail)
    # -32768 with and without fix16; under DEEP16 with fix16 its symbol is 32 bits
    tile = F.ljpeg_tile("min", 3, run + 7, "uniform16")
    tile[:, 1::3] = tile[:, 0:-1:3] ^ 0x8000
    for fix16 in (False, True):
        r = _check_ljpeg(gpu, oracle, tile, 1, [F.DEEP16], [0], [0], 2, fix16, tail)
    wide = np.tile(np.array([[0x8000, 0]], np.uint16), (1, run))  # 32 bits a symbol throughout
    r = _check_ljpeg(gpu, oracle, wide, 1, [F.DEEP16], [0], [0], None, True, tail)
    assert r.symbol_bits == 32 * wide.size


def test_ljpeg_plan_of_mixed_jobs_twice(gpu):
    """three jobs of different geometry, the middle one lacking a category, and one whose out_cap
    is one byte short; the same plan twice on one stream writes the same bytes (that a run zeroes
    the scratch words two workgroups share is test_ljpeg_scratch_words_are_zeroed_by_the_run's)"""
    run = F.ljpeg_run()
    specs = [("p0", 5, 2 * run + 3, 1, F.FULL17, "uniform16", None, F.TAIL_VACUUMER, 0),
             ("p1", 3, 40, 2, F.NIKON14, "uniform16", 1, F.TAIL_JPEG, 0),   # lacks 15 and 16
             ("p2", 9, run // 2, 4, F.DEEP16, "uniform16", 2, F.TAIL_JPEG, 0),
             ("p3", 4, 66, 3, F.FULL17, "uniform16", 3, F.TAIL_JPEG, -1)]   # one byte short
    jobs, imgs, wants, expect = [], [], [], []
    img_off, out_off = 0, 1
    for name, rows, n, nc, tab, kind, rpi, tail, short in specs:
        tile = F.ljpeg_tile(name, rows, n // nc * nc, kind)
        img = _place(tile, (2, 1))
        d = F.ljpeg_desc((2, 1, tile.shape[1], rows), img, nc, [tab], [0] * nc, [9] * nc, rpi)
        st, want, r, _ = F.host_ljpeg(d, img, tail)
        if st == F.OK and short:
            cap = int(r.bytes) + short
            st, want, r, _ = F.host_ljpeg(d, img, tail, cap)
        else:
            cap = len(want) - 16
        jobs.append(abi.encode_ljpeg_job(d, tail, img_off, out_off, cap, img.dim_x, img.dim_y, 1,
                                         img.pitch))
        expect.append((st, int(r.bytes), int(r.symbol_bits)))
        wants.append((out_off, cap, want[:r.bytes]))
        imgs.append((img_off, img.buf))
        img_off += (len(img.buf) + 15) // 16 * 16
        out_off += cap + 3
    assert [e[0] for e in expect] == [F.OK, F.BAD_HUFFMAN_CODE, F.OK, F.INPUT_OVERFLOW]
    src = np.zeros(img_off, np.uint8)
    for off, buf in imgs:
        src[off:off + len(buf)] = buf
    dsrc = _dev(src)
    plan = gpu.encode_ljpeg_plan(jobs)
    for _ in range(2):
        dout = _guarded(out_off + 16)
        plan.run(dsrc.data_ptr(), dout.data_ptr())
        rc, st, cons = plan.results()
        assert rc == F.INPUT_OVERFLOW and st == [e[0] for e in expect]
        assert cons == [e[1] for e in expect]
        back = dout.cpu().numpy()
        keep = np.ones(len(back), bool)
        for k, (off, cap, want) in enumerate(wants):
            rs, r = plan.result(k)
            assert rs == F.OK and (r.status, r.bytes, r.symbol_bits) == expect[k]
            if expect[k][0] == F.OK:
                assert np.array_equal(back[off:off + len(want)], want), k
                keep[off:off + len(want)] = False
            else:
                keep[off:off + cap] = False  # may hold anything up to out_cap
        assert (back[keep] == GUARD).all()


def test_ljpeg_scratch_words_are_zeroed_by_the_run(gpu):
    """One plan on three images of one geometry in turn, through the base pointer of the run: first
    data whose every stream bit is 1 (31-bit symbols of ones: every scratch word is left all ones),
    then data whose every stream bit is 0 (difference 0 under a code of one 0 bit), then noise.  A
    word two workgroups share that the run did not zero itself would keep the ones of the run
    before.  Workgroups end inside words (run + 5 symbols of 1 and of 31 bits)."""
    run = F.ljpeg_run()
    rows, n = 3, 2 * run + 5
    ones = F.ff_tile(rows, n)
    zeros = np.zeros((rows, n), np.uint16)
    noise = F.ljpeg_tile("scratch_noise", rows, n, "uniform16")
    for tail in TAILS:
        for rpi in (None, 2):
            imgs = [F.Img(t) for t in (ones, zeros, noise, ones)]
            d = F.ljpeg_desc((0, 0, n, rows), imgs[0], 1, [F.ALL_ONES], [0], [0], rpi)
            wants = [F.host_ljpeg(d, im, tail) for im in imgs]
            cap = len(wants[0][1]) - 16
            plan = gpu.encode_ljpeg_plan([abi.encode_ljpeg_job(d, tail, 0, 1, cap, n, rows, 1,
                                                               imgs[0].pitch)])
            for im, (st, want, r, _) in zip(imgs, wants):
                assert st == F.OK
                dimg, dout = _dev(im.buf), _guarded(1 + len(want))
                plan.run(dimg.data_ptr(), dout.data_ptr())
                rc, sts, cons = plan.results()
                assert rc == F.OK and cons == [int(r.bytes)]
                back = dout.cpu().numpy()
                assert back[0] == GUARD and np.array_equal(back[1:], want)
            assert wants[1][2].symbol_bits == rows * n  # a 0 bit a sample
            if rpi is None:
                assert not wants[1][1][:wants[1][2].bytes - 1].any()


def test_ljpeg_histogram_and_its_table(gpu):
    run = F.ljpeg_run()
    tile = F.ljpeg_tile("hist", 6, 4 * (run // 2 + 3), "noise14")
    img = _place(tile, (1, 1))
    init = [8192] * 4
    d = F.ljpeg_desc((1, 1, tile.shape[1], 6), img, 4, [F.NIKON14], [0] * 4, init, 4)
    want = F.model_histogram(tile, 4, init, 4)
    st, got = gpu.encode_ljpeg_histogram(d, img.view())
    assert st == F.OK and np.array_equal(got, want)
    dimg = _dev(img.buf)
    st, got = gpu.encode_ljpeg_histogram(d, img.view(dimg.data_ptr()))
    assert st == F.OK and np.array_equal(got, want)
    assert int(got.sum()) == tile.size and got[:, 15:].sum() == 0
    # a table per component from its counts: no more bits than under the Nikon tree
    from rawspeed_amd import capi
    tabs = []
    for c in range(4):
        st, t = capi.encode_huff_from_histogram(got[c])
        assert st == F.OK
        tabs.append(F.table_of(t))
    out = np.empty(1 << 20, np.uint8)  # (held in a name: the call writes through its address)
    nikon = gpu.encode_ljpeg(d, img.view(), F.TAIL_JPEG, out.ctypes.data, out.size)
    d2 = F.ljpeg_desc((1, 1, tile.shape[1], 6), img, 4, tabs, [0, 1, 2, 3], init, 4)
    own = gpu.encode_ljpeg(d2, img.view(), F.TAIL_JPEG, out.ctypes.data, out.size)
    assert nikon[0] == own[0] == F.OK
    assert own[1].symbol_bits <= nikon[1].symbol_bits
    assert own[1].symbol_bits == sum(F.cost_bits(tabs[c], got[c]) for c in range(4))
