"""The bad-pixel stage fused behind the decoders that produce bad pixels, in front of their one
download, against model-decode then model-fix.  Panasonic V4 (rsx_panasonic_v4_decompress_fixed):
the image equals tests/rw2_v4_files.py's decode put through tests/bad_pixels_files.py's fix, and the
map equals the model's.  DNG (rsx_dng_finish, rsx_dng_decompress_ljpeg_finish,
rsx_dng_decompress_uncompressed_finish): tests/dng_post_files.py's list and look-up, then the fix
on the positions they yield -- FixBadPixelsConstant and FixBadPixelsList in front of a look-up
table, so that the fix is seen to work on looked-up values."""
import numpy as np
import pytest
import torch

import bad_pixels_files as B
import cases as C
import dng_post_files as K
import rw2_v4_files as P4
from oracle_lib import HostImage
from rawspeed_amd import abi

pytestmark = pytest.mark.gpu

OK = abi.RSX_OK
FRAMES = ((28, 4), (126, 10), (560, 30))  # (the last: 1200 packets, more than one 0x4000 block)


@pytest.fixture(scope="module")
def gpu():
    import gpu_util
    return gpu_util.ctx()


def _stream(kind, split, w, h):
    rng = np.random.default_rng([11, w, h, split])
    if kind == "all":
        return np.zeros(P4.consumed(split, w, h), np.uint8)
    if kind == "few":
        return P4.random_stream(rng, split, w, h, "sparse" if w * h < 2000 else "uniform")
    # no zero pixel: every field nonzero, no scaling
    packets = [P4.pack_v4(rng.integers(1, 256, P4.N), (0, 0, 0, 0),
                          (int(rng.integers(0, 16)), int(rng.integers(0, 16))))
               for _ in range(w * h // P4.N)]
    return P4.stream_from_packets(split, packets)


@pytest.mark.parametrize("kind", ("none", "few", "all"))
@pytest.mark.parametrize("split", P4.SPLITS)
@pytest.mark.parametrize("w,h", FRAMES)
def test_v4_decode_then_fix(gpu, w, h, split, kind):
    data = _stream(kind, split, w, h)
    decoded, zeros = P4.model_decode(split, w, h, data)
    assert {"none": len(zeros) == 0, "few": 0 < len(zeros) < w * h, "all": len(zeros) == w * h}[kind]
    if kind == "all" and w * h > 2000:
        # (the model walks pixel by pixel, here through the whole frame for each of 16800: what a
        # frame with no good pixel becomes needs no walk -- 0 everywhere, every bit set)
        assert not decoded.any()
        want, wmap = decoded, B.bits_map(np.ones((h, w), bool))
        n_bad, n_fixed = w * h, min(w, (w + 15) // 32 * 32) * h
    else:
        want, wmap, n_bad, n_fixed = B.model_fix(decoded, True, [int(z) for z in zeros])
    for pitch in (None, 2 * w + 6):
        got = HostImage(w, h, pitch=pitch)
        st, r, m = gpu.panasonic_v4_decompress_fixed(split, 1, data, got.view())
        assert st == OK
        assert np.array_equal(got.pixels(), want)
        assert (got.u16()[:, w:] == 0xA5A5).all(), "the pitch padding was written"
        assert (r.n_bad, r.n_fixed, r.map_made) == (n_bad, n_fixed, int(wmap is not None))
        if wmap is None:  # (no zero pixel: the reference makes no map)
            assert m is None
        else:
            assert m.tobytes() == wmap.tobytes()
    # without the map, and the flag off: the plain decode
    got = HostImage(w, h)
    st, r, m = gpu.panasonic_v4_decompress_fixed(split, 1, data, got.view(), want_map=False)
    assert st == OK and m is None and np.array_equal(got.pixels(), want) and r.n_bad == n_bad
    got = HostImage(w, h)
    st, r, m = gpu.panasonic_v4_decompress_fixed(split, 0, data, got.view())
    assert st == OK and m is None and (r.n_bad, r.n_fixed, r.map_made) == (0, 0, 0)
    assert np.array_equal(got.pixels(), decoded)


def test_v4_fixed_equals_the_plain_call_then_the_stage(gpu):
    """the two-call route an application takes today: the list down, the fix on its own"""
    w, h, split = 126, 10, P4.SPLITS[1]
    data = _stream("few", split, w, h)
    plain = HostImage(w, h)
    st, n, bad = gpu.panasonic_v4_decompress(split, 1, data, plain.view(), w * h)
    assert st == OK and n > 0
    d, keep, map_out = abi.bad_pixels_desc(bad, (w, h))
    st, r = gpu.bad_pixels_fix(d, plain.view())
    assert st == OK and r.n_bad == n
    fused = HostImage(w, h)
    st, r2, m = gpu.panasonic_v4_decompress_fixed(split, 1, data, fused.view())
    assert st == OK and np.array_equal(fused.buf, plain.buf)
    assert m.tobytes() == map_out.tobytes() and (r2.n_bad, r2.n_fixed) == (r.n_bad, r.n_fixed)


def test_v4_fixed_refusals_write_nothing(gpu):
    w, h = 28, 4
    data = _stream("few", 0, w, h)
    got = HostImage(w, h)
    before = got.buf.copy()
    st, _, m = gpu.panasonic_v4_decompress_fixed(0, 1, data[:-1], got.view())
    assert st == abi.RSX_ERR_IO and np.array_equal(got.buf, before)
    odd = HostImage(w, h, pitch=2 * w + 3)
    st, _, m = gpu.panasonic_v4_decompress_fixed(0, 1, data, odd.view())
    assert st == abi.RSX_ERR_INVALID_ARG and (odd.buf == 0xA5).all()


# ---------------------------------------------------------------------------------------------
# DNG: the fix behind the opcode list and the look-up (rsx_dng_finish and the two fan-outs)
# ---------------------------------------------------------------------------------------------
DNG_CASES = {c[0]: c for c in K.file_cases()}


def _dng_model(img, cpp, crop, opcodes, table, bad_cap=1 << 16):
    """DP.apply, then the fix on its positions: (status, image, info, map or None)"""
    mst, after, info = K.apply(img, cpp, crop, opcodes, table)
    if mst != K.OK or not info["bad"] or len(info["bad"]) > bad_cap:
        return mst, after, info, None
    fixed, m, _, _ = B.model_fix(np.ascontiguousarray(after), True, info["bad"])
    return mst, fixed, info, m


def _check_map(m, want):
    if want is None:
        assert (m == 0xA5).all(), "a map was written although the reference makes none"
    else:
        assert m.tobytes() == want.tobytes()


@pytest.mark.parametrize("name", ["several", "trim_in_the_middle", "active_area_list", "bad_list",
                                  "rgb_bad_constant", "table_256", "bad_point_outside", "truncated_list"])
def test_dng_finish_on_the_reference_cases(gpu, name):
    case = DNG_CASES[name]
    _, img, cpp, opcodes, table, _ = case
    crop = K.case_crop(case)
    h, ws = img.shape
    mst, want, info, wmap = _dng_model(img, cpp, crop, opcodes, table)
    d, keep = abi.dng_post_desc(opcodes, table, crop)
    # host pointer
    out = HostImage(ws // cpp, h, cpp=cpp)
    out.pixels()[:] = img
    st, r, bad, m = gpu.dng_finish(d, out.view())
    assert st == mst
    assert np.array_equal(out.pixels(), want)
    assert (out.u16()[:, ws:] == 0xA5A5).all()
    if st == OK:
        assert (r.n_applied, r.crop(), bad) == (info["n_applied"], info["crop"], info["bad"])
    _check_map(m, wmap)
    # device pointer, a pitch wider than the row
    pitch = 2 * ws + 6
    host = np.full((h, pitch), 0xA5, np.uint8)
    host[:, :2 * ws] = img.view(np.uint8).reshape(h, -1)
    dev = torch.from_numpy(host.copy()).cuda()
    st, r, bad, m = gpu.dng_finish(d, abi.Image(dev.data_ptr(), pitch, ws // cpp, h, cpp, 1))
    back = dev.cpu().numpy()
    assert st == mst
    assert back[:, :2 * ws].tobytes() == want.tobytes() and (back[:, 2 * ws:] == 0xA5).all()
    _check_map(m, wmap)


def _list_and_table(rng, w, h, value, points):
    ops = [K.op_bad_constant(value),
           K.op_delta(10, (0, 0, h, w), rng.uniform(-0.01, 0.01, size=h).astype(np.float32)),
           K.op_bad_list(points, [(2, 3, 4, 6)])]
    return K.opcode_list(ops), np.sort(rng.integers(0, 65536, size=900)).astype(np.uint16)


def test_the_fix_sees_looked_up_values(gpu):
    """a FixBadPixelsConstant and a FixBadPixelsList in front of a look-up table: fixing before the
    look-up gives another image"""
    rng = np.random.default_rng(21)
    w, h = 70, 20
    img = rng.integers(0, 900, size=(h, w)).astype(np.uint16)
    img[::4, ::3] = 77
    opcodes, table = _list_and_table(rng, w, h, 77, [(1, 2), (19, 69), (7, 7)])
    crop = (0, 0, w, h)
    mst, want, info, wmap = _dng_model(img, 1, crop, opcodes, table)
    assert mst == K.OK and len(info["bad"]) > 20 and wmap is not None
    _, before_lookup, _ = K.apply(img, 1, crop, opcodes, None)
    other = K.apply(B.model_fix(before_lookup, True, info["bad"])[0], 1, crop, None, table)[1]
    assert not np.array_equal(other, want)
    d, keep = abi.dng_post_desc(opcodes, table, crop)
    out = HostImage(w, h)
    out.pixels()[:] = img
    st, r, bad, m = gpu.dng_finish(d, out.view())
    assert st == OK and np.array_equal(out.pixels(), want) and bad == info["bad"]
    _check_map(m, wmap)


def _unpack_tiles(img, tw, th):
    h, w = img.shape
    descs, datas = [], []
    for ty in range(0, h, th):
        for tx in range(0, w, tw):
            tile = np.zeros((th, tw), np.uint16)
            part = img[ty:ty + th, tx:tx + tw]
            tile[:part.shape[0], :part.shape[1]] = part
            datas.append(tile.view(np.uint8).reshape(-1))
            descs.append(abi.UnpackDesc(tx, ty, part.shape[1], part.shape[0], 2 * tw, 16, abi.ORDER_LSB))
    return descs, datas


def test_uncompressed_fan_out_with_the_fix(gpu):
    rng = np.random.default_rng(22)
    w, h = 70, 20
    img = rng.integers(0, 900, size=(h, w)).astype(np.uint16)
    img[::4, ::3] = 77
    opcodes, table = _list_and_table(rng, w, h, 77, [(1, 2), (19, 69)])
    crop = (0, 0, w, h)
    descs, datas = _unpack_tiles(img, 40, 12)
    mst, want, info, wmap = _dng_model(img, 1, crop, opcodes, table)
    d, keep = abi.dng_post_desc(opcodes, table, crop)
    got = HostImage(w, h)
    rc, st, r, bad, m = gpu.dng_decompress_uncompressed_finish(descs, datas, d, got.view())
    assert rc == OK and not any(st)
    assert np.array_equal(got.pixels(), want) and (got.u16()[:, w:] == 0xA5A5).all()
    assert (r.n_applied, bad) == (info["n_applied"], info["bad"])
    _check_map(m, wmap)
    # a list past bad_cap: the image as the _post call leaves it, unfixed
    post, fin = HostImage(w, h), HostImage(w, h)
    cap = len(info["bad"]) - 1
    prc, pst, pr, pbad = gpu.dng_decompress_uncompressed_post(descs, datas, d, post.view(), bad_cap=cap)
    rc, st, r, bad, m = gpu.dng_decompress_uncompressed_finish(descs, datas, d, fin.view(), bad_cap=cap)
    assert rc == prc == K.UNSUPPORTED and st == pst and r.n_bad == pr.n_bad == len(info["bad"])
    assert np.array_equal(fin.buf, post.buf) and not np.array_equal(fin.pixels(), want)
    _check_map(m, None)
    # a failing tile: the plain call's status and image, nothing applied
    descs[1] = abi.UnpackDesc(descs[1].crop_x, descs[1].crop_y, descs[1].crop_w, 12, 5, 16, abi.ORDER_LSB)
    plain, got = HostImage(w, h), HostImage(w, h)
    prc, pst = gpu.dng_decompress_uncompressed(descs, datas, plain.view())
    rc, st, r, bad, m = gpu.dng_decompress_uncompressed_finish(descs, datas, d, got.view())
    assert prc != OK and (rc, st) == (prc, pst) and np.array_equal(got.buf, plain.buf)
    _check_map(m, None)


def test_three_components_with_positions_are_refused_before_the_decode(gpu):
    rng = np.random.default_rng(23)
    w, h = 22, 12
    img = rng.integers(0, 65536, size=(h, 3 * w)).astype(np.uint16)
    descs, datas = _unpack_tiles(img, 3 * w, h)
    for i in range(len(descs)):  # (tiles in pixels, three samples each)
        descs[i] = abi.UnpackDesc(0, 0, w, h, 6 * w, 16, abi.ORDER_LSB)
    with_list = K.opcode_list([K.op_bad_list([(1, 2)])])
    without = K.opcode_list([K.op_table((0, 0, h, w), np.arange(256, dtype=np.uint16), planes=(0, 3))])
    for opcodes, verdict in ((with_list, K.UNSUPPORTED), (without, OK)):
        d, keep = abi.dng_post_desc(opcodes, None, (0, 0, w, h))
        got = HostImage(w, h, cpp=3)
        rc, st, r, bad, m = gpu.dng_decompress_uncompressed_finish(descs, datas, d, got.view())
        assert rc == verdict
        _check_map(m, None)
        if verdict == OK:
            assert np.array_equal(got.pixels(), K.apply(img, 3, (0, 0, w, h), opcodes, None)[1])
        else:
            assert (got.buf == 0xA5).all() and st == [-1]
        inplace = HostImage(w, h, cpp=3)
        inplace.pixels()[:] = img
        st2, r, bad, m = gpu.dng_finish(d, inplace.view())
        assert st2 == verdict
        if verdict != OK:
            assert np.array_equal(inplace.pixels(), img)


def _ljpeg_tiles(rng, W, H, tw, th):
    descs, datas = [], []
    for ty in range(2):
        for tx in range(2):
            d, data, _, _ = C.make_ljpeg_case(rng, img_w=W, img_h=H, cpp=1,
                                              tile=(tx * tw, ty * th, min(tw, W - tx * tw), min(th, H - ty * th)),
                                              mcu=(2, 1), frame=(tw // 2, th))
            descs.append(d)
            datas.append(data)
    return descs, datas


def test_ljpeg_fan_out_with_the_fix(gpu):
    rng = np.random.default_rng(24)
    W, H = 250, 61
    descs, datas = _ljpeg_tiles(rng, W, H, 128, 32)
    plain = HostImage(W, H)
    rc, st, _ = gpu.dng_decompress_ljpeg(descs, datas, plain.view())
    assert rc == OK
    decoded = plain.pixels().copy()
    value = int(np.bincount(decoded.reshape(-1)).argmax())
    ops = [K.op_bad_constant(value), K.op_bad_list([(0, 0), (60, 249), (30, 100)], [(10, 20, 14, 90)])]
    opcodes = K.opcode_list(ops)
    table = np.sort(rng.integers(0, 65536, size=1000)).astype(np.uint16)
    crop = (0, 0, W, H)
    mst, want, info, wmap = _dng_model(decoded, 1, crop, opcodes, table)
    assert mst == K.OK and wmap is not None and len(info["bad"]) > 4 * 70
    d, keep = abi.dng_post_desc(opcodes, table, crop)
    got = HostImage(W, H)
    rc, st, r, bad, m = gpu.dng_decompress_ljpeg_finish(descs, datas, d, got.view())
    assert rc == OK and not any(st)
    assert np.array_equal(got.pixels(), want) and (got.u16()[:, W:] == 0xA5A5).all()
    assert (r.n_applied, bad) == (info["n_applied"], info["bad"])
    _check_map(m, wmap)
    # a failing tile: the plain call, nothing applied
    datas[2] = datas[2][:len(datas[2]) // 3]
    plain, got = HostImage(W, H), HostImage(W, H)
    prc, pst, _ = gpu.dng_decompress_ljpeg(descs, datas, plain.view())
    rc, st, r, bad, m = gpu.dng_decompress_ljpeg_finish(descs, datas, d, got.view())
    assert prc != OK and (rc, st) == (prc, pst) and np.array_equal(got.buf, plain.buf)
    _check_map(m, None)


def test_dng_finish_past_bad_cap_leaves_the_image_unfixed(gpu):
    """rsx_dng_finish on a host and on a device pointer: the image as rsx_dng_post leaves it,
    RSX_ERR_UNSUPPORTED, the map untouched"""
    rng = np.random.default_rng(25)
    w, h = 70, 20
    img = rng.integers(0, 900, size=(h, w)).astype(np.uint16)
    img[::4, ::3] = 77
    opcodes, table = _list_and_table(rng, w, h, 77, [(1, 2), (19, 69)])
    crop = (0, 0, w, h)
    mst, want, info, _ = _dng_model(img, 1, crop, opcodes, table)
    cap = len(info["bad"]) - 1
    assert mst == K.OK and cap > 20
    d, keep = abi.dng_post_desc(opcodes, table, crop)
    post, fin = HostImage(w, h), HostImage(w, h)
    post.pixels()[:] = img
    fin.pixels()[:] = img
    pst, pr, pbad = gpu.dng_post(d, post.view(), bad_cap=cap)
    st, r, bad, m = gpu.dng_finish(d, fin.view(), bad_cap=cap)
    assert st == pst == K.UNSUPPORTED and r.n_bad == pr.n_bad == len(info["bad"])
    assert np.array_equal(fin.buf, post.buf) and not np.array_equal(fin.pixels(), want)
    _check_map(m, None)
    dev = torch.from_numpy(img.copy()).cuda()
    st, r, bad, m = gpu.dng_finish(d, abi.Image(dev.data_ptr(), 2 * w, w, h, 1, 1), bad_cap=cap)
    assert st == K.UNSUPPORTED and r.n_bad == len(info["bad"])
    assert np.array_equal(dev.cpu().numpy(), post.pixels())
    _check_map(m, None)


def test_ljpeg_finish_past_bad_cap_leaves_the_image_unfixed(gpu):
    rng = np.random.default_rng(26)
    W, H = 250, 61
    descs, datas = _ljpeg_tiles(rng, W, H, 128, 32)
    plain = HostImage(W, H)
    rc, st, _ = gpu.dng_decompress_ljpeg(descs, datas, plain.view())
    assert rc == OK
    decoded = plain.pixels().copy()
    opcodes = K.opcode_list([K.op_bad_list([(0, 0), (60, 249)], [(10, 20, 14, 90)])])
    table = np.sort(rng.integers(0, 65536, size=1000)).astype(np.uint16)
    crop = (0, 0, W, H)
    mst, want, info, _ = _dng_model(decoded, 1, crop, opcodes, table)
    cap = len(info["bad"]) - 1
    assert mst == K.OK and cap > 4 * 70
    d, keep = abi.dng_post_desc(opcodes, table, crop)
    post, fin = HostImage(W, H), HostImage(W, H)
    prc, pst, pr, pbad = gpu.dng_decompress_ljpeg_post(descs, datas, d, post.view(), bad_cap=cap)
    rc, st, r, bad, m = gpu.dng_decompress_ljpeg_finish(descs, datas, d, fin.view(), bad_cap=cap)
    assert rc == prc == K.UNSUPPORTED and st == pst and r.n_bad == pr.n_bad == len(info["bad"])
    assert np.array_equal(fin.buf, post.buf) and not np.array_equal(fin.pixels(), want)
    _check_map(m, None)
