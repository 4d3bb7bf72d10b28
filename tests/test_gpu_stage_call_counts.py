"""rsx_ctx_host_calls over the stage calls (rsx_iiq_correct, rsx_bad_pixels_fix, rsx_dng_post,
rsx_dng_finish) and the calls that run a stage in front of their download: every entry point counts
once on the paths where it serves a call, a call refused by its validation included (the count is
taken in front of it), and not at all where the fused uncompressed call returns before it has
chosen a route.  What the calls compute is pinned by the suites of the stages; here every image is
32 x 8 or smaller and only the counter is read."""
import numpy as np
import pytest
import torch

import bad_pixels_files as B
import cases as C
import dng_post_files as K
import iiq_corr_files as Q
import iiq_files as F
import rw2_v4_files as P4
from oracle_lib import HostImage
from rawspeed_amd import abi

pytestmark = pytest.mark.gpu

OK = abi.RSX_OK
W, H = 32, 8


@pytest.fixture(scope="module")
def gpu():
    import gpu_util
    return gpu_util.ctx()


def _delta(gpu, call):
    """(what `call` returns, what it added to the counter)"""
    before = gpu.host_calls()
    got = call()
    return got, gpu.host_calls() - before


def _image(seed):
    return np.random.default_rng(seed).integers(1, 65536, size=(H, W)).astype(np.uint16)


def _host(img, cpp=1):
    out = HostImage(img.shape[1] // cpp, H, cpp=cpp)
    out.pixels()[:] = img
    return out


def _device(img, cpp=1):
    """(the tensor that keeps the memory, the view of it)"""
    dev = torch.from_numpy(img.copy()).cuda()
    return dev, abi.Image(dev.data_ptr(), img.shape[1] * 2, img.shape[1] // cpp, H, cpp, 1)


def test_iiq_correct(gpu):
    rng = np.random.default_rng(1)
    img = _image(1)
    payload = Q.ff_random(rng, (0, 0, W, H, 8, 4))
    d, keep = abi.iiq_corr([("ff", payload, 0)])
    st, n = _delta(gpu, lambda: gpu.iiq_correct(d, _host(img).view()))
    assert (st, n) == (OK, 1)
    dev, view = _device(img)
    st, n = _delta(gpu, lambda: gpu.iiq_correct(d, view))
    assert (st, n) == (OK, 1)
    none, keep0 = abi.iiq_corr([])
    st, n = _delta(gpu, lambda: gpu.iiq_correct(none, _host(img).view()))
    assert (st, n) == (OK, 1)
    short, keep1 = abi.iiq_corr([("ff", payload[:-1], 0)])
    st, n = _delta(gpu, lambda: gpu.iiq_correct(short, _host(img).view()))
    assert (st, n) == (abi.RSX_ERR_IO, 1)


def test_bad_pixels_fix(gpu):
    img = _image(2)
    positions = (B.pos(3, 2), B.pos(31, 7))
    d, keep, map_out = abi.bad_pixels_desc(positions, (W, H))
    (st, r), n = _delta(gpu, lambda: gpu.bad_pixels_fix(d, _host(img).view()))
    assert (st, r.n_bad, n) == (OK, 2, 1)
    dev, view = _device(img)
    (st, r), n = _delta(gpu, lambda: gpu.bad_pixels_fix(d, view))
    assert (st, r.n_bad, n) == (OK, 2, 1)
    empty, keep0, _ = abi.bad_pixels_desc((), (W, H))
    (st, r), n = _delta(gpu, lambda: gpu.bad_pixels_fix(empty, _host(img).view()))
    assert (st, r.n_bad, n) == (OK, 0, 1)
    outside, keep1, _ = abi.bad_pixels_desc((B.pos(W, 0),), (W, H))
    (st, r), n = _delta(gpu, lambda: gpu.bad_pixels_fix(outside, _host(img).view()))
    assert (st, n) == (abi.RSX_ERR_INVALID_ARG, 1)


def _dng_list():
    ops = [K.op_bad_constant(9), K.op_delta(10, (0, 0, H, W), np.full(H, 0.01, np.float32))]
    return K.opcode_list(ops), np.arange(0, 65536, 64, dtype=np.uint16)


@pytest.mark.parametrize("call", ["dng_post", "dng_finish"])
def test_dng_post_and_finish(gpu, call):
    img = _image(3)
    img[::3, ::5] = 9
    opcodes, table = _dng_list()
    d, keep = abi.dng_post_desc(opcodes, table, (0, 0, W, H))
    fn = getattr(gpu, call)
    got, n = _delta(gpu, lambda: fn(d, _host(img).view()))
    assert (got[0], n) == (OK, 1) and got[1].n_bad > 0
    dev, view = _device(img)
    got, n = _delta(gpu, lambda: fn(d, view))
    assert (got[0], n) == (OK, 1)


def test_dng_finish_refused_before_the_pass(gpu):
    """three components and positions: refused behind the count, before anything runs"""
    rgb = np.random.default_rng(4).integers(0, 65536, size=(H, 3 * 10)).astype(np.uint16)
    d, keep = abi.dng_post_desc(K.opcode_list([K.op_bad_list([(1, 2)])]), None, (0, 0, 10, H))
    out = _host(rgb, cpp=3)
    got, n = _delta(gpu, lambda: gpu.dng_finish(d, out.view()))
    assert (got[0], n) == (K.UNSUPPORTED, 1)
    assert np.array_equal(out.pixels(), rgb)


def test_phase_one_decompress_corrected(gpu):
    rng = np.random.default_rng(5)
    img = F.sample_image(rng, W, H)
    blob = F.iiq_file(F.encode(img, 3), W, rng, gap_max=5)
    raw, strips, _, _ = F.iiq_strips(blob)
    raw = np.frombuffer(raw, np.uint8)
    ops = [("ff", Q.ff_random(rng, (0, 0, W, H, 8, 4)), 0)]
    st, want = Q.apply(img, ops)
    for ops_given, expect in ((ops, want), ([], img)):
        d, keep = abi.iiq_corr(ops_given)
        out = HostImage(W, H)
        (st, rows), n = _delta(gpu, lambda: gpu.phase_one_decompress_corrected(raw, strips, d, out.view()))
        assert (st, n) == (OK, 1) and np.array_equal(out.pixels(), expect)


def test_panasonic_v4_decompress_fixed(gpu):
    w, h, split = 28, 4, P4.SPLITS[0]
    data = P4.random_stream(np.random.default_rng(6), split, w, h, "sparse")
    for zero_is_bad in (1, 0):
        out = HostImage(w, h)
        (st, r, m), n = _delta(gpu, lambda: gpu.panasonic_v4_decompress_fixed(split, zero_is_bad, data,
                                                                              out.view()))
        assert (st, n) == (OK, 1)


def _ljpeg_tiles():
    rng = np.random.default_rng(7)
    descs, datas = [], []
    for tx in range(2):
        d, data, _, _ = C.make_ljpeg_case(rng, img_w=W, img_h=H, cpp=1, tile=(tx * 16, 0, 16, H),
                                          mcu=(2, 1), frame=(8, H))
        descs.append(d)
        datas.append(data)
    return descs, datas


@pytest.mark.parametrize("call", ["dng_decompress_ljpeg_post", "dng_decompress_ljpeg_finish"])
def test_ljpeg_fan_out(gpu, call):
    descs, datas = _ljpeg_tiles()
    opcodes, table = _dng_list()
    d, keep = abi.dng_post_desc(opcodes, table, (0, 0, W, H))
    out = HostImage(W, H)
    got, n = _delta(gpu, lambda: getattr(gpu, call)(descs, datas, d, out.view()))
    assert (got[0], got[1], n) == (OK, [OK, OK], 1)


def _unpack_tiles(xs=(0, 16)):
    rng = np.random.default_rng(8)
    descs = [abi.UnpackDesc(x, 0, 16, H, 32, 16, abi.ORDER_LSB) for x in xs]
    datas = [rng.integers(0, 256, size=H * 32, dtype=np.uint8) for _ in xs]
    return descs, datas


@pytest.mark.parametrize("call", ["dng_decompress_uncompressed_post", "dng_decompress_uncompressed_finish"])
def test_uncompressed_fan_out(gpu, call):
    fn = getattr(gpu, call)
    opcodes, table = _dng_list()
    d, keep = abi.dng_post_desc(opcodes, table, (0, 0, W, H))
    # the fused path
    descs, datas = _unpack_tiles()
    out = HostImage(W, H)
    got, n = _delta(gpu, lambda: fn(descs, datas, d, out.view()))
    assert (got[0], got[1], n) == (OK, [OK, OK], 1)
    # a tile that does not validate: the plain call, counted by that call alone
    descs[1] = abi.UnpackDesc(16, 0, 16, H, 5, 16, abi.ORDER_LSB)
    out = HostImage(W, H)
    got, n = _delta(gpu, lambda: fn(descs, datas, d, out.view()))
    assert got[0] == abi.RSX_ERR_TILE_ERRORS and got[1][0] == OK and got[1][1] != OK and n == 1
    # tiles that do not tile the image: returned before the call has taken a route
    descs, datas = _unpack_tiles((0, 12))
    out = HostImage(W, H)
    got, n = _delta(gpu, lambda: fn(descs, datas, d, out.view()))
    assert (got[0], got[1], n) == (K.UNSUPPORTED, [-1, -1], 0)
    assert (out.buf == 0xA5).all()
