"""The baseline-DCT JPEG writer on the device (rsx_dctwrite_*, rawspeed_amd/csrc/rsx_dctwrite.hip)
through the C-ABI, held byte for byte against the recorded streams of Pillow's encoder
(tests/golden/dctwrite_ref.json) and, where a case has no recorded stream, against the numpy model
that tests/test_dctwrite_model.py pins to them.  Every output buffer starts as a guard pattern and
is compared whole."""
import numpy as np
import pytest
import torch

import dctwrite_files as D
import dng_jpeg_files as J
from oracle_lib import HostImage
from rawspeed_amd import abi, capi

pytestmark = pytest.mark.gpu

GUARD = 0x5A


@pytest.fixture(scope="module")
def gpu():
    import gpu_util
    return gpu_util.ctx()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(n):
    return torch.full((n,), GUARD, dtype=torch.uint8, device="cuda")


def _result(r):
    return int(r.status), int(r.bytes), int(r.scan_bytes), int(r.symbol_bits)


def _want(c, jfif=True, restart=None):
    """(stream, result tuple) by the model; the recorded stream where the case is as recorded"""
    stats = {}
    s = D.model_case(c, jfif=jfif, restart=restart, stats=stats)
    if jfif and restart is None and c.get("stream"):
        assert s == c["stream"]
    return s, (D.OK, len(s), stats["scan_bytes"], stats["symbol_bits"])


@pytest.mark.parametrize("c", D.cases(), ids=lambda c: c["name"])
def test_device_stream_is_the_recorded_stream(gpu, c):
    """host pointers, then device pointers with the output 3 bytes into its buffer and no APP0"""
    img = D.Img(c["pixels"], c["cpp"], pad=1)
    want, res = _want(c)
    n = len(want)
    out = np.full(n + 32, GUARD, np.uint8)
    calls = gpu.host_calls()
    st, r = gpu.dctwrite([abi.DctWriteTile(D.desc_of(c), out.ctypes.data, n)], img.view())
    assert gpu.host_calls() == calls + 1
    assert st == D.OK and _result(r[0]) == res
    assert out[:n].tobytes() == want and (out[n:] == GUARD).all()
    want, res = _want(c, jfif=False)
    assert want == J.without_marker(c["stream"], 0xE0)
    n = len(want)
    dimg, dout = _dev(img.buf), _guarded(3 + n + 32)
    st, r = gpu.dctwrite([abi.DctWriteTile(D.desc_of(c, jfif=False), dout.data_ptr() + 3, n)],
                         img.view(dimg.data_ptr()))
    assert st == D.OK and _result(r[0]) == res
    back = dout.cpu().numpy()
    assert back[3:3 + n].tobytes() == want
    assert (back[:3] == GUARD).all() and (back[3 + n:] == GUARD).all()


def _plan_of(cases, lead=3, gap=5):
    """all cases as the jobs of one plan: the images 16-byte aligned in one buffer, the streams at
    offsets that are no multiples of 4, `gap` guard bytes between them"""
    imgs, jobs, wants = [], [], []
    img_off, out_off = 0, lead
    for k, c in enumerate(cases):
        img = D.Img(c["pixels"], c["cpp"], pad=k % 3)
        want, res = _want(c, jfif=bool(k % 2 == 0))
        jobs.append(abi.dctwrite_job(D.desc_of(c, jfif=bool(k % 2 == 0)), img_off, out_off, len(want),
                                     img.dim_x, img.dim_y, img.cpp, img.pitch_bytes))
        wants.append((out_off, want, res))
        raw = img.buf.view(np.uint8).reshape(-1)
        imgs.append((img_off, raw))
        img_off += (len(raw) + 15) // 16 * 16
        out_off += len(want) + gap + (1 if (out_off + len(want) + gap) % 4 == 0 else 0)
    src = np.zeros(img_off, np.uint8)
    for off, raw in imgs:
        src[off:off + len(raw)] = raw
    return src, jobs, wants, out_off + 16


def test_one_plan_of_all_fixtures_twice(gpu):
    src, jobs, wants, total = _plan_of(D.cases())
    assert any(off % 4 for off, _, _ in wants)
    dsrc = _dev(src)
    plan = gpu.dctwrite_plan(jobs)
    runs = []
    for _ in range(2):
        dout = _guarded(total)
        plan.run(dsrc.data_ptr(), dout.data_ptr())
        rc, st, cons = plan.results()
        assert rc == D.OK and st == [D.OK] * len(jobs)
        assert cons == [len(w) for _, w, _ in wants]
        back = dout.cpu().numpy()
        keep = np.ones(total, bool)
        for k, (off, want, res) in enumerate(wants):
            got_st, r = plan.result(k)
            assert got_st == D.OK and _result(r) == res, k
            assert back[off:off + len(want)].tobytes() == want, k
            keep[off:off + len(want)] = False
        assert (back[keep] == GUARD).all()  # the guard pattern around every job's range
        runs.append(back)
    assert np.array_equal(runs[0], runs[1])
    plan.close()


@pytest.mark.parametrize("name", ["c444_noise_q100_ri5", "c420_40x37_noise_q95_ri2",
                                  "c422_40x21_noise_q60", "grey_noise_q100_ri1"])
def test_restart_intervals(gpu, name):
    """none, one MCU, one MCU row, and one that does not divide the MCU count"""
    c = D.case(name)
    hs, vs = D.SAMPLINGS[c["subsampling"]]
    mcus_x = -(-c["frame"][2] // (8 * hs))
    n_mcu = mcus_x * -(-c["frame"][3] // (8 * vs))
    odd = next(r for r in (7, 5, 3, 2) if n_mcu % r)
    img = D.Img(c["pixels"], c["cpp"])
    tiles, wants, outs = [], [], []
    for restart in (0, 1, mcus_x, odd):
        want, res = _want(c, restart=restart)
        out = np.full(len(want) + 8, GUARD, np.uint8)
        tiles.append(abi.DctWriteTile(D.desc_of(c, restart=restart), out.ctypes.data, len(want)))
        wants.append((want, res))
        outs.append(out)
    st, r = gpu.dctwrite(tiles, img.view())
    assert st == D.OK
    for (want, res), out, rr in zip(wants, outs, r):
        assert _result(rr) == res
        assert out[:len(want)].tobytes() == want and (out[len(want):] == GUARD).all()


def test_value_range_and_capacity_fail_their_tile_only(gpu):
    """three tiles of one image: the middle one reads a sample of 256, the last one is a byte short;
    the first is written.  Device pointers, then host pointers."""
    c = D.case("c420_smooth_q85_row")  # 64 x 40
    px = c["pixels"].astype(np.uint16)
    px[20, 40, 1] = 256
    img = D.Img(px, 3)
    frames = ([0, 0, 32, 40], [32, 0, 32, 40], [0, 8, 24, 16])
    parts = [dict(c, frame=f, stream=None) for f in frames]
    ok = dict(parts[1], pixels=c["pixels"])
    wants = [_want(parts[0])[0], _want(ok)[0], _want(parts[2])[0]]
    caps = [len(wants[0]), len(wants[1]), len(wants[2]) - 1]
    statuses = [D.OK, D.VALUE_RANGE, D.OVERFLOW]
    offs = [1, 1 + caps[0] + 7, 1 + caps[0] + 7 + caps[1] + 9]
    total = offs[2] + caps[2] + 32
    dimg, dout = _dev(img.buf), _guarded(total)
    tiles = [abi.DctWriteTile(D.desc_of(p), dout.data_ptr() + o, n) for p, o, n in zip(parts, offs, caps)]
    st, r = gpu.dctwrite(tiles, img.view(dimg.data_ptr()))
    assert st == D.TILE_ERRORS
    assert [int(x.status) for x in r] == statuses
    assert [int(x.bytes) for x in r] == [caps[0], 0, 0]
    back = dout.cpu().numpy()
    assert back[offs[0]:offs[0] + caps[0]].tobytes() == wants[0]
    keep = np.ones(total, bool)
    keep[offs[0]:offs[0] + caps[0]] = False
    assert (back[keep] == GUARD).all()  # nothing of the failed tiles, nothing past a cap
    outs = [np.full(n + 16, GUARD, np.uint8) for n in caps]
    tiles = [abi.DctWriteTile(D.desc_of(p), o.ctypes.data, n) for p, o, n in zip(parts, outs, caps)]
    st, r = gpu.dctwrite(tiles, img.view())
    assert st == D.TILE_ERRORS and [int(x.status) for x in r] == statuses
    assert outs[0][:caps[0]].tobytes() == wants[0] and (outs[0][caps[0]:] == GUARD).all()
    assert (outs[1] == GUARD).all() and (outs[2] == GUARD).all()
    # the same tiles with the sample in range and room for the last byte
    good = D.Img(c["pixels"], 3)
    outs = [np.full(len(w) + 16, GUARD, np.uint8) for w in wants]
    tiles = [abi.DctWriteTile(D.desc_of(p), o.ctypes.data, len(w)) for p, o, w in zip(parts, outs, wants)]
    st, r = gpu.dctwrite(tiles, good.view())
    assert st == D.OK
    for o, w in zip(outs, wants):
        assert o[:len(w)].tobytes() == w and (o[len(w):] == GUARD).all()


def test_refused_tile_and_mixed_pointers(gpu):
    c = D.case("size_17x16_c420")
    img = D.Img(c["pixels"], 3)
    want, res = _want(c)
    out = np.full(len(want), GUARD, np.uint8)
    bad = D.desc_of(c)
    bad.h_samp = 4
    o2 = np.full(64, GUARD, np.uint8)
    st, r = gpu.dctwrite([abi.DctWriteTile(D.desc_of(c), out.ctypes.data, len(want)),
                          abi.DctWriteTile(bad, o2.ctypes.data, 64)], img.view())
    assert st == D.TILE_ERRORS and [int(x.status) for x in r] == [D.OK, D.UNSUPPORTED]
    assert out.tobytes() == want and (o2 == GUARD).all()
    dout = _guarded(len(want))
    st, _ = gpu.dctwrite([abi.DctWriteTile(D.desc_of(c), dout.data_ptr(), len(want))], img.view())
    assert st == D.INVALID_ARG  # a host image with a device output


@pytest.mark.parametrize("c", D.cases(), ids=lambda c: c["name"])
def test_round_trip_on_the_device(gpu, c):
    """rsx_dctwrite, then rsx_dng_decompress_jpeg of the written tile: the image Pillow's decoder
    made of Pillow's stream; rsx_dng_jpeg_validate reports the geometry the tile was written with"""
    img = D.Img(c["pixels"], c["cpp"])
    d = D.desc_of(c, jfif=bool(len(c["name"]) % 2))
    cap = capi.dctwrite_bound(d, img.view())
    out = np.zeros(cap, np.uint8)
    st, r = gpu.dctwrite([abi.DctWriteTile(d, out.ctypes.data, cap)], img.view())
    assert st == D.OK
    stream = out[:int(r[0].bytes)]
    w, h = c["frame"][2], c["frame"][3]
    got = HostImage(w, h, c["cpp"])
    st, info = capi.dng_jpeg_validate(stream, (0, 0), got.view())
    hs, vs = D.SAMPLINGS[c["subsampling"]]
    n_mcu = -(-w // (8 * hs)) * -(-h // (8 * vs))
    assert st == D.OK
    assert (info.width, info.height, info.components, info.h_samp, info.v_samp) == (w, h, c["cpp"], hs, vs)
    assert info.colour_space == (J.GREY if c["cpp"] == 1 else J.YCBCR)
    assert info.restart_interval == c["restart"]
    assert info.n_segments == -(-n_mcu // (c["restart"] or n_mcu))
    rc, tst = gpu.dng_decompress_jpeg([stream], [(0, 0)], got.view())
    assert rc == D.OK and tst == [D.OK]
    assert J.sha(got.pixels()) == c["sha256"]


def test_a_scan_over_several_workgroups(gpu):
    """one interval of 1536 blocks: six workgroups of 256 blocks whose bit offsets need the carry
    of the three-phase scan, and a scratch stream of more than one workgroup of 1024 words.  The
    frame is a grey fixture tiled 4 x 8 (256 x 384); with an interval of 5 MCUs the same blocks make
    308 intervals, more than one word workgroup's search range."""
    c = D.tiled(D.case("grey_noise_q100_ri1"), 4, 8)
    img = D.Img(c["pixels"], 1)
    tiles, wants, outs = [], [], []
    for restart in (0, 5):
        want, res = _want(c, restart=restart)
        assert res[3] > 32 * 1024 * 3  # symbol bits: at least three word workgroups
        out = np.full(len(want) + 8, GUARD, np.uint8)
        tiles.append(abi.DctWriteTile(D.desc_of(c, restart=restart), out.ctypes.data, len(want)))
        wants.append((want, res))
        outs.append(out)
    st, r = gpu.dctwrite(tiles, img.view())
    assert st == D.OK
    for (want, res), out, rr in zip(wants, outs, r):
        assert _result(rr) == res
        assert out[:len(want)].tobytes() == want and (out[len(want):] == GUARD).all()
