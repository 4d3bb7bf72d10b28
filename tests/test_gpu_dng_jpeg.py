"""Lossy-JPEG DNG tiles on the device (rsx_dng_jpeg_*, rawspeed_amd/csrc/rsx_dng_jpeg.hip) through
the C-ABI: the host-pointer call and device plans against what libjpeg-turbo's default decoder made
of the committed streams (tests/golden/dng_jpeg_ref.json, recorded through Pillow; nothing here
imports it).  An undamaged fixture must come back RSX_OK and equal -- a refusal does not pass; a
damaged one is either refused with the image untouched or equal to what was recorded."""
import functools

import numpy as np
import pytest
import torch

import dng_jpeg_files as J
from oracle_lib import HostImage
from rawspeed_amd import abi

pytestmark = pytest.mark.gpu
FILL = 0xA5A5


@pytest.fixture(scope="module")
def gpu():
    import gpu_util
    return gpu_util.ctx()


@functools.lru_cache(maxsize=None)
def _frame(name):
    """(status, the whole frame) of a fixture by the model, held against the recorded hash once"""
    c = J.case(name)
    st, got = J.model_decode(c["stream"], c["cpp"])
    assert st == J.OK and J.sha(got) == c["sha256"], name
    got.setflags(write=False)
    return got


def _host(gpu, tiles, dim_x, dim_y, cpp, pad=6):
    """tiles: [(stream, off_x, off_y)] of one image -> (rc, statuses, the samples); the pitch
    padding must stay as it was"""
    pitch = (2 * cpp * dim_x + 15) // 16 * 16 + pad
    img = HostImage(dim_x, dim_y, cpp, pitch=pitch, is_cfa=False)
    rc, st = gpu.dng_decompress_jpeg([t[0] for t in tiles], [(t[1], t[2]) for t in tiles], img.view())
    rows = img.buf.reshape(dim_y, pitch)
    assert (rows[:, 2 * cpp * dim_x:] == 0xA5).all(), "the pitch padding was written"
    return rc, st, img.pixels().copy()


def _want(frames, dim_x, dim_y, cpp):
    """frames: [(frame or None, off_x, off_y)] -> the image with the windows pasted"""
    want = np.full((dim_y, cpp * dim_x), FILL, np.uint16)
    for frame, ox, oy in frames:
        if frame is not None:
            J.paste(want, frame, ox, oy, cpp)
    return want


# --------------------------------------------------------------------------- every fixture
@pytest.mark.parametrize("name", [c["name"] for c in J.cases()])
def test_fixture_is_decoded_and_equal(gpu, name):
    c = J.case(name)
    w, h, cpp = c["width"], c["height"], c["cpp"]
    rc, st, got = _host(gpu, [(c["stream"], 1, 2)], w + 2, h + 3, cpp)
    assert (rc, st) == (J.OK, [J.OK]), (name, rc, st)
    window = got[2:2 + h, cpp:cpp * (1 + w)]
    assert J.sha(window) == c["sha256"], name
    assert np.array_equal(got, _want([(_frame(name), 1, 2)], w + 2, h + 3, cpp)), \
        "samples around the window were written"


@pytest.mark.parametrize("c", J.damaged() + J.forged(), ids=lambda c: c["name"])
def test_damaged_is_refused_or_equal(gpu, c):
    cpp = c["cpp"]
    w, h = (c["width"], c["height"]) if c["sha256"] else (64, 96)
    rc, st, got = _host(gpu, [(c["stream"], 1, 1)], w + 2, h + 2, cpp)
    if st[0] != J.OK:
        assert rc == J.TILE_ERRORS
        assert (got == FILL).all(), "a refused tile wrote into the image"
    else:
        assert c["sha256"] is not None, "libjpeg raised, the device decoded"
        assert rc == J.OK and J.sha(got[1:1 + h, cpp:cpp * (1 + w)]) == c["sha256"]
        got[1:1 + h, cpp:cpp * (1 + w)] = FILL
        assert (got == FILL).all()


def test_overshoot_fork_is_the_saturating_one(gpu):
    """the forged stream that leaves the sample range by more than 512 decodes, as libjpeg-turbo's
    SIMD code does; the one that leaves 16 bits is refused"""
    by = {c["name"]: c for c in J.forged()}
    c = by["overshoot_moderate"]
    rc, st, got = _host(gpu, [(c["stream"], 0, 0)], c["width"], c["height"], 1)
    assert (rc, st) == (J.OK, [J.OK]) and J.sha(got) == c["sha256"]
    c = by["overshoot_extreme"]
    rc, st, got = _host(gpu, [(c["stream"], 0, 0)], 16, 8, 1)
    assert st == [J.UNSUPPORTED] and (got == FILL).all()


# --------------------------------------------------------------------------------- windows
@pytest.mark.parametrize("name,off,dim", [
    ("grey_33x50", (5, 7), (21, 31)), ("grey_33x50", (3, 1), (36, 20)),
    ("420_47x71", (3, 5), (29, 37)), ("422_47x71", (7, 3), (54, 41)),
    ("444_48x72", (1, 9), (30, 80)), ("420_17x17", (15, 15), (16, 16)),
    ("restart3_420_64x96", (9, 11), (70, 50)),
])
def test_window_cut_by_the_image(gpu, name, off, dim):
    c = J.case(name)
    rc, st, got = _host(gpu, [(c["stream"], off[0], off[1])], dim[0], dim[1], c["cpp"], pad=2)
    assert (rc, st) == (J.OK, [J.OK])
    want = _want([(_frame(name), off[0], off[1])], dim[0], dim[1], c["cpp"])
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]


# --------------------------------------------------------------------------------- batches
GRID = ["444_48x72", "420_47x71", "422_47x71", "444_48x72"]


def _grid(names):
    return [(n, 48 * (k % 2), 72 * (k // 2)) for k, n in enumerate(names)]


def test_batch_of_ragged_tiles(gpu):
    tiles = _grid(GRID)
    rc, st, got = _host(gpu, [(J.case(n)["stream"], x, y) for n, x, y in tiles], 80, 100, 3)
    assert (rc, st) == (J.OK, [J.OK] * 4)
    want = _want([(_frame(n), x, y) for n, x, y in tiles], 80, 100, 3)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]


def test_batch_with_a_damaged_tile(gpu):
    bad = next(c for c in J.damaged() if c["name"].endswith("restart3_420_64x96/rst_renumbered"))
    tiles = _grid(GRID)
    streams = [J.case(n)["stream"] for n, _, _ in tiles]
    streams[2] = bad["stream"]
    rc, st, got = _host(gpu, [(s, x, y) for s, (_, x, y) in zip(streams, tiles)], 80, 100, 3)
    assert rc == J.TILE_ERRORS and [s == J.OK for s in st] == [True, True, False, True], st
    want = _want([(None if k == 2 else _frame(n), x, y) for k, (n, x, y) in enumerate(tiles)], 80, 100, 3)
    assert np.array_equal(got, want), "the damaged tile's window, or a neighbour, is wrong"


def test_batch_that_fills_the_image(gpu):
    """four tiles that tile the image exactly: one rectangle comes back"""
    tiles = _grid(["444_48x72"] * 4)
    rc, st, got = _host(gpu, [(J.case(n)["stream"], x, y) for n, x, y in tiles], 96, 144, 3, pad=0)
    assert (rc, st) == (J.OK, [J.OK] * 4)
    assert np.array_equal(got, _want([(_frame(n), x, y) for n, x, y in tiles], 96, 144, 3))


def test_mixed_grey_tiles_with_their_own_tables(gpu):
    tiles = [("grey_8x8", 0, 0), ("grey_33x50", 9, 1), ("optimize_grey_24x40", 43, 3),
             ("q1_noise_grey_40x16", 1, 52), ("q100_noise_grey_24x24", 44, 45),
             ("restart1_grey_80x8", 0, 70), ("grey_1x1", 79, 0)]
    rc, st, got = _host(gpu, [(J.case(n)["stream"], x, y) for n, x, y in tiles], 80, 75, 1)
    assert (rc, st) == (J.OK, [J.OK] * len(tiles))
    want = _want([(_frame(n), x, y) for n, x, y in tiles], 80, 75, 1)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]


# ---------------------------------------------------------------------------- device plans
def test_plan_of_six_jobs_run_twice(gpu):
    """six images in one output buffer: mixed sampling, a two-tile job, a job with a refused tile
    and one whose header the host refuses; everything outside the windows stays as it was"""
    bad = next(c for c in J.damaged() if c["name"].endswith("grey_33x50/cut_mid_scan"))
    specs = [  # (cpp, dim_x, dim_y, pitch slack, [(stream or fixture name, off_x, off_y)])
        (3, 50, 75, 4, [("420_47x71", 2, 3)]),
        (1, 40, 52, 2, [("grey_33x50", 3, 1)]),
        (3, 96, 72, 0, [("444_48x72", 0, 0), ("422_47x71", 48, 0)]),
        (1, 35, 51, 6, [(bad["stream"], 1, 1)]),
        (3, 64, 96, 10, [("restart1_420_64x96", 0, 0)]),
        (3, 20, 20, 0, [(J.case("grey_8x8")["stream"], 0, 0), ("420_17x17", 2, 2)]),  # cpp mismatch
    ]
    jobs, keeps, parts, where = [], [], [], []
    in_off, img_off = 0, 0
    for cpp, dx, dy, slack, tiles in specs:
        pitch = 2 * cpp * dx + slack
        streams = [J.case(t[0])["stream"] if isinstance(t[0], str) else t[0] for t in tiles]
        job, keep, packed = abi.dng_jpeg_job(streams, [(t[1], t[2]) for t in tiles],
                                             abi.Image(None, pitch, dx, dy, cpp, 0), img_off, in_off,
                                             align=1)  # (streams at odd addresses, back to back)
        jobs.append(job)
        keeps.append(keep)
        parts.append(packed)
        where.append((img_off, pitch))
        in_off += packed.size
        img_off += pitch * dy + 2 * (len(jobs) % 2)
    inp = torch.from_numpy(np.concatenate(parts)).cuda()
    out = torch.empty(img_off + 16, dtype=torch.uint8, device="cuda")
    plan = gpu.dng_jpeg_plan(jobs)
    for _ in range(2):  # (a plan runs again on the same scratch)
        out.fill_(0xA5)
        plan.run(inp.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        rc, st, _ = plan.results()
        assert st == [J.OK, J.OK, J.OK, J.TILE_ERRORS, J.OK, J.TILE_ERRORS], st
        assert rc == J.TILE_ERRORS
        tile_st = [plan.tile_status(k, len(s[4]))[1] for k, s in enumerate(specs)]
        assert tile_st[3][0] not in (J.OK, J.TILE_ERRORS)
        assert tile_st[5] == [J.INVALID_ARG, J.OK]
        assert all(t == [J.OK] * len(t) for k, t in enumerate(tile_st) if k not in (3, 5))
        host = out.cpu().numpy()
        want = np.full(host.size, 0xA5, np.uint8)
        for (off, pitch), (cpp, dx, dy, _, tiles), ts in zip(where, specs, tile_st):
            img = np.full((dy, cpp * dx), FILL, np.uint16)
            for (t, ox, oy), s in zip(tiles, ts):
                if s == J.OK:
                    J.paste(img, _frame(t), ox, oy, cpp)
            for y in range(dy):
                want[off + y * pitch:off + y * pitch + 2 * cpp * dx] = img[y].view(np.uint8)
        assert np.array_equal(host, want), np.flatnonzero(host != want)[:6]
    plan.close()


def test_one_host_call_per_image(gpu):
    tiles = _grid(GRID)
    before = gpu.host_calls()
    _host(gpu, [(J.case(n)["stream"], x, y) for n, x, y in tiles], 80, 100, 3)
    assert gpu.host_calls() == before + 1
