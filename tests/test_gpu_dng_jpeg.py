"""Lossy-JPEG DNG tiles on the device (rsx_dng_jpeg_*, rawspeed_amd/csrc/rsx_dng_jpeg.hip) through
the C-ABI: the host-pointer call and device plans against what libjpeg-turbo's default decoder made
of the committed streams (tests/golden/dng_jpeg_ref.json, recorded through Pillow; nothing here
imports it).  An undamaged fixture must come back RSX_OK and equal -- a refusal does not pass; a
damaged one is either refused with the image untouched or equal to what was recorded (a run of fill
bytes is no damage: it must be equal).  The last section takes streams past one byte window of the
block kernel and rows past one workgroup of the finish kernel."""
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
    if "repeat" in c:  # a run of fill bytes in front of a stuffed pair: libjpeg skips it
        assert c["sha256"] == J.case(c["base"])["sha256"]
        assert (rc, st) == (J.OK, [J.OK]), "fill bytes were refused"
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


# ------------------------------------------- past one byte window and one finish workgroup
# jpeg_blocks_kernel keeps 8192 bytes of a segment in LDS, from the 16-byte unit of the input
# address that holds the walk's position, and reloads them once the walk is more than 4096 bytes
# in; jpeg_finish_kernel's workgroup covers 128 units of 8 samples of a row.  What the fixtures
# below must be for that to matter is asserted without a device in test_dng_jpeg_model.py.
POISON = b"\xff\xd0\xff\x00"  # behind and in front of every stream: a marker and a stuffed pair


def _run_plan(gpu, specs, runs=1):
    """One device plan.  specs: a job each, (cpp, dim_x, dim_y, pitch, lead, tiles): the image
    `lead` bytes behind the one in front, tiles [(stream, frame or None, off_x, off_y, residue)]:
    the stream's first byte at an input address of that residue mod 16 (None: wherever it lands,
    back to back), at least eight POISON bytes between two streams, `frame` None where the tile
    must be refused.  Every run must leave exactly the frames' windows in an output of 0xA5.
    -> (the output's address, [(offset, pitch)] of the images, the tiles' statuses per job)"""
    data, jobs, keeps, where = bytearray(POISON * 4), [], [], []
    img_off = 0
    for cpp, dx, dy, pitch, lead, tiles in specs:
        img_off += lead
        job, keep, _ = abi.dng_jpeg_job([t[0] for t in tiles], [(t[2], t[3]) for t in tiles],
                                        abi.Image(None, pitch, dx, dy, cpp, 0), img_off, 0, align=1)
        for k, t in enumerate(tiles):
            data += POISON * 2
            while t[4] is not None and len(data) % 16 != t[4]:
                data += POISON[len(data) % 4:len(data) % 4 + 1]
            keep[2][k] = len(data)  # (the job's in_offsets)
            data += t[0]
        jobs.append(job)
        keeps.append(keep)
        where.append((img_off, pitch))
        img_off += pitch * dy
    data += POISON * 8
    inp = torch.from_numpy(np.frombuffer(bytes(data), np.uint8).copy()).cuda()
    out = torch.empty(img_off + 16, dtype=torch.uint8, device="cuda")
    assert inp.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    want = np.full(img_off + 16, 0xA5, np.uint8)
    for (off, pitch), (cpp, dx, dy, _, _, tiles) in zip(where, specs):
        img = np.full((dy, cpp * dx), FILL, np.uint16)
        for _, frame, ox, oy, _ in tiles:
            if frame is not None:
                J.paste(img, frame, ox, oy, cpp)
        rows = want[off:off + pitch * dy].reshape(dy, pitch)
        rows[:, :2 * cpp * dx] = img.view(np.uint8)
    plan = gpu.dng_jpeg_plan(jobs)
    for _ in range(runs):  # (a plan runs again on the same scratch)
        out.fill_(0xA5)
        plan.run(inp.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        rc, st, _ = plan.results()
        tile_st = [plan.tile_status(k, len(s[5]))[1] for k, s in enumerate(specs)]
        for k, (s, ts) in enumerate(zip(specs, tile_st)):
            assert [t == J.OK for t in ts] == [t[1] is not None for t in s[5]], (k, ts)
            assert st[k] == (J.OK if all(t == J.OK for t in ts) else J.TILE_ERRORS), (k, st[k])
        host = out.cpu().numpy()
        assert np.array_equal(host, want), np.flatnonzero(host != want)[:6]
    plan.close()
    return out.data_ptr(), where, tile_st


LONG = ["long_grey_96x96", "long_420_64x64", "long_restart_grey_96x96"]


def test_long_streams_at_every_input_address(gpu):
    """every long stream with its first byte at each residue mod 16, so the window's first unit
    is cut at each place, with bytes that belong to nobody in front of and behind it; twice"""
    specs = []
    for r in range(16):
        for name in LONG:
            c = J.case(name)
            cpp, ox, oy = c["cpp"], r % 3, r % 2
            dx, dy = c["width"] + ox + (r & 1), c["height"] + oy
            specs.append((cpp, dx, dy, 2 * cpp * dx + 2 * (r % 4), 2 * (r % 3),
                          [(c["stream"], _frame(name), ox, oy, r)]))
    _run_plan(gpu, specs, runs=2)


def test_fill_runs_through_a_plan(gpu):
    """runs of FF in front of a stuffed pair that end just below, at and just above the reload
    threshold and past the whole window: the walk leaves the window for global memory, and the
    next batch's window starts far ahead of the last one"""
    frame = _frame("long_grey_96x96")
    fills = [c for c in J.damaged() if c.get("repeat", (0, 0))[1] in (4095, 4096, 4097, 9000)]
    assert len(fills) == 8
    specs = [(1, 98, 97, 2 * 98 + 2 * (k % 3), 2 * (k % 2),
              [(c["stream"], frame, 1 + k % 2, k % 2, (5 * k + 3) % 16)]) for k, c in enumerate(fills)]
    _run_plan(gpu, specs, runs=2)


WIDE_CUTS = {1: (1023, 1024, 1025, 2047, 2048, 2049), 3: (341, 342, 682, 683)}


@pytest.mark.parametrize("name", ["wide_grey_2064x8", "wide_444_704x8", "wide_422_704x8", "wide_420_704x16"])
def test_wide_tile_across_the_finish_workgroups(gpu, name):
    """rows of more than 2048 samples (three workgroups): off_x 0 .. 7, rows at all eight places
    of the 16-byte grid, and windows cut by the image so that copy_w * cpp ends one sample (grey)
    or inside one pixel (three components) on either side of unit 128 and unit 256"""
    c = J.case(name)
    cpp, w, h = c["cpp"], c["width"], c["height"]
    specs = []
    for ox in range(8):
        for k, cw in enumerate(WIDE_CUTS[cpp] + (w,)):
            n = len(specs)
            dx = ox + cw + (1 if cw == w else 0)  # (the whole tile: a pixel of the image behind it)
            oy = n % 3
            dy = oy + h - (n % 2)  # (every other window loses its last row)
            slack = (2, 6, 0, 10, 14, 4, 8, 12)[(ox + k) % 8]
            specs.append((cpp, dx, dy, 2 * cpp * dx + slack, 2 * (n % 8),
                          [(c["stream"], _frame(name), ox, oy, None)]))
    base, where, _ = _run_plan(gpu, specs)
    assert any(pitch % 4 == 2 for _, pitch in where)
    for ox in range(8):  # every off_x met a window row at each place of the 16-byte grid
        rows = {((base + off + y * pitch) >> 1) & 7
                for (off, pitch), s in zip(where, specs) if s[5][0][2] == ox
                for y in range(s[5][0][3], s[2])}
        assert rows == set(range(8)), (ox, rows)


def test_wide_tile_among_the_smallest(gpu):
    """the finish grid has the size of the plan's largest tile: three workgroups a row for
    wide_grey_2064x8 and the 96 rows of a tile the kernel refuses (its data ends at byte 6000, in
    front of an EOI); the lanes and rows that grey_1x1 and 420_2x2 do not own write nothing"""
    bad = next(c for c in J.damaged() if c["name"] == "long_grey_96x96/cut_at_6000_eoi_kept")
    one, two = J.case("grey_1x1")["stream"], J.case("420_2x2")["stream"]
    wide = J.case("wide_grey_2064x8")["stream"]
    specs = [
        (1, 2070, 110, 2 * 2070 + 6, 2, [(wide, _frame("wide_grey_2064x8"), 3, 1, 7),
                                         (one, _frame("grey_1x1"), 2069, 109, 15),
                                         (bad["stream"], None, 10, 12, 9),
                                         (one, _frame("grey_1x1"), 0, 0, 1)]),
        (3, 9, 5, 2 * 3 * 9 + 2, 6, [(two, _frame("420_2x2"), 7, 3, 3), (two, _frame("420_2x2"), 0, 0, 0)]),
    ]
    _, _, tile_st = _run_plan(gpu, specs, runs=2)
    assert tile_st[0][2] == J.OVERFLOW


def test_one_host_call_per_image(gpu):
    tiles = _grid(GRID)
    before = gpu.host_calls()
    _host(gpu, [(J.case(n)["stream"], x, y) for n, x, y in tiles], 80, 100, 3)
    assert gpu.host_calls() == before + 1
