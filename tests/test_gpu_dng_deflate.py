"""Deflate DNG tiles on the device (rsx_dng_deflate_*, rawspeed_amd/csrc/rsx_dng_deflate.hip)
through the C-ABI: the host-pointer call and device plans against the model of
tests/dng_deflate_files.py (libz's verdict and bytes, the oracle's widening), and against the
tiles recorded from the reference in tests/golden/dng_deflate_ref.json."""
import json
import os
import zlib

import numpy as np
import pytest
import torch

import dng_deflate_files as D
from oracle_lib import HostImage
from rawspeed_amd import abi

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dng_deflate_ref.json")


@pytest.fixture(scope="module")
def gpu():
    import gpu_util
    return gpu_util.ctx()


def _host(gpu, bps, predictor, cpp, dim_x, dim_y, tiles, pad=0):
    """tiles: [(geom, data)] of one image -> (rc, statuses, the image's words, padding intact)"""
    pitch = (4 * cpp * dim_x + 15) // 16 * 16 + pad
    img = HostImage(dim_x, dim_y, cpp, pitch=pitch, bpc=4)
    rc, st = gpu.dng_decompress_deflate(bps, predictor, [g for g, _ in tiles], [d for _, d in tiles],
                                        img.view())
    rows = img.buf.reshape(dim_y, pitch)
    assert (rows[:, 4 * cpp * dim_x:] == 0xA5).all(), "the pitch padding was written"
    return rc, st, rows[:, :4 * cpp * dim_x].copy().view(np.uint32)


def _expect(bps, predictor, cpp, dim_x, dim_y, tiles):
    want = np.full((dim_y, cpp * dim_x), 0xA5A5A5A5, np.uint32)
    status = []
    for geom, data in tiles:
        v, bits, _ = D.model_decode(data, bps, predictor, cpp, geom)
        status.append(D.STATUS[v])
        if v == D.OK:
            D.paste(want, geom, bits)
    return status, want


def _plan(gpu, cases, in_gap=3, twice=False):
    """cases: [(bps, predictor, cpp, geom, data)], each into an image of its own window inside one
    output buffer -> per case (status, consumed, the window's words); everything else of the
    buffer must stay 0xA5"""
    jobs, parts, where = [], [np.full(in_gap, 0x5A, np.uint8)], []
    in_off, img_off = in_gap, 0
    for k, (bps, predictor, cpp, geom, data) in enumerate(cases):
        tile_w, tile_h, off_x, off_y, width, height = geom
        dim_x, dim_y = -(-(off_x + width) // cpp) + (k % 2), off_y + height + (k % 3 == 1)
        pitch = 4 * cpp * dim_x + 4 * (k % 3)
        j = abi.DngDeflateJob()
        j.desc = abi.DngDeflateDesc(bps, predictor)
        j.tile_w, j.tile_h, j.off_x, j.off_y, j.width, j.height = geom
        j.in_offset, j.in_bytes, j.img_offset = in_off, len(data), img_off
        j.img = abi.Image(None, pitch, dim_x, dim_y, cpp, 0)
        jobs.append(j)
        parts.append(np.frombuffer(bytes(data), np.uint8))
        parts.append(np.full(1 + k % 5, 0x5A, np.uint8))  # (bytes between the jobs: nobody's)
        where.append((img_off, pitch, geom))
        in_off += len(data) + 1 + k % 5
        img_off += pitch * dim_y + 4 * (k % 2)
    inp = torch.from_numpy(np.concatenate(parts)).cuda()
    out = torch.full((img_off + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    plan = gpu.dng_deflate_plan(jobs)
    for _ in range(2 if twice else 1):  # (a plan runs again on the same scratch)
        out.fill_(0xA5)
        plan.run(inp.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        rc, st, cons = plan.results()
    plan.close()
    host = out.cpu().numpy()
    covered = np.zeros(host.size, bool)
    res = []
    for (off, pitch, geom), s, c in zip(where, st, cons):
        tile_w, tile_h, off_x, off_y, width, height = geom
        rows = []
        for r in range(height):
            a = off + (off_y + r) * pitch + 4 * off_x
            rows.append(host[a:a + 4 * width].copy().view(np.uint32))
            covered[a:a + 4 * width] = True
        res.append((s, c, np.stack(rows)))
    assert (host[~covered] == 0xA5).all(), "bytes outside the tiles' windows were written"
    return rc, res


def _check_plan(gpu, cases, **kw):
    rc, res = _plan(gpu, cases, **kw)
    n_bad = 0
    for (bps, predictor, cpp, geom, data), (st, cons, got) in zip(cases, res):
        v, bits, used = D.model_decode(data, bps, predictor, cpp, geom)
        assert st == D.STATUS[v], (geom, st, v)
        if v == D.OK:
            assert cons == used
            assert np.array_equal(got, bits), (bps, predictor, cpp, geom, np.argwhere(got != bits)[:4])
        else:
            n_bad += 1
            assert (got == 0xA5A5A5A5).all(), "a failed tile wrote into its window"
    assert (rc == 0) == (n_bad == 0)
    return res


def _raw_case(data, dst_len):
    """a stream of dst_len bytes as a one-row tile of the widest sample that divides it"""
    bps = 32 if dst_len % 4 == 0 else 16 if dst_len % 2 == 0 else 24
    w = dst_len // (bps // 8)
    return (bps, 3, 1, (w, 1, 0, 0, w, 1), data)


# ------------------------------------------------------------------------------- geometry
@pytest.mark.parametrize("bps", D.BPS)
@pytest.mark.parametrize("predictor", sorted(D.PREDICTORS))
@pytest.mark.parametrize("cpp", (1, 3))
def test_every_depth_predictor_and_cpp(gpu, bps, predictor, cpp):
    """tile widths around the row scan's chunk (64 lanes x 16, 15 or 12 bytes) and rows shorter
    than predFactor"""
    rng = np.random.default_rng([0xD8, bps, predictor, cpp])
    cases = []
    piece = {1: 16, 2: 16, 4: 16, 3: 15, 6: 12, 12: 12}[D.PREDICTORS[predictor] * cpp]
    chunk = 64 * piece
    widths = [1, 3, 5, 21, 63, 64, 65, 257, 1025, 4099]
    widths += [-(-(chunk + d) // (bps // 8)) for d in (-1, 0, 1)]  # (row bytes around one chunk)
    for k, tw in enumerate(widths):
        tile_w, tile_h = tw * cpp, (1, 2, 5)[k % 3]
        s = D.random_samples(rng, bps, tile_h, tile_w, ("mixed", "bits", "smooth")[k % 3])
        data = D.write_tile(s, bps, predictor, cpp, level=(6, 1, 9, 0)[k % 4])
        cases.append((bps, predictor, cpp, (tile_w, tile_h, 0, 0, tile_w, tile_h), data))
    _check_plan(gpu, cases)


@pytest.mark.parametrize("pad", (0, 16, 18))
@pytest.mark.parametrize("cpp", (1, 3))
def test_edge_tiles_of_one_image_in_one_call(gpu, pad, cpp):
    """a 2 x 2 grid of tiles whose right and bottom ones are cropped, with the pitch padded by 0,
    16 and 18 bytes (18: rows that are not 4-byte aligned are refused)"""
    bps, predictor = 16, 34894
    tw, th, dim_x, dim_y = 24, 7, 41, 11
    rng = np.random.default_rng([0xE1, pad, cpp])
    tiles = []
    for ty in range(2):
        for tx in range(2):
            w, h = min(tw, dim_x - tx * tw), min(th, dim_y - ty * th)
            geom = (tw * cpp, th, tx * tw * cpp, ty * th, w * cpp, h)
            s = D.random_samples(rng, bps, th, tw * cpp)
            tiles.append((geom, D.write_tile(s, bps, predictor, cpp)))
    if pad % 4:
        img = HostImage(dim_x, dim_y, cpp, pitch=(4 * cpp * dim_x + 15) // 16 * 16 + pad, bpc=4)
        rc, st = gpu.dng_decompress_deflate(bps, predictor, [g for g, _ in tiles], [d for _, d in tiles],
                                            img.view())
        assert rc == abi.RSX_ERR_TILE_ERRORS and st == [abi.RSX_ERR_INVALID_ARG] * 4
        assert (img.buf == 0xA5).all()
        return
    calls = gpu.host_calls() if hasattr(gpu, "host_calls") else None
    rc, st, got = _host(gpu, bps, predictor, cpp, dim_x, dim_y, tiles, pad)
    status, want = _expect(bps, predictor, cpp, dim_x, dim_y, tiles)
    assert rc == 0 and st == status == [0] * 4
    assert np.array_equal(got, want)
    if calls is not None:
        assert gpu.host_calls() == calls + 1


def test_a_failed_tile_leaves_its_window_and_the_neighbours_are_written(gpu):
    bps, predictor, cpp = 24, 3, 1
    rng = np.random.default_rng(0xF7)
    tiles = []
    for tx in range(3):
        geom = (16, 6, 16 * tx, 1, 16, 5)
        data = D.write_tile(D.random_samples(rng, bps, 6, 16), bps, predictor, cpp)
        if tx == 1:
            data = data[:-1]  # (the Adler-32 cut)
        tiles.append((geom, data))
    short = D.write_tile(D.random_samples(rng, bps, 5, 16), bps, predictor, cpp)
    tiles.append(((16, 6, 48, 1, 16, 5), short))  # (a row short: Z_OK with fewer bytes)
    tiles.append(((16, 6, 64, 1, 16, 5), b""))
    rc, st, got = _host(gpu, bps, predictor, cpp, 80, 7, tiles)
    status, want = _expect(bps, predictor, cpp, 80, 7, tiles)
    assert status == [0, abi.RSX_ERR_IO, 0, abi.RSX_ERR_UNSUPPORTED, abi.RSX_ERR_IO]
    assert rc == abi.RSX_ERR_TILE_ERRORS and st == status
    assert np.array_equal(got, want)


def test_recorded_tiles_of_the_reference(gpu):
    with open(GOLDEN) as f:
        g = json.load(f)
    cases, wants = [], []
    for t in g["tiles"]:
        cases.append((t["bps"], t["predictor"], t["cpp"], tuple(t["geom"]), bytes.fromhex(t["input_hex"])))
        wants.append(np.frombuffer(bytes.fromhex(t["output_hex"]), "<u4").reshape(t["geom"][5], t["geom"][4]))
    for (st, _, got), want in zip(_plan(gpu, cases)[1], wants):
        assert st == 0 and np.array_equal(got, want)


# ------------------------------------------------------------------------------- inflate
def test_inflate_shapes(gpu):
    """sizes around the 32 KiB window and three times it, every level and strategy, stored
    blocks, window sizes, flushes, bytes behind the stream"""
    _check_plan(gpu, [_raw_case(data, n) for _, data, n in D.inflate_shapes()], twice=True)


def test_hand_assembled_streams_and_verdicts(gpu):
    streams = D.hand_streams()
    res = _check_plan(gpu, [_raw_case(data, n) for _, data, n, _ in streams])
    for (name, data, n, made_for), (st, _, _) in zip(streams, res):
        assert D.inflate_verdict(data, n)[0] == made_for, name
        assert st == D.STATUS[made_for], name


def test_mutation_corpus(gpu):
    """single-byte mutants of small valid tiles in one plan: OK exactly where libz says Z_OK with
    the full length, and the same floats there.  (tests/test_dng_deflate_host.py runs the same
    mutants through the host build of the inflate core.)"""
    m = D.mutants()
    verdicts = {D.inflate_verdict(d, (b // 8) * g[0] * g[1])[0] for b, _, _, g, d in m}
    assert D.OK in verdicts and D.FAIL in verdicts and len(m) >= 300
    _check_plan(gpu, m)


# ------------------------------------------------------------------------------- plans
def test_two_streams_and_kernel_names(gpu):
    rng = np.random.default_rng(0x2B)
    bps, predictor, cpp, geom = 32, 34895, 1, (70, 9, 2, 1, 66, 8)
    data = D.write_tile(D.random_samples(rng, bps, 9, 70), bps, predictor, cpp)
    v, bits, used = D.model_decode(data, bps, predictor, cpp, geom)
    assert v == D.OK and used == len(data)
    j = abi.DngDeflateJob()
    j.desc = abi.DngDeflateDesc(bps, predictor)
    j.tile_w, j.tile_h, j.off_x, j.off_y, j.width, j.height = geom
    j.in_offset, j.in_bytes, j.img_offset = 0, len(data) + 7, 0  # (bytes behind the stream)
    j.img = abi.Image(None, 4 * 72, 72, 10, 1, 0)
    inp = torch.from_numpy(np.frombuffer(data + bytes(7), np.uint8).copy()).cuda()
    plan = gpu.dng_deflate_plan([j])
    plan.set_timing(True)
    outs, streams = [], [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for s in streams:
        out = torch.full((4 * 72 * 10,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        plan.run(inp.data_ptr(), out.data_ptr(), s.cuda_stream)
        rc, st, cons = plan.results()
        assert (rc, st, cons) == (0, [0], [len(data)])
        outs.append(out.cpu().numpy().view(np.uint32).reshape(10, 72))
    names = [n for n, _ in plan.kernel_table()[0]]
    plan.close()
    assert names == ["dfl_inflate_kernel", "dfl_row_kernel"]
    for o in outs:
        assert np.array_equal(o[1:9, 2:68], bits)
        o[1:9, 2:68] = 0xA5A5A5A5
        assert (o == 0xA5A5A5A5).all()


def test_a_plan_over_the_scratch_limit_is_refused(gpu):
    j = abi.DngDeflateJob()
    j.desc = abi.DngDeflateDesc(32, 3)
    j.tile_w, j.tile_h, j.off_x, j.off_y, j.width, j.height = 16384, 8192, 0, 0, 16, 16
    j.in_offset, j.in_bytes, j.img_offset = 0, 64, 0
    j.img = abi.Image(None, 64, 16, 16, 1, 0)
    from rawspeed_amd.capi import RsxError
    with pytest.raises(RsxError) as e:
        gpu.dng_deflate_plan([j, j, j])  # 3 x 512 MiB of inflated bytes
    assert e.value.status == abi.RSX_ERR_UNSUPPORTED
