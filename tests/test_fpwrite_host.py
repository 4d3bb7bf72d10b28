"""The host build of the F32 writers' core (rawspeed_amd/librsx_fpwrite_host.so) against the numpy
model of tests/fpwrite_files.py: the narrowing on every binary16 and binary24 pattern and on the
neighbours of their images, the packed stream of every case byte for byte, the oracle's unpack of
it, inexact samples, and the width of windows.  No GPU needed."""
import numpy as np
import pytest

import fpwrite_files as F
from oracle_lib import HostImage, Oracle
from rawspeed_amd import abi


@pytest.mark.parametrize("bps", (16, 24))
def test_narrowing_is_the_models_on_every_pattern_and_neighbour(bps):
    p = np.arange(1 << bps, dtype=np.uint32)
    images = F.model_widen(p, bps)
    n, exact = F.host_narrow(images, bps)
    assert exact.all() and np.array_equal(n, p)
    # the core's own widening (what its check program inverts) is the model's on every pattern
    assert np.array_equal(F.host_widen_all(bps), images)
    assert (F.host_fit_bps(images) <= bps).all()
    for y in (images + np.uint32(1), images - np.uint32(1)):
        assert (F.host_fit_bps(y) > bps).all()
        _, want = F.model_narrow(y, bps)
        _, got = F.host_narrow(y, bps)
        assert np.array_equal(got, want) and not got.any()


@pytest.mark.parametrize("bps", (16, 24))
def test_narrowing_of_random_patterns_subnormals_and_large_exponents(bps):
    rng = np.random.default_rng(bps)
    frac, expw = F.FORMAT[bps]
    top = 127 + (1 << (expw - 1))
    x = np.concatenate([
        rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32),
        # a narrow mantissa under every exponent: the subnormal range and both ends of the normal one
        (rng.integers(0, 1 << 9, 1 << 20, dtype=np.uint64).astype(np.uint32) << np.uint32(23)) |
        (rng.integers(0, 1 << frac, 1 << 20, dtype=np.uint64).astype(np.uint32) << np.uint32(23 - frac)),
        np.arange(1, 4096, dtype=np.uint32), np.array([0x7FFFFF, 0x807FFFFF], np.uint32),
        np.array([(e << 23) | f for e in range(top, 255) for f in (0, 1 << (23 - frac))], np.uint32),
        F.specials(32)])
    want_n, want_exact = F.model_narrow(x, bps)
    got_n, got_exact = F.host_narrow(x, bps)
    assert np.array_equal(got_exact, want_exact)
    assert np.array_equal(got_n[want_exact], want_n[want_exact])
    assert 0 < want_exact.sum() < x.size
    # the fit's predicate (no pattern computed) gives the same classes
    e16, e24 = F.model_narrow(x, 16)[1], F.model_narrow(x, 24)[1]
    assert np.array_equal(F.host_fit_bps(x), np.where(e16, 16, np.where(e24, 24, 32)))


@pytest.mark.parametrize("case", F.pack_cases(), ids=lambda c: c[0])
def test_pack_is_the_models_and_unpacks_under_the_oracle(case):
    d, img = F.pack_case(case)
    want, _ = F.model_pack(d, img)
    st, out, r = F.host_pack(d, img)
    assert st == F.OK and (r.bytes_written, r.stream_bytes, r.inexact) == (
        len(want), d.crop_h * d.input_pitch_bytes, 0)
    assert np.array_equal(out[:len(want)], want) and (out[len(want):] == 0x5A).all()
    got = HostImage(img.dim_x, img.dim_y, img.cpp, fill=0, bpc=4)
    assert Oracle().unpack_f32(d, out[:len(want)], got) == abi.RSX_OK
    x0 = F.first_sample(d, img.cpp)
    win = got.u32()[d.crop_y:d.crop_y + d.crop_h, x0:x0 + d.crop_w * img.cpp]
    assert np.array_equal(win, F.window_of(d, img))


@pytest.mark.parametrize("bps", (16, 24))
def test_inexact_samples_give_value_range_and_are_counted(bps):
    case = [c for c in F.pack_cases() if c[0] == "cpp2%dm" % bps][0]
    d, img = F.pack_case(case)
    x0 = F.first_sample(d, img.cpp)
    px = img.px.copy()
    # three inside the window, the last one in its last row and column; two outside it
    cols = d.crop_w * img.cpp
    for y, x in ((d.crop_y, x0), (d.crop_y + 1, x0 + 3), (d.crop_y + d.crop_h - 1, x0 + cols - 1),
                 (d.crop_y + d.crop_h, x0), (d.crop_y, x0 + cols)):
        px[y, x] = 0x3F800001
    bad = F.Img32(px, cpp=img.cpp, pad=img.pitch - 4 * px.shape[1])
    _, want_count = F.model_pack(d, bad)
    st, out, r = F.host_pack(d, bad)
    assert want_count == 3 and st == F.VALUE_RANGE
    assert (r.bytes_written, r.inexact) == (0, 3)
    assert (out[F.round_up4(d.crop_h * d.input_pitch_bytes):] == 0x5A).all()
    # the same image narrows at 32 bits
    d32 = F.pack_desc(0, d.crop_y, d.crop_w, d.crop_h, d.crop_w * img.cpp * 4, 32, d.bit_order)
    assert F.host_pack(d32, bad)[0] == F.OK


def test_fit_of_windows():
    px = F.exact_samples("fit", 16, 9, 37)
    wins = [(0, 0, 37, 9), (1, 1, 5, 3), (30, 6, 7, 3), (0, 8, 37, 1), (36, 8, 1, 1)]
    for pad in (0, 8):
        img = F.Img32(px, pad=pad)
        assert F.host_fit(img, wins) == (F.OK, [16] * 5)
        q = px.copy()
        q[8, 36] = 0x3F800080  # binary24, in the last row and column
        assert F.host_fit(F.Img32(q, pad=pad), wins) == (F.OK, [24, 16, 24, 24, 24])
        q[2, 3] = 0x3F800001
        assert F.host_fit(F.Img32(q, pad=pad), wins) == (F.OK, [32, 32, 24, 24, 24])
        for st, got in [F.host_fit(F.Img32(q, pad=pad), wins)]:
            assert got == [F.model_fit(q[y:y + h, x:x + w]) for x, y, w, h in wins]
    img = F.Img32(px)
    for bad in ((30, 6, 8, 3), (0, 8, 37, 2), (-1, 0, 2, 2), (0, 0, 0, 1)):
        assert F.host_fit(img, [bad])[0] == F.INVALID_ARG


# ---------------------------------------------------------------------------------------------
# deflate tiles: the host build of rsx_deflate_core.h against libz, the project's own inflate and
# the model of the reader
# ---------------------------------------------------------------------------------------------
import ctypes as C  # noqa: E402
import heapq  # noqa: E402
import zlib  # noqa: E402

import dng_deflate_files as DF  # noqa: E402
from rawspeed_amd import build  # noqa: E402


def _inflate_host(stream, n):
    L = C.CDLL(build.build_inflate_host()[0])
    L.rsx_inflate_host.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    src = np.frombuffer(stream, np.uint8).copy()
    out = np.full(n + 16, 0xA5, np.uint8)
    produced, consumed = C.c_uint32(0), C.c_uint32(0)
    v = L.rsx_inflate_host(src.ctypes.data, src.size, out.ctypes.data, n, C.byref(produced),
                           C.byref(consumed))
    return v, out[:produced.value].tobytes(), consumed.value


@pytest.mark.parametrize("case", F.deflate_cases(), ids=lambda c: c[0])
def test_deflate_stream_decodes_through_libz_the_inflate_core_and_the_model(case):
    name, bps, pred, cpp, geom, kind = case
    d, geom, img, tile = F.deflate_case(case)
    raw = DF.tile_bytes(tile, bps, DF.PREDICTORS[pred] * cpp)
    st, out, r = F.host_deflate(d, geom, img)
    stream = out[:r.bytes].tobytes()
    assert st == F.OK and r.status == F.OK and (out[r.bytes:] == 0x5A).all()
    assert stream[0] == 0x78 and (stream[0] * 256 + stream[1]) % 31 == 0 and not stream[1] & 0x20
    assert zlib.decompress(stream) == raw
    assert _inflate_host(stream, len(raw)) == (DF.OK, raw, len(stream))
    verdict, got, used = DF.model_decode(stream, bps, pred, cpp, geom)
    tile_w, tile_h, off_x, off_y, width, height = geom
    assert verdict == DF.OK and used == len(stream)
    assert np.array_equal(got, img.px[off_y:off_y + height, off_x:off_x + width])
    assert r.bytes <= F.bound_model(len(raw)) and r.adler == zlib.adler32(raw)
    assert r.blocks == -(-len(raw) // F.BLOCK) and r.stored_blocks <= r.blocks
    if kind == "bits" and len(raw) > 64:  # every pattern: the stored form is chosen
        assert r.stored_blocks == r.blocks
        assert len(stream) == 2 + 4 + len(raw) + 5 * r.blocks  # (behind the wrapper blocks are aligned)
    if kind in ("smooth", "zero"):
        assert r.stored_blocks < r.blocks


def test_deflate_crafted_blocks_reach_their_rules():
    assert F.host_block_stats(F.crafted_bytes("nomatch")) == (0, 0)  # no match, one distance code sent
    s, r = F.host_deflate_bytes(F.crafted_bytes("nomatch"))
    assert r.stored_blocks == 0 and zlib.decompress(s.tobytes()) == F.crafted_bytes("nomatch").tobytes()
    matches, dists = F.host_block_stats(np.zeros(F.BLOCK, np.uint8))
    assert dists == 1 and matches == -(-(F.BLOCK - 1) // 258)  # distance 1, length 258 chained
    one = np.array([7], np.uint8)
    s, r = F.host_deflate_bytes(one)
    assert zlib.decompress(s.tobytes()) == one.tobytes()
    d = F.crafted_bytes("all256")
    assert len(set(d[:F.BLOCK].tolist())) == 256
    # rows that repeat at exactly 32768 bytes are matched, at 32768 + 512 they cannot be
    s64, r64 = F.host_deflate_bytes(F.crafted_bytes("period64"))
    s65, r65 = F.host_deflate_bytes(F.crafted_bytes("period65"))
    # (the one candidate of a position is the latest with its hash, so not every byte of the
    # repeat is matched: the block of the repeat is dynamic and shorter than its bytes, no more)
    assert r64.stored_blocks == r64.blocks - 1 and len(s64) < 72 * 512
    assert r65.stored_blocks == r65.blocks and len(s65) > 73 * 512
    for s, name in ((s64, "period64"), (s65, "period65")):
        assert zlib.decompress(s.tobytes()) == F.crafted_bytes(name).tobytes()


@pytest.mark.parametrize("n", (F.BLOCK - 1, F.BLOCK, F.BLOCK + 1, 2 * F.BLOCK, 2 * F.BLOCK + 1))
def test_deflate_block_boundaries(n):
    rng = np.random.default_rng(n)
    for data in (rng.integers(0, 4, n).astype(np.uint8), rng.integers(0, 256, n).astype(np.uint8),
                 np.zeros(n, np.uint8)):
        s, r = F.host_deflate_bytes(data)
        assert zlib.decompress(s.tobytes()) == data.tobytes()
        assert r.blocks == -(-n // F.BLOCK) and len(s) <= F.bound_model(n) and r.adler == zlib.adler32(data)


def _huffman_depth(counts):
    h = [(c, i, 0) for i, c in enumerate(counts) if c]
    heapq.heapify(h)
    k = len(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (a[0] + b[0], k, max(a[2], b[2]) + 1))
        k += 1
    return h[0][2]


def _kraft(lengths, maxbits):
    return sum(1 << (maxbits - int(l)) for l in lengths if l)


def test_length_limiter_engages_and_keeps_a_complete_code():
    lit = np.zeros(286, np.uint32)
    lit[40:40 + len(F.LIMITER_COUNTS)] = F.LIMITER_COUNTS
    assert sum(F.LIMITER_COUNTS) == 8343 and _huffman_depth(F.LIMITER_COUNTS) == 16
    lit[256] = 1  # end of block
    assert _huffman_depth(lit) > 15
    used, lens = F.host_limit(lit, 15)
    assert used == 18 and lens.max() == 15 and _kraft(lens, 15) == 1 << 15
    assert all((lens[i] > 0) == (lit[i] > 0) for i in range(286))
    # a code-length histogram that would pass 7
    cl = np.array([1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 0, 0, 0, 0, 233, 377, 610], np.uint32)
    assert _huffman_depth(cl) > 7
    used, lens = F.host_limit(cl, 7)
    assert used == 15 and lens.max() == 7 and _kraft(lens, 7) == 1 << 7
    # unlimited trees come out as they are: Kraft's sum is 1 as well
    for seed in range(50):
        f = np.random.default_rng(seed).integers(0, 50, 286).astype(np.uint32)
        f[256] = 1
        used, lens = F.host_limit(f, 15)
        assert used == int((f > 0).sum()) and _kraft(lens, 15) == 1 << 15
    # the counts as data: a block of those bytes in shuffled order round-trips
    data = F.crafted_bytes("limiter")
    s, r = F.host_deflate_bytes(data)
    assert r.stored_blocks == 0 and zlib.decompress(s.tobytes()) == data.tobytes()


@pytest.mark.parametrize("bps", F.BPS)
def test_deflate_size_against_libz(bps):
    """128 x 128 tiles, predictor 3, seed 1: a table per block and a working match finder are not
    larger than Z_HUFFMAN_ONLY on the smooth and mixed kinds; the bits kind stays within the bound"""
    for kind in ("smooth", "mixed", "bits"):
        s = DF.random_samples(np.random.default_rng(1), bps, 128, 128, kind)
        raw = DF.tile_bytes(s, bps, 1)
        ours, r = F.host_deflate_bytes(np.frombuffer(raw, np.uint8))
        c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY)
        huff = len(c.compress(raw) + c.flush())
        print(kind, bps, "ours", len(ours), "Z_HUFFMAN_ONLY", huff, "level 1", len(zlib.compress(raw, 1)),
              "level 6", len(zlib.compress(raw, 6)))
        assert zlib.decompress(ours.tobytes()) == raw
        if kind == "bits":
            assert len(ours) <= F.bound_model(len(raw))
        else:
            assert len(ours) <= huff


def test_deflate_overflow_and_inexact():
    case = [c for c in F.deflate_cases() if c[0] == "ragged_both"][0]
    d, geom, img, tile = F.deflate_case(case)
    st, out, r = F.host_deflate(d, geom, img)
    n = int(r.bytes)
    st, out, r2 = F.host_deflate(d, geom, img, cap=n)
    assert st == F.OK and r2.bytes == n
    st, out, r2 = F.host_deflate(d, geom, img, cap=n - 1)
    assert st == F.INPUT_OVERFLOW and r2.bytes == 0 and (out == 0x5A).all()
    case = [c for c in F.deflate_cases() if c[0] == "ragged_right"][0]
    d, geom, img, tile = F.deflate_case(case)
    px = img.px.copy()
    tile_w, tile_h, off_x, off_y, width, height = geom
    px[off_y + height - 1, off_x + width - 1] = 0x3F800001  # the last sample of the window
    st, out, r = F.host_deflate(d, geom, F.Img32(px, pad=img.pitch - 4 * px.shape[1]))
    assert st == F.VALUE_RANGE and r.bytes == 0 and (out == 0x5A).all()
    px = img.px.copy()
    px[off_y + height, off_x] = 0x3F800001  # below the window: not read
    assert F.host_deflate(d, geom, F.Img32(px, pad=img.pitch - 4 * px.shape[1]))[0] == F.OK
