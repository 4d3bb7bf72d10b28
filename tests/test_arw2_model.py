"""SonyArw2Decompressor: the model of the device decode (tests/arw2_files.py) against the
unmodified reference's whole-file decode (RawParser -> ArwDecoder -> SonyArw2Decompressor),
with and without the curve (uncorrectedRawValues), and the jump-ahead dither against plain
stepping.  No GPU needed; the reference comparisons need oracle/_ref (the stored answers of the
`ref` fixture cannot decode new files)."""
import numpy as np
import pytest

import arw2_files as A
from oracle_lib import Ref


@pytest.fixture(scope="module")
def ref():
    return Ref()


def _points(rng, kind):
    return {0: (0, 0, 0, 0), 1: A.REALISTIC_CURVE, 2: A.random_monotone_points(rng)}[kind]


def _check(ref, data, w, h, points, uncorrected):
    st, dec = ref.decode_file(A.arw2_file(w, h, data, points), uncorrected=uncorrected)
    if uncorrected:
        mst, img, rows = A.model_decode(data, w, h)
    else:
        mst, img, rows = A.model_decode(data, w, h, A.DITHER,
                                        A.table_dither(A.decode_curve(points)))
    assert st == mst, (st, mst, ref.last_error())
    if st == 0:
        got = dec.u16()[:h, :w]
        assert np.array_equal(got, img), np.argwhere(got != img)[:5]
    return st, rows


@pytest.mark.ref
@pytest.mark.skipif(not Ref.available(), reason="oracle/_ref not built")
@pytest.mark.parametrize("chunk", range(6))
def test_model_matches_reference_on_random_files(ref, chunk):
    for seed in range(50 * chunk, 50 * chunk + 50):
        rng = np.random.default_rng([0xA2, seed])
        w = 32 * int(rng.choice([1, 2, 3, int(rng.integers(1, 301))]))
        h = 2 * int(rng.integers(1, 4))
        data = A.random_stream(rng, w, h)
        st, _ = _check(ref, data, w, h, _points(rng, seed % 3), bool(seed & 4))
        assert st == 0, seed


@pytest.mark.ref
@pytest.mark.skipif(not Ref.available(), reason="oracle/_ref not built")
@pytest.mark.parametrize("uncorrected", [False, True])
def test_every_width_at_small_height(ref, uncorrected):
    rng = np.random.default_rng(int(uncorrected))
    for w in range(32, 9601, 32):
        data = A.random_stream(rng, w, 2)
        _check(ref, data, w, 2, A.REALISTIC_CURVE, uncorrected)


def _edge_blocks():
    """(max, min, imax, imin, fields): every sh, max < min, the clamp, imax / imin at 0 and 15"""
    out = []
    f_hi = [127] * 14
    f_mix = [(11 * k + 3) & 127 for k in range(14)]
    for diff in (0x7F, 0x80, 0xFF, 0x100, 0x1FF, 0x200, 0x3FF, 0x400, 0x7FF):
        mn = 0 if diff == 0x7FF else 100
        out.append((mn + diff, mn, 3, 9, f_mix))
        out.append((mn + diff, mn, 0, 15, f_hi))
    out += [(5, 900, 1, 2, f_hi), (0, 0x7FF, 15, 0, f_mix), (0x7FF, 0x7F0, 0, 1, f_hi),
            (0x7FF, 0x700, 15, 14, f_hi), (0x7F0, 0x600, 14, 15, f_hi),  # clamp at 0x7ff
            (1000, 990, 0, 15, [0] * 14), (0, 0, 15, 0, [0] * 14), (0x7FF, 0x7FF, 7, 8, f_hi)]
    for imax in (0, 15, 7):
        for imin in (0, 15, 8):
            if imax != imin:
                out.append((1500, 200, imax, imin, f_mix))
    return out


@pytest.mark.ref
@pytest.mark.skipif(not Ref.available(), reason="oracle/_ref not built")
@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("uncorrected", [False, True])
def test_planted_edges(ref, kind, uncorrected):
    rng = np.random.default_rng([kind, uncorrected])
    blocks = _edge_blocks()
    w = 32 * ((len(blocks) + 1) // 2)
    data = A.random_stream(rng, w, 2)
    for k, blk in enumerate(blocks):
        data = A.set_block(data, w, k & 1, k, A.pack_block(*blk))
    # every sh is reached, and the clamp
    P, bad = A.model_values(data, w, 2)
    assert not bad.any() and P.max() == 0x7FF
    st, _ = _check(ref, data, w, 2, _points(rng, kind), uncorrected)
    assert st == 0


@pytest.mark.ref
@pytest.mark.skipif(not Ref.available(), reason="oracle/_ref not built")
@pytest.mark.parametrize("row", ["first", "last"])
@pytest.mark.parametrize("block", ["first", "last"])
def test_imax_equal_imin_fails_the_decode(ref, row, block):
    rng = np.random.default_rng([len(row), len(block)])
    w, h = 96, 4
    y = 0 if row == "first" else h - 1
    b = 0 if block == "first" else w // 16 - 1
    data = A.set_block(A.random_stream(rng, w, h), w, y, b, A.pack_block(900, 100, 6, 6, [1] * 14))
    for unc in (False, True):
        st, rows = _check(ref, data, w, h, A.REALISTIC_CURVE, unc)
        assert st == A.TILE_ERRORS  # "Too many errors" (SonyArw2Decompressor.cpp:143-147)
        assert "ARW2 invariant failed" in ref.last_error()
        assert rows == [A.INVALID_ARG if r == y else 0 for r in range(h)]


@pytest.mark.parametrize("mode", [A.NONE, A.PLAIN, A.DITHER])
def test_jump_ahead_dither_equals_stepping(mode):
    """The model's state at step 16 b + i is seed * 15700^(16 b + i) mod m; the reference
    steps once per pixel.  Plain tables and no table take the same path."""
    rng = np.random.default_rng(17 + mode)
    curve = A.decode_curve(A.random_monotone_points(rng))
    table = {A.NONE: None, A.PLAIN: A.table_plain(curve), A.DITHER: A.table_dither(curve)}[mode]
    for w in (32, 64, 480, 1024):
        h = 3
        data = A.random_stream(rng, w, h)
        data[0] = data[1] = 255  # (a large seed; imax, imin untouched)
        data[2] |= 0x3F
        st, img, rows = A.model_decode(data, w, h, mode, table)
        for y in range(h):
            ok, vals = A.stepping_row(data[y * w:(y + 1) * w], w, mode, table)
            assert ok and np.array_equal(img[y], np.array(vals, np.uint16)), (w, y)
