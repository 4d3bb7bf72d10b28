"""The numpy model of VC5Decompressor (tests/vc5_files.py) against the unmodified reference: whole
compression-9 DNG files through RawParser -> DngDecoder -> AbstractDngDecompressor ->
VC5Decompressor, so the tag parse, the code book, the log table, the band decode, the wavelets
and the merge are all the reference's own.  Where oracle/_ref is not built those tests skip;
tests/golden/vc5_ref.json holds the SHA-256 of the reference's images, its verdicts and the log
tables of the white levels used, and the model is held against that file everywhere
(test_model_matches_recorded_reference never skips), so a machine without the reference does not
depend on its own libm for the curve.  record_golden() rewrites the file from the reference
(python tests/test_vc5_model.py)."""
import json
import os

import numpy as np
import pytest

import vc5_files as V
from oracle_lib import Ref


@pytest.fixture(scope="module")
def ref():
    if not Ref.available():
        pytest.skip("oracle/_ref is not built")
    return Ref()


def _ref_decode(ref, tile):
    blob, data, bands = tile.dng()
    st, dec = ref.decode_file(blob)
    img = None
    if st == 0 and dec is not None and not dec.errors():
        img = dec.u16()[:tile.h, :tile.w].copy()
    return img, data, bands


def test_code_book_is_what_the_library_takes():
    b = V.book()
    assert len(b) == 264 and all(len(r) == 4 for r in b)
    assert all(1 <= s <= 26 and 0 <= bits < (1 << s) and 0 <= n <= 511 and 0 <= v <= 1023
               for s, bits, n, v in b)
    starts = sorted((bits << (26 - s), 1 << (26 - s)) for s, bits, n, v in b)
    assert all(a + n <= c for (a, n), (c, _) in zip(starts, starts[1:]))        # prefix-free
    assert sum(n for _, n in starts) == 1 << 26                                  # and complete
    assert [r for r in b if r[2] == 0] == [(26, 0x3114BA3, 0, 1)]                # the end marker
    assert sorted(r[2] for r in b if r[2] > 1) == sorted(V.RUNS[:-1])


def test_recorded_cases_use_every_row_with_both_signs():
    used = set()
    by_key = {(s, bits): i for i, (s, bits, n, v) in enumerate(V.book())}
    for name, tile in V.golden_cases():
        if name != "every_row":
            continue
        for c in range(4):
            for s in range(1, 10):
                bits = V.bit_string(tile.chunks[c][s])
                pos, n, p = 0, None, 0
                while True:
                    size, count, value, length = V.read_symbol(bits, pos)
                    used.add((by_key[(size, int(bits[pos:pos + size], 2))], value < 0))
                    if count == 0:
                        break
                    pos += length
    rows = {r for r, _ in used}
    assert rows == set(range(264))
    assert all((i, True) in used and (i, False) in used
               for i, (s, b, n, v) in enumerate(V.book()) if v != 0 and n == 1)


def test_fast_writer_matches_the_plain_one():
    rng = np.random.default_rng(3)
    for density in (0.0, 0.02, 0.5, 1.0):
        v = V.random_band(rng, 61, 47, density, 1023)
        assert np.array_equal(V.encode_values_fast(v), V.encode_values(v))


def test_model_matches_the_reference(ref):
    for name, tile in V.golden_cases():
        img, data, bands = _ref_decode(ref, tile)
        st, want, _ = V.model_decode(tile, data, bands)
        assert st == V.OK and img is not None, (name, ref.last_error())
        assert np.array_equal(img, want), name


def test_model_fails_where_the_reference_fails(ref):
    for name, tile, expect in V.failing_cases():
        img, data, bands = _ref_decode(ref, tile)
        st, want, _ = V.model_decode(tile, data, bands)
        assert (st == V.OK) == (img is not None), (name, st)
        if expect is not None:
            assert st == expect, (name, st)
        if img is not None:
            assert np.array_equal(img, want), name


def record_golden():
    ref = Ref()
    rec = {"tables": {str(w): [int(x) for x in V.log_table(w)] for w in V.WHITES}, "cases": {},
           "failing": {}}
    for name, tile in V.golden_cases():
        img, data, bands = _ref_decode(ref, tile)
        st, want, _ = V.model_decode(tile, data, bands)
        # the tables go into the file only as the ones the reference agreed with
        assert st == V.OK and img is not None and np.array_equal(img, want), name
        rec["cases"][name] = {"w": tile.w, "h": tile.h, "white": tile.white,
                              "input": V.sha(data.astype(np.uint16)), "image": V.sha(img)}
    for name, tile, expect in V.failing_cases():
        img, data, bands = _ref_decode(ref, tile)
        rec["failing"][name] = {"input": V.sha(data.astype(np.uint16)),
                                "image": None if img is None else V.sha(img)}
    with open(V.GOLDEN, "w") as f:
        json.dump(rec, f, indent=None, sort_keys=True, separators=(",", ":"))
        f.write("\n")


def test_golden_file_is_current(ref):
    rec = V.load_golden()
    assert set(rec["cases"]) == {n for n, _ in V.golden_cases()}
    assert set(rec["failing"]) == {n for n, _, _ in V.failing_cases()}
    for name, tile in V.golden_cases():
        img, _, _ = _ref_decode(ref, tile)
        assert img is not None and V.sha(img) == rec["cases"][name]["image"], name


def test_model_matches_recorded_reference():
    rec = V.load_golden()
    assert os.path.getsize(V.GOLDEN) < 1 << 20 and len(rec["cases"]) >= 19
    tables = {int(k): np.array(v, np.uint16) for k, v in rec["tables"].items()}
    assert set(tables) == set(V.WHITES) and all(t.size == 4096 for t in tables.values())
    for name, tile in V.golden_cases():
        c = rec["cases"][name]
        data, bands = tile.vc5_block()
        assert (c["w"], c["h"], c["white"]) == (tile.w, tile.h, tile.white), name
        assert c["input"] == V.sha(data.astype(np.uint16)), name  # (the seeds give the same bytes)
        st, img, _ = V.model_decode(tile, data, bands, tables[tile.white])
        assert st == V.OK and V.sha(img) == c["image"], name
    for name, tile, expect in V.failing_cases():
        c = rec["failing"][name]
        data, bands = tile.vc5_block()
        assert c["input"] == V.sha(data.astype(np.uint16)), name
        st, img, _ = V.model_decode(tile, data, bands, tables[tile.white])
        assert (st == V.OK) == (c["image"] is not None), name
        if img is not None:
            assert V.sha(img) == c["image"], name


if __name__ == "__main__":
    record_golden()
