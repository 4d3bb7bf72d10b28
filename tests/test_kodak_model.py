"""The Python model of KodakDecompressor (tests/kodak_files.py) against the reference's recorded
answers (tests/golden/kodak_ref.json) on every case, both routes; the reach counters that show
every edge of the case list was hit; the closed forms of include/rsx.h section 3w against the
literal reader on random segments; and, where oracle/_ref is built, the recorder's comparison
replayed live."""
import hashlib
import os
import random
import sys

import numpy as np
import pytest

import kodak_files as F
from oracle_lib import Ref

NAMES = F.names()


def test_status_codes_are_the_library_s():
    F._status_codes()


def test_golden_covers_the_case_list():
    g = F.golden()
    assert sorted(g) == sorted(NAMES)
    for name in NAMES:
        c = F.case(name)
        assert (g[name]["width"], g[name]["height"], g[name]["bps"]) == \
            (c["width"], c["height"], c["bps"])
        assert g[name]["in_bytes"] == len(F.build_case(name)["data"])


@pytest.mark.parametrize("name", NAMES)
def test_model_against_the_reference_s_record(name):
    g = F.golden()[name]
    for route, mode in (("uncorrected", F.NONE), ("corrected", F.DITHER)):
        st, px = F.expected(name, mode)
        assert st == g[route][0], route
        if st == F.OK:
            assert F.sha_rows(px) == g[route][1], route
        else:
            assert g[route][1] is None


def test_every_edge_is_reached():
    stats = F.reach()
    missing = [k for k in F.REACH if stats[k] == 0]
    assert not missing, missing


def test_the_case_list_covers_every_shape_and_verdict():
    cases = {c["name"]: c for c in F.case_list()}
    widths = {c["width"] for c in cases.values()}
    heights = {c["height"] for c in cases.values()}
    assert {4, 12, 252, 256, 260, 264, 516, 4516} <= widths
    assert {1, 2, 65, 130} <= heights
    assert {c["bps"] for c in cases.values()} == {10, 12}
    assert len(F.build_case("g_264x300_long")["data"]) > 65535
    statuses = {F.model_values(n)[0] for n in NAMES}
    assert statuses == {F.OK, F.ERR_IO, F.ERR_VALUE_RANGE}
    # the order of the verdicts
    assert F.model_values("o_range_then_cut")[0] == F.ERR_VALUE_RANGE
    assert F.model_values("o_cut_then_range")[0] == F.ERR_IO
    assert F.model_values("o_same_segment")[0] == F.ERR_IO
    # a stream that ends at its last segment's last byte, with and without bytes behind it
    b = F.build_case("t_exact")
    assert len(b["data"]) == len(b["whole"]) == F.model_values("t_exact")[2]
    b = F.build_case("t_exact_trailing")
    assert len(b["data"]) == len(b["whole"]) + 91
    assert F.model_values("t_exact_trailing")[2] == len(b["whole"])
    assert F.model_values("t_last_byte")[0] == F.ERR_IO
    # one below area / 2 is the constructor's refusal
    for name in ("t_below_half", "t_below_half_516"):
        c = cases[name]
        assert len(F.build_case(name)["data"]) == c["width"] * c["height"] // 2 - 1


def test_the_wild_curve_tells_the_table_modes_apart():
    for bps in (10, 12):
        c = F.curve("wild", bps)
        assert (np.diff(c.astype(np.int64)) < 0).any(), "not monotonic"
        d = F.dither_table(c)
        v = np.arange(1 << bps)
        assert (d[1::2] > 4096).any(), "large deltas"
        assert (d[2 * v] != c[v]).mean() > 0.5, "the base is not the curve"
        assert (d[v] != d[2 * v]).mean() > 0.5, "tables[v] is not tables[2 v]"
        # what a decoder that did dither would store for a generator other than 0
        r = 1234
        dithered = d[2 * v].astype(np.int64) + ((d[2 * v + 1].astype(np.int64) * (r & 2047) + 1024) >> 12)
        assert (dithered != d[2 * v]).mean() > 0.3
    assert F.dither_table(F.curve("camera", 12)).size == 8192
    assert F.plain_table(F.curve("camera", 10)).size == 1024


def test_closed_forms_against_the_literal_reader_on_random_segments():
    rng = random.Random(20)
    for trial in range(400):
        length = rng.choice([4, 8, 12, 20, 100, 252, 256])
        top = rng.choice([0, 1, 3, 7, 15, 15])
        lens = [rng.randint(0, top) for _ in range(length)]
        if trial % 7 == 0:  # sums around a read of 4 bytes
            lens = [0] * length
            for _ in range(rng.choice([15, 16, 17, 31, 32, 33, 47, 48, 49])):
                i = rng.randrange(length)
                if lens[i] < 15:
                    lens[i] += 1
        fields = [rng.getrandbits(n) if n else 0 for n in lens]
        data = F.encode_segment(lens, fields, rng)
        assert len(data) == F.segment_bytes(length, sum(lens)) <= F.segment_bound(length)
        s = F._Stream(data)
        diffs, blen = F.read_segment(s, length)
        assert blen == lens and s.pos == len(data)
        assert diffs == [F.extend(f, n) for f, n in zip(fields, lens)]
        assert F.closed_segment(data + b"\x55", 0, length) == (diffs, len(data))
        # one byte short, wherever that falls: both refuse
        assert F.closed_segment(data[:-1], 0, length) is None
        with pytest.raises(F.Eof):
            F.read_segment(F._Stream(data[:-1]), length)


def test_the_reader_never_holds_32_spare_bits():
    """why r = ceil(max(0, sum - init) / 32): a read happens only when the bits held are fewer
    than the next length, and a length is at most 15"""
    for length in (4, 8, 12, 256):
        for total in range(0, 15 * length + 1):
            init = F.init_bits(length)
            r = (max(0, total - init) + 31) // 32
            assert init + 32 * r >= total
            assert r == 0 or init + 32 * (r - 1) < total
            assert F.segment_bytes(length, total) == length // 2 + init // 8 + 4 * r


def test_image_bound_is_never_exceeded():
    for name in NAMES:
        c = F.case(name)
        assert len(F.build_case(name)["whole"]) <= F.image_bound(c["width"], c["height"])
    assert F.image_bound(4516, 3012) == 3012 * (17 * 610 + (82 + 2 + 4 * 77))


def test_the_c_writer_and_the_model_agree():
    from rawspeed_amd import synth
    rng = np.random.RandomState(5)
    for w, h in ((4, 3), (12, 5), (260, 4), (516, 3), (256, 2)):
        target = rng.randint(0, 4096, (h, w)).astype(np.uint16)
        data = synth.kodak_encode(target)
        st, px, consumed = F.decode(data, w, h, 12)
        assert st == F.OK and consumed == len(data)
        assert np.array_equal(px, target)


@pytest.mark.skipif(not Ref.available(), reason="oracle/_ref not built")
def test_the_recorder_s_comparison_live():
    sys.path.insert(0, os.path.join(os.path.dirname(F.HERE), "scripts"))
    import record_kodak_ref as R
    ref = Ref()
    g = F.golden()
    for name in NAMES:
        entry, wrong = R.compare(ref, name)
        assert not wrong, wrong
        assert entry["uncorrected"] == g[name]["uncorrected"]
        assert entry["corrected"] == g[name]["corrected"]


def test_whole_files_are_what_dcr_decoder_reads():
    blob = F.case_file("g_12x2").tobytes()
    data = F.build_case("g_12x2")["data"]
    assert blob.endswith(data), "the strip is the last thing in the file"
    assert hashlib.sha256(F.case_file("g_12x2").tobytes()).digest() == hashlib.sha256(blob).digest()
    assert b"Kodak\0" in blob
