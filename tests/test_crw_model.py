"""The Python model of CrwDecompressor (tests/crw_files.py) against what the unmodified reference
answered for every case (tests/golden/crw_ref.json, recorded by scripts/record_crw_ref.py through
whole CIFF files), what the cases reach, the bound on the carry, and the segment speculation of
rsx_crw.hip as a model: after the rounds and the settling walk it is the serial parse on every
case, whatever the number of rounds."""
import numpy as np
import pytest

import crw_files as F

NAMES = F.case_names()


@pytest.fixture(scope="module")
def golden():
    return F.golden()


def test_the_golden_file_is_of_this_case_list(golden):
    assert sorted(golden["cases"]) == sorted(NAMES)
    for name in NAMES:
        c, g = F.build_case(name), golden["cases"][name]
        assert (g["width"], g["height"], g["table"], g["in_bytes"]) == (
            c["width"], c["height"], c["table"], len(c["data"])), name


@pytest.mark.parametrize("name", NAMES)
def test_model_against_the_reference(golden, name):
    st, px = F.expected(name, True)
    want_st, want_sha = golden["cases"][name]["lowbits"]
    assert st == want_st
    if st == F.OK:
        assert F.sha_rows(px) == want_sha


@pytest.mark.parametrize("name", NAMES)
def test_the_route_without_low_bits(golden, name):
    """the statuses do not depend on the low bits, and where the low bits are all zero (and the
    width is not 2672) the recorded image is this one << 2"""
    c = F.build_case(name)
    st, px = F.expected(name, False)
    assert st == golden["cases"][name]["lowbits"][0]
    if st == F.OK and golden["cases"][name]["zero_low"] and c["width"] != 2672:
        assert F.sha_rows(px.astype(np.uint16) << 2) == golden["cases"][name]["lowbits"][1]


def test_the_validation_cases_against_the_reference(golden):
    for name, w, h, table, low_short, cpp, pitch, want in F.VALIDATION:
        got = F.validate(w, h, table, True, max(0, w * h // 4) - low_short, 64, cpp, pitch)
        assert got == want, name
        if name in golden["validation"]:
            assert golden["validation"][name] == want, name
    assert {"width_0", "width_6", "width_4104", "width_4108", "height_0", "height_3048",
            "height_3049", "area_4x4", "table_3"} <= set(golden["validation"])


def test_every_reach_counter_is_above_zero():
    for name in NAMES:
        F.expected(name, True)
    zero = sorted(k for k, v in F.REACH.items() if v == 0)
    assert not zero, zero


def test_the_carry_stays_far_from_the_int16_wrap():
    """a pixel in range bounds |carry| below 2048 and one step adds less than 2048, so the range
    check fires before diffBuf[0] += carry can wrap (the model asserts it in every block)"""
    for name in NAMES:
        F.expected(name, True)
    assert 0 < F.REACH["max_carry"] < 4096


def test_the_long_streams_span_at_least_three_windows():
    for name in ("noise_1024x256_t0", "noise_1024x256_t1", "noise_1024x256_t2", "nonzero_1024x256"):
        data, _ = F.unstuff(F.build_case(name)["data"])
        assert 8 * len(data) >= 3 * F.WIN_BITS, name
    # the stream of non-zero coefficients has no 00 in it: no block ends early
    reach = F.new_reach()
    c = F.build_case("nonzero_1024x256")
    assert F.decode(c["width"], c["height"], c["table"], c["data"], None, reach)[0] == F.OK
    assert reach["eob"] == 0 and reach["zero_at_0"] == 0


# (segment bits, window segments): the shipped ones on the streams that span windows, small ones
# on everything so that every case has many segments and windows
SMALL = (64, 4)


def _speculation_case(name, seg_bits, win_segs, rounds):
    c = F.build_case(name)
    if len(c["data"]) < 8:
        return None
    data, _ = F.unstuff(c["data"])
    bits = F.Bits(data, 64 + seg_bits // 8 + 8)  # (a segment that is only ever peeked into)
    n_segs = (8 * (len(data) + 64) + seg_bits - 1) // seg_bits
    want = F.serial_entries(bits, c["table"], n_segs, seg_bits)
    got, stats = F.speculate(bits, c["table"], n_segs, seg_bits, win_segs, rounds)
    assert got == want, (name, seg_bits, win_segs, rounds)
    return stats


# the streams of several windows at the shipped sizes: they run there, for every round count
LONG = ("noise_1024x256_t0", "noise_1024x256_t1", "noise_1024x256_t2", "nonzero_1024x256")


@pytest.mark.parametrize("rounds", [0, 1, 4])
def test_speculation_equals_the_serial_parse_small_segments(rounds):
    """every case but the four long streams (no case of fewer than 8 bytes has a scan to parse)"""
    ran = 0
    for name in NAMES:
        if name not in LONG:
            ran += _speculation_case(name, SMALL[0], SMALL[1], rounds) is not None
    assert ran == len(NAMES) - len(LONG) - 1  # (reader_7_bytes)


@pytest.mark.parametrize("rounds", [0, 1, 4])
@pytest.mark.parametrize("name", LONG + ("edge_code_straddles_window",
                                         "reader_ff_across_window_edge"))
def test_speculation_equals_the_serial_parse_shipped_segments(name, rounds):
    stats = _speculation_case(name, F.SEG_BITS, F.WIN_SEGS, rounds)
    if name in LONG:
        assert stats[0] >= 3
    assert stats[2] <= rounds
    if rounds == 0:
        assert stats[3] == 1  # (a guessed head is not the truth: the walk has work)


def test_the_inlined_segment_parse_is_the_symbol_step():
    """parse_segment (what the speculation model runs) against symbol() a symbol at a time, from
    the true entry and from the guess, bad codes included"""
    for name in ("noise_68x16_t0_wide", "noise_68x16_t1_wide", "noise_68x16_t2_wide",
                 "sym_extend_ends_t0", "sym_run_passes_63_bits_dropped", "sym_run_passes_63_len0",
                 "sym_00_at_63", "verdict_bad_code_middle", "reader_marker_mid_frame"):
        c = F.build_case(name)
        data, _ = F.unstuff(c["data"])
        bits = F.Bits(data, 64 + 16)
        n_segs = (8 * (len(data) + 64) + 63) // 64
        for s, e in enumerate(F.serial_entries(bits, c["table"], n_segs, 64)):
            for entry in (e, (0, 1), (3, 63), (0, 0)):
                assert (F.parse_segment(bits, c["table"], s, entry, 64) ==
                        F.parse_segment_by_symbols(bits, c["table"], s, entry, 64)), (name, s, entry)
