"""The Python model of OlympusDecompressor (tests/olympus_files.py) against the reference's
recorded verdicts and hashes (tests/golden/olympus_ref.json, scripts/record_olympus_ref.cpp), the
model's two encoders against the C writers of rawspeed_amd/csrc/synth, the reach statistics of the
case list, and the closed form of the over-read rule against the reader's bookkeeping."""
import numpy as np
import pytest

import olympus_files as F
from rawspeed_amd import synth

CASES = F.case_list()
NAMES = [c["name"] for c in CASES]


def test_status_codes_are_the_headers():
    F._status_codes()


def test_the_golden_file_covers_the_case_list():
    g = F.golden()
    assert sorted(g) == sorted(NAMES)
    for c in CASES:
        e = g[c["name"]]
        if c["kind"] == "refused":
            # the constructor refuses: no image, no hash
            assert not e["ok"] and "sha256" not in e and e["exception"] == "RawDecoderException"
        assert e["ok"] == ("sha256" in e)
    assert "model_only" not in open(F.GOLDEN).read()


@pytest.mark.parametrize("name", NAMES)
def test_model_against_the_reference(name):
    g = F.golden()[name]
    rc, px = F.expected(name)
    assert g["ok"] == (rc == F.OK)
    if g["ok"]:
        assert F.sha_rows(px) == g["sha256"]
    else:
        want = {F.ERR_INVALID_ARG: "RawDecoderException", F.ERR_IO: "IOException",
                F.ERR_INPUT_OVERFLOW: "IOException"}[rc]
        assert g["exception"] == want
        assert ("overflow" in g["message"].lower()) == (rc == F.ERR_INPUT_OVERFLOW)
        assert ("MaxProcessBytes" in g["message"]) == (name in ("r_2x2_7_bytes", "r_2x2_10_bytes"))


@pytest.mark.parametrize("name", [c["name"] for c in CASES if c["kind"] == "pixels"])
def test_a_pixel_case_decodes_to_its_target(name):
    c = F.case(name)
    rc, px = F.expected(name)
    assert rc == F.OK
    assert np.array_equal(px, F.content(c["content"], c["width"], c["height"], c["seed"]))


@pytest.mark.parametrize("name", [n for n in NAMES if not n.startswith("f_1024")])
def test_the_two_encoders_write_the_same_bytes(name):
    assert F.build_case(name, "c")["data"] == F.build_case(name, "model")["data"]


def test_the_two_encoders_on_a_mid_size_image():
    img = F.content("noise16", 96, 64, 7)
    data = synth.olympus_encode(img)
    assert data == F.encode(img)
    rc, px = F.decode(data, 96, 64)
    assert rc == F.OK and np.array_equal(px, img)


def test_reach_statistics():
    s = F.reach()
    for k in F.REACH_ITEMS + F.REACH_PRED:
        assert s[k] >= 1, k
    for k in range(13):
        assert s["nlz_%d" % k] >= 1, k
    for k in range(2, 15):
        assert s["low_bits_%d" % k] >= 1, k
    assert not [k for k in s if k.startswith("low_bits_") and not 2 <= int(k[9:]) <= 14]
    # L + (U - NW) lies between U and L where the two differences have opposite signs
    assert s["l_plus_b_out_of_range"] == 0


@pytest.mark.parametrize("plant,keys", [
    ("low_bits_2", ["low_bits_2"]), ("low_bits_14", ["low_bits_14"]),
    ("bias_switch", ["c2_2_to_3", "low_bits_5"]), ("carry0_16_17", ["c0_is_16", "c0_is_17"]),
    ("truncation", ["truncation_changes_low_bits"]), ("escape_high_1", ["escape_high_bits_1"]),
    ("escape_high_13", ["escape_high_bits_13"]), ("symbol_31", ["symbol_31_bits"]),
    ("negative_carry1", ["negative_carry1_rounds_down"]),
    ("row_reset_off_byte", ["row_start_off_byte"]),
    ("every_high", ["nlz_%d" % k for k in range(12)]),
    ("odd_low_bits", ["low_bits_%d" % k for k in (3, 5, 7, 9, 11, 13)])])
def test_a_planted_stream_reaches_its_item(plant, keys):
    s = F.reach({"p_" + plant})
    for k in keys:
        assert s[k] >= 1, (k, dict(s))


def test_the_predictor_image_reaches_every_branch():
    s = F.reach({"c_%dx4_predictor" % (4 * len(F.PRED_PAIRS))})
    for k in F.REACH_PRED[:-2]:
        assert s[k] >= 1, k
    s = F.reach({"c_130x6_wrap"})
    assert s["wrap_above"] >= 1 and s["wrap_below"] >= 1


def test_over_read_rule():
    """the closed form 4 ceil(c / 32) > size + 8 against the reader's books (words loaded, level)
    on symbol lengths of every kind, and the verdicts of the cut family on both sides of it"""
    rng = np.random.default_rng(11)
    for size in list(range(4, 40)) + [1000, 1001, 1002, 1003]:
        pos, loaded, level = 0, 0, 0
        for used in rng.integers(4, 32, 400):
            failed = False
            if level < 32:
                failed = 4 * loaded > size + 8
                loaded += 1
                level += 32
            assert failed == F.fill_fails(pos, size), (size, pos)
            assert failed == (pos > F.host_lib().rsx_olympus_host_fill_limit(size))
            if failed:
                break
            pos += int(used)
            level -= int(used)
        else:
            assert size >= 1000
    verdicts = [F.expected("r_cut_%d" % k)[0] for k in range(6)]
    assert verdicts == [F.OK] + [F.ERR_INPUT_OVERFLOW] * 5
    assert [F.golden()["r_cut_%d" % k]["ok"] for k in range(6)] == [True] + [False] * 5
    lengths = [len(F.build_case("r_cut_%d" % k)["data"]) for k in range(6)]
    assert lengths == list(range(lengths[0], lengths[0] - 6, -1))


def test_reader_refusals():
    assert [F.expected("r_2x2_%d_bytes" % n)[0] for n in (6, 7, 10, 11)] == \
        [F.ERR_IO, F.ERR_IO, F.ERR_IO, F.OK]
    assert not F.expected("r_2x2_11_bytes")[1].any()  # (zero is the escape form of value 0)
    for name in ("r_130x6_zeros", "r_130x6_ones"):
        assert F.expected(name)[0] == F.OK
