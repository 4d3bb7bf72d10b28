"""The Python model of OlympusDecompressor (tests/olympus_files.py) against the reference's
recorded verdicts and hashes (tests/golden/olympus_ref.json, scripts/record_olympus_ref.cpp), the
model's two encoders against the C writers of rawspeed_amd/csrc/synth, the reach statistics of the
case list -- those of the codec's arithmetic and those of the parse kernel's byte window and of
the stream's tail --, and the closed form of the over-read rule against the reader's bookkeeping."""
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


@pytest.mark.parametrize("name", [n for n in NAMES if n not in F.SLOW])
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


DENSE = ["d_%dx%d" % s for s in F.DENSE]
MIXED = "d_mixed_%dx%d" % F.DENSE_MIXED


def test_the_window_model_mirrors_the_kernels_constants():
    k = F.kernel_constants()
    start, top = F.window_top()
    assert 0 < start and top < k["OL_WIN_WORDS"]
    # what OL_BATCH_WORDS reserves in front of a batch against what a batch can load
    assert start + k["OL_BATCH_WORDS"] - 1 - top == 2, "DESIGN.md 4.20 states two words of slack"
    assert (start, top) == (192, 253), "DESIGN.md 4.20 states these"


def test_window_reach():
    """Conditions on the inputs: the dense rows start batches at the last offset that goes without
    a reload and at several next to it, and put a non-zero word at every index of the window's top
    up to the highest one a fill can load; no case loads above it."""
    start, top = F.window_top()
    # the last offset: the 198-wide rows; the sweep: all three widths
    assert start in F.window("d_198x8").starts
    assert {187, 188, 190} <= F.window("d_194x8").starts
    assert {186, 187, 190} <= F.window("d_196x8").starts
    assert {186, 187, 191, 192} <= F.window("d_198x8").starts
    swept = set().union(*(F.window(n).starts for n in DENSE)) & set(range(start - 6, start + 1))
    assert len(swept) >= 5, swept
    # the reload rule itself: OL_BATCH_WORDS has two words of slack, so a rule one or two words
    # too lenient loses nothing; three words too lenient, the 202-wide rows outrun the window
    slack = start + F.kernel_constants()["OL_BATCH_WORDS"] - 1 - top
    assert not any(F.window(n).late_reload_overruns(slack) for n in NAMES)
    assert F.window("d_202x8").late_reload_overruns(slack + 1)
    # every index of the top with data in it: 224 .. 251 by each width, 252 and 253 by 198
    for n in DENSE[:3]:
        assert set(range(F.Window.TOP, top - 1)) <= F.window(n).nonzero, n
    assert set(range(F.Window.TOP, top + 1)) <= F.window("d_198x8").nonzero
    for n in DENSE[:3] + [MIXED]:
        w = F.window(n)
        assert F.expected(n)[0] == F.OK
        assert w.nonzero_top >= 60, (n, w.nonzero_top)
        assert len([1 for j in w.nonzero if j >= 240]) >= 8, n
    for n in NAMES:
        w = F.window(n)
        assert not w.loaded or max(w.loaded) <= top, n
        assert not w.starts or max(w.starts) <= start, n
    # the mixed rows: regular symbols of every length among the 31-bit ones, numLowBits up to 14
    s = F.reach({MIXED})
    assert all(s["nlz_%d" % k] >= 1 for k in range(13))
    assert len([k for k in s if k.startswith("low_bits_")]) >= 10 and s["low_bits_14"] >= 1


@pytest.mark.parametrize("seed", F.TRUNC_SEEDS)
def test_truncated_streams_lie_on_both_sides_of_the_rule(seed):
    """cut 1 .. 6 bytes short the stream still decodes, from zeros behind its end, to another
    image; cut 7 .. 12 bytes short the reader refuses it"""
    names = ["t_%d_cut_%d" % (seed, k) for k in F.TRUNC_CUTS]
    assert [F.expected(n)[0] for n in names] == [F.OK] * 6 + [F.ERR_INPUT_OVERFLOW] * 6
    assert [F.golden()[n]["ok"] for n in names] == [True] * 6 + [False] * 6
    full = F.content("noise16", 6, 6, seed)
    assert F.decode(F.encode(full), 6, 6)[0] == F.OK
    for n in names[:6]:
        changed = int((F.expected(n)[1] != full).sum())
        assert changed >= 1, n
        assert F.window(n).past_end


def test_tail_reach():
    """for every size % 4 an accepted case that consumes bits behind the stream's end, for 1, 2
    and 3 with non-zero bytes in the partial last word; from both seeds"""
    lengths = [len(F.encode(F.content("noise16", 6, 6, s))) - F.SKIP for s in F.TRUNC_SEEDS]
    assert lengths[0] % 4 != lengths[1] % 4
    for by_residue in (["t_901_cut_3", "t_901_cut_2", "t_901_cut_1", "t_901_cut_4"],
                       ["t_902_cut_2", "t_902_cut_1", "t_902_cut_4", "t_902_cut_3"]):
        for r, n in enumerate(by_residue):
            w = F.window(n)
            assert F.expected(n)[0] == F.OK and w.residue == r and w.past_end, n
            assert w.partial_nonzero == (r != 0), n


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
