"""The Python model of the compressed-RAF strip codec (tests/fuji_files.py) against the reference's
recorded answers (tests/golden/fuji_ref.json, scripts/record_fuji_ref.cpp), its encoder against
the C writer (rsx_synth_fuji_encode_strip) byte for byte, its decode of every encoded strip
against the pixels the encoder reached, and the encoder's statistics: every mechanism of the
codec is reached by the case list."""
import functools

import numpy as np
import pytest

import fuji_files as F
from rawspeed_amd import synth

CASES = F.case_list()
GOOD = [c["name"] for c in CASES if c["fault"] is None]


@functools.lru_cache(maxsize=None)
def _model_strips(name):
    """[(bytes, reached pixels, Strip)] of the case's strips from the model's encoder"""
    c, P, lines, img, n = F._built(name)
    return [F.encode_strip(P, lines, img[:, s * F.BLOCK:(s + 1) * F.BLOCK], F.plant_of(c, s))
            for s in range(n)]


def test_case_list_covers_the_shapes_and_types():
    for raw_type, raw_bits in F.TYPES:
        tag = "%s%d" % ("x" if raw_type == 16 else "b", raw_bits)
        shapes = {(c["width"], c["height"]) for c in CASES
                  if c["name"].startswith(tag) and c["fault"] is None}
        assert shapes == set(F.SHAPES)
    assert len(F.golden()) == len(CASES)


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_model_against_the_reference(name):
    g = F.golden()[name]
    rc, sts, px = F.expected(name)
    assert g["ok"] == (rc == F.OK)
    if g["ok"]:
        assert g["sha256"] == F.sha_rows(px)
    else:
        # the reference reports one error for the image: the statuses are the model's
        assert (g["status"], g["strip_status"]) == (rc, sts)
        assert g["model_only"] == (sum(st != F.OK for st in sts) > 1)


@pytest.mark.parametrize("name", [c["name"] for c in CASES
                                  if c["fault"] is None or c["fault"][0] == "plant"])
def test_the_two_encoders_agree_and_the_model_decodes_what_they_reached(name):
    c, P, lines, img, n = F._built(name)
    for s, (data, reached, strip) in enumerate(_model_strips(name)):
        target = img[:, s * F.BLOCK:(s + 1) * F.BLOCK]
        cdata, creached, planted = synth.fuji_encode_strip(c["raw_type"], c["raw_bits"], lines,
                                                           target, F.plant_of(c, s))
        assert cdata == data and np.array_equal(creached, reached)
        assert planted == bool(strip.stats["planted"]) == (F.plant_of(c, s) is not None)
        st, px = F.decode_strip(P, lines, data)
        assert st == (F.ERR_VALUE_RANGE if planted else F.OK)
        assert np.array_equal(px, reached)
        if not P.xtrans and not planted:
            assert np.array_equal(reached, target)  # (every Bayer position is coded)


def test_every_mechanism_is_reached():
    total = {k: 0 for k in F.REACH}
    per_type = {}
    clamps = 0
    indices = [set(), set()]
    no_bits = set()
    for name in GOOD:
        for _, _, strip in _model_strips(name):
            for k in F.REACH:
                total[k] += strip.stats[k]
                per_type.setdefault(name[:3], {k: 0 for k in F.REACH})[k] += strip.stats[k]
            clamps += strip.stats["clamp_low"] + strip.stats["clamp_high"]
            indices[0] |= strip.indices[0]
            indices[1] |= strip.indices[1]
            no_bits |= strip.no_bits_rows
    assert all(total[k] > 0 for k in F.REACH), total
    # per type everything but bitDiff's cap: value1 <= max_diff + n total / 2 against value2 =
    # 1 + n keeps the difference at 14 bits at the most on 14-bit data
    for tag, st in per_type.items():
        assert [k for k in F.REACH if st[k] == 0] == (["bit_diff_15"] if tag[1:] == "14" else []), tag
    assert indices[0] == indices[1] == set(range(41))
    # the X-Trans positions without bits, every (pass, line of the pass, parity) of :710-713
    assert no_bits == {(r, comp, par) for r in range(6) for comp in range(2) for par in range(2)
                       if F.Strip.no_bits(r, par, comp)} and len(no_bits) == 12
    # the two clamps behind the wrap (:498-501) cannot be reached by a code the range check lets
    # through: the prediction lies in [0, q4] and the residual in [-total / 2, total / 2), so the
    # sum is in [-total / 2, q4 + total / 2] and one wrap by total brings it into [0, q4]
    assert clamps == 0


def test_planted_codes_are_in_both_forms():
    for name in ("x14_plant_regular", "b16_plant_regular", "x16_plant_escape", "b14_plant_escape"):
        (data, _, strip), = _model_strips(name)
        assert strip.stats["planted"] == 1 and strip.n_coded >= F.PLANT_AT
        assert F.expected(name)[:2] == (F.ERR_VALUE_RANGE, [F.ERR_VALUE_RANGE])


def test_over_read_rule():
    """a fill at c bits consumed fails iff 4 ceil(c / 32) > size + 8: an all-zero strip of `size`
    bytes fails at the first fill behind that bound, counted here batch by batch"""
    P = F.Params(0, 14)
    for size in (4, 5, 7, 8, 12, 13, 600):
        s = F.Strip(P, 1, data=bytes(size))
        assert s.run() == F.ERR_INPUT_OVERFLOW
        assert s.c % 32 == 0 and 4 * (s.c // 32) > size + 8 >= 4 * (s.c // 32 - 1)
    assert F.Strip(P, 1, data=bytes(3)).run() == F.ERR_IO
