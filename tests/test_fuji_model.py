"""The Python model of the compressed-RAF strip codec (tests/fuji_files.py) against the reference's
recorded answers (tests/golden/fuji_ref.json, scripts/record_fuji_ref.cpp), its encoder against
the C writer (rsx_synth_fuji_encode_strip) byte for byte, its decode of every encoded strip
against the pixels the encoder reached, and the encoder's statistics: every mechanism of the
codec is reached by the case list -- and, by a model of the device's window schedule
(fuji_files.Schedule), every mechanism that exists in the kernel only."""
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
        last = {F.header(0, 14, w, h)["raw_width"] - F.BLOCK * (-(-w // F.BLOCK) - 1)
                for w, h in shapes}
        assert last == {768, 24, 48, 384, 744}  # the widths of the frames' last strips
        # the long escapes, the zero tails at every size % 4, the failing strips with a neighbour
        faults = sorted((c["fault"][0], c["fault"][2]) for c in CASES
                        if c["name"].startswith(tag) and c["fault"] and c["width"] == 768
                        and c["fault"][0] in ("long_escape", "zero_tail"))
        P = F.Params(raw_type, raw_bits)
        runs = [P.max_bits - raw_bits, 96, F.LONG_MEDIUM[tag][0], 20000]
        runs += [(1 << 20) + 40] if tag in ("x14", "b16") else []
        assert [a[0] for k, a in faults if k == "long_escape"] == sorted(runs)
        assert 4096 <= F.LONG_MEDIUM[tag][0] <= 16384 and F.LONG_MEDIUM[tag][0] % 32 == 0
        assert [a for k, a in faults if k == "zero_tail"] == [2400, 2401, 2402, 2403]
        assert sorted((c["fault"][0], c["fault"][2]) for c in CASES if c["name"].startswith(tag)
                      and c["fault"] and c["fault"][1] == 0 and c["width"] == 1560) == [
            ("cut", -9), ("cut", -8), ("cut", -4), ("zero_tail", 2401), ("zero_tail", 2403)]
    assert len(F.golden()) == len(CASES) == len({c["name"] for c in CASES})


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


@pytest.mark.parametrize("name", [c["name"] for c in CASES if c["fault"] is None
                                  or c["fault"][0] in ("plant", "long_escape")])
def test_the_two_encoders_agree_and_the_model_decodes_what_they_reached(name):
    c, P, lines, img, n = F._built(name)
    for s, (data, reached, strip) in enumerate(_model_strips(name)):
        target = img[:, s * F.BLOCK:(s + 1) * F.BLOCK]
        cdata, creached, planted = synth.fuji_encode_strip(c["raw_type"], c["raw_bits"], lines,
                                                           target, F.plant_of(c, s))
        assert cdata == data and np.array_equal(creached, reached)
        assert planted == bool(strip.stats["planted"]) == (F.plant_of(c, s) is not None)
        assert F.build_case(name)["strips"][s] == data
        st, px, _ = F.traced(name, s)  # (the decode test_every_device_mechanism_is_reached reads)
        stops = planted and c["fault"][0] == "plant"
        assert st == (F.ERR_VALUE_RANGE if stops else F.OK)
        assert np.array_equal(px, reached)
        if not P.xtrans and not stops:
            assert np.array_equal(reached, target)  # (every Bayer position is coded)


def test_a_long_escape_changes_the_bytes_and_not_the_pixels():
    for raw_type, raw_bits in F.TYPES:
        tag = "%s%d" % ("x" if raw_type == 16 else "b", raw_bits)
        P = F.Params(raw_type, raw_bits)
        escape_at = P.max_bits - raw_bits - 1
        names = [c["name"] for c in CASES if c["name"].startswith(tag + "_long")]
        # the same strip without the plant
        plain, reached, base = F.encode_strip(P, 1, F._built(names[0])[3])
        for name in names:
            z, at = F._built(name)[0]["fault"][2]
            (data, px, strip), = _model_strips(name)
            assert strip.stats["planted"] == 1 and strip.n_coded == base.n_coded > at
            assert np.array_equal(px, reached)
            # Z zeros, a 1 and raw_bits bits in the place of 1 to escape_at + 1 + raw_bits bits
            grown = 8 * (len(data) - len(plain))
            assert z - escape_at - 8 < grown < z + raw_bits + 8
            rc, sts, got = F.expected(name)
            assert (rc, sts) == (F.OK, [F.OK]) and np.array_equal(got, reached)


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


def test_every_device_mechanism_is_reached():
    """what exists in fuji_strip_kernel only -- the chunks, the window and its refills, the
    fallback read outside the window, the saturating zero count -- over the cases the device tests
    run, by the model's trace of every strip's decode (conditions, not measurements)"""
    K = F.device_constants()
    assert (K["FJ_WIN"], K["FJ_CHUNK_WORDS"]) > (0, 0) and K["FJ_CHUNK_WORDS"] < K["FJ_WIN"]
    seen = set()
    for c in CASES:
        for s in range(F._built(c["name"])[4]):
            data = F.build_case(c["name"])["strips"][s]
            if len(data) < 4:
                continue  # (refused in front of the walk)
            st, _, t = F.traced(c["name"], s)
            assert (t.failed is not None) == (st == F.ERR_INPUT_OVERFLOW)
            for first, left, spans in t.refills:
                seen.add("refill_first_chunk" if first else "refill_later_chunk")
                if left is not None and left > K["FJ_WIN"]:
                    seen.add("refill_behind_a_run_that_left_the_window")
                if spans:
                    seen.add("window_spans_end_%d" % (len(data) % 4))
            if len(t.refills) >= 50:
                seen.add("50_refills")
            if t.runs_ok:
                seen.add("fallback_in_run_sample_ok")
            for k, in_zeros, bytewise in t.fallback:
                if not in_zeros:
                    seen.add("fallback_outside_the_zero_loop")
                if bytewise:
                    seen.add("fallback_bytewise")
            if t.failed and t.failed[1]:
                seen.add("fallback_failing_fill_%d" % (len(data) % 4))
            if t.max_zeros > K["ZEROS_CAP"]:
                assert st == F.OK
                seen.add("zeros_over_cap")
    want = {"refill_first_chunk", "refill_later_chunk", "50_refills", "fallback_in_run_sample_ok",
            "fallback_outside_the_zero_loop", "refill_behind_a_run_that_left_the_window",
            "fallback_bytewise", "zeros_over_cap"}
    want |= {"fallback_failing_fill_%d" % r for r in range(4)}
    want |= {"window_spans_end_%d" % r for r in (1, 2, 3)}
    assert want <= seen, sorted(want - seen)
    # the medium run of every type is shorter than the window, leaves it, and its chunk goes on
    for tag, (z, at) in F.LONG_MEDIUM.items():
        st, _, t = F.traced("%s_long%d" % (tag, z), 0)
        assert st == F.OK and z // 32 < K["FJ_WIN"] and t.runs_ok
        assert sum(not f[1] for f in t.fallback) >= 5
        assert any(left is not None and left > K["FJ_WIN"] for _, left, _ in t.refills)
    # the zero tails start in window 0 and fail outside it, at word 828
    for c in CASES:
        if c["fault"] and c["fault"][0] == "zero_tail" and c["width"] == 768:
            st, _, t = F.traced(c["name"], 0)
            assert st == F.ERR_INPUT_OVERFLOW and t.failed == (828, True) and len(t.refills) == 1


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
