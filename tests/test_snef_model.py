"""The numpy model of NefDecoder::DecodeNikonSNef (tests/snef_files.py) against the unmodified
reference: whole sNEF files through RawParser -> NefDecoder -> DecodeSNefUncompressed, so the
white balance, gammaCurve, the dithering TableLookUp and the pixel loop are all the reference's
own.  Where oracle/_ref is not built those tests skip; tests/golden/snef_ref.json holds the
reference's 4095-entry curve and SHA-256 of its images for a fixed list of seeded cases, and
the model is held against that file everywhere (test_model_matches_recorded_reference never
skips), so a machine without the reference does not depend on its own libm for the curve.
record_golden() rewrites the file from the reference (python tests/test_snef_model.py)."""
import json
import os

import numpy as np
import pytest

import snef_files as S
from oracle_lib import Ref

from snef_files import GOLDEN, fma_case, golden_cases, load_golden

N_FILES = 220


@pytest.fixture(scope="module")
def ref():
    if not Ref.available():
        pytest.skip("oracle/_ref is not built")
    return Ref()


def _model(seed, table):
    w, h, wb_r, wb_b, data = S.make_case(seed)
    return S.model_decode(data, w, h, S.inv_wb(wb_r), S.inv_wb(wb_b), table)


def fused_differences(w, h, data):
    """the green samples of the image at which a fused evaluation gives another 12-bit value"""
    v = S.model_values(data, w, h).reshape(h, w // 2, 6)
    a = np.asarray(data, np.uint8).reshape(h, w // 2, 6).astype(np.int64)
    y = [a[..., 0] | ((a[..., 1] & 15) << 8), (a[..., 1] >> 4) | (a[..., 2] << 4)]
    cb = (a[..., 3] | ((a[..., 4] & 15) << 8)).astype(np.float64)
    cr = ((a[..., 4] >> 4) | (a[..., 5] << 4)).astype(np.float64)
    cb2, cr2 = cb.copy(), cr.copy()
    cb2[:, :-1], cr2[:, :-1] = (cb[:, 1:] + cb[:, :-1]) / 2, (cr[:, 1:] + cr[:, :-1]) / 2
    diff = []
    for k, (b, r) in enumerate(((cb, cr), (cb2, cr2))):
        for row in range(h):
            for g in range(1, w // 2):
                f = S.green_fused(int(y[k][row, g]), float(b[row, g]) - 2048, float(r[row, g]) - 2048)
                if min(max(f, 0), 4095) != v[row, g, 3 * k + 1]:
                    diff.append((row, g, k))
    return diff


def test_the_integer_test_finds_34_pairs_and_16_of_them_are_whole():
    pairs = S.fma_pairs()
    assert len(pairs) == len(set(pairs)) == 34
    assert sum(1 for a, b in pairs if a % 2 == 0 and b % 2 == 0) == 16
    for n1, n2 in pairs:
        assert (337633 * n1 + 698001 * n2) % 2000000 == 0
    # the issue's two examples: unfused 1406 and 730, fused 1407 and 729
    for cb, cr, unfused, fused in ((396, 3764, 1406, 1407), (3011, 3469, 730, 729)):
        assert (2 * (cb - 2048), 2 * (cr - 2048)) in pairs
        d = np.zeros(18, np.uint8)
        S.set_group(d, 6, 0, 0, 2047, 0, cb, cr)
        assert S.model_values(d, 6, 1)[0, 1] == unfused
        assert S.green_fused(2047, cb - 2048, cr - 2048) == fused


def test_planted_pairs_tell_fused_from_unfused():
    """the FMA case would catch a kernel that contracts the green expression"""
    w, h, data = fma_case()
    diff = fused_differences(w, h, data)
    assert len(diff) >= 9, len(diff)
    assert {k for _, _, k in diff} == {0, 1}  # in pixel 1 and, through two neighbours, in pixel 2


def test_jump_matches_stepping():
    rng = np.random.default_rng(3)
    seeds = np.concatenate([[0, 1, 0xFFFFFF, 0x800000], rng.integers(0, 1 << 24, 28)]).astype(np.uint64)
    n = 3 * S.MAX_W  # up to 11 039 steps
    a, b = S.states_by_jump(seeds, n), S.states_by_stepping(seeds, n)
    assert np.array_equal(a, b)
    assert not a[0].any()  # a seed of 0 stays 0
    table = S.arbitrary_table(rng)
    for seed in (0, 5, 10, 21):
        w, h, wb_r, wb_b, data = S.make_case(seed)
        args = (data, w, h, S.inv_wb(wb_r), S.inv_wb(wb_b), table)
        assert np.array_equal(S.model_decode(*args), S.model_decode(*args, jump=False))


def test_cases_cover_what_they_claim():
    res, wbs, zero_seed, clamps = set(), set(), 0, np.zeros((6, 2), bool)
    for seed in range(N_FILES):
        w, h, wb_r, wb_b, data = S.make_case(seed)
        assert w % 2 == 0 and 6 <= w <= S.MAX_W
        res.add(((w // 2) % S.RUN, h))
        wbs.update((S.inv_wb(wb_r), S.inv_wb(wb_b)))
        zero_seed += int((S.row_seeds(data, w, h) == 0).any())
        # an expression outside 0 .. 4095 before the clamp: redo the arithmetic without it
        a = np.asarray(data, np.uint8).reshape(h, w // 2, 6).astype(np.int64)
        cr = ((a[..., 4] >> 4) | (a[..., 5] << 4)) - 2048.0
        cb = (a[..., 3] | ((a[..., 4] & 15) << 8)) - 2048.0
        y1 = (a[..., 0] | ((a[..., 1] & 15) << 8)).astype(np.float64)
        y2 = ((a[..., 1] >> 4) | (a[..., 2] << 4)).astype(np.float64)
        cb2, cr2 = cb.copy(), cr.copy()
        cb2[:, :-1], cr2[:, :-1] = (cb[:, 1:] + cb[:, :-1]) / 2, (cr[:, 1:] + cr[:, :-1]) / 2
        es = [y1 + 1.370705 * cr, y1 - 0.337633 * cb - 0.698001 * cr, y1 + 1.732446 * cb,
              y2 + 1.370705 * cr2, y2 - 0.337633 * cb2 - 0.698001 * cr2, y2 + 1.732446 * cb2]
        for k, e in enumerate(es):
            clamps[k] |= [(e < 0).any(), (e >= 4096).any()]
    assert res == {(r, h) for r in range(S.RUN) for h in (1, 2, 3)}
    assert {S.INV_WB_MIN, S.INV_WB_MAX} <= wbs
    assert zero_seed >= 10 and clamps.all()


def test_white_balance_limits():
    assert S.inv_wb(S.WB_LOW) == S.INV_WB_MAX and S.inv_wb(S.WB_HIGH) == S.INV_WB_MIN
    assert S.INV_WB_MAX * 65535 + 512 <= 2 ** 31 - 1


def test_model_matches_the_reference(ref):
    table = S.host_table()
    for seed in range(N_FILES):
        w, h, wb_r, wb_b, data = S.make_case(seed)
        st, dec = ref.decode_file(S.snef_file(w, h, data, wb_r, wb_b))
        assert st == 0, (seed, ref.last_error())
        assert (dec.cpp, dec.full_w, dec.full_h) == (3, w, h)
        assert np.array_equal(dec.u16()[:h, :3 * w], _model(seed, table)), (seed, w, h)
    w, h, data = fma_case()
    st, dec = ref.decode_file(S.snef_file(w, h, data))
    assert st == 0
    assert np.array_equal(dec.u16()[:h, :3 * w],
                          S.model_decode(data, w, h, S.inv_wb((2, 1)), S.inv_wb((3, 2)), table))


def test_reference_white_balance_check(ref):
    """the bounds of inv_wb in rsx_nikon_snef_validate are the reference's (NefDecoder.cpp:682-687)"""
    d = np.zeros(3 * 8, np.uint8)
    for wb, ok in ((S.WB_LOW, True), (S.WB_TOO_LOW, False), (S.WB_HIGH, True), ((10000001, 1000000), False)):
        st, _ = ref.decode_file(S.snef_file(8, 1, d, wb, (1, 1)))
        assert (st == 0) == ok, wb
        st, _ = ref.decode_file(S.snef_file(8, 1, d, (1, 1), wb))
        assert (st == 0) == ok, wb


def record_golden():
    ref = Ref()
    table = S.host_table()
    rec = {"curve": [int(x) for x in S.host_curve()], "cases": {}}
    for name, w, h, wb_r, wb_b, data in golden_cases():
        st, dec = ref.decode_file(S.snef_file(w, h, data, wb_r, wb_b))
        img = dec.u16()[:h, :3 * w]
        # the curve goes into the file only as the one the reference agreed with
        assert st == 0 and np.array_equal(img, S.model_decode(data, w, h, S.inv_wb(wb_r), S.inv_wb(wb_b), table))
        rec["cases"][name] = {"w": w, "h": h, "inv_wb": [S.inv_wb(wb_r), S.inv_wb(wb_b)],
                              "input": S.sha(data.astype(np.uint16)), "image": S.sha(img)}
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=None, sort_keys=True, separators=(",", ":"))
        f.write("\n")


def test_golden_file_is_current(ref):
    curve, cases = load_golden()
    assert set(cases) == {c[0] for c in golden_cases()}
    for name, w, h, wb_r, wb_b, data in golden_cases():
        st, dec = ref.decode_file(S.snef_file(w, h, data, wb_r, wb_b))
        assert st == 0 and S.sha(dec.u16()[:h, :3 * w]) == cases[name]["image"], name


def test_model_matches_recorded_reference():
    curve, cases = load_golden()
    assert len(curve) == 4095 and len(cases) >= 20
    assert os.path.getsize(GOLDEN) < 1 << 20
    table = S.host_table(curve)
    for name, w, h, wb_r, wb_b, data in golden_cases():
        c = cases[name]
        assert (c["w"], c["h"], c["inv_wb"]) == (w, h, [S.inv_wb(wb_r), S.inv_wb(wb_b)]), name
        assert c["input"] == S.sha(data.astype(np.uint16)), name  # (the seeds give the same bytes)
        img = S.model_decode(data, w, h, c["inv_wb"][0], c["inv_wb"][1], table)
        assert S.sha(img) == c["image"], name


if __name__ == "__main__":
    record_golden()
