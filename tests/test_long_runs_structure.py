"""The planned inputs of tests/long_runs.py have exactly their planned resets.  No GPU needed.

This is the condition that gives the device tests on these inputs (test_gpu_long_runs.py) their
meaning: a header walk over every encoded row finds the raw groups (Phase One) or the upward
blocks (Samsung V0) exactly where the plan put them and nowhere else, and the longest run without
one is the planned one -- the whole row, 1497 groups at w = 11976 and 347 blocks at w = 5546, for
the plans without a reset.  The same walk over the random inputs of test_gpu_phase_one.py and
test_gpu_samsung_v0.py finds at most 123 groups of 1496 (18 .. 39 with the non-zero `choices`)
and 19 blocks of 347 (27 in the largest frame).  An encoder change that turned a planned free
run into a reset-dense one fails here."""
import numpy as np
import pytest

import iiq_files as I
import long_runs as L
import srw_v0_files as S
import test_samsung_v0_model as M


def _planned_run(resets_per_sequence, n):
    """the longest run of 0 .. n - 1 without a planned reset, over the sequences (counted here
    position by position, not with the helper under test)"""
    best = 0
    for resets in resets_per_sequence:
        run = 0
        for k in range(n):
            run = 0 if k in resets else run + 1
            best = max(best, run)
    return best


# ---- Phase One ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.p1_files(), ids=lambda c: c[0])
def test_phase_one_rows_have_exactly_their_planned_raw_groups(case):
    name, w, pattern, keep, plans = case
    ng = w >> 3
    img, rows, _ = L.p1_build(case)
    assert img.shape == (len(plans), w) and len(rows) == len(plans)
    longest = {}
    for (plan_name, plan), row in zip(plans, rows):
        even, odd, keeps = I.header_walk(row, w)
        assert (tuple(even), tuple(odd)) == (tuple(plan[0]), tuple(plan[1])), (name, plan_name)
        # (the plain encoder never keeps; the all-keep one does nothing else behind group 0)
        assert keeps == (2 * (ng - 1) if keep else 0), (name, plan_name, keeps)
        run = max(I.longest_free_run(even, ng), I.longest_free_run(odd, ng))
        assert run == _planned_run(plan, ng), (name, plan_name)
        longest[plan_name] = run
    # one parity of every plan but "early" is free from the first group to the last
    assert all(run == ng for n, run in longest.items() if n != "early"), longest
    assert longest.get("early", ng - 10) == ng - 10
    if w == 11976:
        assert longest["none"] == 1497
    if w == 11974:
        assert longest["none"] == 1496 and w & 7 == 6 and ng % 8 == 0  # (the tail: a lane of its own)


def test_phase_one_plans_reach_every_lane_and_wave_edge():
    names = {w: dict(L.p1_plans(w)) for w in L.P1_WIDTHS}
    assert set(names) == {4096, 4160, 8192, 8256, 11976, 11974, 11966}
    for w, plans in names.items():
        groups = {g for e, o in plans.values() for g in e + o}
        ng = w >> 3
        assert {0, 511, ng - 1, 9, 12} <= groups
        assert (512 in groups) == (ng > 512) and (1023 in groups) == (ng > 1023)
        assert (1024 in groups) == (ng > 1024)
        assert any(g % 8 == 3 for g in groups) and any(g % 8 == 4 for g in groups)
        for parity in (0, 1):  # every single group in either parity alone
            singles = {p[parity][0] for p in plans.values() if len(p[parity]) == 1 and not p[1 - parity]}
            assert {g for g in (0, 511, 512, 1023, 1024, ng - 1) if g < ng} <= singles
    kinds = {(pattern, keep) for _, _, pattern, keep, _ in L.p1_files()}
    assert kinds == {(p, False) for p in I.PATTERNS} | {("small", True)}


def test_phase_one_value_patterns():
    """the differences of a free run are what the pattern says; 4096 wraps 2^16 every 16 pixels"""
    w = 4160
    plans = [((), ()), ((17,), (300,))]
    for pattern, want in (("plus4096", 4096), ("minus4095", -4095)):
        img, rows = I.planned_rows(w, plans, pattern)
        for r, plan in enumerate(plans):
            for p in (0, 1):
                v = np.concatenate([[0], img[r, p::2].astype(np.int64)])
                d = ((v[1:] - v[:-1] + 0x8000) & 0xFFFF) - 0x8000
                jumps = np.flatnonzero(d != want)
                assert list(jumps) == [4 * g for g in plan[p]] and (abs(d[jumps]) > 4096).all()
        if want == 4096:
            assert (img[0, 0::2][15::16] == 0).all()  # (16 x 4096 = 2^16)
    img, rows = I.planned_rows(w, plans, "small")
    even, odd, _ = I.header_walk(rows[0], w)
    assert not even and not odd
    d = np.diff(img[0, 0::2].astype(np.int64))
    d = ((d + 0x8000) & 0xFFFF) - 0x8000
    assert abs(d).max() <= 4095 and len({int(x).bit_length() for x in abs(d)}) >= 10
    with pytest.raises(ValueError):
        I.planned_rows(w, plans, "small", keep=True)  # (a raw length would be kept as well)
    with pytest.raises(ValueError):
        I.planned_rows(w, [((w >> 3,), ())], "small")


# ---- Samsung V0 -----------------------------------------------------------------------------
@pytest.mark.parametrize("w", L.V0_WIDTHS)
def test_samsung_v0_frames_have_exactly_their_planned_upward_blocks(w):
    frames = [c for c in L.v0_frames() if c[1] == w]
    nblk = (w + 15) // 16
    assert len(frames) >= 8
    for case in frames:
        name, _, h, plan = case
        rows = L.v0_build(case)
        assert h in (5, 6) and len(rows) == h and set(plan) <= set(range(2, h))
        longest = 0
        for y in range(2, h):
            st, dirs, _ = S.parse_row(rows[y], y, w)
            assert st == S.OK
            assert tuple(np.flatnonzero(dirs)) == tuple(plan.get(y, ())), (name, y)
            run = I.longest_free_run([int(b) for b in np.flatnonzero(dirs)], nblk)
            assert run == _planned_run([plan.get(y, ())], nblk), (name, y)
            longest = max(longest, run)
        if name.endswith("_dense"):
            assert longest == 1  # (only the last block is not upward)
        elif name.endswith("_two"):
            assert longest == 199 and all(b[1] - b[0] == 200 for b in plan.values())
        else:
            assert longest == nblk, name  # a row without any upward block
        if name == "v0_5546_none":
            assert longest == 347


def test_samsung_v0_plans_reach_every_wave_and_pass_edge():
    by_w = {}
    for name, w, h, plan in L.v0_frames():
        by_w.setdefault(w, []).append((name, h, plan))
    assert {w: (w + 15) // 16 for w in by_w} == {1040: 65, 3072: 192, 3088: 193, 5546: 347}
    for w, frames in by_w.items():
        nblk = (w + 15) // 16
        want = {b for b in (0, 1, 63, 64, 127, 128, 191, 192, 193, nblk - 2) if b < nblk - 1}
        for row in (2, 3):
            assert {p[row][0] for _, _, p in frames if list(p) == [row] and len(p[row]) == 1} == want
        assert any(p == {} for _, _, p in frames)
        assert any(all(len(p.get(y, ())) == nblk - 1 for y in range(2, h)) for _, h, p in frames)
    assert any(n.endswith("_two") for n, _, _ in by_w[5546])


def test_explicit_dirs_leave_the_existing_samsung_v0_cases_as_they_were():
    """the bytes of random_case (hashes taken before encode_row had `dirs`) and of large_case
    (recorded with the reference's image in samsung_v0_ref.json)"""
    before = {0: "46e4a3e70d59fdc298da1e837467f89cfd4d4583613d0021163be1f2fcf8a0c6",
              3: "6885fe44a90ebf44cf72c5eeea78d98d480ea6f947351f4d955de12646ef0012",
              7: "789504eed686ba5e1d9d7195f66cc13f928a2c54c2fef628fd97b2fe49de7d3e"}
    for seed, digest in before.items():
        assert M._sha_rows(M.random_case(seed)[2]) == digest, seed
    import json
    with open(M.GOLDEN) as f:
        rec = json.load(f)
    assert M._sha_rows(M.large_case()[2]) == rec["large"]["input_sha256"]


def test_explicit_dirs_respect_the_first_rows_and_the_last_block():
    rng = np.random.default_rng(1)
    w = 80
    for row, dirs in ((0, [True] + [False] * 4), (1, [False, True, False, False, False]),
                      (2, [False] * 4 + [True]), (2, [False] * 4)):
        with pytest.raises(ValueError):
            S.encode_row(rng, w, row, dirs=dirs)
    data = S.encode_row(rng, w, 2, dirs=[True, False, True, True, False])
    assert list(S.parse_row(data, 2, w)[1]) == [True, False, True, True, False]
    with pytest.raises(ValueError):
        S.encode_row(rng, w, 2, dirs=[False] * 6)
    assert S.planned_dirs(w, 4, {3: (1,)}) == {2: [False] * 5, 3: [False, True, False, False, False]}
    # rows that the dict does not name are drawn as ever
    rows = S.random_rows(np.random.default_rng(5), w, 4, p_up=1.0, dirs={2: [False] * 5})
    assert not S.parse_row(rows[2], 2, w)[1].any() and S.parse_row(rows[3], 3, w)[1][:4].all()
