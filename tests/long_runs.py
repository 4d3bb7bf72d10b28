"""TEST INFRASTRUCTURE: Phase One rows and Samsung V0 frames with a planned run structure.

p1_row_kernel and sv0_parse_kernel rebuild a row with a segmented scan over the lanes of a
workgroup: a shuffle ladder inside a wave (d = 1 .. 32), per-wave totals in LDS, a loop over the
waves (and the pass) before, a carry in front of the lane's first reset.  The random inputs of the
other tests place a reset every few elements, so that a flag in the nearer operand wins every
combine of the upper ladder steps, of the totals and of the pass carry.  Measured with a header
walk over those inputs, the longest run without a reset was
  Phase One     123 groups of 1496 in one parity (w = 11974, seed 0: 15 of 188 lanes; 18 .. 39
                groups with the non-zero `choices`), no wave without a reset, no row that runs
                from pixel 0 on the carry that starts at 0
  Samsung V0    19 blocks of 347 in rows >= 2 of test_shapes, 27 in the largest frame (a lane
                owns one block): a root code never travelled more than 27 lanes, never across a
                wave or the pass boundary from afar
The inputs here are the opposite: every reset is planned, and the runs between them are as long
as the row (1497 groups at w = 11976, 347 blocks at w = 5546).  tests/test_long_runs_structure.py
holds every input to its plan on the CPU.

  p1_files()   (name, width, pattern, keep, plans): one file per width and value pattern, one
               image row per reset plan (a workgroup decodes a row)
  v0_frames()  (name, width, height, plan {row: upward blocks})
  golden()     tests/golden/long_runs_ref.json: SHA-256 of the reference's decoded image of each

  python tests/long_runs.py --golden    rewrites that file from the reference's whole-file
                                        decodes (oracle/_ref); refuses unless the models of
                                        iiq_files.py / srw_v0_files.py agree with every answer
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "long_runs_ref.json")

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))

import iiq_files as I  # noqa: E402
import srw_v0_files as S  # noqa: E402

# ---- Phase One ------------------------------------------------------------------------------
# A lane owns 8 groups (64 pixels), a wave 512.  4096: exactly one wave of lanes; 4160: one lane
# into wave 1; 8192 / 8256: the same at wave 2; 11976: the widest row, 188 lanes, the last one
# holds 8 pixels; 11974: 1496 groups, the 6-pixel raw tail has a checkpoint (a lane) of its own;
# 11966: a tail that shares its lane with seven groups.
P1_WIDTHS = (4096, 4160, 8192, 8256, 11976, 11974, 11966)


def p1_plans(width):
    """[(name, (raw groups of the even columns, of the odd columns))]"""
    ng = width >> 3
    plans = [("none", ((), ()))]
    # one raw group in one parity, the other parity free: the first group of lane 0, the last of
    # lane 63, the first of lane 64, the last of lane 127, the first of lane 128, the last group
    for g in sorted({g for g in (0, 511, 512, 1023, 1024, ng - 1) if g < ng}):
        plans.append(("even_%d" % g, ((g,), ())))
        plans.append(("odd_%d" % g, ((), (g,))))
    # in the middle of a lane (groups 3 and 4 of its 8): the lane's first reset is an interior
    # pixel, the pixels before it take the carry, those behind it must not
    lane = 70 if 8 * 70 + 4 < ng else 30
    plans.append(("mid3_even", ((8 * lane + 3,), ())))
    plans.append(("mid4_odd", ((), (8 * lane + 4,))))
    # early (lane 1) and nothing after: the flagged sum travels to the end of the row
    plans.append(("early", ((9,), (12,))))
    return plans


def p1_files():
    """(name, width, pattern, keep, plans).  The all-keep encoder goes with the plan without
    resets only (it would keep a raw length as well): one row per value pattern's seed."""
    out = []
    for w in P1_WIDTHS:
        for pattern in I.PATTERNS:
            out.append(("p1_%d_%s" % (w, pattern), w, pattern, False, p1_plans(w)))
        out.append(("p1_%d_keep" % w, w, "small", True, [("none", ((), ()))] * 2))
    return out


def p1_build(case):
    """(img, rows, the IIQ file)"""
    name, w, pattern, keep, plans = case
    img, rows = I.planned_rows(w, [p for _, p in plans], pattern, seed=len(name), keep=keep)
    rng = np.random.default_rng([0x10E6, w, len(name)])
    return img, rows, I.iiq_file(rows, w, rng, gap_max=5, tail_gap=3)


# ---- Samsung V0 -----------------------------------------------------------------------------
# A lane owns a block of 16 columns, a wave 64, a pass 192.  1040: 65 blocks, one into wave 1;
# 3072: exactly pass 0; 3088: one block into pass 1; 5546: 347 blocks, the last one 10 pixels.
V0_WIDTHS = (1040, 3072, 3088, 5546)
V0_SINGLES = (0, 1, 63, 64, 127, 128, 191, 192, 193)


def v0_frames():
    """(name, width, height, plan).  plan {row: upward blocks} covers every row from row 2 on;
    rows 0 and 1 are random rows as everywhere.  Heights 5 and 6: behind the planned row come
    rows that take even pixels from one row up and odd ones from two rows up."""
    out = []
    for w in V0_WIDTHS:
        nblk = (w + 15) // 16
        eligible = range(nblk - 1)  # (the last block is never upward)
        out.append(("v0_%d_none" % w, w, 5, {}))
        for b in sorted({b for b in V0_SINGLES + (nblk - 2,) if b in eligible}):
            out.append(("v0_%d_row2_%d" % (w, b), w, 5, {2: (b,)}))
            out.append(("v0_%d_row3_%d" % (w, b), w, 6, {3: (b,)}))
        out.append(("v0_%d_dense" % w, w, 5, {y: tuple(eligible) for y in range(2, 5)}))
        if nblk > 206:  # the later mark replaces the earlier one after a long carry
            out.append(("v0_%d_two" % w, w, 6, {2: (5, 205), 3: (140, 340), 4: (0, 200), 5: (63, 263)}))
    return out


def v0_build(case):
    """the rows of the frame"""
    name, w, h, plan = case
    rng = np.random.default_rng([0x10E7, w, h, len(name), sum(map(ord, name))])
    return S.random_rows(rng, w, h, dirs=S.planned_dirs(w, h, plan))


# ---- the recorded reference -----------------------------------------------------------------
def sha(img):
    return hashlib.sha256(np.ascontiguousarray(img, dtype="<u2").tobytes()).hexdigest()


def sha_rows(rows):
    m = hashlib.sha256()
    for r in rows:
        m.update(len(r).to_bytes(4, "little") + bytes(r))
    return m.hexdigest()


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def write_golden():
    """The reference's decode of every file -> tests/golden/long_runs_ref.json, unless a model
    disagrees with one answer (nothing is written then).  "input": the encoded rows the image
    belongs to, so that a changed generator shows."""
    from oracle_lib import Ref
    ref = Ref()
    out = {"phase_one": {}, "samsung_v0": {}}
    for case in p1_files():
        img, rows, blob = p1_build(case)
        h, w = img.shape
        st, dec = ref.decode_file(blob)
        assert st == 0, (case[0], ref.last_error())
        got = dec.u16()[:h, :w]
        mst, mimg, mrows = I.model_file(blob)
        assert mst == 0 and not any(mrows), (case[0], mrows)
        assert np.array_equal(got, mimg) and np.array_equal(got, img), case[0]
        out["phase_one"][case[0]] = {"input": sha_rows(rows)[:16], "image": sha(got)}
    for case in v0_frames():
        name, w, h, _ = case
        rows = v0_build(case)
        st, dec = ref.decode_file(S.rows_file(w, h, rows))
        assert st == 0, (name, ref.last_error())
        got = dec.u16()[:h, :w]
        mst, _, mimg = S.model_decode(w, h, rows)
        assert mst == S.OK and np.array_equal(got, mimg), name
        out["samsung_v0"][name] = {"input": sha_rows(rows)[:16], "image": sha(got)}
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    return len(out["phase_one"]) + len(out["samsung_v0"])


if __name__ == "__main__":
    if sys.argv[1:2] == ["--golden"]:
        print(write_golden(), "images agree with the models")
    else:
        sys.exit(__doc__)
