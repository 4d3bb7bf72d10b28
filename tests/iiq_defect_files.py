"""TEST INFRASTRUCTURE: the sensor defects of a Phase One IIQ correction block (entry 0x400), a
Python model of IiqDecoder::correctSensorDefects (decoders/IiqDecoder.cpp:499-576) written from the
reference's source, and the cases the host build of the core and the device are held against.

The reference itself cannot run correctBadColumn in this repository: a whole-file decode without a
camera database has no CFA and throws "No CFA size set".  So, as for chroma, the model is the
yardstick of the bad columns; what the reference can pin -- an entry 0x400 that holds no bad column
inside the image leaves the decode as it is -- is pinned by pinned_file() and
tests/golden/iiq_defects_ref.json.

  records()           [(col, row, type)] -> the bytes of entry 0x400 (8-byte records)
  lround()            std::lround of a value >= 0 as r = int(x); r += (x - r >= 0.5)
  green() / other()   the two per-pixel formulas
  bad_column()        correctBadColumn
  defects()           correctSensorDefects: (status, image, mBadPixelPositions)
  apply()             a list of ops (iiq_corr_files.apply plus ("defects", payload))
  ties()              the (diags, horiz) pairs whose value is an exact decimal tie x.5
  tie_pairs()         ... and the ones the cases use, near misses included
  cases()             the case list
"""
import json
import os
import struct

import numpy as np

import iiq_corr_files as K

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "iiq_defects_ref.json")
OK, INVALID_ARG, IO, UNSUPPORTED = 0, 1, 2, 7  # include/rsx.h: rsx_status
MAX_BAD_COLUMNS = 4096  # include/rsx.h section 3n

RGGB = (2, 2, (0, 1, 1, 2))
GRBG = (2, 2, (1, 0, 2, 1))
SKEW = (2, 2, (1, 1, 0, 2))    # green at (0, 0) and (1, 0): not symmetric under transposition
NO_GREEN = (2, 2, (0, 2, 2, 0))
CFA_2X4 = (2, 4, (0, 1, 1, 2, 2, 1, 1, 0))


def records(recs, tail=b""):
    """[(col, row, type)] in file order; the 2 ignored bytes are not zero"""
    return b"".join(struct.pack("<HHHH", c, r, t, 0xBEEF) for c, r, t in recs) + tail


def columns(cols, type_=131):
    return records([(c, 0, type_) for c in cols])


def lround(x):
    r = int(x)
    r += (x - r >= 0.5)
    return r


def green(val):
    """val: the pixels at (row - 1, col - 1), (row + 1, col - 1), (row - 1, col + 1), (row + 1,
    col + 1)"""
    total = sum(val)
    dev = [abs(4 * v - total) for v in val]
    mx = 0
    for i in range(4):
        if dev[mx] < dev[i]:
            mx = i
    return (total - val[mx] + 1) // 3


def other(diags, horiz):
    return lround(diags * 0.0732233 + horiz * 0.3535534)  # (binary64, each operation on its own)


def colour_at(cfa, col, row):
    """the reference's getColorAt(col, row)"""
    cw, ch, c = cfa
    return c[(col % cw) + (row % ch) * cw]


def bad_column(img, col, cfa):
    """in place; rows 2 .. h - 3, every pixel from the image as it stands (only other columns are
    read)"""
    h = img.shape[0]
    p = img.astype(np.int64)
    for row in range(2, h - 2):
        if colour_at(cfa, col, row) == 1:
            v = green([int(p[row - 1, col - 1]), int(p[row + 1, col - 1]), int(p[row - 1, col + 1]),
                       int(p[row + 1, col + 1])])
        else:
            diags = int(p[row + 2, col - 2] + p[row - 2, col - 2] + p[row + 2, col + 2] + p[row - 2, col + 2])
            horiz = int(p[row, col - 2] + p[row, col + 2])
            v = other(diags, horiz)
        assert 0 <= v <= 65535
        img[row, col] = v


def defects(img, payload, cfa=None):
    """(status, image, positions) as include/rsx.h section 3n states them; the image is the input
    when the status is not OK"""
    src = np.array(img, dtype=np.uint16)
    out = src.copy()
    h, w = out.shape
    if len(payload) % 8:
        return IO, src, []
    positions, n_cols = [], 0
    for k in range(len(payload) // 8):
        col, row, type_ = struct.unpack_from("<HHH", payload, 8 * k)
        if col >= w:
            continue
        if type_ == 129:
            positions.append((row << 16) + col)
        elif type_ in (131, 137) and h >= 5:
            if cfa is None or cfa[0] <= 0 or cfa[1] <= 0 or cfa[0] * cfa[1] > 64:
                return INVALID_ARG, src, []
            if col < 2 or col > w - 3:
                return UNSUPPORTED, src, []
            n_cols += 1
            if n_cols > MAX_BAD_COLUMNS:
                return UNSUPPORTED, src, []
            bad_column(out, col, cfa)
    return OK, out, positions


def apply(img, ops, cfa=None):
    """iiq_corr_files.apply with ("defects", payload) ops; a second defects op is INVALID_ARG.
    (status, image)"""
    src = np.array(img, dtype=np.uint16)
    if sum(op[0] == "defects" for op in ops) > 1:
        return INVALID_ARG, src
    out = src
    for op in ops:
        if op[0] == "defects":
            st, out, _ = defects(out, op[1], cfa)
        else:
            st, out = K.apply(out, [op], cfa)
        if st != OK:
            return st, src
    return OK, out


# ---------------------------------------------------------------------------------------
# the binary64 line: diags * 0.0732233 + horiz * 0.3535534 is a multiple of 1e-7, so it comes close
# to a half only where 732233 diags + 3535534 horiz = 5000000 (mod 10000000)
# ---------------------------------------------------------------------------------------
def ties(residue=5000000):
    """[(diags, horiz)], diags <= 4 * 65535, horiz <= 2 * 65535, by horiz: the 65535 exact ties
    (diags = 2 horiz, horiz odd: 2 * 732233 + 3535534 = 5000000); residue 4999997 / 5000003 gives
    the pairs three ten-millionths below / above a half, the nearest there are"""
    inv = pow(732233, -1, 10 ** 7)
    out = []
    for horiz in range(2 * 65535 + 1):
        diags = (residue - 3535534 * horiz) * inv % 10 ** 7
        if diags <= 4 * 65535:
            out.append((diags, horiz))
    return out


def tie_pairs():
    """96 exact ties over the whole range, and 32 pairs each just below and just above a half
    (binary32 gets many of the latter wrong)"""
    return ties()[::683] + ties(4999997)[::330][:32] + ties(5000003)[::330][:32]


def _split(total, parts):
    """`parts` values of at most 65535 with the given total"""
    out = []
    for k in range(parts):
        v = min(65535, total - sum(out), max(0, total // parts + (k % 2) * 7 - 3))
        out.append(v if k < parts - 1 else total - sum(out))
    assert sum(out) == total and all(0 <= v <= 65535 for v in out), (total, out)
    return out


def tie_image(pairs, rng):
    """(image, {row: (diags, horiz)}): 9 columns, 5 rows a pair; row 2 + 5 k of column 4 has the
    k-th pair's diags and horiz around it.  For a bad column 4 under a CFA without green, where
    every row takes the second formula."""
    h = 5 * len(pairs) + 4
    img = rng.integers(0, 65536, size=(h, 9)).astype(np.uint16)
    want = {}
    for k, (diags, horiz) in enumerate(pairs):
        row = 2 + 5 * k
        d = _split(diags, 4)
        hz = _split(horiz, 2)
        img[row - 2, 2], img[row - 2, 6], img[row + 2, 2], img[row + 2, 6] = d
        img[row, 2], img[row, 6] = hz
        want[row] = (diags, horiz)
    return img, want


# ---------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------
def _img(rng, w, h):
    return rng.integers(0, 65536, size=(h, w)).astype(np.uint16)


def green_probe():
    """[(name, 5 x 5 image, the value (row 2, column 2) must get)] under an all-green CFA: one
    neighbourhood of the first formula each, the expected value worked out by hand"""
    out = []

    def one(name, v, want):
        img = np.full((5, 5), 7, np.uint16)
        img[1, 1], img[3, 1], img[1, 3], img[3, 3] = v
        out.append((name, img, want))

    one("four_equal", (300, 300, 300, 300), 300)                  # drops val[0]: (900 + 1) // 3
    one("all_65535", (65535,) * 4, 65535)
    one("all_0", (0,) * 4, 0)
    # Two equal largest deviations: 130 and 70 around two values of 100 (sum 400, 4 * 130 - 400 =
    # 120, 4 * 70 - 400 = -120), in every pair of positions and both ways round.  The FIRST is
    # dropped: without 130 the result is 271 // 3 = 90, without 70 it is 331 // 3 = 110.
    for i in range(4):
        for j in range(i + 1, 4):
            v = [100] * 4
            v[i], v[j] = 130, 70
            one("tie_hi%d_lo%d" % (i, j), tuple(v), 90)
            v[i], v[j] = 70, 130
            one("tie_lo%d_hi%d" % (i, j), tuple(v), 110)
    # 4 val - sum negative at the largest deviation
    one("negative_dev", (60000, 61000, 5, 60500), (60000 + 61000 + 60500 + 1) // 3)
    one("rounding", (1, 1, 2, 0), 1)                              # sum 4, drops the 2: 3 // 3
    return out


ALL_GREEN = (1, 1, (1,))


def cases():
    """[(name, image, ops, cfa)]: the lists the host core and the device run against apply()"""
    rng = np.random.default_rng(0x400)
    out = []
    for cfa_name, cfa in (("rggb", RGGB), ("grbg", GRBG), ("skew", SKEW), ("no_green", NO_GREEN),
                          ("2x4", CFA_2X4)):
        for w, h in ((5, 5), (7, 6), (13, 9), (64, 40)):
            cols = sorted({2, w - 3, (w // 2) | 1 if w > 12 else 2})
            out.append(("edges_%s_%dx%d" % (cfa_name, w, h), _img(rng, w, h),
                        [("defects", columns(cols))], cfa))
    # dim_y of 4: the loop has no row -- nothing is read, not even the CFA or the column range
    out.append(("dim_y_4", _img(rng, 9, 4), [("defects", columns([0, 4, 8]))], None))
    out.append(("dim_y_5", _img(rng, 9, 5), [("defects", columns([4], 137))], RGGB))
    for name, img, _ in green_probe():
        out.append(("green_" + name, img, [("defects", columns([2]))], ALL_GREEN))
    out.append(("all_65535", np.full((9, 9), 65535, np.uint16), [("defects", columns([2, 5]))], RGGB))
    out.append(("all_0", np.zeros((9, 9), np.uint16), [("defects", columns([2, 5]))], RGGB))
    timg, _ = tie_image(tie_pairs(), np.random.default_rng(0x7E))
    out.append(("decimal_ties", timg, [("defects", columns([4]))], NO_GREEN))
    # dependent columns
    base = _img(rng, 16, 12)
    for name, cols in (("chain_up", [6, 7, 8]), ("chain_down", [8, 7, 6]),
                       ("same_twice", [6, 7, 6]), ("two_apart", [5, 7, 9, 7, 5]),
                       ("mixed", [3, 12, 4, 11, 5, 3, 8])):
        out.append((name, base, [("defects", columns(cols))], RGGB))
    # in front of, between and behind a luma flat field and the quadrant curves
    img = _img(rng, 64, 40)
    ff = ("ff", K.ff_random(rng, (3, 2, 56, 30, 7, 5)), 0)
    chroma = ("ff", K.ff_random(rng, (0, 0, 64, 40, 8, 8), planes=2, lo=36000, hi=50000), 1)
    quad = ("quad", K.random_curves(rng), 17, 29, 1200)
    d = ("defects", records([(10, 0, 131), (70, 3, 131), (11, 5, 129), (30, 7, 7), (31, 0, 137),
                             (64, 1, 129), (12, 9, 131), (50, 39, 129), (50, 40, 129)]))
    out.append(("defects_ff_quad", img, [d, ff, quad], GRBG))
    out.append(("ff_defects_quad", img, [ff, d, quad], GRBG))
    out.append(("ff_quad_defects", img, [ff, quad, d], GRBG))
    out.append(("chroma_defects_ff", img, [chroma, d, ff], GRBG))
    out.append(("defects_alone_72x38", _img(rng, 72, 38),
                [("defects", records([(2, 0, 131), (69, 0, 137), (72, 0, 131), (40, 2, 129)]))], CFA_2X4))
    out.append(("empty_payload", img, [ff, ("defects", b""), quad], None))
    out.append(("only_129_and_unknown", img,
                [("defects", records([(0, 1, 129), (63, 2, 129), (1, 0, 7), (500, 0, 131)]))], None))
    return out


def chain_case(w, n_far, n_chain, rng):
    """a `w` x 8 image with n_far bad columns no two of which lie within 2 of each other, and behind
    them n_chain adjacent columns, rising, interleaved with bad pixels"""
    far = list(range(2, 2 + 3 * n_far, 3))
    chain = list(range(far[-1] + 3, far[-1] + 3 + n_chain))
    assert chain[-1] <= w - 3, (w, chain[-1])
    order = [far[i] for i in rng.permutation(n_far)]
    recs = [(c, 0, 131 if c % 2 else 137) for c in order] + [(5, 3, 129)] + [(c, 0, 131) for c in chain]
    return _img(rng, w, 8), [("defects", records(recs))], RGGB


# ---------------------------------------------------------------------------------------
# what the reference can pin
# ---------------------------------------------------------------------------------------
def pinned_file():
    """(image, the file without entry 0x400, the file with it, payload): the entry holds bad pixels,
    columns outside the image and unknown types only, so no CFA is needed"""
    rng = np.random.default_rng(0x129)
    img = _img(rng, 64, 40)
    luma = K.ff_random(rng, (3, 2, 56, 30, 7, 5))
    payload = records([(7, 3, 129), (64, 0, 131), (9, 1, 7), (63, 39, 129), (200, 5, 137),
                       (0, 0, 129), (65535, 2, 129), (7, 3, 129), (12, 300, 129), (3, 0, 130)])
    plain = K.iiq_corr_file(img, K.meta_block([(0x410, luma)]))
    with_entry = K.iiq_corr_file(img, K.meta_block([(0x400, payload), (0x410, luma)]))
    return img, plain, with_entry, payload, luma


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)
