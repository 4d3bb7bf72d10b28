"""NefDecoder::DecodeNikonSNef (Nikon "RAW S", 12-bit Y/Y/Cb/Cr packets) test material: a writer
of minimal sNEF files, the curve and white balance the reference's host code derives, the chroma
pairs at which a fused multiply-add changes the green expression, seeded test cases, and a numpy
model of the pixel loop (include/rsx.h section 3m).

Row y of a w-pixel image is the bytes [3 w y, 3 w (y + 1)).  A group of 6 bytes is four 12-bit
fields, LSB first: y1, y2, cb, cr.  Every byte string of 3 w h bytes is a valid stream."""
import hashlib
import json
import math
import os

import numpy as np

import rawfiles as R
from arw2_files import M, table_dither

MAX_W, MAX_H = 3680, 2456           # NefDecoder.cpp:389-391
INV_WB_MIN, INV_WB_MAX = 102, 32768  # int(1024.0F / wb) for the wb NefDecoder.cpp:682-687 lets through
RUN = 4                              # groups a lane's run holds (rsx_nikon_snef.hip)
WB_LOW = (4194241, 134217728)        # float(13421568.0 / 429496627.0), the lowest the reference accepts
WB_TOO_LOW = (16776963, 536870912)   # the binary32 number below it
WB_HIGH = (10, 1)


# ---------------------------------------------------------------------------- the file
def snef_file(w, h, data, wb_r=(2, 1), wb_b=(3, 2), gap=0):
    """NefDecoder's sNEF branch (NefDecoder.cpp:73-99): make "NIKON CORPORATION", the raw IFD
    carries CFAPATTERN, compression is not 1, one strip of exactly 3 w h bytes
    (NEFIsUncompressedRGB), and 32 bits per sample so that NEFIsUncompressed (:157-195) sees too
    few pixels in the strip and says no.  Tag 12 holds the white balance as four RATIONALs."""
    data = np.asarray(data, np.uint8)
    assert data.size == 3 * w * h
    raw = R.Ifd()
    raw.add(R.IMAGEWIDTH, R.LONG, w).add(R.IMAGELENGTH, R.LONG, h)
    raw.add(R.BITSPERSAMPLE, R.SHORT, 32)
    raw.add(R.COMPRESSION, R.LONG, 34713)
    raw.add(R.PHOTOMETRIC, R.SHORT, 32803)
    raw.add(R.CFAREPEATPATTERNDIM, R.SHORT, [2, 2])
    raw.add(R.CFAPATTERN, R.BYTE, [0, 1, 1, 2])
    raw.add(12, R.RATIONAL, [tuple(wb_r), tuple(wb_b), (1, 1), (1, 1)])
    raw.add_blobs(R.STRIPOFFSETS, R.STRIPBYTECOUNTS, [data])
    root = R.Ifd()
    root.add(R.MAKE, R.ASCII, "NIKON CORPORATION").add(R.MODEL, R.ASCII, "NIKON RSX")
    root.add_sub(raw)
    return R.tiff_file(root, gap, big=True)


def inv_wb(rational):
    """int(1024.0F / wb) with wb = float(num) / float(den) (TiffEntry::getFloat,
    NefDecoder.cpp:679-694), in binary32 like the reference"""
    wb = np.float32(rational[0]) / np.float32(rational[1])
    return int(np.float32(1024.0) / wb)


def gamma_curve(pwr, ts, imax):
    """NefDecoder::gammaCurve (NefDecoder.cpp:797-850, after dcraw): 65536 entries"""
    g = [pwr, ts, 0.0, 0.0, 0.0, 0.0]
    bnd = [0.0, 0.0]
    bnd[1 if g[1] >= 1 else 0] = 1.0
    if abs(g[1]) > 0 and (g[1] - 1) * (g[0] - 1) <= 0:
        for _ in range(48):
            g[2] = (bnd[0] + bnd[1]) / 2
            if abs(g[0]) > 0:
                bnd[1 if (math.pow(g[2] / g[1], -g[0]) - 1) / g[0] - 1 / g[2] > -1 else 0] = g[2]
            else:
                bnd[1 if g[2] / math.exp(1 - 1 / g[2]) < g[1] else 0] = g[2]
        g[3] = g[2] / g[1]
        if abs(g[0]) > 0:
            g[4] = g[2] * (1 / g[0] - 1)
    if abs(g[0]) > 0:
        g[5] = 1 / (g[1] * g[3] * g[3] / 2 - g[4] * (1 - g[3]) +
                    (1 - math.pow(g[3], 1 + g[0])) * (1 + g[4]) / (1 + g[0])) - 1
    else:
        g[5] = 1 / (g[1] * g[3] * g[3] / 2 + 1 - g[2] - g[3] - g[2] * g[3] * (math.log(g[3]) - 1)) - 1
    curve = [0xFFFF] * 0x10000
    for i in range(0x10000):
        r = i / imax
        if r >= 1:
            continue
        if r < g[2]:
            v = r / g[1]
        elif abs(g[0]) > 0:
            v = math.pow((r + g[4]) / (1 + g[4]), 1 / g[0])
        else:
            v = math.exp((r - 1) / g[2])
        curve[i] = int(0x10000 * v) & 0xFFFF
    return curve


_CURVE = None


def host_curve():
    """the 4095 entries DecodeNikonSNef installs (:696-705): gammaCurve(1 / 2.4, 12.92, 4095),
    each entry clampBits(c << 2, 16)"""
    global _CURVE
    if _CURVE is None:
        c = np.array(gamma_curve(1 / 2.4, 12.92, 4095)[:4096], np.int64)
        _CURVE = np.minimum(c << 2, 65535)[:4095]
    return _CURVE


def host_table(curve=None):
    """the dithering TableLookUp of that curve, the 8192 entries the loop can read"""
    return table_dither(host_curve() if curve is None else curve, 8192)


def arbitrary_table(rng):
    """any table the ABI takes: non-monotone bases near the top with large deltas, so that
    base + dither passes 65535 and the store's modulo 2^16 shows"""
    t = rng.integers(0, 65536, 8192).astype(np.uint16)
    t[0:8192:8] = rng.integers(65000, 65536, 1024)   # bases that wrap
    t[1:8192:8] = rng.integers(40000, 65536, 1024)   # with deltas of up to 16 after the shift
    return t


# ---------------------------------------------------------------------------- the stream
def pack_group(y1, y2, cb, cr):
    v = (y1 & 0xFFF) | ((y2 & 0xFFF) << 12) | ((cb & 0xFFF) << 24) | ((cr & 0xFFF) << 36)
    return np.frombuffer(v.to_bytes(6, "little"), np.uint8)


def set_group(data, w, row, g, y1, y2, cb, cr):
    o = 3 * w * row + 6 * g
    data[o:o + 6] = pack_group(y1, y2, cb, cr)


def fma_pairs():
    """The (n1, n2) = (2 (cb - 2048), 2 (cr - 2048)) for which 0.337633 cb + 0.698001 cr is a
    whole number: there the green expression lands within 1e-12 of an integer and the sequence
    of roundings decides.  cb, cr in steps of 1/2 over -2048 .. 2047 (pixel 2 has halves)."""
    out = []
    for n1 in range(-4096, 4095):
        # 698001 n2 = -337633 n1 (mod 2000000); 698001 is a unit mod 2000000
        n2 = (-337633 * n1 * pow(698001, -1, 2000000)) % 2000000
        for cand in (n2, n2 - 2000000):
            if -4096 <= cand <= 4094 and (n1, cand) != (0, 0):
                out.append((n1, cand))
    return out


def plant_fma_pair(data, w, row, g, pair, y):
    """pair in group g of `row`: whole chroma goes into pixel 1 (and, with an equal neighbour,
    pixel 2); chroma with halves into pixel 2 through the two neighbouring groups g, g + 1"""
    n1, n2 = pair
    if n1 % 2 == 0 and n2 % 2 == 0:
        cb, cr = n1 // 2 + 2048, n2 // 2 + 2048
        set_group(data, w, row, g, y, y, cb, cr)
        set_group(data, w, row, g + 1, y, y, cb, cr)
        return
    s1, s2 = n1 + 4096, n2 + 4096  # cb + cb', cr + cr' of the two groups
    cb = min(max(s1 // 2 + 7, s1 - 4095), min(4095, s1))  # both of a sum within 0 .. 4095
    cr = min(max(s2 // 2 + 5, s2 - 4095), min(4095, s2))
    set_group(data, w, row, g, y, y, cb, cr)
    set_group(data, w, row, g + 1, y, y, s1 - cb, s2 - cr)


CLAMP_GROUPS = [
    # (y1, y2, cb, cr): each of the six expressions below 0 and above 4095
    (0, 0, 2048, 0), (4095, 4095, 2048, 4095),       # e0 / e3: y + 1.37 cr
    (0, 0, 4095, 4095), (4095, 4095, 0, 0),          # e1 / e4: y - 0.34 cb - 0.70 cr
    (0, 0, 0, 2048), (4095, 4095, 4095, 2048),       # e2 / e5: y + 1.73 cb
]


def make_case(seed):
    """Test case `seed`: (w, h, wb_r, wb_b, data).  The seeds walk over every residue of the
    lane's run (w / 2 mod 4) and h = 1..3, both white-balance limits, the FMA pairs (two a case,
    all 34 within 17 cases), the clamps of all six expressions and a row seed of 0."""
    rng = np.random.default_rng([0x5EF, seed])
    groups = 3 + (seed % 4) + 4 * int(rng.integers(0, 6))   # >= 3: w >= 6; residue seed % 4
    if seed % 11 == 10:
        groups = 4 * int(rng.integers(60, 120)) + seed % 4  # more than one workgroup round
    if seed % 3 == 0 and groups < 4:
        groups += 4                                          # room for two planted pairs
    w, h = 2 * groups, 1 + (seed // 4) % 3
    lim = [WB_LOW, WB_HIGH, (2, 1), (3, 2), (1, 3), (1000, 999)]
    wb_r, wb_b = lim[seed % 6], lim[(seed // 6) % 6]
    data = rng.integers(0, 256, 3 * w * h, dtype=np.uint8)
    pairs = fma_pairs()
    ys = [2047, 0, 4095, 1000, 3000, 1, 2048]
    kind = seed % 3
    if kind == 0 and groups >= 4:        # two FMA pairs, in the first and the last two groups
        p = pairs[(2 * (seed // 3)) % len(pairs)], pairs[(2 * (seed // 3) + 1) % len(pairs)]
        plant_fma_pair(data, w, 0, 0, p[0], ys[seed % 7])
        plant_fma_pair(data, w, h - 1, groups - 2, p[1], ys[(seed + 3) % 7])
    elif kind == 1:                      # clamps, two groups of them at a time
        for k in range(2):
            set_group(data, w, (seed + k) % h, (seed + 2 * k) % groups,
                      *CLAMP_GROUPS[(2 * (seed // 3) + k) % 6])
    if seed % 5 == 0:                    # a row whose seed is 0: the generator stays at 0
        data[3 * w * (h - 1):3 * w * (h - 1) + 3] = 0
    return w, h, wb_r, wb_b, data


def sha(img):
    return hashlib.sha256(np.ascontiguousarray(img, np.dtype("<u2")).tobytes()).hexdigest()


# ---------------------------------------------------------------------------- the model
def model_values(data, w, h):
    """the six 12-bit values of every group, (h, 3 w): float32 interpolation, float64 with a
    rounding after every product and every sum (numpy fuses nothing), truncation, clamp"""
    a = np.asarray(data[:3 * w * h], np.uint8).reshape(h, w // 2, 6).astype(np.int64)
    y1 = a[..., 0] | ((a[..., 1] & 15) << 8)
    y2 = (a[..., 1] >> 4) | (a[..., 2] << 4)
    cb = (a[..., 3] | ((a[..., 4] & 15) << 8)).astype(np.float32)
    cr = ((a[..., 4] >> 4) | (a[..., 5] << 4)).astype(np.float32)
    cb2, cr2 = cb.copy(), cr.copy()
    cb2[:, :-1] = (cb[:, 1:] + cb[:, :-1]) * np.float32(0.5)
    cr2[:, :-1] = (cr[:, 1:] + cr[:, :-1]) * np.float32(0.5)
    two48 = np.float32(2048)
    cb, cr, cb2, cr2 = cb - two48, cr - two48, cb2 - two48, cr2 - two48
    out = np.zeros((h, w // 2, 6), np.int64)
    for k, (y, b, r) in enumerate(((y1, cb, cr), (y2, cb2, cr2))):
        y, b, r = y.astype(np.float64), b.astype(np.float64), r.astype(np.float64)
        pr, pg1, pg2, pb = 1.370705 * r, 0.337633 * b, 0.698001 * r, 1.732446 * b
        e = (y + pr, (y - pg1) - pg2, y + pb)
        for j in range(3):
            out[..., 3 * k + j] = np.clip(np.trunc(e[j]).astype(np.int64), 0, 4095)
    return out.reshape(h, 3 * w)


def row_seeds(data, w, h):
    rows = np.asarray(data[:3 * w * h], np.uint8).reshape(h, 3 * w).astype(np.uint64)
    return rows[:, 0] + (rows[:, 1] << np.uint64(8)) + (rows[:, 2] << np.uint64(16))


def states_by_jump(seeds, n):
    """the generator's state in front of sample 0 .. n - 1 of every row: seed 15700^k mod M"""
    p = np.empty(n, np.uint64)
    x = 1
    for i in range(n):
        p[i] = x
        x = x * 15700 % M
    return ((seeds[:, None] * p[None, :]) % np.uint64(M)).astype(np.int64)


def states_by_stepping(seeds, n):
    """the same, the reference's way: one step per sample"""
    r = seeds.astype(np.int64)
    out = np.empty((len(seeds), n), np.int64)
    for i in range(n):
        out[:, i] = r
        r = (15700 * (r & 65535) + (r >> 16)) & 0xFFFFFFFF
    return out


def model_decode(data, w, h, inv_r, inv_b, table, jump=True):
    """The loop of NefDecoder.cpp:714-792: the image (h, 3 w) uint16"""
    data = np.asarray(data, np.uint8)
    v = model_values(data, w, h)
    states = states_by_jump if jump else states_by_stepping
    r = states(row_seeds(data, w, h), 3 * w)
    t = np.asarray(table, np.int64)
    x = (t[2 * v] + ((t[2 * v + 1] * (r & 2047) + 1024) >> 12)) & 0xFFFF
    out = x.copy()
    out[:, 0::3] = np.minimum(32767, (inv_r * x[:, 0::3] + 512) >> 10)
    out[:, 2::3] = np.minimum(32767, (inv_b * x[:, 2::3] + 512) >> 10)
    return out.astype(np.uint16)


def green_fused(y, cb, cr):
    """what a device that contracts the green expression into fused operations computes:
    fma(-0.698001, cr, fma(-0.337633, cb, y)), each fma rounded once (exact rational arithmetic)"""
    from fractions import Fraction as F
    inner = float(F(y) - F(0.337633) * F(cb))
    return int(float(F(inner) - F(0.698001) * F(cr)))


# ---------------------------------------------------------------------------- recorded answers
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "snef_ref.json")
GOLDEN_SEEDS = list(range(0, 51, 3)) + [1, 4, 10, 21]  # every FMA pair, clamps, limits, a wide one
YS = [2047, 0, 4095, 1000, 3000, 1, 2048]


def fma_case():
    """Every FMA pair with each of seven luma values: (w, h, data); row k holds pair k, two
    groups a luma, the first group random (its bytes are the row's seed)"""
    pairs = fma_pairs()
    groups = 1 + 2 * len(YS)
    w, h = 2 * groups, len(pairs)
    data = np.random.default_rng(0xF3A).integers(0, 256, 3 * w * h, dtype=np.uint8)
    for k, p in enumerate(pairs):
        for i, y in enumerate(YS):
            plant_fma_pair(data, w, k, 1 + 2 * i, p, y)
    return w, h, data


def golden_cases():
    out = [("seed%d" % s,) + make_case(s) for s in GOLDEN_SEEDS]
    w, h, data = fma_case()
    out.append(("fma_pairs", w, h, (2, 1), (3, 2), data))
    return out


def load_golden():
    with open(GOLDEN) as f:
        rec = json.load(f)
    return np.array(rec["curve"], np.int64), rec["cases"]
