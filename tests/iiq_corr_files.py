"""TEST INFRASTRUCTURE: Phase One IIQ files with a correction block, and numpy models of the
pixel passes of IiqDecoder::CorrectPhaseOneC (include/rsx.h section 3n).

  iiq_corr_file()    a whole IIQ "L" file like iiq_files.iiq_file(), with the entries 0x110 (the
                     correction block), 0x21d (black level << 2), 0x222 (split column) and 0x224
                     (split row) on top; it goes through the reference's front door
  meta_block()       the correction block: 8 bytes, the u32 offset of the entry table, at that
                     offset a count, 4 bytes, then (tag, len, offset) triples
                     (IiqDecoder.cpp:280-325)
  flat_field()       PhaseOneFlatField (:410-479) in numpy binary32, luma and chroma as one function:
                     the running sums as repeated additions, every operation rounded on its own
  quadrant()         CorrectQuadrantMultipliersCombined's pixel loop (:375-404) for given curves
  quadrant_curves()  the four curves of a 0x431 payload: the control points of :338-373 through
  spline_curve()     Spline<>::calculateCurve (common/Spline.h) restated in binary64
  apply()            a list of ops, one after the other, on a copy of the image
"""
import hashlib
import json
import os
import struct

import numpy as np

import iiq_files as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "iiq_corr_ref.json")
OK, INVALID_ARG, UNSUPPORTED, IO = 0, 1, 6, 2
f32 = np.float32


# ---------------------------------------------------------------------------------------
# the file
# ---------------------------------------------------------------------------------------
def meta_block(entries):
    """entries: [(tag, payload bytes)] in file order"""
    out = bytearray(12)
    pos = 12
    offs = []
    for _, data in entries:
        offs.append(pos)
        out += data
        pos += len(data)
    struct.pack_into("<I", out, 8, pos)
    out += struct.pack("<II", len(entries), 0)
    for (tag, data), off in zip(entries, offs):
        out += struct.pack("<III", tag, len(data), off)
    return bytes(out)


def iiq_corr_file(img, meta=None, black=None, split_row=None, split_col=None, seed=1,
                  make="Phase One A/S", model="IQ180", wb=(2.0, 1.0, 1.5)):
    """img: (h, w) uint16, w even.  meta: meta_block() bytes or None (no 0x110 entry).  black is
    what IiqDecoder::black_level becomes (the file holds black << 2)."""
    h, width = img.shape
    rows = F.encode(img, seed)
    raw = bytearray()
    offsets = []
    for r in rows:
        offsets.append(len(raw))
        raw += r
    tiff = F._ifd([(271, 2, len(make) + 1, make.encode() + b"\0"),
                   (272, 2, len(model) + 1, model.encode() + b"\0")], 24)
    pos = 24 + len(tiff)
    pos += -pos % 4
    extra = [(0x110, 0, None)] if meta is not None else []
    if black is not None:
        extra.append((0x21D, 4, black << 2))
    if split_col is not None:
        extra.append((0x222, 4, split_col))
    if split_row is not None:
        extra.append((0x224, 4, split_row))
    n_entries = 6 + len(extra)
    ent_abs = pos
    wb_abs = ent_abs + 8 + 16 * n_entries
    off_abs = wb_abs + 12
    raw_abs = off_abs + 4 * len(offsets)
    meta_abs = raw_abs + len(raw)
    rel = lambda a: a - 8  # noqa: E731  (IIQ offsets are relative to byte 8)
    entries = [(0x107, 12, rel(wb_abs)), (0x108, 4, width), (0x109, 4, h), (0x10E, 4, 3),
               (0x10F, len(raw), rel(raw_abs)), (0x21C, 4 * len(offsets), rel(off_abs))]
    for tag, length, data in extra:
        entries.append((tag, len(meta), rel(meta_abs)) if tag == 0x110 else (tag, length, data))
    out = bytearray(meta_abs + (len(meta) if meta is not None else 0))
    out[0:8] = b"II" + struct.pack("<HI", 42, 24)
    out[8:12] = b"IIII"
    struct.pack_into("<II", out, 16, rel(ent_abs), 0)
    out[24:24 + len(tiff)] = tiff
    struct.pack_into("<II", out, ent_abs, n_entries, 0)
    for i, (tag, length, data) in enumerate(entries):
        struct.pack_into("<IIII", out, ent_abs + 8 + 16 * i, tag, 0, length, data)
    struct.pack_into("<3f", out, wb_abs, *wb)
    struct.pack_into("<%dI" % len(offsets), out, off_abs, *offsets)
    out[raw_abs:meta_abs] = raw
    if meta is not None:
        out[meta_abs:] = meta
    return np.frombuffer(bytes(out), dtype=np.uint8).copy()


# ---------------------------------------------------------------------------------------
# flat field
# ---------------------------------------------------------------------------------------
def ff_payload(head, values, planes=1):
    """head: the first six (or eight) head fields; values: (high, wide[, planes]) u16"""
    h = list(head) + [0] * (8 - len(head))
    v = np.asarray(values, dtype="<u2")
    return struct.pack("<8H", *h) + v.tobytes()


def ff_shape(head):
    """(wide, high) or None when a head field 2..5 is zero"""
    if 0 in head[2:6]:
        return None
    return -(-head[2] // head[4]), -(-head[3] // head[5])


def ff_random(rng, head, planes=1, lo=24000, hi=44000):
    wide, high = ff_shape(head)
    return ff_payload(head, rng.integers(lo, hi + 1, size=(high, wide, planes)), planes)


def flat_field(img, payload, chroma=False, cfa=None, sums=True):
    """(status, image).  IO: the payload ends before the values the reference reads (it throws
    half-way, the file fails).  cfa = (cfa_w, cfa_h, colours).  sums=False computes the running
    sums as a + k * step instead of k additions -- NOT what the reference does (a test shows the
    golden file tells the two apart)."""
    img = np.array(img, dtype=np.uint16)
    planes = 2 if chroma else 1
    if len(payload) < 16:
        return IO, img
    head = struct.unpack_from("<8H", payload, 0)
    if ff_shape(head) is None:
        return OK, img
    wide, high = ff_shape(head)
    if len(payload) < 16 + 2 * high * wide * planes:
        return IO, img
    v = np.frombuffer(payload, dtype="<u2", count=high * wide * planes, offset=16)
    num = (v.astype(f32) / f32(32768.0)).reshape(high, wide, planes)
    H, W = img.shape
    h0, h1, h2, h3, h4, h5 = head[:6]
    mrow = num[0].copy()
    if chroma:
        cw, ch, colours = cfa
        colours = np.asarray(colours, dtype=np.int64)
    for y in range(1, high):
        slope = ((num[y] - mrow) / f32(h5)).astype(f32)
        row0, k = h1 + (y - 1) * h5, 0
        base = mrow.copy()
        for row in range(row0, min(H, row0 + h5, h1 + h3 - h5)):
            for x in range(1, wide):
                c0 = h0 + (x - 1) * h4
                c1 = min(W, c0 + h4, h0 + h2 - h4)
                if c1 <= c0:
                    break
                n = c1 - c0
                mult = mrow[x - 1].copy()                                # (planes,)
                step = ((mrow[x] - mult) / f32(h4)).astype(f32)
                if sums:
                    acc = np.empty((n, planes), f32)
                    acc[0] = mult
                    for j in range(1, n):
                        acc[j] = acc[j - 1] + step
                else:
                    acc = (mult[None, :] + np.arange(n, dtype=f32)[:, None] * step[None, :]).astype(f32)
                cols = np.arange(c0, c1)
                px = img[row, c0:c1].astype(f32)
                if chroma:
                    colour = colours[(row % cw) + (cols % ch) * cw]
                    plane = np.where(colour == 2, 1, 0)
                    on = (colour & 1) == 0
                else:
                    plane = np.zeros(n, np.int64)
                    on = np.ones(n, bool)
                prod = (px * acc[np.arange(n), plane]).astype(f32)
                val = np.clip(np.trunc(np.maximum(prod, f32(0)).astype(np.float64)), 0, 65535)
                img[row, c0:c1] = np.where(on, val.astype(np.uint16), img[row, c0:c1])
            if sums:
                mrow = (mrow + slope).astype(f32)
            else:
                k += 1
                mrow = (base + f32(k) * slope).astype(f32)
    return OK, img


# ---------------------------------------------------------------------------------------
# quadrant curves
# ---------------------------------------------------------------------------------------
def spline_curve(points):
    """Spline<uint16_t>(points).calculateCurve(): points [(x, y)], x from 0 to 65535 rising"""
    n = len(points)
    ns = n - 1
    xs = [int(p[0]) for p in points]
    a = [float(p[1]) for p in points]
    h = [float(xs[i + 1] - xs[i]) for i in range(ns)]
    alpha = [0.0] * ns
    for i in range(1, ns):
        alpha[i] = (3. / h[i]) * (a[i + 1] - a[i]) - (3. / h[i - 1]) * (a[i] - a[i - 1])
    mu, z = [0.0] * n, [0.0] * n
    for i in range(1, ns):
        l = 2 * (xs[i + 1] - xs[i - 1]) - (h[i - 1] * mu[i - 1])
        mu[i] = h[i] / l
        z[i] = (alpha[i] - h[i - 1] * z[i - 1]) / l
    c = [0.0] * n
    b, d = [0.0] * ns, [0.0] * ns
    for i in range(ns - 1, -1, -1):
        c[i] = z[i] - mu[i] * c[i + 1]
        b[i] = (a[i + 1] - a[i]) / h[i] - h[i] * (c[i + 1] + 2 * c[i]) / 3.
        d[i] = (c[i + 1] - c[i]) / (3. * h[i])
    curve = np.zeros(65536, np.uint16)
    for i in range(ns):
        diff = np.arange(0, xs[i + 1] - xs[i] + 1, dtype=np.float64)
        diff_2 = diff * diff
        diff_3 = diff * diff * diff
        v = a[i] + b[i] * diff + c[i] * diff_2 + d[i] * diff_3
        curve[xs[i]:xs[i + 1] + 1] = np.minimum(np.maximum(v, 0.0), 65535.0).astype(np.uint16)
    return curve


def quad_payload(xs, mults):
    """xs: the seven middle x coordinates; mults: (2, 2, 7) in ten-thousandths"""
    return struct.pack("<7I", *xs) + struct.pack("<28I", *np.asarray(mults).reshape(28))


def quadrant_curves(payload):
    """(4, 65536) uint16, [quadRow * 2 + quadCol]"""
    xs = [0] + list(struct.unpack_from("<7I", payload, 0)) + [65535]
    m = struct.unpack_from("<28I", payload, 28)
    out = np.empty((4, 65536), np.uint16)
    for q in range(4):
        pts = [(0, 0)] + [(xs[i], m[7 * q + i - 1] * xs[i] // 10000) for i in range(1, 8)] + \
              [(65535, 65535)]
        out[q] = spline_curve(pts)
    return out


def quadrant(img, curves, split_row, split_col, black):
    img = np.array(img, dtype=np.uint16)
    H, W = img.shape
    q = (np.arange(H)[:, None] >= split_row) * 2 + (np.arange(W)[None, :] >= split_col)
    px = img.astype(np.int64)
    diff = np.where(px < black, px, black & 0xFFFF)
    return ((np.asarray(curves).reshape(4, 65536)[q, px - diff].astype(np.int64) + diff) & 0xFFFF).astype(np.uint16)


def random_curves(rng):
    """four arbitrary curves: every entry its own value (sums that wrap past 65535 included)"""
    return rng.integers(0, 65536, size=(4, 65536)).astype(np.uint16)


# ---------------------------------------------------------------------------------------
# lists
# ---------------------------------------------------------------------------------------
def apply(img, ops, cfa=None, sums=True):
    """ops as abi.iiq_corr takes them: ("ff", payload, chroma) / ("quad", curves, split_row,
    split_col, black).  (status, image): the image is the input when the status is not OK."""
    out = np.array(img, dtype=np.uint16)
    for op in ops:
        if op[0] == "ff":
            st, out = flat_field(out, op[1], bool(op[2]), cfa, sums)
            if st != OK:
                return st, np.array(img, dtype=np.uint16)
        else:
            out = quadrant(out, op[1], op[2], op[3], op[4])
    return OK, out


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---------------------------------------------------------------------------------------
# the cases held against the reference (tests/test_iiq_corr_model.py, the golden file)
# ---------------------------------------------------------------------------------------
QX = (2000, 6000, 12000, 20000, 32000, 45000, 60000)


def _quad_payload(rng):
    return quad_payload(QX, rng.integers(9000, 10600, size=(2, 2, 7)))


def file_cases():
    """(name, image, [(tag, payload)], black, split_row, split_col).  Luma 0x410 and 0x431 only: the
    reference's chroma needs a CFA, which a decode without a camera database does not have."""
    rng = np.random.default_rng(0x11C)
    img = rng.integers(0, 65536, size=(40, 64)).astype(np.uint16)
    img[:4] = rng.integers(0, 3000, size=(4, 64))
    luma = {
        "offset_7x5": ff_random(rng, (3, 2, 56, 30, 7, 5)),
        "cells_8x8": ff_random(rng, (0, 0, 64, 40, 8, 8)),
        "past_13x11": ff_random(rng, (5, 3, 130, 121, 13, 11)),
        "cells_1x1": ff_payload((0, 0, 40, 20, 1, 1), np.full((20, 40), 65535)),
        "drift": ff_payload((0, 0, 64, 40, 16, 13),
                            np.where(np.arange(4)[:, None] % 2 == 0, 0, 3)
                            * np.ones((1, 4), np.int64) + np.array([[0, 1, 0, 7]])),
    }
    q = _quad_payload(rng)
    cases = [(n, img, [(0x410, p)], None, None, None) for n, p in luma.items()]
    cases += [("quad_black%d" % b, img, [(0x431, q)], b, 17, 29) for b in (0, 1500, 70000)]
    cases += [("quad_split_0_0", img, [(0x431, q)], 800, 0, 0),
              ("quad_split_full", img, [(0x431, q)], 800, 40, 64),
              ("luma_quad", img, [(0x410, luma["offset_7x5"]), (0x431, q)], 900, 20, 32),
              ("quad_luma", img, [(0x431, q), (0x410, luma["past_13x11"])], 900, 20, 32),
              ("two_luma", img, [(0x410, luma["cells_8x8"]), (0x410, luma["offset_7x5"])], None, None, None),
              ("short_payload", img, [(0x410, luma["cells_8x8"][:-1])], None, None, None),
              ("short_head", img, [(0x410, luma["cells_8x8"][:15])], None, None, None),
              ("head_zero", img, [(0x410, ff_payload((0, 0, 64, 40, 0, 8), []))], None, None, None)]
    return cases


def case_ops(entries, black, split_row, split_col):
    """the op list of a file's entries, as abi.iiq_corr takes it"""
    ops = []
    for tag, p in entries:
        if tag == 0x431:
            ops.append(("quad", quadrant_curves(p), split_row or 0, split_col or 0, black or 0))
        else:
            ops.append(("ff", p, tag == 0x40B))
    return ops


def case_file(case):
    name, img, entries, black, split_row, split_col = case
    return iiq_corr_file(img, meta_block(entries), black, split_row, split_col)


def curve_pin_file():
    """512 x 512, split at (256, 256), every quadrant holds each value 0 .. 65535 once, black level
    0: the decoded image IS the four curves.  Returns (file, payload, positions): positions[q] the
    flat index order of quadrant q's values."""
    rng = np.random.default_rng(0x431)
    img = np.empty((512, 512), np.uint16)
    perms = []
    for q in range(4):
        perm = rng.permutation(65536).astype(np.uint16)
        perms.append(perm)
        img[(q >> 1) * 256:(q >> 1) * 256 + 256, (q & 1) * 256:(q & 1) * 256 + 256] = perm.reshape(256, 256)
    payload = _quad_payload(rng)
    return iiq_corr_file(img, meta_block([(0x431, payload)]), 0, 256, 256), payload, perms


def curves_from_image(dec, perms):
    out = np.empty((4, 65536), np.uint16)
    for q in range(4):
        blk = dec[(q >> 1) * 256:(q >> 1) * 256 + 256, (q & 1) * 256:(q & 1) * 256 + 256].reshape(-1)
        out[q][perms[q]] = blk
    return out


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)
