"""SonyArw2Decompressor (8 bits per pixel "compressed" ARW) test material: a block writer that
plants chosen fields, random streams, an ARW2 TIFF writer, the curve and TableLookUp tables
the reference builds, and a numpy model of the decode (include/rsx.h section 3i).

Row y of a w-pixel image is the bytes [y w, (y + 1) w).  A row is w / 16 blocks of 16 bytes;
block b holds the columns 32 (b >> 1) + (b & 1) + 2 i.  In a block (LSB first): max bits 0-10,
min 11-21, imax 22-25, imin 26-29, fourteen 7-bit fields from bit 30.  The codec is fixed
rate, so any bytes with imax != imin in every block are a valid stream."""
import numpy as np

import rawfiles as R

M = 15700 * 65536 - 1  # the dither generator's modulus (tests/test_dither_jump_model.py)
NONE, PLAIN, DITHER = 0, 1, 2
TILE_ERRORS, INVALID_ARG = 9, 1


def pack_block(mx, mn, imax, imin, fields):
    """16 bytes: max, min, imax, imin and the 14 7-bit fields"""
    assert len(fields) == 14
    v = (mx & 0x7FF) | ((mn & 0x7FF) << 11) | ((imax & 15) << 22) | ((imin & 15) << 26)
    for k, f in enumerate(fields):
        v |= (int(f) & 0x7F) << (30 + 7 * k)
    return v.to_bytes(16, "little")


def random_stream(rng, w, h):
    """w * h random bytes, imax != imin forced in every block"""
    a = rng.integers(0, 256, size=(h, w // 16, 16), dtype=np.uint8)
    b3 = a[:, :, 3]
    imax = (a[:, :, 2] >> 6) | ((b3 & 3) << 2)
    imin = (b3 >> 2) & 15
    same = imax == imin
    b3[same] = (b3[same] & ~np.uint8(0x3C)) | ((((imin[same] + 1) & 15) << 2).astype(np.uint8))
    return a.reshape(-1)


def set_block(data, w, row, b, blk):
    data = np.array(data, dtype=np.uint8, copy=True)
    o = row * w + 16 * b
    data[o:o + 16] = np.frombuffer(blk, np.uint8)
    return data


def arw2_file(w, h, data, curve_points=(0, 0, 0, 0), gap=0, tag_h=None):
    """ArwDecoder's compression-32767 file whose strip size is exactly w * h (so not ARW1):
    bps 8, the SONYCURVE points, SONYRAWIMAGESIZE = the whole image (no crop)."""
    raw = R.Ifd()
    raw.add(R.IMAGEWIDTH, R.LONG, w).add(R.IMAGELENGTH, R.LONG, h if tag_h is None else tag_h)
    raw.add(R.BITSPERSAMPLE, R.SHORT, 8)
    raw.add(R.COMPRESSION, R.SHORT, 32767)
    raw.add(R.PHOTOMETRIC, R.SHORT, 32803)
    raw.add(R.SAMPLESPERPIXEL, R.SHORT, 1)
    raw.add(R.SONYCURVE, R.SHORT, list(curve_points))
    raw.add(R.SONYRAWIMAGESIZE, R.LONG, [w, h])
    raw.add_blobs(R.STRIPOFFSETS, R.STRIPBYTECOUNTS, [np.asarray(data, np.uint8)])
    root = R.Ifd()
    root.add(R.MAKE, R.ASCII, "SONY").add(R.MODEL, R.ASCII, "ILCE-RSX")
    root.add_sub(raw)
    return R.tiff_file(root, gap)


REALISTIC_CURVE = (8000, 10400, 12900, 14100)  # (the SONYCURVE of many Sony bodies)


def decode_curve(points):
    """ArwDecoder::decodeCurve (ArwDecoder.cpp:147-162): 0x4001 entries"""
    sc = [0] + [(int(p) >> 2) & 0xFFF for p in points] + [4095]
    curve = list(range(0x4001))
    for i in range(5):
        for j in range(sc[i] + 1, sc[i + 1] + 1):
            curve[j] = (curve[j - 1] + (1 << i)) & 0xFFFF
    return np.array(curve, np.int64)


def table_plain(curve, n=4096):
    """TableLookUp::setTable without dither (TableLookUp.cpp): the first n entries"""
    c = np.asarray(curve, np.int64)
    i = np.arange(n)
    return c[np.minimum(i, len(c) - 1)].astype(np.uint16)


def table_dither(curve, n=8192):
    """TableLookUp::setTable with dither: [2 i] = base, [2 i + 1] = delta; the first n entries"""
    c = np.asarray(curve, np.int64)
    nf = len(c)
    t = np.zeros(2 * max(nf, n // 2), np.int64)
    lower = np.concatenate([c[:1], c[:-1]])
    upper = np.concatenate([c[1:], c[-1:]])
    lower = np.minimum(lower, c)
    upper = np.maximum(upper, c)
    delta = upper - lower
    t[0:2 * nf:2] = np.clip(c - (delta + 2) // 4, 0, 65535)
    t[1:2 * nf:2] = delta
    t[2 * nf::2] = c[-1]
    return t[:n].astype(np.uint16)


def random_monotone_points(rng):
    return tuple(sorted(int(x) for x in rng.integers(0, 1 << 14, 4)))


def _fields(data, w, h):
    """(max, min, imax, imin, fields (h, bpr, 14)) of every block"""
    a = np.asarray(data[:w * h], np.uint8).reshape(h, w // 16, 16)
    W = a.view("<u4").astype(np.uint64)  # (h, bpr, 4)

    def bits(q, n):
        lo, s = q >> 5, q & 31
        v = W[:, :, lo] >> np.uint64(s)
        if s + n > 32:
            v |= W[:, :, lo + 1] << np.uint64(32 - s)
        return (v & np.uint64((1 << n) - 1)).astype(np.int64)

    F = np.stack([bits(30 + 7 * k, 7) for k in range(14)], axis=-1)
    return bits(0, 11), bits(11, 11), bits(22, 4), bits(26, 4), F


def model_values(data, w, h):
    """p (before p << 1) of every pixel in decode order: (h, bpr, 16), and the bad rows"""
    mx, mn, imax, imin, F = _fields(data, w, h)
    diff = mx - mn
    sh = (diff >= 0x80).astype(np.int64) + (diff >= 0x100) + (diff >= 0x200) + (diff >= 0x400)
    out = np.zeros(mx.shape + (16,), np.int64)
    for i in range(16):
        k = i - (i > imax).astype(np.int64) - (i > imin)
        f = np.take_along_axis(F, np.clip(k, 0, 13)[..., None], axis=-1)[..., 0]
        p = np.minimum(0x7FF, (f << sh) + mn)
        p = np.where(imin == i, mn, p)
        p = np.where(imax == i, mx, p)
        out[..., i] = p
    bad = (imax == imin).any(axis=1)
    return out, bad


def _powers(n):
    p = np.empty(n, np.uint64)
    x = 1
    for i in range(n):
        p[i] = x
        x = x * 15700 % M
    return p


def model_decode(data, w, h, mode=NONE, table=None):
    """The device's decode: (status, image (h, w) uint16, row statuses).  The dither state of
    step n = 16 b + i of a row is its seed * 15700^n mod M (the jump-ahead)."""
    data = np.asarray(data, np.uint8)
    P, bad = model_values(data, w, h)  # (h, bpr, 16)
    v = (P << 1).reshape(h, w)          # decode order: step n = 16 b + i
    if mode == PLAIN:
        t = np.asarray(table, np.int64)
        v = t[v]
    elif mode == DITHER:
        t = np.asarray(table, np.int64)
        rows = data[:w * h].reshape(h, w).astype(np.uint64)
        seed = rows[:, 0] | (rows[:, 1] << np.uint64(8)) | (rows[:, 2] << np.uint64(16))
        r = (seed[:, None] * _powers(w)[None, :]) % np.uint64(M)
        r = r.astype(np.int64)
        base, delta = t[2 * v], t[2 * v + 1]
        v = (base + ((delta * (r & 2047) + 1024) >> 12)) & 0xFFFF
    bpr = w // 16
    b = np.arange(bpr)[:, None]
    i = np.arange(16)[None, :]
    cols = (32 * (b >> 1) + (b & 1) + 2 * i).reshape(-1)
    img = np.zeros((h, w), np.uint16)
    img[:, cols] = v.astype(np.uint16)
    rows = [INVALID_ARG if x else 0 for x in bad]
    return (TILE_ERRORS if bad.any() else 0), img, rows


class _Bits:
    """BitStreamerLSB over one row (what decompressRow reads)"""

    def __init__(self, row):
        self.v, self.pos = int.from_bytes(bytes(row), "little"), 0

    def peek(self, n):
        return (self.v >> self.pos) & ((1 << n) - 1)

    def get(self, n):
        x = self.peek(n)
        self.pos += n
        return x


def stepping_row(row_bytes, w, mode=NONE, table=None):
    """One row the reference's way, literally: a bit reader, and the dither generator stepped
    once per pixel (SonyArw2Decompressor.cpp:56-110).  Returns (ok, values)."""
    bits = _Bits(row_bytes)
    r = bits.peek(24)
    out = [0] * w
    col = 0
    while col < w:
        mx, mn, imax, imin = bits.get(11), bits.get(11), bits.get(4), bits.get(4)
        if imax == imin:
            return False, out
        sh = 0
        while sh < 4 and (0x80 << sh) <= mx - mn:
            sh += 1
        for i in range(16):
            if i == imax:
                p = mx
            elif i == imin:
                p = mn
            else:
                p = min(0x7FF, (bits.get(7) << sh) + mn)
            v = p << 1
            if mode == PLAIN:
                v = int(table[v])
            elif mode == DITHER:
                base, delta = int(table[2 * v]), int(table[2 * v + 1])
                v = (base + ((delta * (r & 2047) + 1024) >> 12)) & 0xFFFF
                r = (15700 * (r & 65535) + (r >> 16)) & 0xFFFFFFFF
            out[col + 2 * i] = v
        col += 31 if col & 1 else 1
    return True, out
