"""NikonDecompressor test inputs: the makernote linearisation blob the reference
constructor parses (NikonDecompressor.cpp:473-513, createCurve :381-445), a
restatement of that parse (what fills rsx_nikon_desc on the reference side), and
two stream generators."""
import numpy as np

from rawspeed_amd import abi, synth


def metadata(v0, v1, p_up, points=None, split=0, pad_to=600):
    """Big-endian blob: v0, v1, [2110 skipped bytes], pUp x4, csize, curve
    points ..., and the split row at absolute offset 562."""
    b = bytearray([v0, v1])
    if v0 == 73 or v1 == 88:
        b += bytes(2110)
    for p in p_up:
        b += int(p).to_bytes(2, "big")
    points = [] if points is None else list(points)
    b += len(points).to_bytes(2, "big")
    for p in points:
        b += int(p).to_bytes(2, "big")
    if len(b) < pad_to:
        b += bytes(pad_to - len(b))
    if split:
        b[562:564] = int(split).to_bytes(2, "big")
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def parse(meta, bits_ps, dim_y):
    """NikonDecompressor::NikonDecompressor + createCurve, restated."""
    m = bytes(meta)
    pos = 0

    def u16():
        nonlocal pos
        v = int.from_bytes(m[pos:pos + 2], "big")
        pos += 2
        return v

    v0, v1 = m[0], m[1]
    pos = 2
    if v0 == 73 or v1 == 88:
        pos += 2110
    huff_select = 2 if v0 == 70 else 0
    if bits_ps == 14:
        huff_select += 3
    p_up = [u16(), u16(), u16(), u16()]            # [0][0], [1][0], [0][1], [1][1]
    p_up = [[p_up[0], p_up[2]], [p_up[1], p_up[3]]]
    cbits = bits_ps - 2 if (v0 == 68 and v1 == 64) else bits_ps   # Z7 hack
    curve = list(range(((1 << cbits) & 0x7fff) + 1))
    split = 0
    csize = u16()
    step = len(curve) // (csize - 1) if csize > 1 else 0
    if v0 == 68 and v1 in (32, 64) and step > 0:
        assert (csize - 1) * step == len(curve) - 1, "Bad curve segment count"
        for i in range(csize):
            curve[i * step] = u16()
        for i in range(len(curve) - 1):
            b_scale = i % step
            a_pos = i - b_scale
            b_pos = a_pos + step
            a_scale = step - b_scale
            curve[i] = ((a_scale * curve[a_pos] + b_scale * curve[b_pos]) // step) & 0xFFFF
        split = int.from_bytes(m[562:564], "big")
    elif v0 != 70:
        assert 0 < csize <= 0x4001
        curve = [u16() for _ in range(csize)] + [0]
    curve = curve[:-1]
    if split >= dim_y:
        split = 0
    return dict(huff_select=huff_select, p_up=p_up, curve=np.array(curve, np.uint16),
                split=split)


def desc(parsed, bits_ps, uncorrected):
    d = abi.NikonDesc()
    d.bits_ps = bits_ps
    d.split = parsed["split"]
    for r in range(2):
        for c in range(2):
            d.p_up[r][c] = parsed["p_up"][r][c]
    d.uncorrected_raw_values = 1 if uncorrected else 0
    d.set_curve(parsed["curve"])
    hs = parsed["huff_select"]
    d.tables[0] = abi.HuffTable.make(*synth.NIKON_TREE[hs])
    if parsed["split"]:
        d.tables[1] = abi.HuffTable.make(*synth.NIKON_TREE[hs + 1])
    return d


def _canonical(tree):
    counts, values = tree
    out, code, k = [], 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            out.append((code, l, values[k]))
            code += 1
            k += 1
        code <<= 1
    return out


def symbol_stream(rng, n0, tree0, n1=0, tree1=None, tail=8):
    """n0 random symbols of tree0 (plain SSSS values) followed by n1 of tree1
    ("after split": len | shl << 4, len - shl raw bits), as an MSB bit stream.
    The decoded image is whatever the reference makes of it."""
    vals, lens = [], []
    for n, tree, las in ((n0, tree0, False), (n1, tree1, True)):
        if not n:
            continue
        sym = _canonical(tree)
        p = np.array([2.0 ** -l for (_, l, _) in sym])
        idx = rng.choice(len(sym), size=n, p=p / p.sum())
        code = np.array([s[0] for s in sym], np.int64)[idx]
        clen = np.array([s[1] for s in sym], np.int64)[idx]
        v = np.array([s[2] for s in sym], np.int64)[idx]
        nb = np.where(v == 16, 0, (v & 15) - (v >> 4)) if las else np.where(v == 16, 0, v)
        extra = rng.integers(0, 1 << 16, size=n, dtype=np.int64) & ((1 << nb) - 1)
        # keep the walk near the middle: mostly small magnitudes
        vals.append((code << nb) | extra)
        lens.append(clen + nb)
    val, ln = np.concatenate(vals), np.concatenate(lens)
    start = np.concatenate([[0], np.cumsum(ln)[:-1]])
    total = int(ln.sum())
    bits = np.zeros(total + 8, np.uint8)
    for k in range(int(ln.max())):
        m = k < ln
        bits[start[m] + k] = (val[m] >> (ln[m] - 1 - k)) & 1
    return np.concatenate([np.packbits(bits), np.zeros(tail, np.uint8)])


def smooth15(rng, h, w, maxv=16383, sigma=12.0):
    """A 2x2-CFA-like image whose same-colour neighbour differences are small."""
    x = np.arange(w)[None, :]
    y = np.arange(h)[:, None]
    img = (0.25 * maxv + 0.3 * maxv * x / w + 0.2 * maxv * y / h +
           0.05 * maxv * ((x & 1) + 2 * (y & 1)) + rng.normal(0, sigma, size=(h, w)))
    return np.clip(img, 0, maxv).astype(np.uint16)


# ---- PentaxDecompressor ---------------------------------------------------------

def pentax_metadata(tree):
    """The makernote blob SetupPrefixCodeDecoder_Modern (PentaxDecompressor.cpp:
    85-137) turns back into `tree`: depth - 12 (u16), 12 skipped bytes, per
    difference length its code left-aligned in 12 bits (u16), then its length."""
    sym = _canonical(tree)
    depth = len(sym)
    assert 12 <= depth <= 15 and sorted(v for _, _, v in sym) == list(range(depth))
    v0, v1 = [0] * depth, [0] * depth
    for code, l, v in sym:
        assert l <= 12
        v0[v], v1[v] = code << (12 - l), l
    b = bytearray((depth - 12).to_bytes(2, "big")) + bytes(12)
    for x in v0:
        b += x.to_bytes(2, "big")
    b += bytes(v1)
    return np.frombuffer(bytes(b), np.uint8).copy()


def pentax_desc(tree):
    d = abi.PentaxDesc()
    d.table = abi.HuffTable.make(*tree)
    return d


# a "modern" tree: 15 difference lengths, none longer than 12 bits
PENTAX_MODERN = ([0, 1, 3, 3, 2, 2, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0],
                 [4, 3, 5, 2, 6, 1, 7, 0, 8, 9, 10, 11, 12, 13, 14])


def pentax_encode(img, tree):
    """NikonDecompressor's predictor with all four pUp = 0 is PentaxDecompressor's
    (rows 0 and 1 start from 0, later rows from the pixels two rows up)."""
    return synth.nikon_encode(img, [0, 0, 0, 0], tree)


# ---- streams of INT images, and the reconstruction they decode to ----------------------

def _codes(code):
    """{difference length: (code, code length)} of a canonical tree (Nikon / Pentax), or of
    SamsungV1's (encLen, diffLen) pairs in table-fill order (SamsungV1Decompressor.cpp:
    110-117: entry i fills 1024 >> encLen slots of the 10-bit table from where the last one
    stopped, so its code is that slot's top encLen bits)."""
    if len(code) == 2 and len(code[0]) == 16:
        return {v: (c, l) for (c, l, v) in _canonical(code)}
    out, n = {}, 0
    for enc, dif in code:
        out.setdefault(dif, (n >> (10 - enc), enc))
        n += 1024 >> enc
    assert n == 1024
    return out


def prefix_diffs(src, p_up):
    """The differences NikonDecompressor.cpp:518-560 (and, with all four p_up = 0,
    PentaxDecompressor.cpp:155-177 / SamsungV1Decompressor.cpp:123-137) decode `src` -- given
    as INTS, whatever the decoder does with values outside its range -- from: the first pair
    of a row from the row two above, the others from the sample two to the left."""
    src = np.asarray(src, np.int64)
    h, w = src.shape
    pred = np.empty_like(src)
    pred[:, 2:] = src[:, :-2]
    up = np.array(p_up, np.int64).reshape(2, 2)
    for y in range(h):
        pred[y, :2] = up[y & 1]
        up[y & 1] = src[y, :2]
    return src - pred


def prefix_symbols(diff, code):
    """Per difference (row-major) its symbol as (bits, length): the code of its length, then
    the length's low bits of the difference (ones' complement below zero)."""
    diff = np.asarray(diff, np.int64).ravel()
    mag = np.abs(diff)
    ssss = np.where(mag == 0, 0, np.floor(np.log2(np.maximum(mag, 1))).astype(np.int64) + 1)
    by_len = _codes(code)
    missing = set(np.unique(ssss).tolist()) - set(by_len)
    if missing:
        raise ValueError("no code for difference lengths %s" % sorted(missing))
    lut_c = np.zeros(17, np.int64)
    lut_l = np.zeros(17, np.int64)
    for v, (c, l) in by_len.items():
        lut_c[v], lut_l[v] = c, l
    extra = np.where(diff >= 0, diff, diff + (1 << ssss) - 1)
    return (lut_c[ssss] << ssss) | extra, lut_l[ssss] + ssss


def symbol_bits(val, ln):
    """The symbols as one MSB-first bit per byte (np.uint8 of 0 / 1)."""
    out = []
    for k in range(0, val.size, 1 << 20):
        v, l = val[k:k + (1 << 20)], ln[k:k + (1 << 20)]
        assert l.size == 0 or (l.min() >= 1 and l.max() <= 32)
        m = np.unpackbits((v << (32 - l)).astype(">u4").view(np.uint8)).reshape(-1, 32)
        out.append(m[np.arange(32)[None, :] < l[:, None]])
    return np.concatenate(out) if out else np.zeros(0, np.uint8)


def encode_ints(src, p_up, code):
    """The stream of an image given as INTS (values outside the decoder's range are what its
    sums reach before clampBits(., 15) / the range check), `code` a canonical tree or
    SamsungV1's pairs; p_up all zeros for Pentax and SamsungV1."""
    val, ln = prefix_symbols(prefix_diffs(src, p_up), code)
    return np.concatenate([np.packbits(np.concatenate([symbol_bits(val, ln), np.zeros(8, np.uint8)])),
                           np.zeros(16, np.uint8)])


def prefix_model(diff, bits):
    """PentaxDecompressor::decompress (bits = 16) / SamsungV1Decompressor::decompress
    (bits = 12) in plain int64: the running predictor per column parity, rows from 2 on
    starting from out(row - 2, 0 / 1), every value checked with isIntN(value, bits) and stored
    as uint16.  Returns (image, None) or, at the first value out of range, (the image so far
    -- the rows and columns in front of it --, (row, col))."""
    diff = np.asarray(diff, np.int64)
    h, w = diff.shape
    out = np.zeros((h, w), np.uint16)
    for row in range(h):
        pred = np.zeros(2, np.int64) if row < 2 else out[row - 2, :2].astype(np.int64)
        value = np.empty(w, np.int64)
        for c in (0, 1):
            value[c::2] = pred[c] + np.cumsum(diff[row, c::2])
        bad = np.flatnonzero((value < 0) | (value >= (1 << bits)))
        if bad.size:
            col = int(bad[0])
            out[row, :col] = value[:col]
            return out, (row, col)
        out[row] = value
    return out, None


# ---- value edges of the Pentax / SamsungV1 range checks --------------------------------

# name: (code, isIntN bits, the largest difference the code has a length for, base image maxv
# -- the first sample of each parity in rows 0 and 1 is a whole difference from 0)
PREFIX_FAMILY = {
    "pentax_legacy": (synth.PENTAX_TREE, 16, 4095, 4095),
    "pentax_modern": (PENTAX_MODERN, 16, 16383, 16383),
    "samsung_v1": (synth.SAMSUNG_V1_TAB, 12, 8191, 4095),
}
# valid values at both ends of the range (and Pentax's around bit 15), then the first ones out
EDGE_VALUES = {16: (0, 32767, 32768, 65535, 65536, -1), 12: (0, 4095, 4096, -1)}
EDGE_PLACES = ("r0c0", "r1c1", "c0", "c1", "late", "last")
SLOPE = 1700  # per pixel (L1) of a planted peak: same-colour neighbours differ by 2 x SLOPE


def edge_cases(family):
    """(value, place) of a family; a value at the first sample of a parity in rows 0 and 1 (the
    predictor is 0) only if the code has a difference that long."""
    _, bits, reach, _ = PREFIX_FAMILY[family]
    return [(v, p) for v in EDGE_VALUES[bits] for p in EDGE_PLACES
            if p not in ("r0c0", "r1c1") or abs(v) <= reach]


def edge_position(place, value, reach, h, w):
    """Rows 0 and 1 start from 0, a row from 2 on from the row two above: col 0 / 1 of row 2
    where the peak's slope reaches rows 0 and 1 within the code's differences, of a middle row
    otherwise; "late": mid-row near the end of the stream; "last": the frame's last sample."""
    r = 2 if abs(value) <= reach else 2 * (h // 4)
    return {"r0c0": (0, 0), "r1c1": (1, 1), "c0": (r, 0), "c1": (r, 1),
            "late": (h - 3, w // 2 + 1), "last": (h - 1, w - 1)}[place]


def plant(base, y, x, value, slope=SLOPE):
    """`base` (ints) with ONE sample at `value`: a peak (or pit) whose sides fall by `slope` per
    pixel until they meet the base, so every other sample stays on the base's side of `value`
    and no difference is longer than the base's or 2 x slope."""
    yy, xx = np.indices(base.shape)
    d = np.abs(yy - y) + np.abs(xx - x)
    if value >= base[y, x]:
        return np.maximum(base, value - slope * d)
    return np.minimum(base, value + slope * d)


def plateau(base, y, value, slope=SLOPE):
    """Rows y .. y + 2 at `value` (+ 7 on odd columns), falling by `slope` per row above and below:
    rows y + 2 and y + 4 start from a value that large."""
    yy, xx = np.indices(base.shape)
    ridge = value + 7 * (xx & 1) - slope * np.maximum(0, np.abs(yy - (y + 1)) - 1)
    return np.maximum(base, ridge)


def edge_image(family, base, value, place):
    """(image as ints, the planted (row, col) or None for the plateau)."""
    _, _, reach, _ = PREFIX_FAMILY[family]
    h, w = base.shape
    if place == "plateau":
        return plateau(base, 2 * (h // 4), value), None
    y, x = edge_position(place, value, reach, h, w)
    return plant(base, y, x, value), (y, x)
