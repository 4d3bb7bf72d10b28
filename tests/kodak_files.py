"""Kodak DCR (KodakDecompressor, TIFF compression 65000) test material: an independent pure-Python
model of the codec -- a decoder that is a literal transcription of decodeSegment's reader, with its
64-bit buffer and its refill loop, and reach statistics; the closed forms of include/rsx.h section
3w beside it, so that they are checked against the reader and not assumed; an encoder from
lengths and fields and one from pixel differences --, the curves and TableLookUp's two table
forms, the case list (fixed seeds: every machine regenerates the same bytes), the whole-file
builder, the host build's wrapper and the golden file's reader.
"""
import ctypes as C
import functools
import hashlib
import json
import os
import random

import numpy as np

import rawfiles

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "kodak_ref.json")

OK, ERR_INVALID_ARG, ERR_IO, ERR_VALUE_RANGE = 0, 1, 2, 10
NONE, PLAIN, DITHER = 0, 1, 2
MAX_X, MAX_Y, SEGMENT = 4516, 3012, 256
KODAK_IFD, KODAK_LINEARIZATION = 0x8290, 0x090D

# what tests/test_kodak_model.py wants counted at least once over the case list
REACH = (["no_bit_words_init0", "no_bit_words_init16", "over_0", "over_32", "over_33",
          "over_negative", "len15_straddles_units", "len15_straddles_init_edge",
          "value_0", "value_max_10", "value_max_12", "io_in_nibbles", "io_in_init_unit",
          "io_in_read4", "ends_exactly", "tail_only", "no_tail", "tail_init0", "tail_init16",
          "n_full_1", "n_full_2", "n_full_17"] +
         ["range_%s_%s" % (k, w) for k in ("high", "negative") for w in ("first", "tail", "last")] +
         ["extend_%d_%s" % (n, e) for n in range(1, 16) for e in ("lo", "below", "above", "hi")])


def _status_codes():
    from rawspeed_amd import abi
    assert (abi.RSX_OK, abi.RSX_ERR_INVALID_ARG, abi.RSX_ERR_IO, abi.RSX_ERR_VALUE_RANGE) == \
        (OK, ERR_INVALID_ARG, ERR_IO, ERR_VALUE_RANGE)
    assert (abi.RSX_KODAK_TABLE_NONE, abi.RSX_KODAK_TABLE_PLAIN, abi.RSX_KODAK_TABLE_DITHER) == \
        (NONE, PLAIN, DITHER)


# ---------------------------------------------------------------------------------------------
# The closed forms (include/rsx.h section 3w)
# ---------------------------------------------------------------------------------------------
def validate(w, h, bps, in_bytes, pitch=None, cpp=1):
    """the constructor's checks in its order, the pitch, then input.check(area / 2)"""
    if cpp != 1:
        return ERR_INVALID_ARG
    if w <= 0 or h <= 0 or w % 4 or w > MAX_X or h > MAX_Y:
        return ERR_INVALID_ARG
    if bps not in (10, 12):
        return ERR_INVALID_ARG
    if pitch is not None and pitch < 2 * w:
        return ERR_INVALID_ARG
    if in_bytes < w * h // 2:
        return ERR_IO
    return OK


def init_bits(length):
    return 16 if (length & 7) == 4 else 0


def segment_bytes(length, total):
    return length // 2 + init_bits(length) // 8 + 4 * ((max(0, total - init_bits(length)) + 31) // 32)


def segment_bound(length):
    return length // 2 + 2 + 4 * ((15 * length + 31) // 32)


def row_segments(w):
    return [min(SEGMENT, w - c) for c in range(0, w, SEGMENT)]


def image_bound(w, h):
    return h * sum(segment_bound(n) for n in row_segments(w))


def extend(field, n):
    if n == 0:
        return 0
    return field if field & (1 << (n - 1)) else field - ((1 << n) - 1)


def closed_segment(data, pos, length):
    """-> (the differences, the segment's size) by the closed forms, or None where the segment
    reads past the end"""
    if pos + length // 2 > len(data):
        return None
    lens = []
    for k in range(length // 2):
        lens += [data[pos + k] & 15, data[pos + k] >> 4]
    size = segment_bytes(length, sum(lens))
    if pos + size > len(data):
        return None
    area = pos + length // 2
    out, cum = [], 0
    for n in lens:
        field = 0
        for b in range(n):
            p = cum + b
            unit = data[area + 2 * (p // 16)] << 8 | data[area + 2 * (p // 16) + 1]
            field |= ((unit >> (p % 16)) & 1) << b
        out.append(extend(field, n))
        cum += n
    return out, size


# ---------------------------------------------------------------------------------------------
# The model: decodeSegment's reader and decompress(), literally
# ---------------------------------------------------------------------------------------------
class Eof(Exception):
    pass


class _Stream:
    def __init__(self, data):
        self.data, self.pos, self.phase = data, 0, ""

    def get(self):
        if self.pos >= len(self.data):
            raise Eof(self.phase)
        self.pos += 1
        return self.data[self.pos - 1]


def read_segment(s, bsize, stats=None):
    """KodakDecompressor::decodeSegment (:67-118) -> (differences, lengths)"""
    blen = [0] * bsize
    bitbuf, bits = 0, 0
    s.phase = "nibbles"
    for i in range(0, bsize, 2):
        b = s.get()  # (peekByte and getByte of one byte)
        blen[i], blen[i + 1] = b & 15, b >> 4
    if (bsize & 7) == 4:
        s.phase = "init_unit"
        bitbuf = s.get() << 8
        bitbuf += s.get()
        bits = 16
    out = [0] * bsize
    cum = 0
    for i in range(bsize):
        n = blen[i]
        if bits < n:
            s.phase = "read4"
            for j in range(0, 32, 8):
                bitbuf += s.get() << (bits + (j ^ 8))
            bits += 32
            assert bitbuf < 1 << 64
        diff = (bitbuf & 0xFFFFFFFF) & (0xFFFF >> (16 - n))
        bitbuf >>= n
        bits -= n
        out[i] = extend(diff, n) if n else diff
        if stats is not None and n:
            lo, hi = 0, (1 << n) - 1
            for key, f in (("lo", lo), ("below", hi >> 1), ("above", (hi >> 1) + 1), ("hi", hi)):
                if diff == f:
                    stats["extend_%d_%s" % (n, key)] += 1
            if n == 15 and cum % 16 + n > 16:
                stats["len15_straddles_units"] += 1
                if init_bits(bsize) and cum < 16:
                    stats["len15_straddles_init_edge"] += 1
        cum += n
    return out, blen


def decode(data, w, h, bps, stats=None):
    """KodakDecompressor::decompress (:120-150) without the table -> (status, the values as
    (h, w) int32 or None, bytes consumed)"""
    s = _Stream(data)
    px = np.zeros((h, w), np.int32)
    segs = row_segments(w)
    if stats is not None:
        n_full, tail = w // SEGMENT, w % SEGMENT
        stats["n_full_%d" % n_full] += 1
        stats["tail_only" if n_full == 0 else "no_tail" if tail == 0 else "both"] += 1
        if tail:
            stats["tail_init%d" % init_bits(tail)] += 1
    for row in range(h):
        col = 0
        for k, length in enumerate(segs):
            start = s.pos
            try:
                buf, blen = read_segment(s, length, stats)
            except Eof as e:
                if stats is not None:
                    stats["io_in_" + str(e)] += 1
                return ERR_IO, None, s.pos
            assert s.pos - start == segment_bytes(length, sum(blen)), "the closed form of the size"
            if stats is not None:
                total, init = sum(blen), init_bits(length)
                if total == 0:
                    stats["no_bit_words_init%d" % init] += 1
                elif total - init < 0:
                    stats["over_negative"] += 1
                elif total - init in (0, 32, 33):
                    stats["over_%d" % (total - init)] += 1
            pred = [0, 0]
            for i in range(length):
                pred[i & 1] += buf[i]
                v = pred[i & 1]
                if v < 0 or v >> bps:
                    if stats is not None:
                        where = ("first" if row == 0 and k == 0 else
                                 "last" if row == h - 1 and k == len(segs) - 1 else
                                 "tail" if w % SEGMENT and k == len(segs) - 1 else "other")
                        stats["range_%s_%s" % ("negative" if v < 0 else "high", where)] += 1
                    return ERR_VALUE_RANGE, None, s.pos
                if stats is not None and v == 0 and buf[i]:
                    stats["value_0"] += 1
                if stats is not None and v == (1 << bps) - 1:
                    stats["value_max_%d" % bps] += 1
                px[row, col] = v
                col += 1
    if stats is not None and s.pos == len(data):
        stats["ends_exactly"] += 1
    return OK, px, s.pos


# ---------------------------------------------------------------------------------------------
# Curves and tables (common/TableLookUp.cpp:50-85)
# ---------------------------------------------------------------------------------------------
def curve(kind, bps):
    """'camera': a concave tone curve to 16 bits; 'wild': non-monotonic with large steps, so that
    a decoder that dithered, or read tables[v] in dither mode, decodes differently"""
    n = 1 << bps
    x = np.arange(n, dtype=np.float64) / (n - 1)
    if kind == "camera":
        return np.minimum(65535, np.round(65535 * x ** 0.6)).astype(np.uint16)
    r = np.random.RandomState(1000 + bps)
    c = (np.round(40000 * x) + r.randint(0, 20000, n) * (np.arange(n) % 3 == 0)).astype(np.int64)
    c[n // 2:] = c[n // 2:][::-1]
    return np.clip(c, 0, 65535).astype(np.uint16)


def plain_table(c):
    return np.asarray(c, np.uint16).copy()


def dither_table(c):
    c = np.asarray(c, np.int64)
    lower = np.minimum(np.concatenate([c[:1], c[:-1]]), c)
    upper = np.maximum(np.concatenate([c[1:], c[-1:]]), c)
    t = np.zeros(2 * c.size, np.uint16)
    t[0::2] = np.clip(c - (upper - lower + 2) // 4, 0, 65535)
    t[1::2] = upper - lower
    return t


def table_for(mode, c):
    return None if mode == NONE else plain_table(c) if mode == PLAIN else dither_table(c)


def apply_table(values, mode, c):
    """setWithLookUp with the generator at 0: it stays 0, and (delta * 0 + 1024) >> 12 is 0"""
    if mode == NONE:
        return values.astype(np.uint16)
    t = table_for(mode, c)
    return t[2 * values] if mode == DITHER else t[values]


# ---------------------------------------------------------------------------------------------
# Encoders
# ---------------------------------------------------------------------------------------------
def encode_segment(lens, fields, rng):
    """the bytes of a segment with these lengths and fields; bits no field owns are random"""
    length = len(lens)
    assert length % 4 == 0 and 0 < length <= SEGMENT
    out = bytearray(lens[2 * k] | lens[2 * k + 1] << 4 for k in range(length // 2))
    total = sum(lens)
    n_bits = 8 * (segment_bytes(length, total) - length // 2)
    v = rng.getrandbits(n_bits) >> total << total if n_bits > total else 0
    cum = 0
    for n, f in zip(lens, fields):
        assert 0 <= f < 1 << n
        v |= f << cum
        cum += n
    for u in range(n_bits // 16):
        unit = (v >> (16 * u)) & 0xFFFF
        out += bytes([unit >> 8, unit & 255])
    return bytes(out)


def from_diffs(diffs):
    """-> (lengths, fields) with the shortest length for every difference"""
    lens, fields = [], []
    for d in diffs:
        n = abs(d).bit_length()
        assert n <= 15
        lens.append(n)
        fields.append(d if d >= 0 else d + (1 << n) - 1)
    return lens, fields


def diffs_of(values):
    """the differences of one segment's values"""
    pred, out = [0, 0], []
    for i, v in enumerate(values):
        out.append(int(v) - pred[i & 1])
        pred[i & 1] = int(v)
    return out


def noise_values(length, bps, rng):
    """a segment's values: per parity a walk with steps of every size that stays in range"""
    top = (1 << bps) - 1
    cur, out = [0, 0], []
    for i in range(length):
        kind = rng.random()
        if kind < 0.2:
            step = 0
        elif kind < 0.6:
            step = rng.randint(-3, 3)
        else:
            step = rng.randint(-(1 << rng.randint(2, bps)), 1 << rng.randint(2, bps))
        cur[i & 1] = min(top, max(0, cur[i & 1] + step))
        out.append(cur[i & 1])
    return out


# ---------------------------------------------------------------------------------------------
# The cases.  A case is (name, w, h, bps, curve kind, generator, cut, gap): the generator yields
# per segment in decode order (lengths, fields); cut(offsets, size) is the in_bytes of a truncated
# stream (offsets: where each segment starts, and the end); gap: trailing bytes in the file.
# ---------------------------------------------------------------------------------------------
def _gen_noise(w, h, bps, rng, edit=None):
    k = 0
    for row in range(h):
        for length in row_segments(w):
            values = noise_values(length, bps, rng)
            if edit:
                edit(k, values)
            yield from_diffs(diffs_of(values))
            k += 1


def _planted(w, h, plan):
    """plan: {segment index: (lengths, fields)}; every other segment is all zeros"""
    def gen(bps, rng):
        k = 0
        for row in range(h):
            for length in row_segments(w):
                yield plan.get(k, ([0] * length, [0] * length))
                k += 1
    return gen


def _pad(lens, fields, length):
    return lens + [0] * (length - len(lens)), fields + [0] * (length - len(fields))


def _extend_walk(ns):
    """on both parities, for every n: +max, -max, +2^(n-1), -2^(n-1): the four ends of extend,
    the value at 0 and at 2^n - 1"""
    d = []
    for n in ns:
        for step in ((1 << n) - 1, -((1 << n) - 1), 1 << (n - 1), -(1 << (n - 1))):
            d += [step, step]
    return d


def _case_list():
    cases = []

    def add(name, w, h, bps, gen, curve_kind="camera", cut=None, gap=0):
        cases.append(dict(name=name, width=w, height=h, bps=bps, curve=curve_kind, gen=gen,
                          cut=cut, gap=gap))

    def noise(edit=None):
        return lambda w, h: (lambda bps, rng: _gen_noise(w, h, bps, rng, edit))

    # geometry: every width class at every height, depths, curves and trailing bytes alternating
    k = 0
    for w in (4, 12, 252, 256, 260, 264, 516):
        for h in (1, 2, 65, 130):
            add("g_%dx%d" % (w, h), w, h, (10, 12)[k % 2], noise()(w, h),
                ("camera", "wild")[(k // 2) % 2], gap=(0, 37)[(k // 3) % 2])
            k += 1
    add("g_4516x3", 4516, 3, 12, noise()(4516, 3), "wild", gap=5)
    add("g_4516x2_10", 4516, 2, 10, noise()(4516, 2), "camera")
    add("g_264x300_long", 264, 300, 12, noise()(264, 300), "camera", gap=64)

    # segments without bit words, and the sums around a read of 4 bytes
    add("z_8x2", 8, 2, 12, _planted(8, 2, {}))      # init 0
    add("z_4x3", 4, 3, 10, _planted(4, 3, {}))      # init 16
    add("z_12x2", 12, 2, 12, _planted(12, 2, {}))   # init 16
    add("z_256x2", 256, 2, 12, _planted(256, 2, {}))
    add("z_516x2", 516, 2, 10, _planted(516, 2, {}))

    def sums(length, lens):
        l, f = _pad(list(lens), [(1 << n) - 1 if i < 2 else ((1 << n) >> 1) for i, n in
                                 enumerate(lens)], length)
        # +max on each parity, then fields with only the top bit: +2^(n-1)
        return l, f
    # (values: 1 + 1 + ... stay far below 2^10)
    add("s_8_sum32", 8, 2, 10, _planted(8, 2, {0: sums(8, [4] * 8), 1: sums(8, [4] * 8)}))
    add("s_8_sum33", 8, 2, 10, _planted(8, 2, {1: sums(8, [5, 4, 4, 4, 4, 4, 4, 4])}))
    add("s_12_sum16", 12, 2, 12, _planted(12, 2, {0: sums(12, [4, 4, 4, 4]), 1: sums(12, [8, 8])}))
    add("s_12_sum48", 12, 2, 12, _planted(12, 2, {1: sums(12, [4] * 12)}))
    add("s_12_sum49", 12, 2, 12, _planted(12, 2, {0: sums(12, [5] + [4] * 11)}))
    add("s_12_sum5", 12, 2, 10, _planted(12, 2, {0: sums(12, [2, 3]), 1: sums(12, [7, 8])}))
    add("s_260_sum15", 260, 2, 12, _planted(260, 2, {1: sums(4, [1] * 4), 3: sums(4, [7, 8])}))

    # extend at its four ends for every length whose values fit, the values 0 and 2^bps - 1
    add("e_256_12", 256, 1, 12, _planted(256, 1, {0: _pad(*from_diffs(_extend_walk(range(1, 13))),
                                                          256)}), "wild")
    add("e_252_10", 252, 2, 10, _planted(252, 2, {1: _pad(*from_diffs(_extend_walk(range(1, 11))),
                                                          252)}), "wild")
    # ... and for the lengths whose values cannot fit: the verdict is all there is to see
    for n in (13, 14, 15):
        hi = (1 << n) - 1
        for key, f in (("lo", 0), ("below", hi >> 1), ("above", (hi >> 1) + 1), ("hi", hi)):
            add("e_len%d_%s" % (n, key), 12, 2, 12,
                _planted(12, 2, {1: _pad([3, 0, n], [5, 0, f], 12)}))
    # length-15 fields across two units and across the up-front unit's edge
    add("e_straddle_8", 8, 2, 12, _planted(8, 2, {0: _pad([9, 15, 7, 15], [300, 0x5A5A, 99, 0x2BCD],
                                                          8)}))
    add("e_straddle_12", 12, 2, 12, _planted(12, 2, {0: _pad([10, 15, 15], [700, 0x4321, 0x7FFF],
                                                             12)}))

    # the range check at its edges, in the first, a tail and the last segment
    def poke(seg, at, value):
        def edit(k, values):
            if k == seg:
                values[at] = value
        return edit
    for key, v10, v12 in (("high", 1 << 10, 1 << 12), ("negative", -1, -1)):
        add("v_first_%s" % key, 516, 2, 12, noise(poke(0, 7, v12))(516, 2))
        add("v_tail_%s" % key, 516, 3, 10, noise(poke(5, 2, v10))(516, 3))
        add("v_last_%s" % key, 516, 2, 12, noise(poke(5, 3, v12))(516, 2))
    add("v_edges_pass", 260, 2, 12, noise(lambda k, v: v.__setitem__(slice(0, 4), [4095, 0, 0, 4095]))
        (260, 2), "wild")
    add("v_edges_pass_10", 12, 3, 10, noise(lambda k, v: v.__setitem__(slice(0, 4), [0, 1023, 1023, 0]))
        (12, 3), "wild")

    # truncations: seg = index of the segment the cut falls into
    def cut_at(seg, where):
        def cut(offsets, lens_of):
            start, length = offsets[seg], lens_of[seg]
            if where == "nibbles":
                return start + length // 2 - 1
            if where == "init_unit":
                assert init_bits(length)
                return start + length // 2 + 1
            if where == "read4":
                assert offsets[seg + 1] - start > length // 2 + init_bits(length) // 8
                return offsets[seg + 1] - 3
            if where == "last_byte":
                return offsets[seg + 1] - 1
            return offsets[seg + 1] + where  # (a number: bytes behind the segment)
        return cut
    add("t_nibbles", 260, 4, 12, noise()(260, 4), cut=cut_at(6, "nibbles"))
    add("t_init_unit", 260, 4, 12, noise()(260, 4), cut=cut_at(7, "init_unit"))
    add("t_read4", 260, 4, 12, noise()(260, 4), cut=cut_at(6, "read4"))
    add("t_read4_full", 516, 3, 10, noise()(516, 3), cut=cut_at(7, "read4"))
    add("t_last_byte", 264, 3, 12, noise()(264, 3), cut=cut_at(5, "last_byte"))
    add("t_exact", 264, 3, 12, noise()(264, 3), cut=cut_at(5, 0))
    add("t_exact_trailing", 264, 3, 12, noise()(264, 3), cut=cut_at(5, 0), gap=91)
    add("t_one_more", 264, 3, 12, noise()(264, 3), cut=cut_at(5, 1), gap=1)
    add("t_12_init_unit", 12, 9, 10, noise()(12, 9), cut=cut_at(8, "init_unit"))
    add("t_below_half", 4, 1, 12, _planted(4, 1, {}), cut=lambda offsets, lens_of: 1)
    add("t_below_half_516", 516, 2, 12, _planted(516, 2, {}), cut=lambda offsets, lens_of: 515)
    # which failure is first: the range in an earlier segment than the cut, the reverse, and both
    # in one segment (the read comes first)
    add("o_range_then_cut", 260, 4, 12, noise(poke(2, 9, 4096))(260, 4), cut=cut_at(6, "read4"))
    add("o_cut_then_range", 260, 4, 12, noise(poke(7, 1, -1))(260, 4), cut=cut_at(5, "nibbles"))
    add("o_same_segment", 260, 4, 12, noise(poke(6, 9, 4096))(260, 4), cut=cut_at(6, "read4"))
    add("o_range_row0_range_row1", 516, 2, 10, noise(lambda k, v: v.__setitem__(0, -1) if k in (1, 4)
                                                     else None)(516, 2))
    return cases


@functools.lru_cache(maxsize=None)
def case_list():
    return tuple(_case_list())


def case(name):
    return next(c for c in case_list() if c["name"] == name)


def names():
    return [c["name"] for c in case_list()]


@functools.lru_cache(maxsize=None)
def build_case(name):
    """-> dict(data: the stream as the decompressor gets it, whole: the stream without the cut,
    offsets: the segments' starts and the end, curve)"""
    c = case(name)
    rng = random.Random("kodak:" + name)
    parts, offsets, lens_of, pos = [], [], [], 0
    for lens, fields in c["gen"](c["bps"], rng):
        b = encode_segment(lens, fields, rng)
        offsets.append(pos)
        lens_of.append(len(lens))
        parts.append(b)
        pos += len(b)
    offsets.append(pos)
    whole = b"".join(parts)
    trailing = bytes(rng.getrandbits(8) for _ in range(c["gap"]))
    data = whole + trailing
    if c["cut"]:
        n = c["cut"](offsets, lens_of)
        data = data[:n] if n <= len(whole) else whole + trailing[:n - len(whole)]
        if c["gap"] and n == len(whole):
            data = whole + trailing
    return dict(data=data, whole=whole, offsets=offsets, curve=curve(c["curve"], c["bps"]))


@functools.lru_cache(maxsize=None)
def model_values(name):
    """-> (status, values or None, consumed): validate, then the model's decode"""
    c = case(name)
    data = build_case(name)["data"]
    st = validate(c["width"], c["height"], c["bps"], len(data))
    if st != OK:
        return st, None, 0
    return decode(data, c["width"], c["height"], c["bps"])


def expected(name, mode):
    """-> (status, pixels as (h, w) uint16 or None) under table mode `mode`"""
    st, v, _ = model_values(name)
    if st != OK:
        return st, None
    return st, apply_table(v, mode, build_case(name)["curve"])


def reach():
    """the reach statistics over the whole case list"""
    import collections
    stats = collections.Counter()
    for c in case_list():
        data = build_case(c["name"])["data"]
        if validate(c["width"], c["height"], c["bps"], len(data)) == OK:
            decode(data, c["width"], c["height"], c["bps"], stats)
    return stats


def sha_rows(px):
    return hashlib.sha256(np.ascontiguousarray(px, dtype="<u2").tobytes()).hexdigest()


def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


# ---------------------------------------------------------------------------------------------
# Whole files (DcrDecoder::decodeRawInternal, decoders/DcrDecoder.cpp:58-120)
# ---------------------------------------------------------------------------------------------
def dcr_file(width, height, data, curve_values):
    """make "Kodak", compression 65000, one strip that is the LAST thing in the file -- the
    decompressor gets the rest of the file from the strip's offset --, and KODAK_IFD pointing at a
    second IFD that carries KODAK_LINEARIZATION (1024 SHORTs: 10 bits, 4096: 12)."""
    def build(kodak_at):
        raw = rawfiles.Ifd()
        raw.add(rawfiles.IMAGEWIDTH, rawfiles.LONG, width)
        raw.add(rawfiles.IMAGELENGTH, rawfiles.LONG, height)
        raw.add(rawfiles.COMPRESSION, rawfiles.LONG, 65000)
        raw.add_blobs(rawfiles.STRIPOFFSETS, rawfiles.STRIPBYTECOUNTS, [data])
        kodak = rawfiles.Ifd()
        kodak.add(KODAK_LINEARIZATION, rawfiles.SHORT, [int(x) for x in curve_values])
        root = rawfiles.Ifd()
        root.add(rawfiles.MAKE, rawfiles.ASCII, "Kodak").add(rawfiles.MODEL, rawfiles.ASCII, "RSX")
        root.add(KODAK_IFD, rawfiles.LONG, kodak_at)
        root.add_sub(raw)
        root.next = kodak
        return rawfiles.tiff_file(root), len(root.entries) + 1  # (+ SUBIFDS)
    blob, n = build(0)
    # the root IFD's "next IFD" pointer is where the Kodak IFD went
    kodak_at = int(np.frombuffer(blob[8 + 2 + 12 * n:8 + 2 + 12 * n + 4].tobytes(), "<u4")[0])
    return build(kodak_at)[0]


def case_file(name):
    c, b = case(name), build_case(name)
    return dcr_file(c["width"], c["height"], np.frombuffer(b["data"], np.uint8), b["curve"])


# ---------------------------------------------------------------------------------------------
# The host build (rawspeed_amd/librsx_kodak_host.so)
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_lib():
    from rawspeed_amd import build
    L = C.CDLL(build.LIB_KODAK_HOST)
    L.rsx_kodak_host_validate.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.rsx_kodak_host_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.rsx_kodak_host_segment_bytes.argtypes = [C.c_uint32, C.c_uint32]
    L.rsx_kodak_host_segment_bytes.restype = C.c_uint32
    L.rsx_kodak_host_image_bound.argtypes = [C.c_int32, C.c_int32]
    L.rsx_kodak_host_image_bound.restype = C.c_uint64
    return L


def host_decode(data, w, h, bps, mode, table, pitch=None, cpp=1):
    """-> (status, pixels or None, the whole image buffer, consumed)"""
    from rawspeed_amd import abi
    pitch = 2 * max(w, 0) if pitch is None else pitch
    buf = np.full(max(1, pitch * max(h, 0)), 0xA5, np.uint8)
    img = abi.Image(buf.ctypes.data, pitch, w, h, cpp, 1)
    d, keep = abi.kodak_desc(bps, mode, table)
    a = np.frombuffer(bytes(data) + b"\0", np.uint8)
    consumed = C.c_uint64(0)
    st = host_lib().rsx_kodak_host_decode(C.byref(d), a.ctypes.data, len(data), C.byref(img),
                                          C.byref(consumed))
    px = None
    if st == OK:
        px = np.stack([buf[r * pitch:r * pitch + 2 * w].view(np.uint16) for r in range(h)])
    return st, px, buf, consumed.value
