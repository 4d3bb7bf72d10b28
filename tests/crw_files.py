"""Canon CRW (CrwDecompressor, include/rsx.h section 3x): a pure-Python model, two encoders, a
CIFF whole-file builder and the case list the CRW tests share.  Not a test.

The model is a literal transcription of the reference's reader (BitStreamerJPEG: the cache,
fill(32) in front of every symbol, FF 00 un-stuffing, the marker, the overflow read of
BitStreamerForwardSequentialReplenisher) and of CrwDecompressor::decodeBlock / decompress, with
counters of what a decode reached.  The device, the host build and the closed forms of
rsx_crw_core.h are held against it, and it is held against what the unmodified reference
answered (tests/golden/crw_ref.json, scripts/record_crw_ref.py).

Which cases rest on what: the reference's front door (CrwDecoder) has no camera hints here, so it
always decodes WITH low bits and the golden file holds that route for every case.  The route
without low bits is held against the model, and against this identity: for width != 2672 and
all-zero low bits the recorded image is the image without low bits << 2 (the cases whose `low`
is all zero; test_crw_model.py checks it on them).
"""
import functools
import hashlib
import json
import os
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "crw_ref.json")

OK, ERR_INVALID_ARG, ERR_IO, ERR_BAD_CODE, ERR_OVERFLOW, ERR_VALUE_RANGE = 0, 1, 2, 3, 5, 10

# the shipped segment and window of rsx_crw.hip (test_crw_build.py holds them against the macros)
SEG_BITS, WIN_SEGS = 1024, 256
WIN_BITS = SEG_BITS * WIN_SEGS

FIRST_NCPL = [
    [0, 1, 4, 2, 3, 1, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    [0, 2, 2, 3, 1, 1, 1, 1, 2, 0, 0, 0, 0, 0, 0, 0],
    [0, 0, 6, 3, 1, 1, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0],
]
FIRST_VALUES = [
    bytes.fromhex("040305060207010809000a0bff"),
    bytes.fromhex("030204010500060709080a0bff"),
    bytes.fromhex("0605070408030902000a010bff"),
]
SECOND_NCPL = [
    [0, 2, 2, 2, 1, 4, 2, 1, 2, 5, 1, 1, 0, 0, 0, 139],
    [0, 2, 2, 1, 4, 1, 4, 1, 3, 3, 1, 0, 0, 0, 0, 140],
    [0, 0, 6, 2, 1, 3, 3, 2, 5, 1, 2, 2, 8, 10, 0, 117],
]
SECOND_VALUES = [
    bytes.fromhex(
        "0304020501060708121311140915220021160af02317243132181933254134423551363738297926"
        "1a3956572827525558437659775461f9717875969749b753d774b698474895699991fab868b5b9d6"
        "f7d86746459489f881d5f6b488b12a4472d98766d4f53aa773a9a88662c765c8c9a1f4d1e95a9285"
        "a6e793e8c1c67a64e14a6ae6b3f1d3a58ab29aba84a463e5c5f3d2c482aadae4f2ca83a3a2c3eac2"
        "e2e3ffff"
    ),
    bytes.fromhex(
        "02030104051211061307081422092100231531320a16f02433414219172518513443522935613971"
        "62365326381a37812791795545287259a1b144695458d1fa57e1f1b94947636af95646a82a4a7899"
        "3a75748665c176b696d68985c9f595b4c7f78a97b873b7d8d987a77a488284eaf4a6c55a94a4c692"
        "c368b5c8e4e5e6e9a2a3e3c2666793aad4d5e7f8889ad777c464e298a5cadae8f3f6a9b2b3f2d283"
        "bad3ffff"
    ),
    bytes.fromhex(
        "04050306020701080912131411150a1617f000222118231924323125333837343536397957585928"
        "567827412977264276991a559897f94854968947b749fa7568b66769b9b8d852d788b5745146d9f8"
        "3ad687457a95d5f686b4a994532aa843f5f7d466a75a448ac9e8c8e79a6a734a61c7f4c665e972e6"
        "719193a6da928562f3c5b2a484ba64a5b3d281e5d3aac4caf2b1e4d18363eac3e282f1a3c2a1c1e3"
        "a2e1ffff"
    ),
]
assert all(len(v) == 13 for v in FIRST_VALUES) and all(len(v) == 164 for v in SECOND_VALUES)


class CrwError(Exception):
    def __init__(self, status, text):
        Exception.__init__(self, text)
        self.status = status


@functools.lru_cache(maxsize=None)
def code_book(table, tree):
    """({(length, code): value} as the decoder sees it, {value: (length, code)} of the FIRST code
    with that value, as an encoder uses it)"""
    ncpl = (SECOND_NCPL if tree else FIRST_NCPL)[table]
    values = (SECOND_VALUES if tree else FIRST_VALUES)[table]
    dec, enc, code, at = {}, {}, 0, 0
    for length in range(1, 17):
        for _ in range(ncpl[length - 1]):
            dec[(length, code)] = values[at]
            enc.setdefault(values[at], (length, code))
            code += 1
            at += 1
        code <<= 1
    return dec, enc


def extend(field, n):
    return field if field & (1 << (n - 1)) else field - ((1 << n) - 1)


# ---------------------------------------------------------------------------------------------
# The model
# ---------------------------------------------------------------------------------------------
class Reader:
    """BitStreamerJPEG over BitStreamerForwardSequentialReplenisher: `cache` holds `level` bits,
    the oldest on top; `pos` is the replenisher's position"""

    def __init__(self, data, reach):
        if len(data) < 8:
            raise CrwError(ERR_IO, "Bit stream size is smaller than MaxProcessBytes")
        self.d, self.size, self.pos, self.cache, self.level = bytes(data), len(data), 0, 0, 0
        self.reach = reach

    def push(self, v, n):
        self.cache = (self.cache << n) | v
        self.level += n

    def fill32(self):
        if self.level >= 32:
            return
        if self.pos + 8 <= self.size:
            tmp = self.d[self.pos:self.pos + 8]
        else:
            if self.pos > self.size + 16:
                self.reach["overflow"] += 1
                raise CrwError(ERR_OVERFLOW, "Buffer overflow read in BitStreamer")
            tmp = self.d[self.pos:self.pos + 8]
            tmp = tmp + bytes(8 - len(tmp))
            self.reach["zero_padded_fill"] += 1
        if 0xFF not in tmp[:4]:
            self.push(int.from_bytes(tmp[:4], "big"), 32)
            self.pos += 4
            return
        p = 0
        for i in range(4):
            c0 = tmp[p]
            self.push(c0, 8)
            if c0 != 0xFF:
                p += 1
                continue
            if tmp[p + 1] == 0:
                self.reach["stuffed"] += 1
                self.reach["stuffed_at%d" % i] += 1
                p += 2
                continue
            # FF xx: the end of the stream; un-push the FF, zeros up to 64 bits
            self.reach["marker"] += 1
            self.reach["marker_at%d" % i] += 1
            self.level -= 8
            self.cache >>= 8
            self.cache <<= 64 - self.level
            self.level = 64
            p = (self.size - self.pos) + (4 - i)
            break
        self.pos += p

    def peek(self, n):
        return (self.cache >> (self.level - n)) & ((1 << n) - 1)

    def skip(self, n):
        self.level -= n
        self.cache &= (1 << self.level) - 1

    def get(self, n):
        v = self.peek(n)
        self.skip(n)
        return v


REACH_KEYS = ("eob", "ff", "f0", "zero_at_0", "eob_at_63", "full_block", "pass63_len0",
              "pass63_bits", "code16", "stuffed", "marker", "overflow", "zero_padded_fill",
              "bad_code", "range", "row_mid_block", "plus2", "no_plus2", "low_bits")


def new_reach():
    r = dict.fromkeys(REACH_KEYS, 0)
    r["max_carry"] = 0
    for i in range(4):  # where in a fill's four data bytes
        r["stuffed_at%d" % i] = r["marker_at%d" % i] = 0
    for tree in (0, 1):
        for n in range(1, 12 - tree):
            for end in ((0, 3) if n == 1 else range(4)):  # field 0, 2^(n-1) - 1, 2^(n-1), 2^n - 1
                r["len%d_%d_end%d" % (tree, n, end)] = 0
    return r


@functools.lru_cache(maxsize=None)
def code_lut(table, tree):
    """[the next 16 bits] -> (length, value), or None where no code is a prefix of them"""
    lut = [None] * 65536
    for (length, code), v in code_book(table, tree)[0].items():
        lo = code << (16 - length)
        lut[lo:lo + (1 << (16 - length))] = [(length, v)] * (1 << (16 - length))
    return lut


def decode_code(bs, table, tree, reach):
    hit = code_lut(table, tree)[bs.peek(16)]
    if hit is None:
        reach["bad_code"] += 1
        raise CrwError(ERR_BAD_CODE, "bad Huffman code")
    bs.skip(hit[0])
    if hit[0] == 16:
        reach["code16"] += 1
    return hit[1]


def decode_block(bs, table, reach):
    diff = [0] * 64
    i = 0
    while i < 64:
        bs.fill32()
        cv = decode_code(bs, table, 1 if i > 0 else 0, reach)
        n, index = cv & 15, cv >> 4
        if n == 0 and index == 0 and i:
            reach["eob"] += 1
            if i == 63:
                reach["eob_at_63"] += 1
            break
        if n == 15 and index == 15:
            reach["ff"] += 1
            i += 1
            if i == 64:
                reach["full_block"] += 1
            continue
        i += index
        if n == 0:
            if index == 15:
                reach["f0"] += 1
            if index == 0:
                reach["zero_at_0"] += 1
            i += 1
            if i > 64:
                reach["pass63_len0"] += 1
            if i == 64:
                reach["full_block"] += 1
            continue
        field = bs.get(n)
        if i >= 64:
            reach["pass63_bits"] += 1
            break
        lo, hi = 1 << (n - 1), (1 << n) - 1
        end = {0: 0, lo - 1: 1, lo: 2, hi: 3}.get(field)
        if n == 1:
            end = 0 if field == 0 else 3
        if end is not None:
            reach["len%d_%d_end%d" % (1 if i > 0 else 0, n, end)] += 1
        diff[i] = extend(field, n)
        i += 1
        if i == 64:
            reach["full_block"] += 1
    return diff


def validate(width, height, table, has_low, low_bytes, in_bytes, cpp=1, pitch=None):
    """rsx_crw_validate's answer, in the reference's order"""
    if cpp != 1:
        return ERR_INVALID_ARG
    if (width <= 0 or height <= 0 or width % 4 != 0 or width > 4104 or height > 3048 or
            (width * height) % 64 != 0):
        return ERR_INVALID_ARG
    if table > 2:
        return ERR_INVALID_ARG
    if has_low and low_bytes < width * height // 4:
        return ERR_INVALID_ARG
    if pitch is not None and pitch < 2 * width:
        return ERR_INVALID_ARG
    if in_bytes < 8:
        return ERR_IO
    return OK


def decode(width, height, table, data, low=None, reach=None):
    """-> (status, (height, width) uint16 or None): CrwDecompressor's constructor and decompress()"""
    reach = new_reach() if reach is None else reach
    st = validate(width, height, table, low is not None, len(low) if low is not None else 0, 8)
    if st != OK:
        return st, None
    out = np.zeros(width * height, np.uint16)
    try:
        bs = Reader(data, reach)
        carry, base, row, col, p = 0, [512, 512], 0, 0, 0
        for _ in range(width * height // 64):
            diff = decode_block(bs, table, reach)
            diff[0] += carry
            # (a pixel in range bounds |carry| below 2048 and a step adds less than 2048: the
            # int16 of the reference cannot wrap before the range check fires)
            assert -32768 <= diff[0] <= 32767
            carry = diff[0]
            reach["max_carry"] = max(reach["max_carry"], abs(carry))
            for k in range(64):
                if col == width:
                    col, row = 0, row + 1
                    base = [512, 512]
                    if k:
                        reach["row_mid_block"] += 1
                base[k & 1] += diff[k]
                if not 0 <= base[k & 1] <= 1023:
                    reach["range"] += 1
                    raise CrwError(ERR_VALUE_RANGE, "Error decompressing")
                out[p] = base[k & 1]
                p += 1
                col += 1
    except CrwError as e:
        return e.status, None
    px = out.reshape(height, width)
    if low is not None:
        lb = np.frombuffer(bytes(low[:width * height // 4]), np.uint8).astype(np.uint16)
        two = np.stack([(lb >> (2 * k)) & 3 for k in range(4)], axis=1).reshape(height, width)
        px = (px << 2) | two
        reach["low_bits"] += 1
        if width == 2672:
            reach["plus2"] += int((px < 512).sum())
            reach["no_plus2"] += int((px >= 512).sum())
            px = np.where(px < 512, px + 2, px).astype(np.uint16)
    return OK, px


# ---------------------------------------------------------------------------------------------
# The segment speculation of rsx_crw.hip as a model: states at segment edges over the un-stuffed
# scan, windows settled from guessed heads, R rounds over the windows, then an in-order walk.
# ---------------------------------------------------------------------------------------------
DEAD = -1


def unstuff(data):
    """(the data bytes in front of the first marker, marker found)"""
    out = bytearray()
    for j, b in enumerate(data):
        if b == 0xFF and j + 1 < len(data) and data[j + 1] != 0:
            return bytes(out), True
        if b == 0 and j > 0 and data[j - 1] == 0xFF:
            continue
        out.append(b)
    return bytes(out), False


class Bits:
    def __init__(self, data, pad=64):
        self.d = bytes(data) + bytes(pad + 8)

    def peek32(self, c):
        b = c >> 3
        return (int.from_bytes(self.d[b:b + 5], "big") >> (8 - (c & 7))) & 0xFFFFFFFF


def symbol(table, w, i):
    """rsx_crw_core.h's symbol(): (used, next, at, diff); used 0: a bad code"""
    hit = code_lut(table, 1 if i > 0 else 0)[w >> 16]
    if hit is None:
        return 0, 0, -1, 0
    length, cv = hit
    n = cv & 15
    if cv == 0 and i > 0:
        return length, 0, -1, 0
    used, at, diff = length, -1, 0
    if cv == 0xFF:
        i += 1
    else:
        i += cv >> 4
        if n:
            field = (w >> (32 - length - n)) & ((1 << n) - 1)
            used += n
            if i < 64:
                at, diff = i, extend(field, n)
        i += 1
    return used, (0 if i >= 64 else i), at, diff


def parse_segment(bits, table, s, entry, seg_bits):
    """the state at the next segment's edge: symbol() without its differences, inlined for speed
    (test_crw_model.py holds the two against each other)"""
    if entry == DEAD:
        return DEAD
    d, luts = bits.d, (code_lut(table, 0), code_lut(table, 1))
    end = (s + 1) * seg_bits
    c, i = s * seg_bits + entry[0], entry[1]
    while c < end:
        b = c >> 3
        hit = luts[i > 0][(int.from_bytes(d[b:b + 3], "big") >> (8 - (c & 7))) & 0xFFFF]
        if hit is None:
            return DEAD
        used, cv = hit
        if cv == 0 and i:
            i = 0
        else:
            if cv == 0xFF:
                i += 1
            else:
                i += (cv >> 4) + 1
                used += cv & 15
            if i >= 64:
                i = 0
        c += used
    return (c - end, i)


def parse_segment_by_symbols(bits, table, s, entry, seg_bits):
    """parse_segment through symbol(), one call a symbol"""
    if entry == DEAD:
        return DEAD
    c, i = s * seg_bits + entry[0], entry[1]
    while c < (s + 1) * seg_bits:
        used, i, _, _ = symbol(table, bits.peek32(c), i)
        if used == 0:
            return DEAD
        c += used
    return (c - (s + 1) * seg_bits, i)


def serial_entries(bits, table, n_segs, seg_bits):
    out, e = [], (0, 0)
    for s in range(n_segs):
        out.append(e)
        e = parse_segment(bits, table, s, e, seg_bits)
    return out


def speculate(bits, table, n_segs, seg_bits, win_segs, rounds):
    """-> (entries, stats): entries[s] after round 0, `rounds` rounds over the windows and the
    settling walk; stats = (windows, inner rounds, outer rounds used, settling work)"""
    n_wins = (n_segs + win_segs - 1) // win_segs
    entries = [None] * n_segs
    exits, heads = [None] * n_wins, [None] * n_wins
    inner = [0]

    def settle(W, head, first):
        lo, hi = W * win_segs, min((W + 1) * win_segs, n_segs)
        ent = [(0, 1)] * (hi - lo) if first else entries[lo:hi]
        changed = [first] * (hi - lo)
        changed[0] = first or ent[0] != head
        ent[0] = head
        ex = DEAD if first else exits[W]
        n = 0
        while True:
            nxt = [False] * (hi - lo + 1)
            new = {}
            for t in range(hi - lo):
                if changed[t]:
                    new[t] = parse_segment(bits, table, lo + t, ent[t], seg_bits)
            for t, e in new.items():
                if t + 1 < hi - lo:
                    nxt[t + 1] = e != ent[t + 1]
                    ent[t + 1] = e
                else:
                    ex = e
            n += 1
            changed = nxt[:hi - lo]
            if not any(changed):
                break
        inner[0] = max(inner[0], n)
        entries[lo:hi] = ent
        return ex

    for W in range(n_wins):
        heads[W] = (0, 0) if W == 0 else (0, 1)
        exits[W] = settle(W, heads[W], True)
    outer = 0
    for r in range(1, rounds + 1):
        prev = list(exits)
        for W in range(1, n_wins):
            if prev[W - 1] != heads[W]:
                heads[W] = prev[W - 1]
                exits[W] = settle(W, heads[W], False)
                outer = r
    work = 0
    for W in range(1, n_wins):
        if exits[W - 1] != heads[W]:
            heads[W] = exits[W - 1]
            exits[W] = settle(W, heads[W], False)
            work = 1
    return entries, (n_wins, inner[0], outer, work)


# ---------------------------------------------------------------------------------------------
# Encoders
# ---------------------------------------------------------------------------------------------
class BitWriter:
    def __init__(self):
        self.out = bytearray()
        self.acc = self.held = self.n = 0

    def put(self, v, n):
        self.acc = (self.acc << n) | (v & ((1 << n) - 1))
        self.held += n
        self.n += n
        while self.held >= 8:
            self.held -= 8
            self.out.append(self.acc >> self.held)
            self.acc &= (1 << self.held) - 1

    def data(self):
        """the un-stuffed bytes, the last one padded with zeros"""
        tail = bytes([self.acc << (8 - self.held)]) if self.held else b""
        return bytes(self.out) + tail


def stuff(data):
    return bytes(data).replace(b"\xff", b"\xff\x00")


def put_symbol(bw, table, tree, cv, field=None):
    length, code = code_book(table, tree)[1][cv]
    bw.put(code, length)
    if cv != 0xFF and (cv & 15) and field is not None:
        bw.put(field, cv & 15)


def field_of(d):
    n = abs(d).bit_length()
    return n, (d if d > 0 else d + (1 << n) - 1)


def put_block(bw, table, diff):
    """64 differences as symbols: the shortest length, f0 for runs of 16, 00 behind the last
    coefficient that is not zero"""
    n, f = field_of(diff[0])
    put_symbol(bw, table, 0, n, f)
    last = max([k for k in range(1, 64) if diff[k]] or [0])
    i = 1
    while i <= last:
        run = 0
        while diff[i + run] == 0:
            run += 1
        while run >= 16:
            put_symbol(bw, table, 1, 0xF0)
            run -= 16
            i += 16
        n, f = field_of(diff[i + run])
        put_symbol(bw, table, 1, run << 4 | n, f)
        i += run + 1
    if i < 64:
        put_symbol(bw, table, 1, 0x00)


def image_diffs(px):
    """(blocks, 64) coded differences whose decode is the (h, w) image `px` (values 0..1023)"""
    h, w = px.shape
    v = px.astype(np.int64)
    d = v.copy()
    d[:, 2:] -= v[:, :-2]
    d[:, :2] -= 512
    d = d.reshape(-1, 64)
    first = d[:, 0].copy()
    d[1:, 0] = first[1:] - first[:-1]  # (coefficient 0 carries a running sum)
    return d


def encode_image(px, table):
    bw = BitWriter()
    for diff in image_diffs(np.asarray(px)):
        put_block(bw, table, [int(x) for x in diff])
    return stuff(bw.data())


def encode_plant(table, blocks):
    """blocks: lists of (tree, code value, field or None) or ("bits", value, n) -> BitWriter"""
    bw = BitWriter()
    for block in blocks:
        for sym in block:
            if sym[0] == "bits":
                bw.put(sym[1], sym[2])
            else:
                put_symbol(bw, table, *sym)
    return bw


# ---------------------------------------------------------------------------------------------
# CIFF files
# ---------------------------------------------------------------------------------------------
def ciff_dir(entries):
    """entries: (tag | type, bytes) -> a directory: the values, the count, 10 bytes an entry, and
    the offset of the count in the last four bytes"""
    values, table = b"", b""
    for tagtype, blob in entries:
        table += struct.pack("<HII", tagtype, len(blob), len(values))
        values += blob + bytes(-len(blob) % 2)
    return values + struct.pack("<H", len(entries)) + table + struct.pack("<I", len(values))


def crw_file(width, height, table, data, low):
    """the CIFF file CrwDecoder takes: RAWDATA is low bits || 514 bytes || scan"""
    sensor = struct.pack("<6H", 0, width, height, 0, 0, 0)
    props = ciff_dir([(0x1031, sensor), (0x1835, struct.pack("<2I", table, 0)),
                      (0x080A, b"Canon\0Canon EOS 10D\0")])
    chunk = bytes(low) + bytes(514) + bytes(data)
    root = ciff_dir([(0x2005, chunk), (0x300A, props)])
    return b"II" + struct.pack("<I", 14) + b"HEAPCCDR" + root




# ---------------------------------------------------------------------------------------------
# Cases
# ---------------------------------------------------------------------------------------------
def noise_image(w, h, seed, sigma, nonzero=False):
    """a ramp with Gaussian noise; nonzero: no coded difference is 0 (no 00 anywhere in the scan)"""
    rng = np.random.RandomState(seed)
    ramp = 200 + 600 * np.arange(w)[None, :] / max(w - 1, 1) + 20 * np.arange(h)[:, None] / h
    px = np.clip(np.rint(ramp + rng.normal(0, sigma, (h, w))), 2, 1021).astype(np.int64)
    if nonzero:
        for _ in range(200):
            d = image_diffs(px)
            bad = (d == 0).reshape(h, w)
            if not bad.any():
                break
            px = px + np.where(bad, np.where(px > 512, -1, 1), 0)
        assert not (image_diffs(px) == 0).any()
    return px.astype(np.uint16)


def low_for(w, h, seed):
    return np.random.RandomState(seed).randint(0, 256, w * h // 4).astype(np.uint8).tobytes()


def flat_block(c0=0x00, c0_field=None):
    """a block of zeros: coefficient 0's symbol, then 00"""
    return [(0, c0, c0_field), (1, 0x00, None)]


def c0_block(delta):
    """a block of zeros whose coefficient 0 adds `delta` to the carry"""
    return flat_block(*field_of(delta)) if delta else flat_block()


def value_block(k, delta, more=()):
    """a block of zeros but for coefficient k > 0 (and what `more` appends in front of the 00)"""
    n, f = field_of(delta)
    syms, i = [(0, 0x00, None)], 1
    while k - i >= 16:
        syms.append((1, 0xF0, None))
        i += 16
    syms.append((1, (k - i) << 4 | n, f))
    syms += list(more)
    if k < 63 or more:
        syms.append((1, 0x00, None))
    return syms


def fat_block():
    """a block of about a thousand bits whose pixels stay in range: +300 +300 -300 -300 ..."""
    syms = [(0, 0x00, None)]
    for k in range(1, 61):
        syms.append((1, 0x09, field_of(300 if (k - 1) % 4 < 2 else -300)[1]))
    return syms + [(1, 0x00, None)]


def pair_block(n):
    """a block whose coefficients 1 and 3 are + and - 2^(n-1)"""
    d = 1 << (n - 1)
    return [(0, 0x00, None), (1, n, field_of(d)[1]), (1, 0x10 | n, field_of(-d)[1]), (1, 0x00, None)]


F0_BLOCK = [(0, 0x00, None), (1, 0xF0, None), (1, 0x00, None)]


def blocks_len(table, blocks):
    return encode_plant(table, blocks).n


def fill_to(table, target, budget):
    """blocks that take exactly `target` bits, at most `budget` of them, all pixels in range: fat
    and flat ones, and for the remainder a few with an f0, with a +1 / -1 pair, and one whose
    coefficient 0 is +4 (which the carry keeps)"""
    flat, fat = blocks_len(table, [flat_block()]), blocks_len(table, [fat_block()])
    units = [(blocks_len(table, [flat_block(0x03, 4)]), flat_block(0x03, 4), 1),
             (blocks_len(table, [F0_BLOCK]), F0_BLOCK, flat),
             (blocks_len(table, [pair_block(1)]), pair_block(1), flat),
             (blocks_len(table, [pair_block(2)]), pair_block(2), flat)]
    for n_fat in range(target // fat, max(-1, target // fat - 3), -1):
        for a in range(units[0][2] + 1):
            for b in range(units[1][2] + 1):
                for c in range(units[2][2] + 1):
                    for d in range(units[3][2] + 1):
                        rest = (target - n_fat * fat - a * units[0][0] - b * units[1][0] -
                                c * units[2][0] - d * units[3][0])
                        if rest >= 0 and rest % flat == 0 and (
                                n_fat + a + b + c + d + rest // flat <= budget):
                            return ([fat_block()] * n_fat + [units[0][1]] * a + [units[1][1]] * b +
                                    [units[2][1]] * c + [units[3][1]] * d +
                                    [flat_block()] * (rest // flat))
    raise ValueError("no filling of %d bits" % target)


def planted(w, h, table, blocks, low_seed=None):
    """a case from planted blocks, padded with blocks of zeros to the frame's count (and with zero
    bytes to the reader's minimum)"""
    n = w * h // 64
    assert len(blocks) <= n, (len(blocks), n)
    blocks = list(blocks) + [flat_block()] * (n - len(blocks))
    data = stuff(encode_plant(table, blocks).data())
    data += bytes(max(0, 16 - len(data)))
    low = bytes(w * h // 4) if low_seed is None else low_for(w, h, low_seed)
    return dict(width=w, height=h, table=table, data=data, low=low)


def from_image(px, table, low_seed=None):
    h, w = px.shape
    low = bytes(w * h // 4) if low_seed is None else low_for(w, h, low_seed)
    data = encode_image(px, table)
    return dict(width=w, height=h, table=table, data=data + bytes(max(0, 16 - len(data))), low=low)


BAD16 = ("bits", 0xFFFF, 16)  # no code of a second tree is a prefix of sixteen ones
BAD_BLOCK = [(0, 0x00, None), BAD16]
assert all(symbol(t, 0xFFFF0000, 1)[0] == 0 for t in range(3))

# what zero bits decode to with table 1: coefficient 0 is -7, every other one -3 (257 bits)
ZERO_BLOCK_TABLE = 1
ZERO_DIFFS = [-7] + [-3] * 63


def zero_tail_stream(n_zero_blocks=2):
    """64 x 8, table 1: flat blocks, then blocks whose code is all zero bits -> (case, the bit the
    zeros start at)"""
    bw = encode_plant(ZERO_BLOCK_TABLE, [flat_block()] * (8 - n_zero_blocks))
    start = bw.n
    for _ in range(n_zero_blocks):
        put_block(bw, ZERO_BLOCK_TABLE, ZERO_DIFFS)
    data = bw.data()
    assert not any(data[(start + 7) // 8:]) and 0xFF not in data
    return dict(width=64, height=8, table=ZERO_BLOCK_TABLE, data=data, low=low_for(64, 8, 70)), start


def _make_cases():
    cases = {}

    def add(name, maker):
        assert name not in cases
        cases[name] = maker

    # --- geometry ---
    add("geom_64x1", lambda: from_image(noise_image(64, 1, 1, 3.0), 0, 11))
    add("geom_4x16", lambda: from_image(noise_image(4, 16, 2, 3.0), 0, 12))
    add("geom_8x8", lambda: from_image(noise_image(8, 8, 3, 3.0), 1, 13))
    add("geom_68x16", lambda: from_image(noise_image(68, 16, 4, 4.0), 2, 14))

    def g2672():
        px = noise_image(2672, 4, 5, 6.0).astype(np.int64)
        # values on both sides of 512 (pixel << 2: 128) and on 511 / 512 themselves
        px[0, :8] = [127, 128, 127, 128, 0, 1023, 128, 127]
        px[1, 100:104] = [127, 128, 126, 129]
        return from_image(px.astype(np.uint16), 0, 15)
    add("geom_2672x4_plus2", g2672)
    add("geom_4104x8", lambda: from_image(noise_image(4104, 8, 6, 5.0), 1, 16))

    def tall():
        px = np.full((3048, 64), 512, np.uint16)
        px[::97] = noise_image(64, 1, 7, 2.0)
        return from_image(px, 0)
    add("geom_64x3048_mostly_eob", tall)
    add("noise_1024x256_t0", lambda: from_image(noise_image(1024, 256, 20, 6.0), 0, 30))
    add("noise_1024x256_t1", lambda: from_image(noise_image(1024, 256, 21, 6.0), 1))
    add("noise_1024x256_t2", lambda: from_image(noise_image(1024, 256, 22, 6.0), 2))
    add("nonzero_1024x256", lambda: from_image(noise_image(1024, 256, 24, 5.0, nonzero=True), 0))
    for t in range(3):
        add("noise_68x16_t%d_wide" % t, lambda t=t: from_image(noise_image(68, 16, 40 + t, 60.0), t))

    # --- symbols (64 wide: a block a row) ---
    def sym(name, table, blocks, h=4):
        add(name, lambda: planted(64, h, table, blocks))

    sym("sym_00_at_0", 0, [flat_block()])
    for t in range(3):
        sym("sym_ff_first_tree_t%d" % t, t, [[(0, 0xFF, None), (1, 0x01, 1), (1, 0x00, None)]])
    sym("sym_f0", 0, [[(0, 0x00, None), (1, 0xF0, None), (1, 0x02, 2), (1, 0x00, None)]])
    sym("sym_00_at_63", 0, [[(0, 0x00, None)] + [(1, 0xF0, None)] * 3 + [(1, 0xD1, 1), (1, 0x00, None)]])
    sym("sym_coef63_no_00", 0, [value_block(63, 5)])
    sym("sym_run_passes_63_len0", 0, [[(0, 0x00, None)] + [(1, 0xF0, None)] * 4])
    sym("sym_run_passes_63_bits_dropped", 1,
        [[(0, 0x00, None)] + [(1, 0xF0, None)] * 3 + [(1, 0xFA, 0x2AA)]])
    sym("sym_code16", 0, [[(0, 0x00, None), (1, 0xE3, 0x4), (1, 0x00, None)]])

    def ends(table):
        """every length at the four ends of extend, from a carry / a coefficient 1 that keeps the
        pixel in range; what cannot be (length 11) is in sym_len11_*"""
        blocks = []
        for tree, top in ((0, 11), (1, 10)):
            for n in range(1, top + 1):
                for f in sorted({0, (1 << (n - 1)) - 1, 1 << (n - 1), (1 << n) - 1}):
                    d = extend(f, n)
                    pre = [p for p in (0, -512, 511) if 0 <= 512 + p + d <= 1023]
                    if not pre:
                        continue
                    p = pre[0]
                    if tree == 0:
                        blocks += [c0_block(p), flat_block(n, f), c0_block(-p - d)]
                    else:
                        syms = [(0, 0x00, None)]
                        if p:
                            syms.append((1,) + field_of(p))
                            syms.append((1, 0x10 | n, f))
                        else:
                            syms.append((1, n, f))
                        blocks.append(syms + [(1, 0x00, None)])
        return blocks
    for t in range(3):
        add("sym_extend_ends_t%d" % t, lambda t=t: planted(64, 192, t, ends(t)))
    for e, f in enumerate((0, 1023, 1024, 2047)):
        sym("sym_len11_end%d_out_of_range" % e, 0, [flat_block(11, f)])

    def straddle(edge_bits, h):
        front = fill_to(0, edge_bits - 3, h - 2)
        return planted(64, h, 0, front + [value_block(5, -3)])
    add("edge_code_straddles_segment", lambda: straddle(SEG_BITS, 80))
    add("edge_code_straddles_window", lambda: straddle(WIN_BITS, 400))

    # --- reader ---
    def ff_byte_at(bit, h):
        """a data byte FF (the field of a length-8 symbol) whose first bit is un-stuffed bit `bit`"""
        head = blocks_len(0, [[(0, 0x00, None), (1, 0x08, None)]])
        front = fill_to(0, bit - head, h - 2)
        blk = [(0, 0x00, None), (1, 0x08, 0xFF), (1, 0x18, 0x00), (1, 0x00, None)]
        c = planted(64, h, 0, front + [blk])
        assert unstuff(c["data"])[0][bit // 8:bit // 8 + 2][0] & (0xFF >> (bit % 8)) == 0xFF >> (bit % 8)
        return c
    add("reader_ff_ends_at_segment_edge", lambda: ff_byte_at(SEG_BITS - 8, 80))
    add("reader_ff_across_segment_edge", lambda: ff_byte_at(SEG_BITS - 4, 80))
    add("reader_ff_ends_at_window_edge", lambda: ff_byte_at(WIN_BITS - 8, 400))
    add("reader_ff_across_window_edge", lambda: ff_byte_at(WIN_BITS - 4, 400))

    def chunk_edge():
        # raw byte 4095 an FF, 4096 its 00 (the compaction's chunks are 4096 raw bytes)
        c = ff_byte_at(4095 * 8, 400)
        assert c["data"][4095] == 0xFF and c["data"][4096] == 0 and 0xFF not in c["data"][:4095]
        return c
    add("reader_ff00_across_chunk_edge", chunk_edge)
    # (FF 00 at every place of a fill's four bytes: the wide-noise streams; test_crw_model.py
    # holds the counters stuffed_at0..3 above zero)
    add("reader_ff00_many", lambda: from_image(noise_image(256, 64, 52, 150.0), 0, 53))

    def base_stream(seed):
        return from_image(noise_image(64, 8, seed, 5.0), 0, seed)

    def with_marker(c, at):
        while c["data"][at - 1] == 0xFF or c["data"][at] == 0:
            at += 4
        c["data"] = c["data"][:at] + b"\xff\xd9" + c["data"][at:]
        return c
    add("reader_marker_mid_frame", lambda: with_marker(base_stream(60), 120))
    for phase in range(4):
        add("reader_marker_phase%d" % phase, lambda p=phase: with_marker(base_stream(61), 40 + p))
    add("reader_marker_at_byte_0", lambda: dict(base_stream(61), data=b"\xff\xd9" + bytes(16)))

    def marker_behind():
        c = base_stream(62)
        c["data"] += b"\xff\xd9"
        return c
    add("reader_marker_behind_last_block", marker_behind)
    add("reader_ends_exactly", lambda: base_stream(63))

    def zero_tail(short):
        c, _ = zero_tail_stream()
        c["data"] = c["data"][:len(c["data"]) - short]
        return c
    for short in range(0, 41):
        add("reader_zero_tail_%02d_short" % short, lambda s=short: zero_tail(s))

    def zero_tail_marker(into):
        # the marker `into` bytes into the zeros of ONE zero block: the reader supplies the rest
        c, start = zero_tail_stream(1)
        at = (start + 7) // 8 + into
        c["data"] = c["data"][:at] + b"\xff\xd9" + c["data"][at:]
        return c
    for into in range(0, 24):
        add("reader_marker_%02d_into_zeros" % into, lambda i=into: zero_tail_marker(i))

    def ends_in_ff():
        c = from_image(noise_image(256, 64, 52, 150.0), 0, 53)
        at = c["data"].index(b"\xff\x00", 500)
        c["data"] = c["data"][:at + 1]
        return c
    add("reader_cut_ends_in_ff", ends_in_ff)
    add("reader_trailing_ff", lambda: dict(base_stream(65), data=base_stream(65)["data"] + b"\xff"))
    add("reader_trailing_bytes",
        lambda: dict(base_stream(66), data=base_stream(66)["data"] + bytes(range(1, 200))))
    add("reader_7_bytes", lambda: dict(width=8, height=8, table=0, low=bytes(16), data=bytes(7)))
    add("reader_8_bytes", lambda: dict(width=8, height=8, table=1, low=bytes(16), data=bytes(8)))

    # --- verdicts ---
    sym("verdict_bad_code_block_0", 0, [BAD_BLOCK], h=8)
    sym("verdict_bad_code_middle", 0, [flat_block()] * 4 + [BAD_BLOCK], h=8)
    sym("verdict_bad_code_last", 0, [flat_block()] * 7 + [BAD_BLOCK], h=8)
    sym("verdict_value_0_and_1023", 0, [c0_block(-512), c0_block(1023)], h=2)
    sym("verdict_first_pixel_minus_1", 0, [c0_block(-513)])
    sym("verdict_first_pixel_1024", 0, [c0_block(512)])
    sym("verdict_carry_minus_1", 0, [c0_block(-300), c0_block(-213)])
    sym("verdict_carry_1024", 0, [c0_block(300), c0_block(212)])
    # 68 wide: row 1 begins at coefficient 4 of block 1
    add("verdict_row_start_mid_block_minus_1",
        lambda: planted(68, 16, 0, [flat_block(), value_block(4, -513)]))
    add("verdict_row_start_mid_block_1024",
        lambda: planted(68, 16, 0, [flat_block(), value_block(4, 512)]))
    sym("verdict_last_pixel_minus_1", 0, [flat_block()] * 3 + [value_block(63, -513)])
    sym("verdict_last_pixel_1024", 0, [flat_block()] * 3 + [value_block(63, 512)])
    sym("verdict_range_then_bad_code", 0,
        [flat_block(), value_block(9, 600), flat_block(), BAD_BLOCK], h=8)
    sym("verdict_bad_code_then_range", 0, [flat_block(), BAD_BLOCK, value_block(9, 600)], h=8)
    sym("verdict_both_in_one_block", 0,
        [flat_block(), [(0, 0x00, None), (1, 0x0A, 0x3FF), BAD16]], h=8)
    return cases


_MAKERS = None


def _makers():
    global _MAKERS
    if _MAKERS is None:
        _MAKERS = _make_cases()
    return _MAKERS


def case_names():
    return list(_makers())


@functools.lru_cache(maxsize=None)
def build_case(name):
    c = dict(_makers()[name]())
    c["name"] = name
    c["data"] = bytes(c["data"])
    c["low"] = bytes(c["low"])
    return c


REACH = new_reach()  # what the model reached over every case decoded so far


@functools.lru_cache(maxsize=None)
def expected(name, lowbits=True):
    """(status, pixels or None) of the model"""
    c = build_case(name)
    st, px = decode(c["width"], c["height"], c["table"], c["data"], c["low"] if lowbits else None,
                    REACH)
    if px is not None:
        px.setflags(write=False)
    return st, px


def case_file(name):
    c = build_case(name)
    return crw_file(c["width"], c["height"], c["table"], c["data"], c["low"])


def sha_rows(px):
    return hashlib.sha256(np.ascontiguousarray(px, dtype="<u2").tobytes()).hexdigest()


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


# (name, width, height, table, low-bit bytes short of width height / 4, cpp, pitch or None, status):
# the constructor's checks and the call's own
VALIDATION = [
    ("width_0", 0, 16, 0, 0, 1, None, ERR_INVALID_ARG),
    ("width_6", 6, 32, 0, 0, 1, None, ERR_INVALID_ARG),
    ("width_4104", 4104, 8, 0, 0, 1, None, OK),
    ("width_4108", 4108, 16, 0, 0, 1, None, ERR_INVALID_ARG),
    ("height_0", 64, 0, 0, 0, 1, None, ERR_INVALID_ARG),
    ("height_3048", 64, 3048, 0, 0, 1, None, OK),
    ("height_3049", 64, 3049, 0, 0, 1, None, ERR_INVALID_ARG),
    ("area_4x4", 4, 4, 0, 0, 1, None, ERR_INVALID_ARG),
    ("table_2", 64, 4, 2, 0, 1, None, OK),
    ("table_3", 64, 4, 3, 0, 1, None, ERR_INVALID_ARG),
    ("low_one_short", 64, 4, 0, 1, 1, None, ERR_INVALID_ARG),
    ("cpp_2", 64, 4, 0, 0, 2, None, ERR_INVALID_ARG),
    ("pitch_below", 64, 4, 0, 0, 1, 126, ERR_INVALID_ARG),
    ("pitch_exact", 64, 4, 0, 0, 1, 128, OK),
]


# ---------------------------------------------------------------------------------------------
# The host build (rawspeed_amd/librsx_crw_host.so)
# ---------------------------------------------------------------------------------------------
_HOST = None


def host_lib():
    global _HOST
    if _HOST is None:
        import ctypes as C
        from rawspeed_amd import build
        _HOST = C.CDLL(build.build_crw_host()[0])
        _HOST.rsx_crw_host_validate.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]
        _HOST.rsx_crw_host_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                              C.c_size_t, C.c_void_p]
    return _HOST


def host_decode(data, low, width, height, table, pitch=None, cpp=1):
    """-> (status, pixels, the whole image buffer): the buffer starts as 0xA5; low None: no low bits"""
    import ctypes as C
    from rawspeed_amd import abi
    pitch = 2 * width if pitch is None else pitch
    buf = np.full(max(1, pitch * max(height, 0)), 0xA5, np.uint8)
    img = abi.Image(buf.ctypes.data, pitch, width, height, cpp, 1)
    d = abi.crw_desc(table, low is not None)
    a = np.frombuffer(bytes(data) + b"\0", np.uint8).copy()
    b = np.frombuffer(bytes(low or b"") + b"\0", np.uint8).copy()
    st = host_lib().rsx_crw_host_decode(C.byref(d), a.ctypes.data, len(data),
                                        b.ctypes.data if low is not None else None,
                                        len(low) if low is not None else 0, C.byref(img))
    px = None
    if st == OK:
        px = np.stack([buf[r * pitch:r * pitch + 2 * width].view(np.uint16) for r in range(height)])
    return st, px, buf
