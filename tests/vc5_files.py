"""VC5Decompressor (GoPro VC-5, DNG compression 9; include/rsx.h section 4c) test material: the
code book (tests/golden/vc5_codebook.json: 264 rows size, bits, count, decompanded value), a
writer of band streams, of the tagged VC-5 block parseVC5 reads and of a compression-9 DNG around
it, the descriptor the C-ABI takes, seeded cases, and a numpy model of the whole decode.

A tile is four channels (gs, rg, bg, gd) of ceil(W/2) x ceil(H/2), each three wavelet levels
deep; level k = 1..3 has bands of dims(W, H)[k].  Subband 0 is the low-pass band of level 3,
subbands 1-3 / 4-6 / 7-9 the high-pass bands 1..3 of level 3 / 2 / 1."""
import contextlib
import hashlib
import json
import os
import struct

import numpy as np

import rawfiles as R

HERE = os.path.dirname(os.path.abspath(__file__))
CODEBOOK = os.path.join(HERE, "golden", "vc5_codebook.json")
GOLDEN = os.path.join(HERE, "golden", "vc5_ref.json")

OK, MARKER, CODE, OVERREAD, RANGE, UNSUPPORTED = 0, 1, 3, 5, 10, 7
SEG_BITS, LANES = 128, 1024          # rsx_vc5.hip: bits of a segment, segments of a window
WIN_BITS = SEG_BITS * LANES
WIN_EXTRA_WORDS = 4                  # words loaded behind a window, for a symbol behind its last segment
MERGE_CELLS, MERGE_ROWS = 256, 32    # cells a row and cell rows of a merge workgroup (64 lanes x 4 cells)
MERGE_LANE_CELLS = 4
LEVEL_X, LEVEL_Y = 64, 4             # cells of a level workgroup
LP_STRIDE = 16 * 256                 # low-pass fields a trip of the loop: 16 workgroups of 256 lanes
MIN_DIM, MAX_DIM = 34, 65534         # image sides the decoder takes
WHITELEVEL = 50717
RUNS = (320, 180, 100, 60, 32, 20, 12, 1)   # the book's zero runs, longest first

_BOOK = None
_DEC = None


def book():
    """[(size, bits, count, value)] x 264 (or the book of the use_book block around the call)"""
    global _BOOK
    if _BOOK is None:
        with open(CODEBOOK) as f:
            _BOOK = [tuple(r) for r in json.load(f)]
    return _BOOK


@contextlib.contextmanager
def use_book(rows):
    """writer and model work with `rows` instead of the reference's book inside the block"""
    global _BOOK, _DEC
    book()
    saved, _BOOK, _DEC = (_BOOK, _DEC), [tuple(r) for r in rows], None
    try:
        yield
    finally:
        _BOOK, _DEC = saved


def book_with_hole():
    """the book without one of its 25-bit words: those 25 bits then begin no word.
    (rows, the (bits, size) that became invalid)"""
    rows = list(book())
    k = next(i for i, r in enumerate(rows) if r[0] == 25)
    gone = rows.pop(k)
    return rows, (gone[1], gone[0])


def dims(w, h):
    """[(w_k, h_k)] for k = 0..3: the channel plane and the three levels"""
    out = []
    for _ in range(4):
        w, h = (w + 1) // 2, (h + 1) // 2
        out.append((w, h))
    return out


def subband(level, band):
    """subband number of band 1..3 of level 1..3 (band 0 of level 3 is subband 0)"""
    return 0 if band == 0 else 3 * (3 - level) + band


def log_table(white):
    """mVC5LogTable (VC5Decompressor.cpp:464-488) for a white level"""
    bits = int(white).bit_length()
    i = np.arange(4096, dtype=np.float64)
    y = 65535.0 * ((np.power(113.0, i / 4095.0) - 1) / 112.0)
    return (y.astype(np.uint32) >> (16 - bits)).astype(np.uint16)


# ---------------------------------------------------------------------------- streams
class Bits:
    """MSB-first bit writer"""

    def __init__(self):
        self.parts = []  # (value, nbits)

    def put(self, value, n):
        self.parts.append((int(value), int(n)))
        return self

    def nbits(self):
        return sum(n for _, n in self.parts)

    def bytes(self, pad_to=1):
        """the bits, zero-padded to a multiple of pad_to bytes"""
        s = "".join(format(x & ((1 << k) - 1), "0%db" % k) for x, k in self.parts if k)
        s += "0" * (-len(s) % (8 * pad_to))
        return np.packbits(np.frombuffer(s.encode(), np.uint8) - 48)


def _rows_by_key():
    b = book()
    return ({v: i for i, (s, c, n, v) in enumerate(b) if n == 1},
            {n: i for i, (s, c, n, v) in enumerate(b) if v == 0 and n >= 1},
            next(i for i, (s, c, n, v) in enumerate(b) if n == 0))


def put_row(bits, row, negative=False):
    """one symbol: word `row` of the book and its sign bit"""
    size, code, count, value = book()[row]
    bits.put(code, size)
    if value != 0:
        bits.put(1 if negative else 0, 1)
    return bits


def symbols_of(values):
    """The rows (row, negative) that encode a flat array of book values: non-zero values one
    symbol each, zero runs greedily by the book's run lengths.  Without the end marker."""
    by_value, by_run, _ = _rows_by_key()
    flat = np.asarray(values, np.int64).ravel()
    out = []
    i, n = 0, flat.size
    while i < n:
        if flat[i] != 0:
            out.append((by_value[abs(int(flat[i]))], bool(flat[i] < 0)))
            i += 1
            continue
        j = i
        while j < n and flat[j] == 0:
            j += 1
        run = j - i
        for r in RUNS:
            while run >= r:
                out.append((by_run[r], False))
                run -= r
        i = j
    return out


def encode_symbols(symbols, marker=True, pad_to=4, tail=None):
    """rows -> stream bytes; marker: the end marker behind them; tail: a Bits appended behind it"""
    b = Bits()
    for row, neg in symbols:
        put_row(b, row, neg)
    if marker:
        put_row(b, _rows_by_key()[2])
    if tail is not None:
        b.parts += tail.parts
    return b.bytes(pad_to)


def encode_values(values, **kw):
    return encode_symbols(symbols_of(values), **kw)


def encode_values_fast(values):
    """encode_values for large bands (bench_vc5.py), vectorised; stream padded to 4 bytes"""
    b = book()
    by_value, by_run, marker = _rows_by_key()
    flat = np.asarray(values, np.int64).ravel()
    nz = flat != 0
    pos_nz = np.flatnonzero(nz)
    starts = np.flatnonzero(~nz & np.concatenate(([True], nz[:-1])))
    ends = np.flatnonzero(~nz & np.concatenate((nz[1:], [True]))) + 1
    counts = np.zeros((starts.size, len(RUNS)), np.int64)
    rem = ends - starts
    for k, r in enumerate(RUNS):
        counts[:, k] = rem // r
        rem = rem % r
    # events in stream order: slot 0..7 a zero run of RUNS[k], slot 8 the non-zero value
    ev_pos = np.concatenate((starts, pos_nz))
    ev_cnt = np.zeros((ev_pos.size, 9), np.int64)
    ev_cnt[:starts.size, :8] = counts
    ev_cnt[starts.size:, 8] = 1
    order = np.argsort(ev_pos, kind="stable")
    ev_cnt, ev_pos = ev_cnt[order], ev_pos[order]
    slot = np.repeat(np.tile(np.arange(9), ev_pos.size), ev_cnt.ravel())
    where = np.repeat(np.repeat(ev_pos, 9), ev_cnt.ravel())
    val = np.where(slot == 8, flat[where], 0)
    size_v = np.zeros(1024, np.int64)
    code_v = np.zeros(1024, np.int64)
    for v, i in by_value.items():
        size_v[v], code_v[v] = b[i][0] + (1 if v else 0), b[i][1] << (1 if v else 0)
    run_size = np.array([b[by_run[r]][0] for r in RUNS] + [0], np.int64)
    run_code = np.array([b[by_run[r]][1] for r in RUNS] + [0], np.int64)
    a = np.abs(val)
    lens = np.where(slot == 8, size_v[a], run_size[slot])
    codes = np.where(slot == 8, code_v[a] | (val < 0), run_code[slot])
    lens = np.concatenate((lens, [b[marker][0] + 1]))
    codes = np.concatenate((codes, [b[marker][1] << 1]))
    first = np.concatenate(([0], np.cumsum(lens)[:-1]))
    total = int(lens.sum())
    sym = np.repeat(np.arange(lens.size), lens)
    k = np.arange(total) - np.repeat(first, lens)
    bit = ((codes[sym] >> (lens[sym] - 1 - k)) & 1).astype(np.uint8)
    pad = -total % 32
    return np.packbits(np.concatenate((bit, np.zeros(pad, np.uint8))))


def pack_lowpass(values, precision):
    """w x h fields of `precision` bits, MSB first, padded to 8 bytes (:657-666)"""
    b = Bits()
    for v in np.asarray(values).ravel():
        b.put(int(v), precision)
    return b.bytes(8)


# ---------------------------------------------------------------------------- a tile
class Tile:
    """What parseVC5 finds in one tile: per channel the ten chunks, the quantisations, the
    low-pass precision and the prescale of each level."""

    def __init__(self, w, h, phase=0, white=65535):
        self.w, self.h, self.phase, self.white = w, h, phase, white
        self.chunks = [[None] * 10 for _ in range(4)]
        self.quant = [[1] * 10 for _ in range(4)]
        self.precision = [16] * 4
        self.prescale = [[0, 0, 0] for _ in range(4)]  # [channel][level - 1]

    def dims(self):
        return dims(self.w, self.h)

    def set_lowpass(self, c, values, precision=16):
        self.precision[c] = precision
        self.chunks[c][0] = pack_lowpass(values, precision)

    def set_band(self, c, level, band, values=None, quant=1, stream=None):
        """values: book values (h_k, w_k); or a ready stream"""
        s = subband(level, band)
        self.quant[c][s] = quant
        self.chunks[c][s] = encode_values(values) if stream is None else np.asarray(stream, np.uint8)

    def layout(self, gap=0):
        """(tile bytes, bands[c][s] = (offset, bytes, quant, precision)): the chunks one after
        the other, `gap` foreign bytes between them"""
        out, bands = [], [[None] * 10 for _ in range(4)]
        at = 0
        for c in range(4):
            for s in range(10):
                ch = self.chunks[c][s]
                bands[c][s] = (at, len(ch), self.quant[c][s] if s else 0, self.precision[c] if s == 0 else 0)
                out.append(ch)
                out.append(np.full(gap, 0xEE, np.uint8))
                at += len(ch) + gap
        return np.concatenate(out), bands

    def vc5_block(self):
        """the tagged block parseVC5 (:490-618) reads: (tile bytes, bands as in layout())"""
        def tag(t, v):
            return struct.pack(">hH", t, v & 0xFFFF)
        out = bytearray(b"VC-5")
        for t, v in ((0x000C, 4), (0x0014, self.w), (0x0015, self.h), (0x000E, 10), (0x0054, 4),
                     (0x0066, 12), (0x006A, 2), (0x006B, 2), (0x006C, 1)):
            out += tag(t, v)
        bands = [[None] * 10 for _ in range(4)]
        for c in range(4):
            out += tag(0x003E, c)
            p = self.prescale[c]
            out += tag(0x006D, (p[0] << 14) | (p[1] << 12) | (p[2] << 10))
            for s in range(10):
                ch = self.chunks[c][s]
                assert len(ch) % 4 == 0, "a chunk of the container is a whole number of 4 bytes"
                out += tag(0x0030, s)
                out += tag(0x0023, self.precision[c]) if s == 0 else tag(0x0035, self.quant[c][s])
                units = len(ch) // 4
                out += tag(0x6000 | (units >> 16), units & 0xFFFF)
                size = len(ch)
                if s == 0:  # LowPassBand takes the 8-byte-rounded size of its fields (:657-666)
                    w3, h3 = self.dims()[3]
                    size = 8 * (-(-w3 * h3 * self.precision[c] // 64))
                bands[c][s] = (len(out), size, self.quant[c][s] if s else 0,
                               self.precision[c] if s == 0 else 0)
                out += bytes(ch)
        return np.frombuffer(bytes(out), np.uint8).copy(), bands

    def dng(self):
        """a compression-9 DNG of one tile: (file bytes, tile bytes, bands)"""
        data, bands = self.vc5_block()
        i = R.Ifd()
        i.add(R.NEWSUBFILETYPE, R.LONG, 0)
        i.add(R.IMAGEWIDTH, R.LONG, self.w).add(R.IMAGELENGTH, R.LONG, self.h)
        i.add(R.BITSPERSAMPLE, R.SHORT, [16])
        i.add(R.COMPRESSION, R.SHORT, 9)
        i.add(R.PHOTOMETRIC, R.SHORT, 32803)
        i.add(R.MAKE, R.ASCII, "RSX").add(R.MODEL, R.ASCII, "Synthetic")
        i.add(R.SAMPLESPERPIXEL, R.SHORT, 1)
        i.add(R.CFAREPEATPATTERNDIM, R.SHORT, [2, 2])
        i.add(R.CFAPATTERN, R.BYTE, [0, 1, 1, 2] if self.phase == 0 else [1, 2, 0, 1])
        i.add(R.DNGVERSION, R.BYTE, [1, 4, 0, 0])
        i.add(R.DNGBACKWARDVERSION, R.BYTE, [1, 1, 0, 0])
        i.add(R.UNIQUECAMERAMODEL, R.ASCII, "RSX Synthetic")
        i.add(WHITELEVEL, R.LONG, self.white)
        i.add(R.TILEWIDTH, R.LONG, self.w).add(R.TILELENGTH, R.LONG, self.h)
        i.add_blobs(R.TILEOFFSETS, R.TILEBYTECOUNTS, [data])
        return R.tiff_file(i), data, bands


def abi_desc(tile, bands, table=None, codes="book"):
    """(abi.Vc5Desc, keep-alive) of a tile laid out as `bands`"""
    from rawspeed_amd import abi
    return abi.vc5_desc(tile.phase, log_table(tile.white) if table is None else table,
                        book() if codes == "book" else codes, bands, tile.prescale)


# ---------------------------------------------------------------------------- the model
def _decoder():
    """(first-12-bits table of (size, count, value) or None, {size: {bits: (count, value)}})"""
    global _DEC
    if _DEC is None:
        lut = [None] * 4096
        long = {}
        for size, bits, count, value in book():
            if size <= 12:
                for k in range(1 << (12 - size)):
                    lut[(bits << (12 - size)) | k] = (size, count, value)
            else:
                long.setdefault(size, {})[bits] = (count, value)
        _DEC = lut, sorted(long.items())
    return _DEC


def bit_string(data):
    return (np.unpackbits(np.asarray(data, np.uint8)) + 48).tobytes().decode() + "0" * 128


def read_symbol(bits, pos):
    """(size, count, value, length) of the symbol at bit `pos`, None when no word starts there"""
    lut, long = _decoder()
    e = lut[int(bits[pos:pos + 12], 2)]
    if e is None:
        for size, words in long:
            hit = words.get(int(bits[pos:pos + size], 2))
            if hit is not None:
                e = (size, hit[0], hit[1])
                break
        else:
            return None
    size, count, value = e
    if value != 0:
        if bits[pos + size] == "1":
            value = -value
        return size, count, value, size + 1
    return size, count, value, size


def start_limit(nbytes):
    return 32 * ((nbytes + 8) // 4)


def model_band(data, quant, n):
    """HighPassBand::decode (:683-742): (status, n coefficients int16 or None)"""
    data = np.asarray(data, np.uint8)
    bits = bit_string(data)
    lim = start_limit(data.size)
    out = np.zeros(n, np.int64)
    pos = p = 0
    while True:
        if pos > lim:
            return OVERREAD, None
        s = read_symbol(bits, pos)
        if s is None:
            return CODE, None
        size, count, value, length = s
        if p == n:
            return (OK, out.astype(np.int16)) if value == 1 and count == 0 else (MARKER, None)
        v = value * quant
        if not -32768 <= v <= 32767:
            return RANGE, None
        if count == 0 or p + count > n:
            return MARKER, None
        out[p:p + count] = v
        p += count
        pos += length


def rounds_needed(data, quant, n, lanes=LANES, carries=None):
    """Parse rounds per window of the band kernel's scheme on this stream of a band of n
    coefficients: every segment parsed from entry 0, then from the exit of the segment in front of
    it as of the round before, until nothing changes.  [rounds of window 0, 1, ..] up to the window
    in which the true chain reaches coefficient n or stops at a symbol that fails the band -- the
    last one the kernel loads: a band that ends with a window's last segment has its end marker
    read from the words behind that window.  carries: a list that gets the entry offset of lane 0
    of every window walked."""
    data = np.asarray(data, np.uint8)
    bits = bit_string(data) + "0" * (SEG_BITS * lanes)
    lim = start_limit(data.size)
    seen = {}

    def walk(pos, end):
        """(exit, coefficients) of the symbols that start in [pos, end); exit None: stopped"""
        count = 0
        while pos < end:
            if pos > lim:
                return None, count
            if pos not in seen:                           # (guessed parses soon read true symbols)
                seen[pos] = read_symbol(bits, pos)
            s = seen[pos]
            if s is None or s[1] == 0 or not -32768 <= s[2] * quant <= 32767:
                return None, count
            count += s[1]
            pos += s[3]
        return pos - end, count

    out, carry, w, p = [], 0, 0, 0
    while True:
        base = w * SEG_BITS * lanes
        if carries is not None:
            carries.append(carry)
        entry = [carry] + [0] * (lanes - 1)
        ex = [walk(base + k * SEG_BITS + entry[k], base + (k + 1) * SEG_BITS) for k in range(lanes)]
        rounds = 1
        while True:
            new = [carry] + [0 if e is None else e for e, _ in ex[:-1]]
            changed = [k for k in range(lanes) if new[k] != entry[k]]
            if not changed:
                break
            rounds += 1
            for k in changed:
                entry[k] = new[k]
                ex[k] = walk(base + k * SEG_BITS + entry[k], base + (k + 1) * SEG_BITS)
        out.append(rounds)
        # the true chain: the first lane that stops, or that holds coefficient n - 1, ends the band
        for e, count in ex:
            if e is None or p + count >= n:
                return out
            p += count
        carry, w = ex[-1][0], w + 1


def rounds_needed_by_stream_alone(data, quant, lanes=LANES):
    """rounds_needed as it was before it took the coefficient count: it walks on until a walk of
    the true chain stops, into windows the kernel never loads when the band ends with a window.
    Kept for the test that shows the difference (tests/test_vc5_core_host.py)."""
    return rounds_needed(data, quant, 1 << 62, lanes)


def symbol_bits(symbol):
    """(bits, coefficients) of a symbol (row, negative)"""
    size, _, count, value = book()[symbol[0]]
    return size + (1 if value != 0 else 0), count


def symbols_ending_at(symbols, target, n=None, last=None):
    """(symbols, coefficients): a stream whose encoded length -- in front of the end marker -- is
    exactly `target` bits.  A prefix of `symbols` up to about target - 80 bits, then value symbols
    whose lengths add up to the rest (the book has value symbols of 3, 4 and 6 .. 27 bits).  With
    n the band has exactly n coefficients: the zero runs that make up for them go in front.
    last: the bits of the last symbol."""
    coins = {}
    for row, (size, _, count, value) in enumerate(book()):
        if count == 1 and value > 0:
            coins.setdefault(size + 1, row)
    if last is not None:
        out, count = symbols_ending_at(symbols, target - last, None if n is None else n - 1)
        return out + [(coins[last], True)], count + 1
    symbols = symbols[:target + 1]                        # (a symbol has a bit at least)
    by_run = _rows_by_key()[1]
    top = 12                                              # (coins enough for 80 bits and more)
    reach = [{0: None}]                                   # reach[c][sum] = the last coin of c coins
    for c in range(1, top + 1):
        reach.append({s + l: l for s in reach[-1] for l in coins})

    def change(c, gap):
        out = []
        while c:
            out.append(reach[c][gap])
            c, gap = c - 1, gap - out[-1]
        return out

    sizes = [symbol_bits(s) for s in symbols]
    at = np.concatenate(([0], np.cumsum([b for b, _ in sizes]))).astype(np.int64)
    got = np.concatenate(([0], np.cumsum([k for _, k in sizes]))).astype(np.int64)
    for m in range(int(np.searchsorted(at, max(target - 80, 0), "right")) - 1, -1, -1):
        for c in range(1, top + 1):
            zeros = 0 if n is None else n - int(got[m]) - c
            if zeros < 0:
                break
            front = []                                    # (as symbols_of writes a zero run)
            for r in RUNS:
                front += [(by_run[r], False)] * (zeros // r)
                zeros %= r
            gap = target - int(at[m]) - sum(symbol_bits(s)[0] for s in front)
            if gap in reach[c]:
                tail = [(coins[l], k % 2 == 1) for k, l in enumerate(change(c, gap))]
                out = front + list(symbols[:m]) + tail
                bits, count = (sum(x) for x in zip(*(symbol_bits(s) for s in out)))
                assert bits == target and (n is None or count == n), (bits, target, count, n)
                return out, count
    raise ValueError("no stream of %d bits%s" % (target, "" if n is None else " and %d coefficients" % n))


def model_lowpass(data, precision, w, h):
    bits = np.unpackbits(np.asarray(data, np.uint8))[:w * h * precision].reshape(w * h, precision)
    v = bits.astype(np.int64) @ (1 << np.arange(precision - 1, -1, -1, dtype=np.int64))
    return v.astype(np.uint16).astype(np.int16).reshape(h, w)


def _conv(m, high, l0, l1, l2, shift):
    lows = (m[1] * l0 + m[2] * l1 + m[3] * l2 + 4) >> 3
    return ((m[0] * high + lows) * (1 << shift)) >> 1


FIRST = ((1, 11, -4, 1), (-1, 5, 4, -1))
MIDDLE = ((1, 1, 8, -1), (-1, -1, 8, 1))
LAST = ((1, -1, 4, 5), (-1, 1, -4, 11))


def _pass(high, low, shift):
    """reconstructPass down axis 0 (:183-232): high (h, w), low at least (h, w) -> (2h, w) int64"""
    h, w = high.shape
    high, low = high.astype(np.int64), low[:h, :w].astype(np.int64)
    out = np.zeros((2 * h, w), np.int64)
    for k in range(2):
        out[k, :] = _conv(FIRST[k], high[0], low[0], low[1], low[2], shift)
        out[2 + k:2 * h - 2:2, :] = _conv(MIDDLE[k], high[1:h - 1], low[0:h - 2], low[1:h - 1], low[2:h], shift)
        out[2 * h - 2 + k, :] = _conv(LAST[k], high[h - 1], low[h - 3], low[h - 2], low[h - 1], shift)
    return out


def _i16(a):
    return a.astype(np.uint16).astype(np.int16)


def model_level(b0, b1, b2, b3, prescale, clamp):
    """one level (createDecodingTasks, :289-372): four (h, w) bands (b0 may be larger) -> (2h, 2w)"""
    lowpass = _i16(_pass(b2, b0, 0))
    highpass = _i16(_pass(b3, b1, 0))
    out = _pass(highpass.T, lowpass.T, 2 if prescale == 2 else 0).T
    if clamp:
        out = np.clip(out, 0, 16383)
    return _i16(out)


def model_merge(planes, w, h, phase, table):
    gs, rg, bg, gd = (p[:h // 2, :w // 2].astype(np.int64) for p in planes)
    rg, bg, gd = rg - 2048, bg - 2048, gd - 2048
    t = np.asarray(table, np.uint16)
    look = lambda v: t[np.clip(v, 0, 4095)]  # noqa: E731
    r, b, g1, g2 = look(gs + 2 * rg), look(gs + 2 * bg), look(gs + gd), look(gs - gd)
    out = np.zeros((h, w), np.uint16)
    if phase == 0:
        out[0::2, 0::2], out[0::2, 1::2], out[1::2, 0::2], out[1::2, 1::2] = r, g1, g2, b
    else:
        out[0::2, 0::2], out[0::2, 1::2], out[1::2, 0::2], out[1::2, 1::2] = g1, b, r, g2
    return out


def model_decode(tile, data, bands, table=None, planes_out=None):
    """(status, image or None; band statuses (4, 10)): the whole decode of a tile laid out as
    `bands` in `data`.  The status is that of the first failing band in (channel, subband) order."""
    d = tile.dims()
    table = log_table(tile.white) if table is None else table
    status = np.zeros((4, 10), np.int32)
    planes = []
    for c in range(4):
        co = {}
        for s in range(10):
            off, n, quant, precision = bands[c][s]
            chunk = np.asarray(data[off:off + n], np.uint8)
            level = 3 if s == 0 else 3 - (s - 1) // 3
            w, h = d[level]
            if s == 0:
                co[(3, 0)] = model_lowpass(chunk, precision, w, h)
            else:
                st, v = model_band(chunk, quant, w * h)
                status[c, s] = st
                co[(level, 1 + (s - 1) % 3)] = v.reshape(h, w) if st == OK else np.zeros((h, w), np.int16)
        for level in (3, 2, 1):
            out = model_level(co[(level, 0)], co[(level, 1)], co[(level, 2)], co[(level, 3)],
                              tile.prescale[c][level - 1], level == 1)
            co[(level - 1, 0)] = out
        planes.append(co[(0, 0)])
    if planes_out is not None:
        planes_out.extend(planes)
    bad = status[status != OK]
    if bad.size:
        return int(bad[0]), None, status
    return OK, model_merge(planes, tile.w, tile.h, tile.phase, table), status


# ---------------------------------------------------------------------------- seeded cases
def book_values():
    """the non-zero values the book can carry"""
    return np.array(sorted(v for s, b, n, v in book() if n == 1 and v > 0), np.int64)


def random_band(rng, w, h, density=0.2, vmax=40):
    """book values (h, w): zeros with `density` non-zero entries up to vmax"""
    vals = book_values()
    vals = vals[vals <= vmax]
    a = np.zeros(w * h, np.int64)
    k = rng.random(w * h) < density
    a[k] = rng.choice(vals, int(k.sum())) * rng.choice([-1, 1], int(k.sum()))
    return a.reshape(h, w)


def make_tile(seed, w, h, phase=0, white=65535, prescale=None, density=0.2, vmax=40, quant=None,
              precision=16, low=(0, 4096)):
    """A valid tile of seeded bands.  prescale: [channel][level - 1]; quant: f(c, level, band)"""
    rng = np.random.default_rng([0x7C5, seed])
    t = Tile(w, h, phase, white)
    if prescale is not None:
        t.prescale = [list(p) for p in prescale]
    d = t.dims()
    for c in range(4):
        w3, h3 = d[3]
        t.set_lowpass(c, rng.integers(low[0], min(low[1], 1 << precision), (h3, w3)), precision)
        for level in (1, 2, 3):
            wk, hk = d[level]
            for band in (1, 2, 3):
                q = int(rng.integers(1, 24)) if quant is None else quant(c, level, band)
                t.set_band(c, level, band, random_band(rng, wk, hk, density, vmax), q)
    return t


def every_row_band(rng, w, h):
    """book values (h, w) that use every non-zero value of the book with both signs; None when
    the band is too small"""
    vals = book_values()
    if w * h < 2 * vals.size + 8:
        return None
    a = np.zeros(w * h, np.int64)
    at = rng.choice(w * h, 2 * vals.size, replace=False)
    a[at[:vals.size]] = vals
    a[at[vals.size:]] = -vals
    return a.reshape(h, w)


def sha(img):
    return hashlib.sha256(np.ascontiguousarray(img, np.dtype("<u2")).tobytes()).hexdigest()


PRESCALES = ([[0, 0, 0]] * 4, [[2, 2, 2]] * 4, [[0, 2, 0], [2, 0, 2], [0, 0, 2], [2, 0, 0]],
             [[1, 3, 2]] * 4)
WHITES = (65535, 16383, 4095)


def golden_cases():
    """[(name, Tile)]: the cases recorded in tests/golden/vc5_ref.json"""
    out = []
    for k, (w, h) in enumerate(((34, 34), (36, 34), (48, 40), (34, 52), (130, 66))):
        for j in range(3):
            seed = 10 * k + j
            out.append(("seed%d" % seed, make_tile(seed, w, h, phase=(seed + k) % 2,
                                                   white=WHITES[j], prescale=PRESCALES[(k + j) % 4],
                                                   precision=(16, 12, 8)[j],
                                                   low=((0, 65536), (0, 4096), (0, 256))[j])))
    # every row of the book with both signs (quant 1; a band of level 1 of a 132 x 100 image)
    rng = np.random.default_rng(0xB00C)
    t = make_tile(100, 132, 100, prescale=PRESCALES[1])
    t.set_band(0, 1, 1, every_row_band(rng, *t.dims()[1]), 1)
    t.set_band(3, 1, 3, every_row_band(rng, *t.dims()[1]), -3)
    by_value, by_run, _ = _rows_by_key()
    w1, h1 = t.dims()[1]  # every zero run of the book, one after the other
    syms = [(by_run[r], False) for r in RUNS] + [(by_value[5], True)]
    t.set_band(1, 1, 2, quant=7, stream=encode_symbols(syms + symbols_of(np.zeros(w1 * h1 - sum(RUNS) - 1))))
    out.append(("every_row", t))
    # the log table end to end: a ramp through the low-pass bands, chroma at 2048
    for white in WHITES:
        t = Tile(512, 384, 0, white)
        t.prescale = [[2, 2, 2]] * 4
        d = t.dims()
        w3, h3 = d[3]
        ramp = np.linspace(0, 4400, w3 * h3).reshape(h3, w3)
        for c in range(4):
            t.set_lowpass(c, ramp if c == 0 else np.full((h3, w3), 2048), 16)
            for level in (1, 2, 3):
                for band in (1, 2, 3):
                    v = np.zeros(d[level][::-1], np.int64)
                    if c == 0 and level == 1:
                        v = random_band(np.random.default_rng(white + band), *d[level], 0.05, 3)
                    t.set_band(c, level, band, v, 2)
        out.append(("ramp%d" % white, t))
    return out


def failing_cases():
    """[(name, Tile, expected status)]: one damaged band each, through the container (chunks
    are whole numbers of 4 bytes there)"""
    out = []
    by_value, by_run, marker = _rows_by_key()
    for k, (c, level, band) in enumerate(((0, 3, 1), (2, 2, 2), (3, 1, 3))):
        w, h = 48, 40
        wk, hk = dims(w, h)[level]
        n = wk * hk
        rng = np.random.default_rng([0xBAD, k])
        vals = random_band(rng, wk, hk, 0.3)
        syms = symbols_of(vals)
        half = len(syms) // 2

        def add(name, stream, status, quant=3):
            t = make_tile(50 + k, w, h)
            t.set_band(c, level, band, quant=quant, stream=stream)
            out.append(("%s_%d" % (name, k), t, status))

        add("marker_early", encode_symbols(syms[:half] + [(marker, False)] + syms[half:]), MARKER)
        add("marker_missing", encode_symbols(syms, marker=False, tail=Bits().put(0, 40)), MARKER)
        add("negative_marker", encode_symbols(syms + [(marker, True)], marker=False), MARKER)
        add("run_past_end", encode_symbols(symbols_of(vals.ravel()[:n - 5]) + [(by_run[12], False)]), MARKER)
        # (the book is complete: every 26 bits begin a word, so the reference meets no invalid
        # code; the library's test of one uses book_with_hole())
        whole = encode_symbols(syms)
        add("truncated", whole[:max(4, (len(whole) // 2) & ~3)], None)  # (whatever the cut gives)
        big = by_value[int(book_values()[-1])]
        add("range", encode_symbols([(big, False)] + symbols_of(np.zeros(n - 1))), RANGE, quant=33)
    return out


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)
