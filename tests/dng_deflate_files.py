"""Deflate-compressed floating-point DNG tiles (include/rsx.h section 4b): a tile writer, a
bit writer for hand-assembled deflate blocks, and the Python model of
DeflateDecompressor::decode (decompressors/DeflateDecompressor.cpp:49-176).

The model inflates with Python's zlib -- libz, the routine the reference calls -- and takes the
widening of binary16 / binary24 from the oracle's F32 unpack, not from a restatement here.
All geometry is in samples: geom = (tile_w, tile_h, off_x, off_y, width, height).
"""
import struct
import zlib

import numpy as np

from rawspeed_amd import abi

OK, SHORT, FAIL = 0, 1, 2
PREDICTORS = {3: 1, 34894: 2, 34895: 4}
BPS = (16, 24, 32)
# the library's status for a verdict
STATUS = {OK: abi.RSX_OK, SHORT: abi.RSX_ERR_UNSUPPORTED, FAIL: abi.RSX_ERR_IO}


# --------------------------------------------------------------------------- writer
def random_samples(rng, bps, h, w, kind="mixed"):
    """(h, w) narrow samples as uint32: 'smooth' compresses, 'bits' is every pattern (NaNs,
    infinities, subnormals), 'mixed' is smooth with patterns planted"""
    top = 1 << bps
    if kind == "bits":
        return rng.integers(0, top, (h, w), dtype=np.uint64).astype(np.uint32)
    x, y = np.arange(w)[None, :], np.arange(h)[:, None]
    f = (0.25 + 0.001 * x + 0.002 * y + rng.normal(0, 0.0005, (h, w))).astype(np.float32)
    s = narrow_from_floats(f, bps)
    if kind == "mixed" and s.size >= 8:
        flat = s.reshape(-1)
        n = max(1, flat.size // 16)
        flat[rng.integers(0, flat.size, n)] = rng.integers(0, top, n, dtype=np.uint64).astype(np.uint32)
        frac = {16: 10, 24: 16, 32: 23}[bps]
        # subnormals, infinities and NaNs of the narrow format
        specials = [1, (1 << frac) - 1, ((1 << (bps - 1 - frac)) - 1) << frac,
                    (((1 << (bps - 1 - frac)) - 1) << frac) | 5, 1 << (bps - 1), 0]
        for k, v in enumerate(specials):
            flat[(k * 7919) % flat.size] = v
    return s


def narrow_from_floats(f, bps):
    """float32 -> the narrow format's bits (bps 24: truncated, normal range only)"""
    f = np.ascontiguousarray(f, dtype=np.float32)
    if bps == 32:
        return f.view(np.uint32).copy()
    if bps == 16:
        return f.astype(np.float16).view(np.uint16).astype(np.uint32)
    u = f.view(np.uint32)
    sign, exp, frac = u >> 31, (u >> 23) & 0xFF, u & 0x7FFFFF
    e = np.clip(exp.astype(np.int64) - 127 + 63, 1, 126).astype(np.uint32)
    out = (sign << 23) | (e << 16) | (frac >> 7)
    return np.where(exp == 0, sign << 23, out).astype(np.uint32)


def tile_bytes(samples, bps, pf):
    """(tile_h, tile_w) narrow samples -> the bytes deflate sees: per row the byte planes, most
    significant first, then b[col] -= b[col - pf] from the end of the row down"""
    bytesps = bps // 8
    s = np.asarray(samples, dtype=np.uint32)
    planes = [((s >> (8 * (bytesps - 1 - c))) & 0xFF).astype(np.uint8) for c in range(bytesps)]
    rows = np.concatenate(planes, axis=1)
    if rows.shape[1] > pf:
        d = rows.copy()
        d[:, pf:] = rows[:, pf:] - rows[:, :-pf]
        rows = d
    return rows.tobytes()


def compress(raw, level=6, wbits=15, strategy=zlib.Z_DEFAULT_STRATEGY, sync_at=None,
             flush_then_finish=False):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    if sync_at is None:
        out = c.compress(raw)
    else:
        out = c.compress(raw[:sync_at]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(raw[sync_at:])
    if flush_then_finish:
        out += c.flush(zlib.Z_FULL_FLUSH)
    return out + c.flush()


def write_tile(samples, bps, predictor, cpp, **kw):
    return compress(tile_bytes(samples, bps, PREDICTORS[predictor] * cpp), **kw)


# --------------------------------------------------------------------------- bit writer
class BitWriter:
    """LSB-first bits, as deflate packs them; Huffman codes go in most significant bit first"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value, n):
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):
        self.bits(int(format(code, "0%db" % n)[::-1], 2) if n else 0, n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def bytes(self, b):
        assert self.n == 0
        self.out += b

    def done(self):
        self.align()
        return bytes(self.out)


def canonical(lengths):
    """{symbol: (code, length)} of the canonical code of `lengths` (RFC 1951 3.2.2)"""
    codes, code = {}, 0
    for n in range(1, 16):
        for s, l in enumerate(lengths):
            if l == n:
                codes[s] = (code, n)
                code += 1
        code <<= 1
    return codes


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115,
            131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537,
             2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def length_symbol(n):
    k = max(i for i in range(29) if LEN_BASE[i] <= n and (i == 28) == (n == 258))
    return 257 + k, n - LEN_BASE[k], LEN_EXTRA[k]


def dist_symbol(d):
    k = max(i for i in range(30) if DIST_BASE[i] <= d)
    return k, d - DIST_BASE[k], DIST_EXTRA[k]


def dynamic_block(w, lit_lens, dist_lens, ops, last=True, cl_syms=None, cl_lens=None,
                  hlit=None, hdist=None):
    """One dynamic block into BitWriter `w`.  ops: ints (literals), (length, distance) pairs,
    ('raw', symbol) / ('rawdist', length, code, extra, nbits); the end-of-block code is added
    when the set has one.  cl_syms: the code length symbols [(sym, extra value)] instead of the
    plain one-per-length coding; cl_lens: the code length code's own lengths."""
    hlit = len(lit_lens) if hlit is None else hlit
    hdist = len(dist_lens) if hdist is None else hdist
    if cl_syms is None:
        cl_syms = [(l, 0) for l in list(lit_lens) + list(dist_lens)]
    if cl_lens is None:
        used = sorted({s for s, _ in cl_syms})
        width = max(1, (len(used) - 1).bit_length())
        cl_lens = [width if s in used else 0 for s in range(19)]
        if len(used) == 1:
            cl_lens[(used[0] + 1) % 19] = 1  # (a complete code of two)
            cl_lens[used[0]] = 1
        else:
            # complete: give the spare codes to symbols nobody uses
            spare = (1 << width) - len(used)
            for s in range(19):
                if spare and cl_lens[s] == 0:
                    cl_lens[s] = width
                    spare -= 1
    w.bits(1 if last else 0, 1)
    w.bits(2, 2)
    w.bits(hlit - 257, 5)
    w.bits(hdist - 1, 5)
    ordered = [cl_lens[s] for s in CL_ORDER]
    while len(ordered) > 4 and ordered[-1] == 0:
        ordered.pop()
    w.bits(len(ordered) - 4, 4)
    for l in ordered:
        w.bits(l, 3)
    cl = canonical(cl_lens)
    for s, extra in cl_syms:
        w.code(*cl[s])
        if s >= 16:
            w.bits(extra, {16: 2, 17: 3, 18: 7}[s])
    lit, dist = canonical(lit_lens), canonical(dist_lens)
    for op in ops:
        if isinstance(op, int):
            w.code(*lit[op])
        elif op[0] == "raw":
            w.code(*lit[op[1]])
        elif op[0] == "rawdist":
            sym, ev, en = length_symbol(op[1])
            w.code(*lit[sym])
            w.bits(ev, en)
            w.code(*dist[op[2]])
            w.bits(op[3], op[4])
        else:
            sym, ev, en = length_symbol(op[0])
            w.code(*lit[sym])
            w.bits(ev, en)
            k, dv, dn = dist_symbol(op[1])
            w.code(*dist[k])
            w.bits(dv, dn)
    if 256 in lit:
        w.code(*lit[256])


def fixed_block(w, ops, last=True):
    lit_lens = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
    lit, dist = canonical(lit_lens), canonical([5] * 32)
    w.bits(1 if last else 0, 1)
    w.bits(1, 2)
    for op in ops:
        if isinstance(op, int):
            w.code(*lit[op])
        elif op[0] == "raw":
            w.code(*lit[op[1]])
        elif op[0] == "rawdist":
            sym, ev, en = length_symbol(op[1])
            w.code(*lit[sym])
            w.bits(ev, en)
            w.code(*dist[op[2]])
            w.bits(op[3], op[4])
        else:
            sym, ev, en = length_symbol(op[0])
            w.code(*lit[sym])
            w.bits(ev, en)
            k, dv, dn = dist_symbol(op[1])
            w.code(*dist[k])
            w.bits(dv, dn)
    w.code(*lit[256])


def stored_block(w, data, last=False):
    w.bits(1 if last else 0, 1)
    w.bits(0, 2)
    w.align()
    w.bytes(struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + data)


def expand(ops, start=b""):
    """what literal / (length, distance) ops produce behind `start`"""
    out = bytearray(start)
    for op in ops:
        if isinstance(op, int):
            out.append(op)
        elif isinstance(op[0], str):
            break  # (a symbol no stream may hold: nothing behind it counts)
        else:
            n, d = op
            if d > len(out):
                break  # (a distance no stream may hold)
            for _ in range(n):
                out.append(out[-d])
    return bytes(out)


def zlib_wrap(deflate, raw, cmf=0x78):
    flg = (31 - (cmf * 256) % 31) % 31
    return bytes([cmf, flg]) + deflate + struct.pack(">I", zlib.adler32(raw))


# --------------------------------------------------------------------------- model
def inflate_verdict(data, dst_len):
    """libz's verdict on uncompress(buf, &dst_len, data): OK (Z_OK and exactly dst_len bytes),
    SHORT (Z_OK and fewer), FAIL; the bytes; the stream's length"""
    d = zlib.decompressobj()
    try:
        out = d.decompress(bytes(data), dst_len + 1)
    except zlib.error:
        return FAIL, b"", 0
    if not d.eof or len(out) > dst_len:
        return FAIL, b"", 0
    used = len(data) - len(d.unused_data)
    return (OK if len(out) == dst_len else SHORT), out, used


def constructor_status(bps, predictor, geom, in_bytes, pitch, dim_x, dim_y, cpp):
    """the checks of DngDecoder / DeflateDecompressor / the image window, in the reference's
    order, as the library's status (rsx_dng_deflate_validate)"""
    tile_w, tile_h, off_x, off_y, width, height = geom
    if bps not in BPS:
        return abi.RSX_ERR_INVALID_ARG
    if predictor not in PREDICTORS:
        return abi.RSX_ERR_INVALID_ARG
    if not 1 <= cpp <= 4 or dim_x <= 0 or dim_y <= 0 or pitch % 4:
        return abi.RSX_ERR_INVALID_ARG
    if min(tile_w, tile_h, width, height) == 0 or width > tile_w or height > tile_h:
        return abi.RSX_ERR_INVALID_ARG
    if off_x + width > dim_x * cpp or off_y + height > dim_y:
        return abi.RSX_ERR_INVALID_ARG
    if pitch < 4 * cpp * dim_x:
        return abi.RSX_ERR_INVALID_ARG
    if in_bytes >= 1 << 32 or (bps // 8) * tile_w * tile_h >= 1 << 32:
        return abi.RSX_ERR_UNSUPPORTED
    return abi.RSX_OK


_oracle = None


def widen(narrow, bps):
    """narrow samples (any shape, uint32) -> binary32 bits, by the oracle's F32 unpack"""
    global _oracle
    narrow = np.asarray(narrow, dtype=np.uint32)
    if bps == 32:
        return narrow.copy()
    from oracle_lib import HostImage, Oracle
    if _oracle is None:
        _oracle = Oracle()
    flat = narrow.reshape(-1)
    n = max(8, flat.size)
    bytesps = bps // 8
    be = np.zeros((n, bytesps), dtype=np.uint8)
    for c in range(bytesps):
        be[:flat.size, c] = (flat >> (8 * (bytesps - 1 - c))) & 0xFF
    img = HostImage(n, 1, 1, bpc=4)
    d = abi.UnpackDesc(0, 0, n, 1, n * bytesps, bps, abi.ORDER_MSB)
    st = _oracle.unpack_f32(d, be.reshape(-1), img)
    assert st == 0, st
    return img.u32()[0, :flat.size].reshape(narrow.shape).copy()


def model_decode(data, bps, predictor, cpp, geom):
    """-> (verdict, (height, width) binary32 bits or None, bytes consumed)"""
    tile_w, tile_h, off_x, off_y, width, height = geom
    bytesps, pf = bps // 8, PREDICTORS[predictor] * cpp
    verdict, raw, used = inflate_verdict(data, bytesps * tile_w * tile_h)
    if verdict != OK:
        return verdict, None, used
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(tile_h, bytesps * tile_w)[:height].copy()
    for r in range(pf):  # b[col] += b[col - pf]: a running sum per residue class
        rows[:, r::pf] = np.cumsum(rows[:, r::pf], axis=1, dtype=np.uint8)
    s = np.zeros((height, width), dtype=np.uint32)
    for c in range(bytesps):
        s = (s << 8) | rows[:, c * tile_w:c * tile_w + width]
    return OK, widen(s, bps), used


def paste(img_u32, geom, bits):
    tile_w, tile_h, off_x, off_y, width, height = geom
    img_u32[off_y:off_y + height, off_x:off_x + width] = bits


# --------------------------------------------------------------------------- corpora
def small_valid_tiles(seed=11):
    """[(name, bps, predictor, cpp, geom, data)]: small tiles (<= 4 KiB inflated) of every depth
    and predictor, written at several levels and strategies"""
    rng = np.random.default_rng(seed)
    out = []
    k = 0
    for bps in BPS:
        for predictor in PREDICTORS:
            for cpp in (1, 3):
                tw, th = (21 if cpp == 1 else 15), 5 + k % 3
                kind = ("smooth", "mixed", "bits")[k % 3]
                s = random_samples(rng, bps, th, tw, kind)
                level, strategy = ((6, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY),
                                   (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED),
                                   (6, zlib.Z_HUFFMAN_ONLY), (6, zlib.Z_RLE),
                                   (0, zlib.Z_DEFAULT_STRATEGY))[k % 7]
                data = write_tile(s, bps, predictor, cpp, level=level, strategy=strategy,
                                  sync_at=(17 if k % 4 == 1 else None))
                out.append(("b%d_p%d_c%d_%s_l%d_s%d" % (bps, predictor, cpp, kind, level, strategy),
                            bps, predictor, cpp, (tw, th, 0, 0, tw, th), data))
                k += 1
    return out


def mutants(seed=5, per_tile=18):
    """single-byte mutants of small_valid_tiles(): [(bps, predictor, cpp, geom, data)].  Both
    verdicts occur: a flipped bit in a stored block's bytes or a literal fails the Adler-32, one
    in the unused bits before a stored block's LEN changes nothing."""
    rng = np.random.default_rng(seed)
    out = []
    for name, bps, predictor, cpp, geom, data in small_valid_tiles():
        for j in range(per_tile):
            d = bytearray(data)
            if j == 0:
                pass  # (the tile itself)
            elif j == 1:
                d += b"\x00"  # (a byte behind the stream)
            else:
                at = int(rng.integers(0, len(d)))
                d[at] ^= 1 << int(rng.integers(0, 8))
            out.append((bps, predictor, cpp, geom, bytes(d)))
    return out


def _wrap_ops(blocks, cmf=0x78):
    """blocks: [('stored', bytes) | ('fixed', ops) | ('dynamic', kwargs)] -> (stream, raw)"""
    w, raw = BitWriter(), b""
    for i, (kind, arg) in enumerate(blocks):
        last = i + 1 == len(blocks)
        if kind == "stored":
            stored_block(w, arg, last)
            raw += arg
        elif kind == "fixed":
            fixed_block(w, arg, last)
            raw = expand(arg, raw)
        else:
            dynamic_block(w, last=last, **arg)
            raw = expand(arg["ops"], raw)
    return zlib_wrap(w.done(), raw, cmf), raw


def hand_streams(seed=23):
    """Hand-assembled streams: [(name, data, dst_len, verdict the case is made for)].  The verdict
    the tests hold the decoders to is libz's (inflate_verdict); the last field says what the
    case was built to be, and the tests check that libz agrees."""
    rng = np.random.default_rng(seed)
    noise = rng.integers(0, 256, 40000, dtype=np.uint8).tobytes()
    out = []

    def add(name, blocks, expect=OK, dst=None, cmf=0x78):
        data, raw = _wrap_ops(blocks, cmf)
        # (a stream that gives nothing still belongs to a tile: of four bytes)
        out.append((name, data, (len(raw) or 4) if dst is None else dst, expect))
        return data, raw

    add("distance_32768", [("stored", noise[:32768]), ("fixed", [(258, 32768), 7, (3, 32768)])])
    add("distance_32768_late", [("stored", noise[:40000]), ("fixed", [(258, 32768), (258, 32768), 9, 9])])
    add("length_258_distance_1", [("fixed", [65, (258, 1), (258, 1), 66])])
    add("distance_below_length", [("fixed", [65, 66, 67, (258, 3), (100, 2), (17, 5), (4, 3)])])
    # 15-bit codes: lengths 1 .. 14, 15, 15 over sixteen symbols, the end-of-block code among them
    lit = [0] * 257
    for k in range(14):
        lit[65 + k] = k + 1
    lit[100], lit[256] = 15, 15
    add("codes_of_15_bits", [("dynamic", dict(lit_lens=lit, dist_lens=[1, 1],
                                              ops=[65, 78, 100, 100, 77, 100, 71, 66]))])
    # repeat codes 16, 17 and 18, a run of equal lengths across the literal/distance boundary
    lit = [0] * 258
    lit[97] = lit[98] = lit[256] = lit[257] = 2
    add("repeats_across_the_boundary",
        [("dynamic", dict(lit_lens=lit, dist_lens=[2, 2, 2, 2], ops=[97, 98, (3, 2), (3, 4), 97],
                          cl_syms=[(18, 86), (2, 0), (2, 0), (18, 127), (17, 7), (17, 6), (2, 0), (16, 2)]))])
    lit = [0] * 258
    lit[97] = lit[98] = lit[256] = lit[257] = 2
    add("one_distance_code", [("dynamic", dict(lit_lens=lit, dist_lens=[1], ops=[97, (3, 1), 98, (3, 1)]))])
    lit = [0] * 257
    lit[97] = 1
    lit[256] = 1
    add("no_distance_code", [("dynamic", dict(lit_lens=lit, dist_lens=[0], ops=[97, 97, 97]))])
    add("empty_stored_blocks_behind_full_output",
        [("fixed", [1, 2, 3]), ("stored", b""), ("stored", b""), ("fixed", [])])
    # --- what libz rejects
    lit = [0] * 258
    lit[97] = lit[98] = lit[256] = lit[257] = 2
    out.append(("the_unused_half_of_one_distance_code", _flip_distance_bit(), 4, FAIL))
    lit = [0] * 257
    lit[97] = lit[98] = lit[256] = 1
    add("over_subscribed", [("dynamic", dict(lit_lens=lit, dist_lens=[1, 1], ops=[]))], FAIL)
    lit = [0] * 257
    lit[97] = lit[256] = 2
    add("incomplete", [("dynamic", dict(lit_lens=lit, dist_lens=[1, 1], ops=[97]))], FAIL, 4)
    lit = [0] * 257
    lit[97] = lit[98] = 1
    add("no_end_of_block_code", [("dynamic", dict(lit_lens=lit, dist_lens=[1, 1], ops=[97]))], FAIL, 4)
    lit = [0] * 258
    lit[97] = lit[98] = lit[256] = lit[257] = 2
    add("repeat_with_nothing_to_repeat",
        [("dynamic", dict(lit_lens=lit, dist_lens=[2, 2, 2, 2], ops=[],
                          cl_syms=[(16, 0), (18, 83), (2, 0), (2, 0), (18, 127), (17, 7), (17, 6), (2, 0), (16, 2)]))],
        FAIL)
    add("repeat_past_the_end",
        [("dynamic", dict(lit_lens=lit, dist_lens=[2, 2, 2, 2], ops=[],
                          cl_syms=[(18, 86), (2, 0), (2, 0), (18, 127), (17, 7), (17, 6), (2, 0), (16, 3)]))],
        FAIL)
    add("hlit_287", [("dynamic", dict(lit_lens=lit, dist_lens=[2, 2, 2, 2], ops=[], hlit=287))], FAIL)
    add("hdist_31", [("dynamic", dict(lit_lens=lit, dist_lens=[2, 2, 2, 2], ops=[], hdist=31))], FAIL)
    add("literal_286_in_a_fixed_block", [("fixed", [65, ("raw", 286)])], FAIL, 4)
    add("distance_code_30", [("fixed", [65, ("rawdist", 3, 30, 0, 0)])], FAIL, 4)
    add("distance_before_the_start", [("fixed", [65, (3, 2)])], FAIL, 4)
    data, raw = _wrap_ops([("fixed", [65, 66, 67, (24, 3)])])
    out.append(("one_byte_too_long", data, len(raw) - 1, FAIL))
    out.append(("one_byte_short", data, len(raw) + 1, SHORT))
    out.append(("no_input", b"", 4, FAIL))
    out.append(("flipped_checksum_bit", data[:-2] + bytes([data[-2] ^ 4]) + data[-1:], len(raw), FAIL))
    out.append(("fdict", bytes([0x78, 0xBB]) + data[2:], len(raw), FAIL))
    out.append(("cm_7", zlib_wrap(data[2:-4], raw, 0x77), len(raw), FAIL))
    out.append(("window_above_15", zlib_wrap(data[2:-4], raw, 0x88), len(raw), FAIL))
    out.append(("window_9", zlib_wrap(data[2:-4], raw, 0x18), len(raw), OK))
    out.append(("bad_fcheck", bytes([data[0], data[1] ^ 1]) + data[2:], len(raw), FAIL))
    w = BitWriter()
    w.bits(1, 1)
    w.bits(3, 2)
    out.append(("btype_3", zlib_wrap(w.done(), b""), 4, FAIL))
    w = BitWriter()
    stored_block(w, b"abcd", True)
    bad = bytearray(w.done())
    bad[3] ^= 0x10
    out.append(("len_not_nlen", zlib_wrap(bytes(bad), b"abcd"), 4, FAIL))
    # truncation: inside the header, a dynamic header, the symbols and the Adler-32
    dyn = compress(bytes(rng.integers(0, 7, 3000, dtype=np.uint8)), 6)
    for cut in (1, 2, 3, 5, 9, 20, 40, len(dyn) // 2, len(dyn) - 5, len(dyn) - 4, len(dyn) - 2, len(dyn) - 1):
        out.append(("truncated_at_%d" % cut, dyn[:cut], 3000, FAIL))
    out.append(("whole", dyn, 3000, OK))
    out.append(("bytes_behind_the_stream", dyn + b"\x01\x02\x03", 3000, OK))
    return out


def _flip_distance_bit():
    """a literal, then a length 3 whose distance bit is 1: the code 1 of a one-code distance set,
    which no symbol has"""
    lit = [0] * 258
    lit[97] = lit[98] = lit[256] = lit[257] = 2
    w2 = BitWriter()
    lits = canonical(lit)
    dynamic_block(w2, lit, [1], [97], last=True)
    # drop the end-of-block code (2 bits) and append: length 3, distance bit 1, end of block
    total_bits = len(w2.out) * 8 + w2.n - 2
    bits = int.from_bytes(bytes(w2.out) + bytes([w2.acc]), "little") & ((1 << total_bits) - 1)
    w3 = BitWriter()
    w3.bits(bits, total_bits)
    w3.code(*lits[257])
    w3.bits(1, 1)
    w3.code(*lits[256])
    return zlib_wrap(w3.done(), b"aaaa")


def inflate_shapes(seed=31):
    """[(name, data, dst_len)]: valid streams of many shapes (sizes around the 32 KiB window,
    levels, strategies, window sizes, flushes)"""
    rng = np.random.default_rng(seed)
    out = []

    def field(n):
        return ((np.cumsum(rng.integers(-2, 3, n)) >> 2) % 256).astype(np.uint8).tobytes()

    for n in (2, 32760, 32776, 192 * 128 * 4):
        raw = field(n)
        out.append(("size_%d" % n, compress(raw, 6), n))
    raw = field(150000)
    out.append(("level_0_stored_blocks", compress(raw, 0), len(raw)))
    out.append(("level_0_noise", compress(rng.integers(0, 256, 70000, dtype=np.uint8).tobytes(), 0), 70000))
    raw = field(50000)
    for level in (1, 6, 9):
        out.append(("level_%d" % level, compress(raw, level), len(raw)))
    for name, strategy in (("fixed", zlib.Z_FIXED), ("huffman_only", zlib.Z_HUFFMAN_ONLY), ("rle", zlib.Z_RLE)):
        out.append((name, compress(raw, 6, strategy=strategy), len(raw)))
    for wbits in (9, 15):
        out.append(("wbits_%d" % wbits, compress(raw, 6, wbits=wbits), len(raw)))
    out.append(("sync_flush_mid_stream", compress(raw, 6, sync_at=12345), len(raw)))
    out.append(("flush_then_finish", compress(raw, 6, flush_then_finish=True), len(raw)))
    out.append(("bytes_behind", compress(raw, 6) + b"tail", len(raw)))
    out.append(("text", compress(b"the quick brown fox " * 3000, 9), 60000))
    out.append(("zeros", compress(bytes(100000), 9), 100000))
    return out
