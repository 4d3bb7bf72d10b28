"""Compressed ORF (OlympusDecompressor) test material: an independent pure-Python model of the
codec -- a decoder with the reference's reader bookkeeping and reach statistics, and, run forward,
an encoder from target pixels and one from planted raw symbols --, a mirror of the parse kernel's
window bookkeeping with its constants read out of rsx_olympus.hip, the case list, the builders of
the cases' streams (through the C writer of rawspeed_amd/csrc/synth or through the model), the
host build's wrapper and the golden file's reader and writer.

  python tests/olympus_files.py --write-cases FILE    the case file of scripts/record_olympus_ref.cpp
                                                      and of rsx_olympus_host_check
  python tests/olympus_files.py --golden LINES        tests/golden/olympus_ref.json from the
                                                      recorder's lines, unless the model disagrees
"""
import collections
import functools
import hashlib
import json
import os
import random
import re
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "olympus_ref.json")

OK, ERR_INVALID_ARG, ERR_IO, ERR_INPUT_OVERFLOW = 0, 1, 2, 5
MAX_X, MAX_Y = 10400, 7792
SKIP = 7

# what tests/test_olympus_model.py wants counted at least once over the case list
REACH_ITEMS = ("c2_2_to_3", "c0_is_16", "c0_is_17", "truncation_changes_low_bits",
               "escape_high_bits_1", "escape_high_bits_13", "symbol_31_bits",
               "negative_carry1_rounds_down", "row_start_off_byte")
REACH_PRED = ("zero", "left", "up", "opposite_at_32", "opposite_at_33", "opposite_far",
              "opposite_near", "a_zero", "b_zero", "abs_equal", "same_a_greater", "same_a_less",
              "wrap_above", "wrap_below")
# L + (U - NW) with L - NW and U - NW of opposite signs lies between U and L: it cannot leave
# 0..65535, so "l_plus_b_out_of_range" is asserted to stay at zero


def _status_codes():
    from rawspeed_amd import abi
    assert (abi.RSX_OK, abi.RSX_ERR_INVALID_ARG, abi.RSX_ERR_IO, abi.RSX_ERR_INPUT_OVERFLOW) == \
        (OK, ERR_INVALID_ARG, ERR_IO, ERR_INPUT_OVERFLOW)


# ---------------------------------------------------------------------------------------------
# The model
# ---------------------------------------------------------------------------------------------
def validate(in_bytes, w, h, pitch=None):
    """the constructor's checks, the pitch, then the reader's refusals before the first bit"""
    if w <= 0 or h <= 0 or w % 2 or h % 2 or w > MAX_X or h > MAX_Y:
        return ERR_INVALID_ARG
    if pitch is not None and pitch < 2 * w:
        return ERR_INVALID_ARG
    if in_bytes < SKIP or in_bytes - SKIP < 4:
        return ERR_IO
    return OK


def low_bits(c0, c2):
    bias = 2 if c2 < 3 else 0
    return max((c0 & 0xFFFF).bit_length() - bias, 2 + bias)


def fill_fails(consumed, size):
    """the closed form of the over-read rule: a fill(32) with `consumed` bits taken"""
    return 4 * ((consumed + 31) // 32) > size + 8


def predict(px, row, col, stats=None):
    if row < 2 and col < 2:
        if stats is not None:
            stats["zero"] += 1
        return 0
    if row < 2:
        if stats is not None:
            stats["left"] += 1
        return int(px[row][col - 2])
    if col < 2:
        if stats is not None:
            stats["up"] += 1
        return int(px[row - 2][col])
    left, up, nw = int(px[row][col - 2]), int(px[row - 2][col]), int(px[row - 2][col - 2])
    a, b = left - nw, up - nw
    if (a < 0) != (b < 0) and a != 0 and b != 0:
        far = abs(a) > 32 or abs(b) > 32
        if stats is not None:
            m = max(abs(a), abs(b))
            stats["opposite_far" if far else "opposite_near"] += 1
            if m in (32, 33):
                stats["opposite_at_%d" % m] += 1
            if far and not 0 <= left + b <= 65535:
                stats["l_plus_b_out_of_range"] += 1
        return left + b if far else (left + up) >> 1
    if stats is not None:
        key = ("a_zero" if a == 0 else "b_zero" if b == 0 else "abs_equal" if abs(a) == abs(b)
               else "same_a_greater" if abs(a) > abs(b) else "same_a_less")
        stats[key] += 1
        if a == 0 and b == 0:
            stats["b_zero"] += 1
    return left if abs(a) > abs(b) else up


@functools.lru_cache(maxsize=None)
def kernel_constants():
    """OL_WIN_REGS, OL_BATCH and OL_BATCH_WORDS as rsx_olympus.hip states them (the expression
    evaluated, not retyped) and OL_WIN_WORDS, 64 words a window register"""
    path = os.path.join(os.path.dirname(HERE), "rawspeed_amd", "csrc", "rsx_olympus.hip")
    src = open(path).read()
    text = {n: re.search(r"constexpr int %s = ([^;]+);" % n, src).group(1)
            for n in ("OL_WIN_REGS", "OL_BATCH", "OL_BATCH_WORDS", "OL_WIN_WORDS")}
    assert text["OL_WIN_WORDS"].replace(" ", "") == "64*OL_WIN_REGS"
    k = dict(OL_WIN_REGS=int(text["OL_WIN_REGS"]), OL_BATCH=int(text["OL_BATCH"]))
    expr = re.sub(r"OL_\w+", lambda m: str(k[m.group(0)]), text["OL_BATCH_WORDS"])
    assert re.fullmatch(r"[\s0-9()+*/-]+", expr), expr
    k["OL_BATCH_WORDS"] = eval(expr.replace("/", "//"))
    k["OL_WIN_WORDS"] = 64 * k["OL_WIN_REGS"]
    return k


def window_top():
    """-> (the highest batch-start offset k - k0 that goes without a reload, the highest window
    index a fill can load).  A batch reloads iff k - k0 + OL_BATCH_WORDS > OL_WIN_WORDS, so it
    starts at offset OL_WIN_WORDS - OL_BATCH_WORDS at most.  Behind a symbol the cache holds at
    least one bit, so every batch but a stream's first (which starts at offset 0) starts with
    level >= 1; its last fill stands in front of its last symbol, behind OL_BATCH - 1 symbols of at
    most 31 bits, and leaves a level of at most 63.  With n words loaded:
    1 + 32 n - 31 (OL_BATCH - 1) <= 63, which for OL_BATCH = 64 is 32 n <= 63 * 31 + 63 - 1 and
    n <= 62.  The stream's first batch loads one more at most, from offset 0."""
    k = kernel_constants()
    start = k["OL_WIN_WORDS"] - k["OL_BATCH_WORDS"]
    words = (31 * (k["OL_BATCH"] - 1) + 63 - 1) // 32
    return start, start + words - 1


class Window:
    """olympus_parse_kernel's window bookkeeping (k, k0, the reload rule in front of every batch of
    OL_BATCH symbols of a row) beside the model's reader: which batch-start offsets k - k0 occur,
    which window indices a fill loads, which of them with a non-zero word, and the stream's tail.
    The model stops at a failing fill where the kernel finishes its batch on zeros."""
    TOP = 224  # (the upper half of the window's last register)

    def __init__(self):
        k = kernel_constants()
        self.batch_syms, self.batch_words, self.win_words = \
            k["OL_BATCH"], k["OL_BATCH_WORDS"], k["OL_WIN_WORDS"]
        self.k0 = None
        self.starts, self.loaded, self.nonzero = set(), set(), set()
        self.reloads = []             # (k - k0 in front of a reload, words its batch then loaded)
        self._reloaded = None
        self.nonzero_top = 0          # words loaded at index TOP or above that were not zero
        self.past_end = False         # bits behind the stream's last byte were consumed
        self.partial_nonzero = False  # ... and size % 4 != 0 with a non-zero byte in the last word
        self.residue = None           # size % 4

    def batch(self, k):
        self._close(k)
        if self.k0 is None:
            self.k0 = k
        elif k - self.k0 + self.batch_words > self.win_words:
            self._reloaded = (k - self.k0, k)
            self.k0 = k
        self.starts.add(k - self.k0)

    def _close(self, k):
        if self._reloaded is not None:
            self.reloads.append((self._reloaded[0], k - self._reloaded[1]))
        self._reloaded = None

    def late_reload_overruns(self, late):
        """whether a reload rule `late` words too lenient would let a batch of this stream run
        past the window: a batch that reloads at an offset the lenient rule lets pass, and then
        loads more words than the window holds behind that offset"""
        start = self.win_words - self.batch_words
        return any(at <= start + late and at + words > self.win_words for at, words in self.reloads)

    def load(self, k, word):
        j = k - self.k0
        assert 0 <= j < self.win_words, "the walk outran its window"
        self.loaded.add(j)
        if word:
            self.nonzero.add(j)
            self.nonzero_top += j >= self.TOP

    def tail(self, bits, pos, k):
        self._close(k)
        size = len(bits)
        self.residue = size % 4
        self.past_end = pos > 8 * size
        self.partial_nonzero = self.past_end and size % 4 != 0 and any(bits[size - size % 4:])


def decode(data, w, h, stats=None, win=None):
    """-> (status, (h, w) uint16 pixels or None).  The reader keeps the reference's books (words
    loaded, fill level), not the closed form; `stats` (a Counter) gets the reach statistics, `win`
    (a Window) the kernel's window bookkeeping."""
    st = validate(len(data), w, h)
    if st != OK:
        return st, None
    bits = bytes(data[SKIP:])
    size = len(bits)
    padded = bits + bytes(16)
    pos, loaded, level = 0, 0, 0
    px = [[0] * w for _ in range(h)]
    batch = win.batch_syms if win is not None else 0
    for row in range(h):
        carry = [[0, 0, 0], [0, 0, 0]]
        if stats is not None and pos % 8:
            stats["row_start_off_byte"] += 1
        prow = px[row]
        for col in range(w):
            if win is not None and col % batch == 0:
                win.batch(loaded)
            # fill(32)
            if level < 32:
                if 4 * loaded > size + 8:
                    return ERR_INPUT_OVERFLOW, None
                if win is not None:
                    word = padded[4 * loaded:4 * loaded + 4].ljust(4, b"\0")
                    win.load(loaded, int.from_bytes(word, "big"))
                loaded += 1
                level += 32
            at = pos >> 3
            window = (int.from_bytes(padded[at:at + 5] if at + 5 <= len(padded)
                                     else bytes(5), "big") >> (8 - (pos & 7))) & 0xFFFFFFFF
            c = carry[col & 1]
            n = low_bits(c[0], c[2])
            b = window >> 17
            sign = -(b >> 14)
            low = (b >> 12) & 3
            nlz = 12 - (b & 4095).bit_length()
            if nlz != 12:
                high, used = nlz, nlz + 4
            else:
                nh = 15 - n
                high = (window >> (17 - nh)) & ((1 << nh) - 1)
                used = 16 + nh
            used += n
            field = (window >> (32 - used)) & ((1 << n) - 1)
            c0 = (high << n) | field
            diff = (c0 ^ sign) + c[1]
            t = 3 * diff + c[1]
            if stats is not None:
                stats["low_bits_%d" % n] += 1
                stats["nlz_%d" % nlz] += 1
                bias = 2 if c[2] < 3 else 0
                if max(c[0].bit_length() - bias, 2 + bias) != n:
                    stats["truncation_changes_low_bits"] += 1
                if nlz == 12:
                    stats["escape_high_bits_%d" % (15 - n)] += 1
                if used == 31:
                    stats["symbol_31_bits"] += 1
                if t < 0 and t % 32:
                    stats["negative_carry1_rounds_down"] += 1
                if c0 in (16, 17):
                    stats["c0_is_%d" % c0] += 1
                if c0 <= 16 and c[2] == 2:
                    stats["c2_2_to_3"] += 1
            c[0] = c0
            c[1] = t >> 5
            c[2] = 0 if c0 > 16 else c[2] + 1
            pos += used
            level -= used
            p = predict(px, row, col, stats)
            v = p + ((diff * 4) | low)
            if stats is not None:
                # the difference's representative next to zero decides what counts as a wrap
                d16 = (((diff * 4) | low) + 32768 & 0xFFFF) - 32768
                if p + d16 > 65535:
                    stats["wrap_above"] += 1
                if p + d16 < 0:
                    stats["wrap_below"] += 1
            prow[col] = v & 0xFFFF
    if win is not None:
        win.tail(bits, pos, loaded)
    return OK, np.array(px, dtype=np.uint16).reshape(h, w)


class BitWriter:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, v, bits):
        if bits:
            self.acc = (self.acc << bits) | (v & ((1 << bits) - 1))
            self.n += bits

    def bytes(self):
        pad = -self.n % 8
        return ((self.acc << pad).to_bytes((self.n + pad) // 8, "big")) if self.n else b""


def _emit(bw, n, sign, low, escape, high, field, skipped):
    bw.put(sign, 1)
    bw.put(low, 2)
    if not escape:
        bw.put(1, high + 1)
    else:
        bw.put(0, 12)
        bw.put(high, 15 - n)
        bw.put(skipped, 1)
    bw.put(field, n)


def _flush(bw, chunks):
    # (big-integer accumulators stay short)
    whole = bw.n // 8
    if whole >= 512:
        rest = bw.n - 8 * whole
        chunks.append((bw.acc >> rest).to_bytes(whole, "big"))
        bw.acc &= (1 << rest) - 1
        bw.n = rest


def encode(target):
    """the model run forward over target pixels -> the stream, 7 leading bytes included"""
    target = np.asarray(target, dtype=np.uint16)
    h, w = target.shape
    px = target.tolist()
    bw, chunks = BitWriter(), [bytes(SKIP)]
    for row in range(h):
        carry = [[0, 0, 0], [0, 0, 0]]
        for col in range(w):
            c = carry[col & 1]
            p = predict(px, row, col)
            diff = ((px[row][col] - p + 32768) & 0xFFFF) - 32768
            low = diff & 3
            x = (diff >> 2) - c[1]
            sign = 1 if x < 0 else 0
            c0 = ~x if sign else x
            n = low_bits(c[0], c[2])
            high, field = c0 >> n, c0 & ((1 << n) - 1)
            if high <= 11:
                _emit(bw, n, sign, low, False, high, field, 0)
            elif c0 < 1 << 15:
                _emit(bw, n, sign, low, True, high, field, 1)
            else:
                raise ValueError("an image the stream cannot reach")
            d = (c0 ^ -sign) + c[1]
            c[0], c[1], c[2] = c0, (3 * d + c[1]) >> 5, (0 if c0 > 16 else c[2] + 1)
        _flush(bw, chunks)
    chunks.append(bw.bytes())
    return b"".join(chunks)


def plant(w, h, syms):
    """the model run forward over planted raw symbols (sign, low, escape, high, field, skipped)"""
    bw, chunks = BitWriter(), [bytes(SKIP)]
    k = 0
    for row in range(h):
        carry = [[0, 0, 0], [0, 0, 0]]
        for col in range(w):
            c = carry[col & 1]
            sign, low, escape, high, field, skipped = syms[k] if k < len(syms) else (0,) * 6
            k += 1
            n = low_bits(c[0], c[2])
            if escape:
                high &= (1 << (15 - n)) - 1
            else:
                assert 0 <= high <= 11
            field &= (1 << n) - 1
            _emit(bw, n, sign & 1, low, escape, high, field, skipped)
            c0 = (high << n) | field
            d = (c0 ^ -(sign & 1)) + c[1]
            c[0], c[1], c[2] = c0, (3 * d + c[1]) >> 5, (0 if c0 > 16 else c[2] + 1)
        _flush(bw, chunks)
    chunks.append(bw.bytes())
    return b"".join(chunks)


# ---------------------------------------------------------------------------------------------
# Contents and planted symbol lists
# ---------------------------------------------------------------------------------------------
PRED_PAIRS = ((32, -1), (-1, 32), (-32, 32), (33, -1), (-1, 33), (-33, 2), (0, 5), (5, 0), (0, 0),
              (7, 7), (7, -7), (9, 3), (-9, -3), (3, 9), (-3, -9), (20, -20))


def predictor_plane():
    """two plane rows: per pair (a, b) the cells NW, U above L, X with L - NW = a, U - NW = b"""
    top, bottom = [], []
    for k, (a, b) in enumerate(PRED_PAIRS):
        nw = 1000 + 37 * k
        top += [nw, nw + b]
        bottom += [nw + a, nw + 3 * k]
    return np.array([top, bottom], dtype=np.uint16)


def content(kind, w, h, seed):
    rng = np.random.default_rng(seed)
    pw, ph = w // 2, h // 2
    if kind == "noise12":
        return rng.integers(0, 4096, (h, w), dtype=np.uint16)
    if kind == "noise16":
        return rng.integers(0, 65536, (h, w), dtype=np.uint16)
    if kind.startswith("flat"):
        return np.full((h, w), int(kind[4:]), np.uint16)
    i, j = np.mgrid[0:ph, 0:pw]
    if kind == "checker":
        plane = (4095 * ((i + j) & 1)).astype(np.uint16)
    elif kind == "steps":
        plane = ((j // 3) * 700 % 4096 + (i // 2) * 300 % 2048).astype(np.uint16)
    elif kind == "wrap":
        # next to both ends of the range, so that pred + diff leaves 0..65535 both ways
        plane = np.where((i + 2 * j) % 3 == 0, 65535 - (j % 5), (i + j) % 7).astype(np.uint16)
    elif kind == "predictor":
        plane = predictor_plane()
        assert plane.shape == (ph, pw)
    else:
        raise KeyError(kind)
    img = np.zeros((h, w), np.uint16)
    for pr in (0, 1):
        for pc in (0, 1):
            img[pr::2, pc::2] = plane
    return img


def _reg(high, field, sign=0, low=0):
    return (sign, low, 0, high, field, 0)


def _esc(high, field, sign=0, low=0, skipped=0):
    return (sign, low, 1, high, field, skipped)


_Z = _reg(0, 0)


def _pairs(seq0, seq1=()):
    """a row's symbols from the sequences of the two column parities"""
    out = []
    for k in range(max(len(seq0), len(seq1))):
        out.append(seq0[k] if k < len(seq0) else _Z)
        out.append(seq1[k] if k < len(seq1) else _Z)
    return out


ONES = (1 << 15) - 1
_RAMP = [_reg(11, ONES)] * 6  # numLowBits 4, 6, ... 14; carry[0] 191 ... 196607

PLANTED = {
    # name: (w, h, symbols)
    "low_bits_2": (16, 2, _pairs([_Z] * 6)),
    "low_bits_14": (16, 2, _pairs(_RAMP + [_reg(3, 5)])),
    "bias_switch": (16, 2, _pairs([_reg(1, 0)] * 5, [_reg(0, 9)] * 5)),  # carry[0] 16: 4 -> 5 bits
    "carry0_16_17": (16, 2, _pairs([_reg(1, 0), _reg(1, 0), _reg(1, 1), _reg(1, 0), _reg(1, 0),
                                    _reg(1, 0), _reg(0, 3)])),
    "truncation": (16, 2, _pairs(_RAMP + [_reg(4, 0), _reg(2, 7), _reg(0, 1)],
                                 _RAMP[:5] + [_reg(11, ONES), _reg(1, 3)])),
    "escape_high_1": (16, 2, _pairs(_RAMP + [_esc(1, 12345, sign=1, low=3, skipped=1),
                                             _esc(0, 99, skipped=0)])),
    "escape_high_13": (16, 2, _pairs([_Z] * 4 + [_esc(0x1ABC, 2, low=1, skipped=1),
                                                 _esc(0x0FFF, 1, sign=1)])),
    "symbol_31": (4, 2, [_esc(0x7FF, 15, 1, 3, 1)] * 8),
    "negative_carry1": (16, 2, _pairs([_reg(0, 0, sign=1), _reg(0, 1, sign=1), _reg(2, 3, sign=1),
                                       _reg(0, 0), _reg(5, 2, sign=1)], [_reg(3, 3, sign=1)] * 6)),
    "row_reset_off_byte": (4, 4, [_reg(1, 5), _reg(11, ONES), _reg(11, ONES), _reg(7, 3),
                                  _reg(2, 9), _reg(0, 1), _reg(10, 0), _esc(77, 5)]),
    "every_high": (32, 2, _pairs([_reg(k, k + 1) for k in range(12)],
                                 [_reg(11 - k, 3 * k) for k in range(12)])),
    # numLowBits 5, 7, ... 13 under the bias (carry[0] 64, 256, ... 16384), then 3 without it
    "odd_low_bits": (32, 2, _pairs([_reg(4, 0), _reg(8, 0), _reg(8, 0), _reg(8, 0), _reg(8, 0),
                                    _reg(0, 1), _Z, _reg(0, 5), _reg(0, 1)],
                                   [_reg(0, 1), _reg(0, 1), _reg(0, 1), _reg(0, 1), _reg(0, 4),
                                    _reg(1, 1)])),
}


def dense_symbols(w, h, seed, mixed=False):
    """w h planted symbols from random.Random(seed), every one the 31-bit escape form with random
    sign, low bits, high field, low field and skipped bit: every word of the stream is then random
    and every pixel depends on it.  `mixed`: behind every third batch of 64 a run of 3 .. 40
    regular symbols of every length, so that carry[0], carry[2] and numLowBits move while the
    window's top is in use."""
    rng = random.Random(seed)
    out, run = [], 0
    for k in range(w * h):
        if mixed and k % 192 == 191:
            run = rng.randrange(3, 41)
        if run:
            run -= 1
            out.append(_reg(rng.randrange(12), rng.getrandbits(15), rng.getrandbits(1),
                            rng.getrandbits(2)))
        else:
            out.append(_esc(rng.getrandbits(13), rng.getrandbits(15), rng.getrandbits(1),
                            rng.getrandbits(2), rng.getrandbits(1)))
    return out


GEOMETRY = ((2, 2), (4, 2), (2, 4), (4, 4), (6, 6), (66, 4), (130, 6), (258, 4), (386, 4),
            (4, 130), (4, 258), (10400, 2), (2, 7792))
CONTENTS = ("flat0", "flat4095", "flat65535", "checker", "steps", "noise16", "wrap")
REFUSED = ((10402, 2), (2, 7794), (3, 2), (2, 3), (0, 2))
CUT_SHAPE = (130, 4, 6)  # a noise image of 130 x 4, read as 130 x 6: the last two rows read zeros
MID = (1024, 768)
# dense rows, 31 bits a symbol: a row's short last batch shifts where the next row's batches start
# in the window, so the first three widths sweep the batch-start offsets up to the last one; the
# 202-wide rows come to a batch at offset 195, the first where a missed reload outruns the window
DENSE = ((194, 8), (196, 8), (198, 8), (202, 8))
DENSE_MIXED = (198, 12)
# a 6 x 6 noise image cut 1 .. 12 bytes short, from two seeds whose full lengths differ mod 4
TRUNC_SEEDS = (901, 902)
TRUNC_CUTS = tuple(range(1, 13))
# plane sizes 63 .. 129 on both axes: ragged last tiles under a second band, short last bands
# over several tiles; 10400 x 130 is the smallest frame whose second band reads the last entry of
# the reconstruction's prev_row
RAGGED = ((126, 130), (128, 128), (130, 130), (258, 130), (130, 258), (254, 126), (256, 258))
WIDEST_BANDED = (MAX_X, 130)
# (not through the model's encoder)
SLOW = ("f_%dx%d_random" % MID, "g_%dx%d_noise16" % WIDEST_BANDED)


@functools.lru_cache(maxsize=None)
def case_list():
    """[{name, kind, width, height, ...}]; kind: pixels (from target pixels), plant, bytes (a
    given byte string), refused (the constructor refuses the geometry: no hash)"""
    cases = []
    for k, (w, h) in enumerate(GEOMETRY):
        cases.append(dict(name="g_%dx%d_noise12" % (w, h), kind="pixels", width=w, height=h,
                          content="noise12", seed=100 + k))
    for k, kind in enumerate(CONTENTS):
        for w, h in ((6, 6), (130, 6)):
            cases.append(dict(name="c_%dx%d_%s" % (w, h, kind), kind="pixels", width=w, height=h,
                              content=kind, seed=200 + k))
    cases.append(dict(name="c_%dx4_predictor" % (4 * len(PRED_PAIRS)), kind="pixels",
                      width=4 * len(PRED_PAIRS), height=4, content="predictor", seed=0))
    for name, (w, h, _) in PLANTED.items():
        cases.append(dict(name="p_" + name, kind="plant", width=w, height=h, plant=name))
    for n in (6, 7, 10, 11):
        cases.append(dict(name="r_2x2_%d_bytes" % n, kind="bytes", width=2, height=2, zeros=n))
    for k in range(6):
        cases.append(dict(name="r_cut_%d" % k, kind="bytes", width=CUT_SHAPE[0],
                          height=CUT_SHAPE[2], cut=k))
    for name, byte in (("zeros", 0x00), ("ones", 0xFF)):
        cases.append(dict(name="r_130x6_%s" % name, kind="bytes", width=130, height=6, byte=byte))
    for s in range(4):
        cases.append(dict(name="f_130x6_seed%d" % s, kind="bytes", width=130, height=6,
                          random=300 + s))
    cases.append(dict(name="f_%dx%d_random" % MID, kind="bytes", width=MID[0], height=MID[1],
                      random=400))
    for w, h in REFUSED:
        cases.append(dict(name="x_%dx%d" % (w, h), kind="refused", width=w, height=h))
    for w, h in DENSE:
        cases.append(dict(name="d_%dx%d" % (w, h), kind="plant", width=w, height=h, dense=w))
    cases.append(dict(name="d_mixed_%dx%d" % DENSE_MIXED, kind="plant", width=DENSE_MIXED[0],
                      height=DENSE_MIXED[1], dense=7, mixed=True))
    for seed in TRUNC_SEEDS:
        for cut in TRUNC_CUTS:
            cases.append(dict(name="t_%d_cut_%d" % (seed, cut), kind="bytes", width=6, height=6,
                              trunc=(seed, cut)))
    for k, (w, h) in enumerate(RAGGED + (WIDEST_BANDED,)):
        cases.append(dict(name="g_%dx%d_noise16" % (w, h), kind="pixels", width=w, height=h,
                          content="noise16", seed=600 + k))
    cases.append(dict(name="g_130x130_wrap", kind="pixels", width=130, height=130, content="wrap",
                      seed=0))
    assert len({c["name"] for c in cases}) == len(cases)
    return tuple(cases)


def case(name):
    return next(c for c in case_list() if c["name"] == name)


def worst_bytes(w, h):
    """a stream of this size decodes whatever it holds: 31 bits a symbol"""
    return SKIP + (w * h * 31 + 7) // 8 + 8


def _encoders(encoder):
    if encoder == "model":
        return encode, plant
    from rawspeed_amd import synth
    return synth.olympus_encode, synth.olympus_plant


def cut_lengths(full):
    """the six stream lengths of the cut family: the size at which the last fill of the 130 x 6
    read stands exactly at size + 8, and the five below"""
    w, h4, h6 = CUT_SHAPE
    # the encoded rows end somewhere in the last byte; the symbols of the two rows behind them read
    # zeros, 31 bits each
    consumed = _consumed(full, w, h4)
    last_fill = consumed + 31 * (w * (h6 - h4) - 1)
    at = 4 * ((last_fill + 31) // 32) - 8
    assert at - 5 >= len(full) - SKIP, "the cuts lie in the zeros behind the encoded rows"
    return [SKIP + at - k for k in range(6)]


def _consumed(data, w, h):
    """bits the symbols of a w x h image take from `data` (the model's walk, no pixels)"""
    bits = bytes(data[SKIP:]) + bytes(16)
    pos = 0
    for _ in range(h):
        carry = [[0, 0], [0, 0]]
        for col in range(w):
            c = carry[col & 1]
            n = low_bits(c[0], c[1])
            at = pos >> 3
            window = (int.from_bytes(bits[at:at + 5], "big") >> (8 - (pos & 7))) & 0xFFFFFFFF
            nlz = 12 - ((window >> 17) & 4095).bit_length()
            if nlz != 12:
                high, used = nlz, nlz + 4 + n
            else:
                high, used = (window >> (2 + n)) & ((1 << (15 - n)) - 1), 31
            c0 = (high << n) | ((window >> (32 - used)) & ((1 << n) - 1))
            c[0], c[1] = c0, (0 if c0 > 16 else c[1] + 1)
            pos += used
    return pos


@functools.lru_cache(maxsize=None)
def _build(name, encoder):
    c = case(name)
    enc, pl = _encoders(encoder)
    w, h = c["width"], c["height"]
    if c["kind"] == "pixels":
        return enc(content(c["content"], w, h, c["seed"]))
    if c["kind"] == "plant":
        if "dense" in c:
            return pl(w, h, dense_symbols(w, h, c["dense"], c.get("mixed", False)))
        return pl(w, h, list(PLANTED[c["plant"]][2]))
    if c["kind"] == "refused":
        return bytes(SKIP + 16)
    if "zeros" in c:
        return bytes(c["zeros"])
    if "byte" in c:
        return bytes([c["byte"]]) * worst_bytes(w, h)
    if "random" in c:
        return np.random.default_rng(c["random"]).bytes(worst_bytes(w, h))
    if "trunc" in c:
        seed, cut = c["trunc"]
        return enc(content("noise16", w, h, seed))[:-cut]
    if "cut" in c:
        full = enc(content("noise12", CUT_SHAPE[0], CUT_SHAPE[1], 500))
        n = cut_lengths(full)[c["cut"]]
        return (full + bytes(n))[:n]
    raise KeyError(name)


def build_case(name, encoder="c"):
    """-> {case, data}: the case's stream, written by the C writer or by the model"""
    return dict(case=case(name), data=_build(name, encoder))


@functools.lru_cache(maxsize=None)
def _model(name):
    c = case(name)
    stats, win = collections.Counter(), Window()
    return decode(_build(name, "c"), c["width"], c["height"], stats, win) + (stats, win)


def expected(name):
    """the model's answer: (status, pixels or None)"""
    return _model(name)[:2]


def window(name):
    """the kernel's window bookkeeping over the case's stream (a Window)"""
    return _model(name)[3]


def reach(names=None):
    """the reach statistics of the model over the case list (or over `names`)"""
    stats = collections.Counter()
    for c in case_list():
        if names is None or c["name"] in names:
            stats.update(_model(c["name"])[2])
    return stats


# ---------------------------------------------------------------------------------------------
# The host build, hashes, the golden file
# ---------------------------------------------------------------------------------------------
_host = None


def host_lib():
    """rawspeed_amd/librsx_olympus_host.so: rsx_olympus_core.h as host C++"""
    global _host
    if _host is None:
        import ctypes as C
        from rawspeed_amd import build
        build.build_olympus_host()
        _host = C.CDLL(build.LIB_OLYMPUS_HOST)
        _host.rsx_olympus_host_validate.argtypes = [C.c_size_t, C.c_void_p]
        _host.rsx_olympus_host_decode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
        _host.rsx_olympus_host_fill_limit.argtypes = [C.c_uint64]
        _host.rsx_olympus_host_fill_limit.restype = C.c_uint64
    return _host


def host_decode(data, w, h, fill=0xA5A5, pad=0):
    """the stream through the host build -> (status, the (h, w + pad) buffer it was given)"""
    import ctypes as C
    from rawspeed_amd import abi
    buf = np.full((max(h, 1), max(w, 0) + pad), fill, np.uint16)
    view = abi.Image(buf.ctypes.data, 2 * (max(w, 0) + pad), w, h, 1, 1)
    # (a pointer for no bytes; what lies behind the stream must not matter, so it is not zero)
    a = np.frombuffer(bytes(data) + b"\xff" * 16, np.uint8)
    rc = host_lib().rsx_olympus_host_decode(a.ctypes.data, len(data), C.byref(view))
    return rc, buf


@functools.lru_cache(maxsize=None)
def host_expected(name):
    """the host build's answer: (status, (h, w) pixels or None)"""
    c = case(name)
    rc, buf = host_decode(_build(name, "c"), c["width"], c["height"])
    return rc, (buf if rc == OK else None)


def sha_rows(px):
    return hashlib.sha256(np.ascontiguousarray(px, dtype="<u2").tobytes()).hexdigest()


def fnv_rows(px):
    v = 0xcbf29ce484222325
    for b in np.ascontiguousarray(px, dtype="<u2").tobytes():
        v = ((v ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return v


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def write_cases(path, pad=0):
    """the case file: "RSXO", a count, per case width, height, pitch, length (u32) and the stream"""
    cases = case_list()
    with open(path, "wb") as f:
        f.write(b"RSXO" + struct.pack("<I", len(cases)))
        for c in cases:
            d = _build(c["name"], "c")
            f.write(struct.pack("<iiII", c["width"], c["height"], 2 * max(c["width"], 0) + pad,
                                len(d)) + d)
    return [c["name"] for c in cases]


def write_golden(lines_path):
    """the recorder's lines (one per case, in case order) -> the golden file: verdicts and hashes
    only, and only when the model agrees with every line"""
    cases = case_list()
    lines = [json.loads(l) for l in open(lines_path) if l.strip()]
    assert len(lines) == len(cases), (len(lines), len(cases))
    out = {}
    for c, ref in zip(cases, lines):
        name = c["name"]
        rc, px = expected(name)
        assert ref["ok"] == (rc == OK), (name, ref, rc)
        entry = dict(ok=ref["ok"])
        if ref["ok"]:
            assert ref["sha256"] == sha_rows(px), name
            entry["sha256"] = ref["sha256"]
        else:
            entry["exception"] = ref["exception"]
            # (the text behind "<function>, line <n>: ")
            entry["message"] = re.sub(r"^.*, line \d+: ", "", ref["message"])
            want = {ERR_INVALID_ARG: "RawDecoderException", ERR_IO: "IOException",
                    ERR_INPUT_OVERFLOW: "IOException"}[rc]
            assert ref["exception"] == want, (name, ref, rc)
            assert ("overflow" in ref["message"].lower()) == (rc == ERR_INPUT_OVERFLOW), (name, ref)
        out[name] = entry
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    return len(out)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    if sys.argv[1:2] == ["--write-cases"]:
        print(len(write_cases(sys.argv[2])), "cases")
    elif sys.argv[1:2] == ["--golden"]:
        print(write_golden(sys.argv[2]), "lines agree")
    else:
        sys.exit(__doc__)
