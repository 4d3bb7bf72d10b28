"""FujiDecompressor (compressed RAF; include/rsx.h section 3u) test material: a pure-Python model
of the strip codec written after the reference's code (decompressors/FujiDecompressor.cpp) -- one
class that decodes a strip or, run forward over target pixels, encodes one --, the container
(header + sizes + padding + strips), the contents and the case list every test uses, and the
recorded answers of the reference (tests/golden/fuji_ref.json, scripts/record_fuji_ref.cpp).

The reference has no encoder.  The encoder here and the C one (rawspeed_amd/csrc/synth/rsx_synth.c,
rsx_synth_fuji_encode_strip) are written independently and must produce identical bytes.  On
X-Trans a fixed pattern of even positions takes no bits, so a strip cannot hold arbitrary pixels:
an encoder returns the pixels it reached next to the bytes, and those are what a decode returns.

  python tests/fuji_files.py --write-cases FILE     the containers for the recorder
  python tests/fuji_files.py --golden LINES         tests/golden/fuji_ref.json from its output;
                                                    refused unless the model agrees with every line
"""
import functools
import hashlib
import json
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "fuji_ref.json")

OK, ERR_INVALID_ARG, ERR_IO, ERR_INPUT_OVERFLOW, ERR_UNSUPPORTED, ERR_VALUE_RANGE = 0, 1, 2, 5, 7, 10

BLOCK = 768
R0, R1, R2, R3, R4, G0, G1, G2, G3, G4, G5, G6, G7, B0, B1, B2, B3, B4 = range(18)
# getAsCFAColors(XTransPhase(0, 0)), common/XTransPhase.h:61-71
XTRANS = ("GGRGGB", "GGBGGR", "BRGRBG", "GGBGGR", "GGRGGB", "RBGBRG")
BAYER = ("RG", "GB")

# what the encoder's statistics must show was reached (test_fuji_model.py)
REACH = ("escape", "code_bits_0", "bit_diff_15", "zeros_over_32", "halving", "wrap_low",
         "wrap_high", "grad_neg", "grad_pos", "even_term_fd", "even_term_fc", "even_term_dc",
         "odd_inside", "odd_outside")


class FujiError(Exception):
    def __init__(self, status):
        super().__init__("status %d" % status)
        self.status = status


class Params:
    """fuji_compressed_params, :189-237"""

    def __init__(self, raw_type, raw_bits):
        self.xtrans = raw_type == 16
        self.raw_bits = raw_bits
        self.total = 1 << raw_bits
        self.q4 = self.total - 1
        self.max_bits = {16: 64, 14: 56}[raw_bits]
        self.max_diff = {16: 1024, 14: 256}[raw_bits]
        self.lw = BLOCK * 2 // 3 if self.xtrans else BLOCK // 2

    def quant(self, v):
        a = abs(v)
        g = 0
        if a > 0:
            g = 1
        if a >= 0x12:
            g = 2
        if a >= 0x43:
            g = 3
        if a >= 0x114:
            g = 4
        return -g if v < 0 else g


def bit_diff(v1, v2):
    dec = max(v1.bit_length() - v2.bit_length(), 0)  # (lz2 - lz1)
    if (v2 << dec) < v1:
        dec += 1
    return min(dec, 15)


def out_index(xtrans, r, x):
    """copy_line, :337-405: (line, position) of image row r of a strip line and strip column x"""
    if xtrans:
        colour = XTRANS[r][x % 6]
        idx = (((x * 2 // 3) & 0x7FFFFFFE) | ((x % 3) & 1)) + ((x % 3) >> 1)
    else:
        colour = BAYER[r % 2][x % 2]
        idx = x >> 1
    line = {"R": R2 + (r >> 1), "G": G2 + r, "B": B2 + (r >> 1)}[colour]
    return line, 1 + idx


@functools.lru_cache(maxsize=None)
def out_map(xtrans):
    """(line, position) arrays of shape (6, 768)"""
    m = np.array([[out_index(xtrans, r, x) for x in range(BLOCK)] for r in range(6)])
    return m[:, :, 0], m[:, :, 1]


CSRC = os.path.join(os.path.dirname(HERE), "rawspeed_amd", "csrc")


@functools.lru_cache(maxsize=None)
def device_constants():
    """FJ_WIN, FJ_CHUNK, FJ_CHUNK_WORDS of rsx_fuji.hip and ZEROS_CAP of rsx_fuji_core.h, read out
    of the sources: the schedule below describes the kernel that is there"""
    import re
    out = {}
    for fname, names in (("rsx_fuji.hip", ("FJ_WIN", "FJ_CHUNK", "FJ_CHUNK_WORDS")),
                         ("rsx_fuji_core.h", ("ZEROS_CAP",))):
        with open(os.path.join(CSRC, fname)) as f:
            text = f.read()
        for name in names:
            m = re.findall(r"^\s*constexpr\s+\w+\s+%s\s*=\s*([\w\s*+<()-]+);" % name, text, re.M)
            assert len(m) == 1, (fname, name, m)
            out[name] = int(eval(m[0], {"__builtins__": {}}, dict(out)))
    return out


class Schedule:
    """What fuji_strip_kernel does around the walk of one strip of `size` bytes: the chunks of a
    pass, the window refills in front of them, and for every word the reader loads whether the
    512-word window served it or the fallback read of memory did (FjSrc::word).  k: the words
    loaded (Bits::k); after a fill at c bits k = ceil(c / 32) + 1."""

    def __init__(self, size):
        K = device_constants()
        self.win, self.chunk_words, self.cap = K["FJ_WIN"], K["FJ_CHUNK_WORDS"], K["ZEROS_CAP"]
        self.chunk_iters = K["FJ_CHUNK"]
        self.size = size
        self.k, self.k0, self.have_window = 0, 0, False
        self.refills = []    # (in front of a pass's first chunk, k - k0 of the window left or None,
        #                       the new window spans the strip's end)
        self.window_reads = 0
        self.fallback = []   # (k, inside the zero-count loop, 4 k + 4 > size)
        self.failed = None   # (k, outside the window) of the fill that failed
        self.runs_ok = 0     # samples that decoded behind fallback reads inside their zero run
        self.max_zeros = 0
        self._run_reads = 0

    def chunk(self, first):
        """in front of iterations [i0, i0 + FJ_CHUNK) of a pass"""
        if not self.have_window or self.k - self.k0 + self.chunk_words > self.win:
            left = self.k - self.k0 if self.have_window else None
            spans = 4 * self.k < self.size < 4 * (self.k + self.win)
            self.refills.append((first, left, spans))
            self.k0, self.have_window = self.k, True

    def fill(self, c, in_zeros):
        """Bits::fill at c bits consumed -> False: it fails"""
        if 32 * self.k - c >= 32:
            return True
        assert self.k == (c + 31) // 32 and self.have_window
        outside = self.k - self.k0 >= self.win
        if 4 * self.k > self.size + 8:
            self.failed = (self.k, outside)
            return False
        if outside:
            self.fallback.append((self.k, in_zeros, 4 * self.k + 4 > self.size))
            self._run_reads += in_zeros
        else:
            self.window_reads += 1
        self.k += 1
        return True

    def sample(self, zeros=None):
        """in front of a sample (None), and behind one that decoded, with its zero count"""
        if zeros is not None:
            self.max_zeros = max(self.max_zeros, zeros)
            self.runs_ok += self._run_reads > 0
        self._run_reads = 0


class Strip:
    """One strip.  data: the bytes to decode; target: (6 total_lines, 768) pixels to encode
    (plant: (kind, sample index), kind 'regular' or 'escape': from that coded sample on, the first
    one that can carry an out-of-range code in that form gets one; ('long_escape', sample index,
    Z): from that coded sample on, the first one whose code is at least 1 is written in the escape
    form behind Z zeros -- any count of at least escape_at is the escape --, and the strip goes on).
    sched: a Schedule that follows a decode."""

    def __init__(self, P, total_lines, data=None, target=None, plant=None, sched=None):
        self.P, self.total_lines = P, total_lines
        self.data, self.target, self.plant = data, target, plant
        self.sched = sched
        self.c = 0  # bits consumed
        self.out = bytearray()
        self.acc, self.nacc = 0, 0
        self.n_coded = 0
        self.planted = False
        self.stats = {k: 0 for k in REACH}
        self.stats.update(clamp_low=0, clamp_high=0, planted=0)
        self.indices = [set(), set()]  # table indices met in the even and the odd phase
        self.no_bits_rows = set()
        w = P.lw + 2
        self.lines = [[0] * w for _ in range(18)]
        self.ge = [[[P.max_diff, 1] for _ in range(41)] for _ in range(3)]
        self.go = [[[P.max_diff, 1] for _ in range(41)] for _ in range(3)]
        self.pixels = np.zeros((6 * total_lines, BLOCK), np.uint16)

    # ---- BitStreamerMSB, every request fill(32): the rule of include/rsx.h 3u ----
    def fill(self, in_zeros=False):
        fails = self.data is not None and 4 * ((self.c + 31) // 32) > len(self.data) + 8
        if self.sched is not None:
            assert self.sched.fill(self.c, in_zeros) == (not fails)
        if fails:
            raise FujiError(ERR_INPUT_OVERFLOW)

    def peek32(self):
        i, s = self.c >> 3, self.c & 7
        v = int.from_bytes(self.data[i:i + 5].ljust(5, b"\0"), "big")
        return (v >> (8 - s)) & 0xFFFFFFFF

    def put(self, value, n):
        self.acc = (self.acc << n) | value
        self.nacc += n
        self.c += n
        while self.nacc >= 8:
            self.nacc -= 8
            self.out.append((self.acc >> self.nacc) & 0xFF)
        self.acc &= (1 << self.nacc) - 1

    def zerobits(self):
        count = 0
        while True:
            self.fill(in_zeros=True)
            batch = self.peek32()
            n = 32 - batch.bit_length()
            count += n
            self.c += n if n == 32 else n + 1
            if n != 32:
                return count

    # ---- fuji_decode_sample, :444-502 (the encoder: the same state run forward) ----
    def sample(self, grad, interp, tbl, want):
        P = self.P
        e = tbl[abs(grad)]
        escape_at = P.max_bits - P.raw_bits - 1
        reg_bits = bit_diff(e[0], e[1])
        if self.data is not None:
            if self.sched is not None:
                self.sched.sample()
            zeros = self.zerobits()
            if zeros < escape_at:
                bits, delta = reg_bits, zeros << reg_bits
            else:
                bits, delta = P.raw_bits, 1
            self.fill()
            code = 0
            if bits:
                code = self.peek32() >> (32 - bits)
                self.c += bits
            code += delta
            if code < 0 or code >= P.total:
                raise FujiError(ERR_VALUE_RANGE)
            if self.sched is not None:
                self.sched.sample(zeros)
        else:
            # the residual that reaches `want`, directly or over either wrap: the smallest code
            s = -1 if grad < 0 else 1
            best = None
            for d in (want - interp, want - interp + P.total, want - interp - P.total):
                d *= s
                code = 2 * d if d >= 0 else -2 * d - 1
                if code < P.total and (best is None or code < best):
                    best = code
            code = best
            bad, long_run = None, None
            if self.plant and not self.planted and self.n_coded >= self.plant[1]:
                if self.plant[0] == "long_escape":
                    long_run = self.plant[2] if code >= 1 else None
                elif self.plant[0] == "escape":
                    bad = ("escape", P.total)
                elif ((escape_at - 1) << reg_bits) >= P.total:
                    bad = ("regular", (escape_at - 1) << reg_bits)
            if bad:
                self.planted = True
                self.stats["planted"] += 1
                code = bad[1]
            if long_run is not None:
                self.planted = True
                self.stats["planted"] += 1
                zeros, bits = long_run, P.raw_bits
                for at in range(0, zeros, 32):
                    self.put(0, min(32, zeros - at))
                self.put(1, 1)
                self.put(code - 1, bits)
            elif (code >> reg_bits) < escape_at and not (bad and bad[0] == "escape"):
                zeros, bits = code >> reg_bits, reg_bits
                self.put(1, zeros + 1)
                if bits:
                    self.put(code & ((1 << bits) - 1), bits)
            else:
                zeros, bits = escape_at, P.raw_bits
                self.put(1, zeros + 1)
                self.put(code - 1, bits)
            if bad:
                raise FujiError(ERR_VALUE_RANGE)  # (a decoder stops here; so does the writer)
            st = self.stats
            st["escape"] += zeros >= escape_at
            st["code_bits_0"] += bits == 0
            st["bit_diff_15"] += bits == 15 and zeros < escape_at
            st["zeros_over_32"] += zeros > 32
            st["grad_neg"] += grad < 0
            st["grad_pos"] += grad > 0
        self.n_coded += 1
        code = -1 - code // 2 if code & 1 else code // 2
        e[0] += abs(code)
        if e[1] == 0x40:
            e[0] >>= 1
            e[1] >>= 1
            self.stats["halving"] += 1
        e[1] += 1
        interp = interp - code if grad < 0 else interp + code
        if interp < 0:
            interp += P.total
            self.stats["wrap_low"] += 1
        elif interp > P.q4:
            interp -= P.total
            self.stats["wrap_high"] += 1
        if interp < 0:
            self.stats["clamp_low"] += 1
            return 0
        if interp > P.q4:
            self.stats["clamp_high"] += 1
        return min(interp, P.q4)

    # ---- the interpolations, :511-563 ----
    def even_inner(self, c, col):
        L, P = self.lines, self.P
        Rb, Rc, Rd, Rf = L[c - 1][1 + 2 * col], L[c - 1][2 * col], L[c - 1][2 + 2 * col], L[c - 2][1 + 2 * col]
        dcb, dfb, ddb = abs(Rc - Rb), abs(Rf - Rb), abs(Rd - Rb)
        if dcb > max(dfb, ddb):
            t1, t2, which = Rf, Rd, "even_term_fd"
        elif ddb > max(dcb, dfb):
            t1, t2, which = Rf, Rc, "even_term_fc"
        else:
            t1, t2, which = Rd, Rc, "even_term_dc"
        self.stats[which] += 1
        return 9 * P.quant(Rb - Rf) + P.quant(Rc - Rb), (2 * Rb + t1 + t2) >> 2

    def odd_inner(self, c, col):
        L, P = self.lines, self.P
        Ra, Rb, Rc = L[c][1 + 2 * col], L[c - 1][2 + 2 * col], L[c - 1][1 + 2 * col]
        Rd, Rg = L[c - 1][3 + 2 * col], L[c][3 + 2 * col]
        interp = Ra + Rg
        if Rb < min(Rc, Rd) or Rb > max(Rc, Rd):
            interp = (interp + 2 * Rb) >> 1
            self.stats["odd_outside"] += 1
        else:
            self.stats["odd_inside"] += 1
        return 9 * P.quant(Rb - Rc) + P.quant(Rc - Ra), interp >> 1

    @staticmethod
    def no_bits(row, i, comp):
        if comp == 0:
            return row == 0 or (row == 2 and i % 2 == 0) or (row == 4 and i % 2 != 0) or row == 5
        return row == 1 or row == 2 or (row == 3 and i % 2 != 0) or (row == 5 and i % 2 == 0)

    def extend(self, first, last):
        L, w = self.lines, self.P.lw + 2
        for i in range(first, last + 1):
            L[i][0] = L[i - 1][1]
            L[i][w - 1] = L[i - 1][w - 2]

    # ---- fuji_decode_block, :605-704 ----
    def block(self, want):
        """want: None, or 18 lists of target line values"""
        P, L = self.P, self.lines
        half = P.lw // 2
        counter = {"R": 0, "G": 0, "B": 0}
        first = {"R": R2, "G": G2, "B": B2}
        ext = {"R": (R2, R4), "G": (G2, G7), "B": (B2, B4)}
        for row in range(6):
            colours = BAYER[row % 2]
            c = []
            for k in colours:
                c.append(first[k] + counter[k])
                counter[k] += 1
            ge, go = self.ge[row % 3], self.go[row % 3]
            for i in range(half + 4):
                if self.sched is not None and i % self.sched.chunk_iters == 0:
                    self.sched.chunk(i == 0)
                if i < half:
                    for comp in range(2):
                        grad, interp = self.even_inner(c[comp], i)
                        if P.xtrans and self.no_bits(row, i, comp):
                            v = interp
                            self.no_bits_rows.add((row, comp, i % 2))
                        else:
                            self.indices[0].add(abs(grad))
                            v = self.sample(grad, interp, ge,
                                            want[c[comp]][1 + 2 * i] if want else None)
                        L[c[comp]][1 + 2 * i] = v
                if i >= 4:
                    col = i - 4
                    for comp in range(2):
                        grad, interp = self.odd_inner(c[comp], col)
                        self.indices[1].add(abs(grad))
                        L[c[comp]][2 + 2 * col] = self.sample(
                            grad, interp, go, want[c[comp]][2 + 2 * col] if want else None)
            for k in colours:
                self.extend(*ext[k])

    # ---- fuji_decode_strip, :734-779 ----
    def run(self):
        """decode: returns the status; the pixels of the lines that decoded are in self.pixels.
        encode: returns the status (ERR_VALUE_RANGE behind a planted code); self.out, self.pixels"""
        P, L = self.P, self.lines
        if self.data is not None and len(self.data) < 4:
            return ERR_IO
        lmap, pmap = out_map(P.xtrans)
        try:
            for cur in range(self.total_lines):
                want = None
                if self.target is not None:
                    want = [[0] * (P.lw + 2) for _ in range(18)]
                    blockpx = self.target[6 * cur:6 * cur + 6]
                    for r in range(6):
                        for x in range(BLOCK):
                            want[lmap[r, x]][pmap[r, x]] = int(blockpx[r, x])
                self.block(want)
                arr = np.array([l + [0] * (MAX_W - len(l)) for l in L], np.uint16)
                self.pixels[6 * cur:6 * cur + 6] = arr[lmap, pmap]
                if cur + 1 == self.total_lines:
                    break
                for a, b in ((R0, 5), (G0, 8), (B0, 5)):
                    L[a], L[a + 1] = list(L[a + b - 2]), list(L[a + b - 1])
                for a in (R0, G0, B0):
                    L[a + 2][P.lw + 1] = L[a + 1][P.lw]
        except FujiError as e:
            self.finish()
            return e.status
        self.finish()
        return OK

    def finish(self):
        if self.data is None and self.nacc:
            self.put(0, 8 - self.nacc)


MAX_W = 514


def encode_strip(P, total_lines, target, plant=None):
    """-> (bytes, the pixels reached, the Strip with its statistics)"""
    s = Strip(P, total_lines, target=target, plant=plant)
    s.run()
    return bytes(s.out), s.pixels, s


def decode_strip(P, total_lines, data, trace=False):
    """-> (status, pixels: what the lines that decoded hold, zero behind a failure); trace: and
    the Schedule of the decode"""
    s = Strip(P, total_lines, data=bytes(data), sched=Schedule(len(data)) if trace else None)
    st = s.run()
    return (st, s.pixels, s.sched) if trace else (st, s.pixels)


# ---------------------------------------------------------------------------------------------
# The container
# ---------------------------------------------------------------------------------------------
def header(raw_type, raw_bits, width, height, **over):
    n = (width + BLOCK - 1) // BLOCK
    h = dict(signature=0x4953, version=1, raw_type=raw_type, raw_bits=raw_bits, raw_height=height,
             raw_rounded_width=n * BLOCK, raw_width=width, block_size=BLOCK, blocks_in_row=n,
             total_lines=height // 6)
    h.update(over)
    return h


def container(h, strips, sizes=None):
    """the 16-byte header, the strips' sizes, the padding, the strips"""
    b = struct.pack(">HBBBHHHHBH", h["signature"], h["version"], h["raw_type"], h["raw_bits"],
                    h["raw_height"], h["raw_rounded_width"], h["raw_width"], h["block_size"],
                    h["blocks_in_row"], h["total_lines"])
    sizes = [len(s) for s in strips] if sizes is None else sizes
    b += b"".join(struct.pack(">I", s) for s in sizes)
    if (4 * len(sizes)) & 0xC:
        b += bytes(0x10 - ((4 * len(sizes)) & 0xC))
    return b + b"".join(strips)


def parse(data):
    """the model of rsx_fuji_parse -> (status, header dict, [(offset, size)])"""
    if len(data) < 16:
        return ERR_IO, None, None
    keys = ("signature", "version", "raw_type", "raw_bits", "raw_height", "raw_rounded_width",
            "raw_width", "block_size", "blocks_in_row", "total_lines")
    h = dict(zip(keys, struct.unpack(">HBBBHHHHBH", data[:16])))
    if not header_ok(h):
        return OK, h, []
    n, pos = h["blocks_in_row"], 16
    if len(data) - pos < 4 * n:
        return ERR_IO, h, None
    sizes = struct.unpack(">%dI" % n, data[pos:pos + 4 * n])
    pos += 4 * n
    if (4 * n) & 0xC:
        pad = 0x10 - ((4 * n) & 0xC)
        if len(data) - pos < pad:
            return ERR_IO, h, None
        pos += pad
    strips = []
    for s in sizes:
        if len(data) - pos < s:
            return ERR_IO, h, None
        strips.append((pos, s))
        pos += s
    return OK, h, strips


def header_ok(h):
    """FujiHeader::operator bool, :919-937"""
    bs = h["block_size"]
    return not (
        h["signature"] != 0x4953 or h["version"] != 1 or h["raw_height"] > 0x3000 or
        h["raw_height"] < 6 or h["raw_height"] % 6 or h["raw_width"] > 0x3000 or
        h["raw_width"] < 0x300 or h["raw_width"] % 24 or h["raw_rounded_width"] > 0x3000 or
        bs != 0x300 or h["raw_rounded_width"] < bs or h["raw_rounded_width"] % bs or
        h["raw_rounded_width"] - h["raw_width"] >= bs or h["blocks_in_row"] > 0x10 or
        h["blocks_in_row"] == 0 or h["blocks_in_row"] != h["raw_rounded_width"] // bs or
        h["blocks_in_row"] != (h["raw_width"] + bs - 1) // bs or h["total_lines"] > 0x800 or
        h["total_lines"] == 0 or h["total_lines"] != h["raw_height"] // 6 or
        h["raw_bits"] not in (12, 14, 16) or h["raw_type"] not in (16, 0))


# ---------------------------------------------------------------------------------------------
# Contents and cases
# ---------------------------------------------------------------------------------------------
def content(kind, raw_bits, width, height, seed):
    """(height, roundUp(width, 768)) target pixels: every strip is coded 768 columns wide"""
    rng = np.random.default_rng(seed)
    q4 = (1 << raw_bits) - 1
    w = (width + BLOCK - 1) // BLOCK * BLOCK
    y, x = np.mgrid[0:height, 0:w]
    if kind == "flat":
        img = np.full((height, w), 1000)
    elif kind == "noisy":
        # a ramp under noise whose size grows along the row: every quantiser class and pair
        sigma = np.linspace(0, 700, w)[None, :] * (1 + (y % 3))
        img = q4 // 3 + 5 * x + 40 * y + rng.normal(0, 1, (height, w)) * sigma
    elif kind == "saturated":
        # blocks of the three extreme values: full-scale residuals, both wraps, the escape
        img = np.array([0, q4 // 2 + 1, q4])[rng.integers(0, 3, (height, (w + 15) // 16))]
        img = np.repeat(img, 16, axis=1)[:, :w]
    elif kind == "checker":
        img = np.where((x + y) & 1, q4, 0)
    elif kind == "steps":
        # long flat runs (halving, code_bits 0) with rare jumps (zero runs over 32)
        img = np.repeat(rng.integers(0, q4 + 1, (height, (w + 255) // 256)), 256, axis=1)[:, :w]
    else:
        raise ValueError(kind)
    return np.clip(img, 0, q4).astype(np.uint16)


SHAPES = ((768, 6), (768, 12), (768, 18), (792, 12), (1560, 12), (12288, 6),
          # last strips of 48, 384 and 744 columns (the others' are 24 wide), and a strip of ten lines
          (816, 6), (1152, 6), (1512, 6), (768, 60))
N_FIRST_SHAPES = 6  # (the cases of these came first: their contents and seeds stay what they were)
CONTENTS = ("noisy", "flat", "saturated", "checker", "steps")
TYPES = ((16, 14), (16, 16), (0, 14), (0, 16))


# The medium long escape per type: (Z, sample index), picked with Schedule among the first samples
# of the chunks in front of which the window stays: the run starts some 250 words into the window,
# is shorter than the window and still leaves it, and the rest of its chunk reads outside the
# window (tests/test_fuji_model.py asserts that it does)
LONG_MEDIUM = {"x14": (8640, 1928), "x16": (8448, 1144), "b14": (8384, 632), "b16": (8512, 1912)}
LONG_AT = 1500  # coded samples in front of the other long escapes
ZERO_TAIL_HEAD = 900  # bytes of the strip in front of a zero tail: 225 words, inside window 0


def case_list():
    """[dict(name, raw_type, raw_bits, width, height, content, seed, fault)] -- fault: None, or
    (kind, strip, argument) applied to the encoded strips"""
    out, later = [], []
    n = m = 0
    for raw_type, raw_bits in TYPES:
        tag = "%s%d" % ("x" if raw_type == 16 else "b", raw_bits)
        for si, (w, h) in enumerate(SHAPES[:N_FIRST_SHAPES]):
            # every content on the one-strip shapes, one (cycling) on the wide ones
            kinds = CONTENTS if w == 768 and h == 6 else (CONTENTS[(si + n) % len(CONTENTS)],)
            for kind in kinds:
                n += 1
                out.append(dict(name="%s_%dx%d_%s" % (tag, w, h, kind), raw_type=raw_type,
                                raw_bits=raw_bits, width=w, height=h, content=kind, seed=100 + n,
                                fault=None))
        base = dict(raw_type=raw_type, raw_bits=raw_bits, width=768, height=6, content="noisy")
        for cut in (-16, -12, -9, -8, -4):
            out.append(dict(base, name="%s_cut%d" % (tag, -cut), seed=7, fault=("cut", 0, cut)))
        out.append(dict(base, name="%s_short" % tag, seed=7, fault=("cut_to", 0, 3)))
        out.append(dict(base, name="%s_plant_regular" % tag, seed=7, fault=("plant", 0, "regular")))
        out.append(dict(base, name="%s_plant_escape" % tag, seed=7, fault=("plant", 0, "escape")))
        out.append(dict(base, name="%s_random0" % tag, seed=7, fault=("random", 0, 11)))
        out.append(dict(base, name="%s_random1" % tag, seed=7, fault=("random", 0, 12)))
        out.append(dict(base, name="%s_zero" % tag, seed=7, fault=("zero", 0, 600)))
        # per-strip statuses of a frame with several failing strips: the reference reports one
        # error for the whole image, so these are held against the model ("model_only")
        out.append(dict(base, name="%s_multi" % tag, width=1560, height=12, seed=8,
                        fault=("multi", None, None)))

        # the later shapes: one content each, cycling on; the tall strip noisy
        for si, (w, h) in enumerate(SHAPES[N_FIRST_SHAPES:]):
            kind = "noisy" if h == 60 else CONTENTS[(si + m) % len(CONTENTS)]
            m += 1
            later.append(dict(name="%s_%dx%d_%s" % (tag, w, h, kind), raw_type=raw_type,
                              raw_bits=raw_bits, width=w, height=h, content=kind, seed=200 + m,
                              fault=None))
        # a valid sample no writer emits: the escape form behind more zeros than escape_at
        escape_at = Params(raw_type, raw_bits).max_bits - raw_bits - 1
        runs = [(escape_at + 1, LONG_AT), (96, LONG_AT), LONG_MEDIUM[tag], (20000, LONG_AT)]
        if tag in ("x14", "b16"):
            runs.append(((1 << 20) + 40, LONG_AT))  # (past ZEROS_CAP; a strip of 131 KB)
        for z, at in runs:
            later.append(dict(base, name="%s_long%d" % (tag, z), seed=7,
                              fault=("long_escape", 0, (z, at))))
        # a zero run that starts in window 0 and ends the strip outside it, at every size % 4
        for z in (2400, 2401, 2402, 2403):
            later.append(dict(base, name="%s_zero_tail%d" % (tag, z), seed=7,
                              fault=("zero_tail", 0, z)))
        # a failing strip 0 with the bytes of strip 1 directly behind it
        three = dict(base, width=1560, height=12, seed=9)
        for cut in (-9, -8, -4):
            later.append(dict(three, name="%s_next_cut%d" % (tag, -cut), fault=("cut", 0, cut)))
        for z in (2401, 2403):
            later.append(dict(three, name="%s_next_zero_tail%d" % (tag, z),
                              fault=("zero_tail", 0, z)))
    return out + later


PLANT_AT = 1500  # coded samples in front of a planted code: the tables have grown by then


@functools.lru_cache(maxsize=None)
def _built(name):
    c = next(c for c in case_list() if c["name"] == name)
    P = Params(c["raw_type"], c["raw_bits"])
    lines = c["height"] // 6
    img = content(c["content"], c["raw_bits"], c["width"], c["height"], c["seed"])
    n = img.shape[1] // BLOCK
    return c, P, lines, img, n


def fault_bytes(c, s, data):
    """the bytes of strip s of case c behind its fault (the plant is the encoder's)"""
    f = c["fault"]
    if f is None or f[0] in ("plant", "long_escape"):
        return data
    kind, which, arg = f
    if kind == "multi":
        rng = np.random.default_rng(5)
        return {0: data, 1: rng.integers(0, 256, 900, dtype=np.uint8).tobytes(), 2: bytes(2)}[s]
    if s != which:
        return data
    if kind == "cut":
        return data[:len(data) + arg]
    if kind == "cut_to":
        return data[:arg]
    if kind == "random":
        return np.random.default_rng(arg).integers(0, 256, 2000, dtype=np.uint8).tobytes()
    if kind == "zero":
        return bytes(arg)
    if kind == "zero_tail":
        return data[:ZERO_TAIL_HEAD] + bytes(arg)
    raise ValueError(kind)


def plant_of(c, s):
    f = c["fault"]
    if f and f[0] == "long_escape" and f[1] == s:
        return ("long_escape", f[2][1], f[2][0])
    return (f[2], PLANT_AT) if f and f[0] == "plant" and f[1] == s else None


def build_case(name, encoder=None):
    """-> dict(case, header, data: the container, strips: [bytes], reached: the pixels the
    encoder reached (height, n 768)).  encoder(P, lines, target, plant) -> (bytes, pixels);
    default: the C writer (test_fuji_model.py holds it against the model's bytes)."""
    c, P, lines, img, n = _built(name)
    if encoder is None:
        from rawspeed_amd import synth
        encoder = lambda P, lines, t, plant: synth.fuji_encode_strip(  # noqa: E731
            16 if P.xtrans else 0, P.raw_bits, lines, t, plant)[:2]
    strips, reached = [], np.zeros_like(img)
    for s in range(n):
        data, px = encoder(P, lines, img[:, s * BLOCK:(s + 1) * BLOCK], plant_of(c, s))
        strips.append(fault_bytes(c, s, data))
        reached[:, s * BLOCK:(s + 1) * BLOCK] = px
    h = header(c["raw_type"], c["raw_bits"], c["width"], c["height"])
    return dict(case=c, header=h, data=container(h, strips), strips=strips, reached=reached)


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> (status of the frame, [strip statuses], pixels (height, width): the model's decode of
    every strip -- for a strip that failed, what its lines held when it stopped)"""
    b = build_case(name)
    c, P, lines, img, n = _built(name)
    sts, px = [], np.zeros((c["height"], n * BLOCK), np.uint16)
    for s in range(n):
        if c["fault"] is None:
            st, p = OK, b["reached"][:, s * BLOCK:(s + 1) * BLOCK]  # (test_fuji_model decodes these)
        else:
            st, p, _ = traced(name, s)
        sts.append(st)
        px[:, s * BLOCK:(s + 1) * BLOCK] = p
    rc = next((st for st in sts if st != OK), OK)
    return rc, sts, px[:, :c["width"]]


@functools.lru_cache(maxsize=None)
def traced(name, s):
    """-> (status, pixels, Schedule) of the model's decode of strip s of a case"""
    c, P, lines, img, n = _built(name)
    return decode_strip(P, lines, build_case(name)["strips"][s], trace=True)


@functools.lru_cache(maxsize=None)
def lines_done(name, s):
    """how many lines of strip s of a case a decoder completes (its rows up to there are the
    reached pixels; the rows behind stay as the caller left them)"""
    rc, sts, px = expected(name)
    if sts[s] == OK:
        return _built(name)[2]
    if len(build_case(name)["strips"][s]) < 4:
        return 0
    strip = Strip(_built(name)[1], _built(name)[2], data=build_case(name)["strips"][s])
    done = [0]
    block = strip.block

    def counted(want):
        block(want)
        done[0] += 1
    strip.block = counted
    strip.run()
    return done[0]


_host = None


def host_lib():
    """rawspeed_amd/librsx_fuji_host.so: rsx_fuji_core.h as host C++"""
    global _host
    if _host is None:
        import ctypes as C
        from rawspeed_amd import build
        build.build_fuji_host()
        _host = C.CDLL(build.LIB_FUJI_HOST)
        _host.rsx_fuji_host_parse.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
        _host.rsx_fuji_host_validate.argtypes = [C.c_void_p, C.c_void_p]
        _host.rsx_fuji_host_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                               C.c_void_p, C.c_int]
    return _host


def host_parse(data):
    """-> (status, abi.FujiDesc)"""
    import ctypes as C
    from rawspeed_amd import abi
    d = abi.FujiDesc()
    a = np.frombuffer(bytes(data) + b"\0", np.uint8)  # (a pointer for no bytes)
    return host_lib().rsx_fuji_host_parse(a.ctypes.data, len(data), C.byref(d)), d


def host_decode(data, fill=0xA5A5, pad=0, threads=1):
    """the container through the host build -> (status, [strip statuses], pixels (h, w))"""
    import ctypes as C
    from rawspeed_amd import abi
    st, d = host_parse(data)
    assert st == OK, st
    w, h = d.raw_width, d.raw_height
    buf = np.full((h, w + pad), fill, np.uint16)
    view = abi.Image(buf.ctypes.data, 2 * (w + pad), w, h, 1, 1)
    a = np.frombuffer(bytes(data), np.uint8)
    ss = (C.c_int32 * 16)(*([-1] * 16))
    rc = host_lib().rsx_fuji_host_decode(C.byref(d), a.ctypes.data, len(data), C.byref(view), ss,
                                         threads)
    return rc, list(ss)[:d.n_strips], buf[:, :w]


def check_pixels(name, got, fill):
    """got (h, w) against the case: the strips that decoded hold the reached pixels; a strip that
    failed holds them in the rows of the lines it completed and `fill` behind"""
    c, P, lines, img, n = _built(name)
    rc, sts, px = expected(name)
    for s in range(n):
        x0, x1 = s * BLOCK, min((s + 1) * BLOCK, c["width"])
        rows = 6 * lines_done(name, s)
        assert np.array_equal(got[:rows, x0:x1], px[:rows, x0:x1]), (name, s)
        assert np.all(got[rows:, x0:x1] == fill), (name, s, "rows behind the failure")


def sha_rows(px):
    return hashlib.sha256(np.ascontiguousarray(px, dtype="<u2").tobytes()).hexdigest()


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def write_cases(path):
    names = [c["name"] for c in case_list()]
    with open(path, "wb") as f:
        f.write(b"RSXF" + struct.pack("<I", len(names)))
        for n in names:
            d = build_case(n)["data"]
            f.write(struct.pack("<I", len(d)) + d)
    return names


def write_golden(lines_path):
    """the recorder's lines (one per case, in case order: {"ok": bool, "sha256": str}) -> the
    golden file, unless the model disagrees with one"""
    names = [c["name"] for c in case_list()]
    lines = [json.loads(l) for l in open(lines_path) if l.strip()]
    assert len(lines) == len(names), (len(lines), len(names))
    out = {}
    for name, ref in zip(names, lines):
        rc, sts, px = expected(name)
        entry = dict(ok=ref["ok"], model_only=sum(st != OK for st in sts) > 1)
        assert ref["ok"] == (rc == OK), (name, ref, rc)
        if ref["ok"]:
            assert ref["sha256"] == sha_rows(px), name
            entry["sha256"] = ref["sha256"]
        else:
            entry["status"], entry["strip_status"] = rc, sts
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
