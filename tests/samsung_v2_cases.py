"""TEST INFRASTRUCTURE: SamsungV2Decompressor streams
(decompressors/SamsungV2Decompressor.cpp:87-338) for the oracle / reference pin of that
codec and for the device tests of rsx_samsung_v2.hip (tests/test_gpu_samsung_v2.py).

  encode()       -- the random writer: it makes every choice the format allows --
                    reference-pixel mode ("motion") per block, scale changes, explicit or
                    relative difference lengths, skipped blocks -- at random, tracks the image
                    the DECODER will reconstruct (clamping included) and codes each block
                    against it, so the decoded image is known exactly.
  RowAsm, assemble()
                 -- the directed assembler: a row given block by block as explicit fields
                    (scale code, motion kept or explicit, skip bit, the four length flags with
                    explicit lengths, sixteen differences), valid or not.
  value_case()   -- the value classes (CLASSES), each seeded from the case's own numbers.
  repeat_rows()  -- a tall frame out of a short one of the writer's, without the writer's cost.
  decode_model() -- a plain Python decoder written from the reference's source, with
                    deliberately wrong variants (VARIANTS) that stand in for a wrong kernel:
                    they are never compared with the GPU, they prove that a class discriminates.
"""
import collections
import functools

import numpy as np


class Msb32Writer:
    """BitStreamerMSB32: 32-bit little-endian words, most significant bit first."""

    def __init__(self):
        self.words, self.acc, self.n = [], 0, 0

    def put(self, value, bits):
        assert 0 <= value < (1 << bits) or bits == 0
        for k in range(bits - 1, -1, -1):
            self.acc = (self.acc << 1) | ((value >> k) & 1)
            self.n += 1
            if self.n == 32:
                self.words.append(self.acc)
                self.acc, self.n = 0, 0

    def bytes_used(self):
        return 4 * len(self.words) + (self.n + 7) // 8

    def finish(self, align=16):
        """the row's bytes: whole 32-bit words, padded to `align`"""
        if self.n:
            self.words.append(self.acc << (32 - self.n))
        b = np.array(self.words, dtype="<u4").view(np.uint8)
        pad = (-b.size) % align
        return np.concatenate([b, np.zeros(pad, np.uint8)])


MOTION_OFFSET = [-4, -2, -2, 0, 0, 2, 4]
MOTION_AVG = [0, 0, 1, 0, 1, 0, 0]


def _baseline(img, row, col, motion, init_val, width):
    if motion == 7:
        if col == 0:
            return [init_val] * 16
        return [int(img[row, col + (i & 1) - 2]) for i in range(16)]
    base = []
    for i in range(16):
        rr, rc = row, col + i + MOTION_OFFSET[motion]
        if (row + i) & 1:
            rr -= 2
        else:
            rr -= 1
            rc += -1 if (i & 1) else 1
        if rc < 0 or rc >= width or (MOTION_AVG[motion] and rc + 2 >= width):
            return None
        if MOTION_AVG[motion]:
            base.append((int(img[rr, rc]) + int(img[rr, rc + 2]) + 1) >> 1)
        else:
            base.append(int(img[rr, rc]))
    return base


def header(bits, w, h, optflags, init_val):
    """the 16 bytes SamsungV2Decompressor's constructor reads (:106-132)"""
    hdr = Msb32Writer()
    for v, n in ((0x100, 16), (0, 4), (bits - 1, 4), (0, 4), (0, 4), (w, 16), (h, 16), (0, 16),
                 (0, 4), (optflags, 4), (0, 8), (0, 8), (0, 8), (0, 2), (init_val, 14)):
        hdr.put(v, n)
    return hdr.finish(align=16)


def encode(rng, target, bits, optflags=0, init_val=None, allow_scale=True, rows_out=None,
           scales=None, negative_scale=False, overshoot=False, stats=None):
    """target: (h, w) wanted values (w % 16 == 0).  Returns (stream incl. the 16-byte
    header, the image a decoder reconstructs -- equal to `target` wherever the quantisation
    scale is 0).

    The options leave the default's random draws as they are:
      scales          explicit scales are drawn from this sequence (default: 0..5)
      negative_scale  the running scale may go below 0 (code 1 at scale 0 gives -2: the
                      reference accepts it)
      overshoot       in half of the blocks, a pixel whose target is 0 or the largest value
                      is, half of the time, coded up to 3 steps further out: the decoder's
                      clamp brings it back
      stats           a dict that receives `below` / `above` (stores whose unclamped value
                      was under 0 / over the largest value), `min_scale`, `max_scale`,
                      `skipped_scaled` (skipped blocks at a scale other than 0), `max_len`"""
    h, w = target.shape
    assert w % 16 == 0
    hi = (1 << bits) - 1
    if init_val is None:
        init_val = int(rng.integers(0, 1 << 14))
    if stats is not None:
        for k in ("below", "above", "min_scale", "max_scale", "skipped_scaled", "max_len"):
            stats.setdefault(k, 0)
    out = [header(bits, w, h, optflags, init_val)]
    img = np.zeros((h, w), np.int64)
    for row in range(h):
        wr = Msb32Writer()
        motion, scale = 7, 0
        mode = [[7, 7] if row < 2 else [4, 4] for _ in range(3)]
        for col in range(0, w, 16):
            if not (optflags & 4) and col % 64 == 0:
                pick = int(rng.integers(0, 4)) if allow_scale else 0
                if pick == 3:
                    scale = int(rng.integers(0, 6)) if scales is None else int(rng.choice(scales))
                    wr.put(3, 2)
                    wr.put(scale, 12)
                else:
                    new = scale + (0, -2, 2)[pick]
                    if new < 0 and not negative_scale:
                        pick, new = 0, scale
                    wr.put(pick, 2)
                    scale = new
            # reference pixels
            cands = [7] if row < 2 else [m for m in range(8)]
            while True:
                m = int(rng.choice(cands))
                if optflags & 2 and m not in (3, 7):
                    continue
                base = _baseline(img, row, col, m, init_val, w)
                if base is not None:
                    break
            if optflags & 2:
                wr.put(1 if m == 3 else 0, 1)
            elif m == motion:
                wr.put(1, 1)
            else:
                wr.put(0, 1)
                wr.put(m, 3)
            motion = m
            # differences (in the shuffled order of the stream), quantised by the scale
            q = 2 * scale + 1
            want = [int(target[row, col + i]) - base[i] for i in range(16)]
            coded = [int(np.floor((d - scale) / q + 0.5)) for d in want]
            lmax = min(15, bits + 1)  # the longest difference field the decoder accepts
            if overshoot and rng.random() < 0.5:
                sign = 1 if q > 0 else -1
                for i in range(16):
                    t = int(target[row, col + i])
                    if t in (0, hi) and rng.random() < 0.5:
                        coded[i] += (1 if t == hi else -1) * sign * int(rng.integers(1, 4))
            coded = [max(-(1 << (lmax - 1)), min((1 << (lmax - 1)) - 1, c)) for c in coded]
            stream_order = [0] * 16
            for i in range(16):
                p = ((i % 8) << 1) - (i >> 3) + 1 if row % 2 else ((i % 8) << 1) + (i >> 3)
                stream_order[i] = coded[p]
            skip = all(c == 0 for c in coded) and not (optflags & 1) and rng.random() < 0.7
            if not (optflags & 1):
                wr.put(1 if skip else 0, 1)
            lens = [0] * 4
            if not skip:
                need = []
                for g in range(4):
                    vals = stream_order[4 * g:4 * g + 4]
                    n = 0
                    while any(not (-(1 << (n - 1)) <= v < (1 << (n - 1))) if n else v != 0
                              for v in vals):
                        n += 1
                    need.append(n)
                flags = []
                sim = [list(m_) for m_ in mode]
                for g in range(4):
                    colornum = (g >> 1) if row % 2 else ((g >> 1) + 2) % 3
                    cur = sim[colornum][0]
                    opts = [3]
                    if cur >= need[g]:
                        opts.append(0)
                    if cur + 1 >= need[g] and cur + 1 <= bits + 1:
                        opts.append(1)
                    if cur >= 1 and cur - 1 >= need[g]:
                        opts.append(2)
                    f = int(rng.choice(opts))
                    n = {0: cur, 1: cur + 1, 2: cur - 1}.get(f)
                    if f == 3:
                        n = int(rng.integers(need[g], lmax + 1))
                    flags.append((f, n))
                    sim[colornum][0] = sim[colornum][1]
                    sim[colornum][1] = n
                for f, _ in flags:
                    wr.put(f, 2)
                for g, (f, n) in enumerate(flags):
                    if f == 3:
                        wr.put(n, 4)
                    lens[g] = n
                mode = sim
                for i in range(16):
                    n = lens[i >> 2]
                    if n:
                        wr.put(stream_order[i] & ((1 << n) - 1), n)
            # what the decoder stores
            for i in range(16):
                c = 0 if skip else coded[i]
                v = base[i] + c * q + scale
                img[row, col + i] = min(max(v, 0), hi)
                if stats is not None:
                    stats["below"] += v < 0
                    stats["above"] += v > hi
            if stats is not None:
                stats["min_scale"] = min(stats["min_scale"], scale)
                stats["max_scale"] = max(stats["max_scale"], scale)
                stats["skipped_scaled"] += bool(skip and scale != 0)
                stats["max_len"] = max([stats["max_len"]] + lens)
        out.append(wr.finish(align=16))
        if rows_out is not None:
            rows_out.append(out[-1])  # the row's bytes, padded to the next 16-byte boundary
    return np.concatenate(out + [np.zeros(16, np.uint8)]), img.astype(np.uint16)


# ---- the directed assembler ---------------------------------------------------------------

class RowAsm:
    """One row, block by block, as explicit fields.  The assembler keeps what the decoder keeps
    (the length history per colour, the running scale) only to know how many bits a relative
    length stands for; it refuses nothing: a forced motion, a length past bits + 1 or a
    relative length under 0 are written as asked (the row ends at the block that throws)."""

    def __init__(self, row, bits, optflags=0):
        self.row, self.bits, self.optflags = row, bits, optflags
        self.wr = Msb32Writer()
        self.mode = [[7, 7] if row < 2 else [4, 4] for _ in range(3)]
        self.nblk, self.scale, self.min_scale, self.max_len = 0, 0, 0, 0
        self.done = None

    def block(self, scale=0, motion=None, skip=False, flags=(3, 3, 3, 3), lens=(0, 0, 0, 0),
              diffs=None):
        """scale: the 2-bit code 0..2 (0, -2, +2), or ("abs", value) for code 3 + 12 bits;
        written where the format has the field (every fourth block, not under QP).
        motion: None keeps the running one (bit 1; under MV: bit 0 = 7), else 0..7 explicit
        (under MV only 3 and 7 exist).  skip: the skip bit (none under SKIP).  flags: the four
        2-bit length flags; lens: the explicit lengths of the flags that are 3 (the others'
        entries are ignored).  diffs: sixteen differences in STREAM order, each masked to its
        group's length."""
        wr, of = self.wr, self.optflags
        if not (of & 4) and self.nblk % 4 == 0:
            if isinstance(scale, tuple):
                wr.put(3, 2)
                wr.put(scale[1], 12)
                self.scale = scale[1]
            else:
                wr.put(scale, 2)
                self.scale += (0, -2, 2)[scale]
            self.min_scale = min(self.min_scale, self.scale)
        if of & 2:
            assert motion in (None, 3, 7)
            wr.put(1 if motion == 3 else 0, 1)
        elif motion is None:
            wr.put(1, 1)
        else:
            wr.put(0, 1)
            wr.put(motion, 3)
        self.nblk += 1
        if not (of & 1):
            wr.put(1 if skip else 0, 1)
            if skip:
                return self
        else:
            assert not skip
        for f in flags:
            wr.put(f, 2)
        n = [0] * 4
        for g, f in enumerate(flags):
            colornum = (g >> 1) if self.row % 2 else ((g >> 1) + 2) % 3
            cur = self.mode[colornum][0]
            if f == 3:
                wr.put(lens[g], 4)
                n[g] = lens[g]
            else:
                n[g] = cur + (0, 1, -1)[f]
            self.mode[colornum][0] = self.mode[colornum][1]
            self.mode[colornum][1] = n[g]
            if n[g] < 0 or n[g] > self.bits + 1:
                return self  # (the decoder throws here)
        self.max_len = max([self.max_len] + n)
        diffs = diffs or [0] * 16
        for i in range(16):
            if n[i >> 2]:
                wr.put(diffs[i] & ((1 << n[i >> 2]) - 1), n[i >> 2])
        return self

    def bytes_used(self):
        """what getStreamPosition() says behind the row: whole bytes"""
        return self.wr.bytes_used()

    def finish(self):
        """the row's bytes, padded to 16 (the same array however often it is asked for)"""
        if self.done is None:
            self.done = self.wr.finish(align=16)
        return self.done


def assemble(bits, w, h, rows, optflags=0, init_val=0, tail=16):
    """header + rows (RowAsm or bytes, each padded to 16 bytes) + `tail` zero bytes"""
    out = [header(bits, w, h, optflags, init_val)]
    for r in rows:
        out.append(r.finish() if isinstance(r, RowAsm) else np.asarray(r, np.uint8))
    return np.concatenate(out + [np.zeros(tail, np.uint8)])


def repeat_rows(bits, w, h, optflags, init_val, rows):
    """A frame of `h` rows out of the rows of a shorter one of the same width: rows 0 and 1 as
    they are, then rows 2.. over and over with their parity kept.  A row's parse depends on
    its own bits and its checks on column and parity only, so the frame is as valid as the
    short one; what it decodes to is the oracle's to say, not the writer's."""
    m = (len(rows) - 2) // 2 * 2
    assert len(rows) >= min(h, 2) and (h <= 2 or m >= 2)
    picked = [rows[r] if r < 2 else rows[2 + (r - 2) % m] for r in range(h)]
    return assemble(bits, w, h, picked, optflags, init_val)


# ---- the value classes --------------------------------------------------------------------

CLASSES = ("sensor", "extremes", "floor", "ceiling", "negative_scale", "max_len")
BIG_SCALES = (0, 1, 5, 64, 1000, 4095)
SEED = 20931

ValueCase = collections.namedtuple("ValueCase", "cls bits optflags w h data want stats")


def sensor_target(rng, h, w, bits):
    """a gradient between 0.3 and 0.8 of full scale with 0.4 % noise"""
    x = np.arange(w)[None, :]
    y = np.arange(h)[:, None]
    hi = (1 << bits) - 1
    t = 0.3 * hi + 0.3 * hi * x / w + 0.2 * hi * y / h + rng.normal(0, 0.004 * hi, (h, w))
    return np.clip(t, 0, hi).astype(np.int64)


def _valid_motions(row, col, w, optflags):
    if row < 2:
        return [7]
    ok = [m for m in range(8)
          if _baseline(np.zeros((row + 1, w), np.int64), row, col, m, 0, w) is not None]
    return [m for m in ok if m in (3, 7)] if optflags & 2 else ok


def _max_len_stream(rng, bits, optflags, w, h):
    """every coded block has at least one explicit length of bits + 1, whose differences sit at
    both ends of the field, next to 0, 1 and -1; motions and scales as they come"""
    L = bits + 1
    ends = [-(1 << (L - 1)), (1 << (L - 1)) - 1, 0, 1, -1]
    rows = []
    stats = dict(min_scale=0, max_len=0)
    for row in range(h):
        ra = RowAsm(row, bits, optflags)
        motion = 7
        for col in range(0, w, 16):
            m = int(rng.choice(_valid_motions(row, col, w, optflags)))
            pick = int(rng.integers(0, 4))
            scale = ("abs", int(rng.choice(BIG_SCALES))) if pick == 3 else \
                (pick if ra.scale + (0, -2, 2)[pick] >= 0 else 0)
            lens = [L if rng.random() < 0.5 else int(rng.integers(0, L + 1)) for _ in range(4)]
            lens[int(rng.integers(0, 4))] = L
            diffs = []
            for i in range(16):
                n = lens[i >> 2]
                d = int(rng.choice(ends)) if n == L else int(rng.integers(0, 1 << n)) if n else 0
                diffs.append(d)
            skip = not (optflags & 1) and rng.random() < 0.15
            ra.block(scale=scale, motion=None if m == motion and not optflags & 2 else m,
                     skip=skip, lens=lens, diffs=diffs)
            motion = m
        stats["max_len"] = max(stats["max_len"], ra.max_len)
        rows.append(ra)
    return assemble(bits, w, h, rows, optflags, int(rng.integers(0, 1 << 14))), stats


@functools.lru_cache(maxsize=None)
def value_case(cls, bits, optflags, w=256, h=40):
    """One stream of a value class (shared between the tests: read-only).  `want` is the image
    the writer tracked, None where the stream is assembled and only a decoder knows it."""
    rng = np.random.default_rng([SEED, CLASSES.index(cls), bits, optflags, w, h])
    hi = (1 << bits) - 1
    stats, want = {}, None
    if cls == "sensor":
        data, want = encode(rng, sensor_target(rng, h, w, bits), bits, optflags, stats=stats)
    elif cls == "extremes":
        target = rng.choice([0, 1, hi // 2, hi - 1, hi], size=(h, w)).astype(np.int64)
        data, want = encode(rng, target, bits, optflags, scales=BIG_SCALES, overshoot=True,
                            stats=stats)
    elif cls in ("floor", "ceiling"):
        target = np.full((h, w), 0 if cls == "floor" else hi, np.int64)
        data, want = encode(rng, target, bits, optflags, overshoot=True, stats=stats)
    elif cls == "negative_scale":
        data, want = encode(rng, sensor_target(rng, h, w, bits), bits, optflags, scales=(0, 1),
                            negative_scale=True, stats=stats)
    else:
        data, stats = _max_len_stream(rng, bits, optflags, w, h)
    data.flags.writeable = False
    if want is not None:
        want.flags.writeable = False
    return ValueCase(cls, bits, optflags, w, h, data, want, stats)


def negative_scale_rows(bits=12):
    """Two hand-assembled 32-pixel rows (and two more so that odd rows take part): scale code 1
    at scale 0 gives -2; a coded block with differences 1 under it stores init + 1 * (2 * -2 + 1)
    - 2, and the skipped block behind it adds the scale once more to the pixels on its left:
    95 and 93 for init_val 100, in every row."""
    rows = []
    for row in range(4):
        ra = RowAsm(row, bits, 0)
        ra.block(scale=1, motion=None, lens=(2, 2, 2, 2), diffs=[1] * 16)
        ra.block(motion=None, skip=True)
        rows.append(ra)
    return assemble(bits, 32, 4, rows, 0, 100), rows


# ---- the model ----------------------------------------------------------------------------

VARIANTS = ("no_clamp_hi", "clamp_hi_minus_1", "no_clamp_0", "truncating_average",
            "skip_without_scale", "odd_shuffle_on_even_rows", "scale_unsigned_16",
            "left_neighbour_col_minus_1", "init_val_in_every_block_0")


class _Bits:
    """BitStreamerMSB32 by position over one row: zeros behind the end of the data"""

    def __init__(self, data, most=1 << 17):
        data = data[:most]  # (no row is longer: 406 blocks of at most 267 bits)
        pad = (-len(data)) % 4 + 64
        w = np.concatenate([data, np.zeros(pad, np.uint8)]).view("<u4")
        self.n = 32 * w.size
        self.all = int.from_bytes(w.astype(">u4").tobytes(), "big")
        self.q = 0

    def get(self, n):
        assert self.q + n <= self.n
        v = (self.all >> (self.n - self.q - n)) & ((1 << n) - 1)
        self.q += n
        return v


def decode_model(data, bits, w, h, variant=None):
    """SamsungV2Decompressor::decompress restated in plain Python from the reference's source
    (SamsungV2Decompressor.cpp:145-338; the header is taken as read).  Returns (status, image):
    0, or 1 where the reference throws over the stream's CONTENT (:172, :192, :214-217, :256,
    :270); what it throws when the stream ENDS early is not restated (bits behind the end read
    as zeros): the model is for streams that are long enough.  `variant`: one of VARIANTS, a
    decoder that is wrong in exactly that way."""
    assert variant is None or variant in VARIANTS
    data = np.asarray(data, np.uint8)
    hi = (1 << bits) - 1
    hdr = _Bits(data[:16])
    hdr.q = 84
    optflags = hdr.get(4)
    hdr.q = 114
    init_val = hdr.get(14)
    img = np.zeros((h, w), np.int64)
    pos = 16
    for row in range(h):
        pos = (pos + 15) // 16 * 16
        b = _Bits(data[pos:])
        motion, scale = 7, 0
        mode = [[7, 7] if row < 2 else [4, 4] for _ in range(3)]
        for col in range(0, w, 16):
            # prepareBaselineValues
            if not (optflags & 4) and col % 64 == 0:
                i = b.get(2)
                scale = scale + (0, -2, 2)[i] if i < 3 else b.get(12)
            if optflags & 2:
                motion = 3 if b.get(1) else 7
            elif not b.get(1):
                motion = b.get(3)
            if row < 2 and motion != 7:
                return 1, img
            if motion == 7 or (variant == "init_val_in_every_block_0" and col == 0):
                if col == 0:
                    base = [init_val] * 16
                elif variant == "left_neighbour_col_minus_1":
                    base = [int(img[row, col - 1])] * 16
                else:
                    base = [int(img[row, col + (i & 1) - 2]) for i in range(16)]
            else:
                slide, avg = MOTION_OFFSET[motion], MOTION_AVG[motion]
                base = []
                for i in range(16):
                    rr, rc = row, col + i + slide
                    if (row + i) & 1:
                        rr -= 2
                    else:
                        rr -= 1
                        rc += -1 if (i & 1) else 1
                    if rc < 0 or rc >= w or (avg and rc + 2 >= w):
                        return 1, img
                    if avg:
                        rnd = 0 if variant == "truncating_average" else 1
                        base.append((int(img[rr, rc]) + int(img[rr, rc + 2]) + rnd) >> 1)
                    else:
                        base.append(int(img[rr, rc]))
            # decodeDiffLengths
            lens = [0] * 4
            skipped = not (optflags & 1) and b.get(1)
            if not skipped:
                flags = [b.get(2) for _ in range(4)]
                for g in range(4):
                    colornum = (g >> 1) if row % 2 else ((g >> 1) + 2) % 3
                    cur = mode[colornum][0]
                    if flags[g] == 3:
                        lens[g] = b.get(4)
                    elif flags[g] == 2:
                        if cur == 0:
                            return 1, img
                        lens[g] = cur - 1
                    else:
                        lens[g] = cur + flags[g]
                    mode[colornum][0] = mode[colornum][1]
                    mode[colornum][1] = lens[g]
                    if lens[g] > bits + 1:
                        return 1, img
            # decodeDifferences
            diffs = []
            for i in range(16):
                n = lens[i >> 2]
                v = b.get(n) if n else 0
                diffs.append(v - (1 << n) if n and v >> (n - 1) else v)
            odd = row % 2 or variant == "odd_shuffle_on_even_rows"
            shuffled = [0] * 16
            for i in range(16):
                shuffled[((i % 8) << 1) - (i >> 3) + 1 if odd else ((i % 8) << 1) + (i >> 3)] = diffs[i]
            s = scale & 0xFFFF if variant == "scale_unsigned_16" else scale
            for i in range(16):
                add = 0 if skipped and variant == "skip_without_scale" else s
                v = base[i] + shuffled[i] * (s * 2 + 1) + add
                if v < 0:
                    v = v & 0xFFFF if variant == "no_clamp_0" else 0
                elif v > hi:
                    v = {"no_clamp_hi": v & 0xFFFF, "clamp_hi_minus_1": hi - 1}.get(variant, hi)
                elif v == hi and variant == "clamp_hi_minus_1":
                    v = hi - 1
                img[row, col + i] = v
        pos += (b.q + 7) // 8  # getStreamPosition(): whole bytes
    return 0, img.astype(np.uint16)


# ---- directed verdict cases ---------------------------------------------------------------

Directed = collections.namedtuple("Directed", "name bits w h data")


def _plain_row(row, bits, nblk, optflags=0):
    ra = RowAsm(row, bits, optflags)
    for k in range(nblk):
        ra.block(lens=(3, 3, 3, 3), diffs=[(k + i) % 7 - 3 for i in range(16)])
    return ra


@functools.lru_cache(maxsize=None)
def motion_cases(bits=12, w=32):
    """Every motion 0..7 forced at the first and at the last block of an even and of an odd
    row >= 2, and at either block of rows 0 and 1; the other blocks keep motion 7.  Which of
    them the reference throws on is the oracle's to say (and the reference's: the model
    test)."""
    nblk, out = w // 16, []
    for row in (0, 1, 2, 3):
        for at in (0, nblk - 1):
            for m in range(8):
                rows = [_plain_row(r, bits, nblk) for r in range(row)]
                ra = RowAsm(row, bits, 0)
                for k in range(nblk):
                    ra.block(motion=m if k == at else (7 if k == at + 1 else None),
                             lens=(2, 2, 2, 2), diffs=[1, -1] * 8)
                rows.append(ra)
                rows += [_plain_row(r, bits, nblk) for r in range(row + 1, 4)]
                out.append(Directed("row%d_blk%d_motion%d" % (row, at, m), bits, w, 4,
                                    assemble(bits, w, 4, rows, 0, 1000 + m)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def length_cases():
    """The difference-length checks (:256, :270), each next to its nearest valid neighbour:
    a relative length under 0, an explicit one past bits + 1, a relative one past bits + 1."""
    out = []

    def add(name, bits, blocks, row=2):
        rows = [_plain_row(r, bits, len(blocks)) for r in range(row)]
        ra = RowAsm(row, bits, 0)
        for kw in blocks:
            ra.block(**kw)
        rows.append(ra)
        out.append(Directed(name, bits, 16 * len(blocks), row + 1,
                            assemble(bits, 16 * len(blocks), row + 1, rows, 0, 77)))

    zero = dict(lens=(0, 0, 0, 0))
    for row in (0, 2, 3):
        # the history of a colour is two deep: two blocks of zero lengths, then "one less"
        add("underflow_row%d" % row, 12, [zero, dict(flags=(2, 0, 0, 0))], row)
        add("underflow_second_pair_row%d" % row, 12, [zero, dict(flags=(0, 0, 0, 2))], row)
        add("no_underflow_row%d" % row, 12, [dict(lens=(1, 1, 1, 1)), dict(flags=(2, 2, 2, 2))],
            row)
    for bits in (12, 14):
        L = bits + 1
        top = [-(1 << (L - 1)), (1 << (L - 1)) - 1] * 8
        add("explicit_longest_%d" % bits, bits, [dict(lens=(L, L, L, L), diffs=top)])
        if L < 15:
            add("explicit_too_long_%d" % bits, bits, [dict(lens=(L, L, L + 1, L))])
            add("explicit_15_%d" % bits, bits, [dict(lens=(15, 0, 0, 0))])
        # "one more" than the longest: groups 0, 1 set the history, the next block's flag 1
        add("relative_too_long_%d" % bits, bits,
            [dict(lens=(L, L, L, L), diffs=top), dict(flags=(1, 0, 0, 0))])
        add("relative_too_long_last_group_%d" % bits, bits,
            [dict(lens=(L, L, L, L), diffs=top), dict(flags=(0, 0, 0, 1))])
        add("relative_longest_%d" % bits, bits,
            [dict(lens=(L - 1, L - 1, L - 1, L - 1)), dict(flags=(1, 1, 1, 1), diffs=top)])
    return tuple(out)


# ---- frames for the geometry tests and the verdict sweeps ---------------------------------

@functools.lru_cache(maxsize=None)
def short_frame(bits, w, optflags, h0=8):
    """(stream, init_val, the rows' bytes) of an h0-row frame of the writer over the sensor
    target: what repeat_rows() makes tall frames of"""
    rng = np.random.default_rng([SEED, 100, bits, w, optflags, h0])
    init_val = int(rng.integers(0, 1 << 14))
    rows = []
    data, _ = encode(rng, sensor_target(rng, h0, w, bits), bits, optflags, init_val=init_val,
                     rows_out=rows)
    return data, init_val, tuple(rows)


def tall_frame(bits, w, h, optflags=0):
    _, init_val, rows = short_frame(bits, w, optflags)
    return repeat_rows(bits, w, h, optflags, init_val, rows)


@functools.lru_cache(maxsize=None)
def sweep_stream(kind):
    """(bits, w, h, stream): "truncate" -- 48 x 6, every length of which is decoded; "flip" --
    16 x 4 without the writer's trailing zeros, at most 150 bytes, every single bit of which
    is flipped"""
    bits = 12
    w, h = (48, 6) if kind == "truncate" else (16, 4)
    rng = np.random.default_rng([SEED, 101, w, h])
    data, _ = encode(rng, sensor_target(rng, h, w, bits), bits, 0)
    if kind == "flip":
        data = data[:-16].copy()
    data.flags.writeable = False
    return bits, w, h, data
