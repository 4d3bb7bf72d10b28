"""TEST INFRASTRUCTURE: cases for the sRaw interpolator (rsx_sraw.hip), and a numpy model of it.

  model()      -- Cr2sRawInterpolator::interpolate restated in int64 numpy, from
                  interpolators/Cr2sRawInterpolator.cpp (interpolate_422 / interpolate_420,
                  YUV_TO_RGB<v>, STORE_RGB): not from the kernel, not from the oracle.  It
                  says "copy" where the reference copies (the last group of a row, the last
                  row); the kernel gets there through mean(x, x).  Its wrong variants (mean=,
                  shift12=, edge=, top=) exist to prove that a case discriminates; they are
                  never compared with the GPU.
  cases()      -- (subsampling, version) x groups per row x rows, per value class
  images()     -- the (descriptor, input pixels) of a case: one image, or as many "takes" of
                  the case's shape as the class needs to reach every value it is after (a
                  2-group row has ONE interpolated pixel: three samples per image)
  PlanLayout   -- the jobs of one device plan in one input and one output buffer, and the
                  comparison of a whole output buffer with the expected one

The value classes:
  sensor    the ranges of golden_cases.build_sraw: clamping almost never fires
  full      any 16-bit Y / Cb / Cr, coefficients 256..4096, |hue| <= 1000: every clamp outcome
            in every channel, and no product leaves 32 bits (the reference's int multiply is
            defined)
  boundary  coefficients 256 (so (256 * x) >> 8 == x): the pre-clamp r, g, b of every pixel
            lands on each of TARGETS, in every channel, over the takes
  rounding  negative, odd chroma sums and negative >> 12 arguments: floor against truncation
            and against dcraw's rounding
  wrap      any 16-bit input, coefficients up to 65535, hue within +-20000: nearly every
            product wraps (signed overflow in the reference: held to the oracle and the model
            only)
"""
import collections
import functools

import numpy as np

from rawspeed_amd import abi

# (subsampling_y, version): what Cr2sRawInterpolator::interpolate accepts
PAIRS = ((1, 0), (1, 1), (1, 2), (2, 1), (2, 2))
# groups per row: every residue mod 4 in one lane and in two, on both sides of the 1024-group
# seam between workgroups (256 lanes x 4 groups), and in a third workgroup
WIDTHS = (2, 3, 4, 5, 6, 7, 8, 9, 1021, 1022, 1023, 1024, 1025, 1026, 1027, 1028, 2049)
NARROW = (2, 3, 5, 1025)                # where the other classes are held to the reference
SEAM = (2, 3, 5, 1023, 1024, 1025)      # where they run on the GPU
# input rows; 4:2:0 with one row runs only the "last two lines" path
ROWS = {1: (1, 2, 3), 2: (1, 2, 3, 4)}
CLASSES = ("sensor", "full", "boundary", "rounding", "wrap")
TARGETS = (-1, 0, 1, 65534, 65535, 65536)
SEED = 20717

# pixel kinds, by position in the 2 x 2 (4:2:2: 2 x 1) pixels of a group
FULL, HORIZ, VERT, DIAG = range(4)

Case = collections.namedtuple("Case", "cls ysf version groups rows")
Model = collections.namedtuple("Model", "out pre max_product kind interp")


def cases(cls, widths=WIDTHS, rows=None, pairs=PAIRS):
    """rows: None = all of ROWS; anything else = the largest row count only"""
    out = []
    for ysf, version in pairs:
        rr = ROWS[ysf] if rows is None else (ROWS[ysf][-1],)
        out += [Case(cls, ysf, version, g, r) for g in widths for r in rr]
    return out


def case_id(c):
    return "%s_42%d_v%d_%dx%d" % (c.cls, 2 if c.ysf == 1 else 0, c.version, c.groups, c.rows)


def out_dims(c):
    """(dim_x in pixels, dim_y) of the output image"""
    return 2 * c.groups, c.ysf * c.rows


# ---- the model ----------------------------------------------------------------------------

def _div(s, n, how):
    """s / n for n = 2, 4, 4096: the reference's >> ("floor"), or towards zero ("trunc")"""
    if how == "floor":
        return s >> (n.bit_length() - 1)
    assert how == "trunc"
    return np.sign(s) * (np.abs(s) // n)


def _mean(terms, how):
    """YCbCr::interpolateCbCr: (p0 + p2) >> 1, (p0 + p1 + p2 + p3) >> 2, no rounding"""
    n = len(terms)
    s = sum(terms)
    if how == "round":  # dcraw: +1 before >> 1, +2 before >> 2
        return (s + n // 2) >> (n // 2)
    return _div(s, n, how)


def _chroma(x, ysf, mean, edge):
    """One of Cb / Cr after process(hue), shape (rows, groups) -> that component of every
    output pixel, shape (ysf * rows, groups, 2); and whether the pixel's is a real mean."""
    rows, n = x.shape
    c = np.empty((ysf * rows, n, 2), np.int64)
    interp = np.zeros((ysf * rows, n, 2), bool)
    past = x[:, -1:] if edge == "copy" else np.zeros((rows, 1), np.int64)  # (edge="zero": wrong)
    right = np.concatenate([x[:, 1:], past], axis=1)  # the group to the right
    top = slice(0, None, ysf)
    c[top, :, 0] = x                                   # first pixel: full
    c[top, :, 1] = _mean([x, right], mean)             # middle pixel, all groups but the last
    c[top, -1, 1] = x[:, -1] if edge == "copy" else _mean([x[:, -1], past[:, 0]], mean)
    interp[top, :-1, 1] = True
    if ysf == 2:
        # interpolate_420_row, rows 0 .. rows - 2: the row below takes part
        a, b = x[:-1], x[1:]
        ar, br = right[:-1], right[1:]
        low = slice(1, 2 * (rows - 1), 2)
        c[low, :, 0] = _mean([a, b], mean)
        c[low, :, 1] = _mean([a, ar, b, br], mean)
        interp[low, :, 0] = True
        interp[low, :-1, 1] = True
        if edge == "copy":  # the last group: CopyCbCr(&MCUs[0][Row][1], MCUs[0][Row][0])
            c[low, -1, 1] = c[low, -1, 0]
        # the last two lines: the second copies the first, pixel by pixel
        c[2 * rows - 1] = c[2 * rows - 2]
    return c, interp


def model(desc, px, mean="floor", shift12=None, edge="copy", top=65535):
    """The output image of Cr2sRawInterpolator::interpolate(version) for the input `px`
    (rows x groups * (2 + 2 * ysf) uint16), as Model:
      out          uint16 (ysf * rows, 6 * groups)
      pre          int64, same shape: r >> 8, g >> 8, b >> 8 before clampBits(.., 16)
      max_product  the largest |sraw_coeffs[k] * (..)| before it is wrapped to 32 bits
      kind, interp (ysf * rows, 2 * groups): FULL / HORIZ / VERT / DIAG by position, and
                   whether the pixel's chroma is a mean (not a copy)
    mean="trunc" / "round", shift12="trunc", edge="zero" and top=65534 are deliberately wrong."""
    ysf, version, hue = desc.subsampling_y, desc.version, desc.hue
    assert (ysf, version) in PAIRS
    shift12 = shift12 or ("trunc" if mean == "trunc" else "floor")
    gs = 2 + 2 * ysf
    rows = px.shape[0]
    g = px.astype(np.int64).reshape(rows, -1, gs)
    n = g.shape[1]
    assert n > 1
    # LoadCbCr, signExtend, applyHue
    cb, interp = _chroma(g[:, :, gs - 2] - 16384 + hue, ysf, mean, edge)
    cr, _ = _chroma(g[:, :, gs - 1] - 16384 + hue, ysf, mean, edge)
    # LoadY: MCU[MCURow][MCUCol] = in[2 * MCURow + MCUCol]
    Y = np.empty((ysf * rows, n, 2), np.int64)
    for mr in range(ysf):
        Y[mr::ysf] = g[:, :, 2 * mr:2 * mr + 2]

    args = []

    def s12(a):
        args.append(a)
        return _div(a, 4096, shift12)

    if version == 0:    # "Algorithm found in EOS 40D"
        inner = [Y + cr - 512, Y + s12(-778 * cb - cr * 2048) - 512, Y + (cb - 512)]
    elif version == 1:
        inner = [Y + s12(50 * cb + 22929 * cr), Y + s12(-5640 * cb - 11751 * cr),
                 Y + s12(29040 * cb - 101 * cr)]
    else:               # "Algorithm found in EOS 5d Mk III"
        inner = [Y + cr, Y + s12(-778 * cb - cr * 2048), Y + cb]
    # everything up to here is int arithmetic in the reference: it must fit
    assert max(int(np.abs(a).max()) for a in args + inner) < 2 ** 31
    pre = np.empty((ysf * rows, n, 2, 3), np.int64)
    max_product = 0
    for k in range(3):
        p = int(desc.sraw_coeffs[k]) * inner[k]
        max_product = max(max_product, int(np.abs(p).max()))
        p = ((p + 2 ** 31) & 0xFFFFFFFF) - 2 ** 31  # int: two's-complement wrap
        pre[..., k] = p >> 8                        # STORE_RGB
    out = np.clip(pre, 0, top).astype(np.uint16)    # clampBits(.., 16)
    kind = np.empty((ysf * rows, n, 2), np.int64)
    kind[0::ysf, :, 0], kind[0::ysf, :, 1] = FULL, HORIZ
    if ysf == 2:
        kind[1::2, :, 0], kind[1::2, :, 1] = VERT, DIAG
    flat = (ysf * rows, -1)
    return Model(out.reshape(flat), pre.reshape(flat), max_product, kind.reshape(flat),
                 interp.reshape(flat))


# ---- the value classes --------------------------------------------------------------------

def _rng(c, take=0):
    return np.random.default_rng([SEED, CLASSES.index(c.cls), c.ysf, c.version, c.groups,
                                  c.rows, take])


def _desc(c, coeffs, hue):
    return abi.SrawDesc.make(c.version, c.ysf, [int(x) for x in coeffs], int(hue))


def _blank(c):
    gs = 2 + 2 * c.ysf
    px = np.zeros((c.rows, c.groups * gs), np.uint16)
    return px, px.reshape(c.rows, c.groups, gs)


def _sensor(c):
    rng = _rng(c)
    px, g = _blank(c)
    g[:, :, :-2] = rng.integers(200, 15000, size=g[:, :, :-2].shape)
    g[:, :, -2:] = rng.integers(16384 - 3000, 16384 + 3000, size=g[:, :, -2:].shape)
    return [(_desc(c, rng.integers(800, 2600, size=3), rng.integers(-600, 600)), px)]


def _full(c):
    rng = _rng(c)
    px, g = _blank(c)
    g[:] = rng.integers(0, 65536, size=g.shape)
    return [(_desc(c, rng.integers(256, 4097, size=3), rng.integers(-1000, 1001)), px)]


def _wrap(c):
    rng = _rng(c)
    px, g = _blank(c)
    g[:] = rng.integers(0, 65536, size=g.shape)
    return [(_desc(c, rng.integers(20000, 65536, size=3), rng.integers(-20000, 20001)), px)]


def _boundary(c):
    """18 takes.  With coefficients 256 and Y = 0 the model's pre-clamp values are the chroma
    terms f of every pixel and channel; Y = target - f then puts that channel on the target.
    Chroma of one sign per take keeps f <= -1 (the targets -1, 0, 1: Y >= 0) or f >= 1 (65534,
    65535, 65536: Y <= 65535) through every mean; g's term has the other sign than r's and
    b's.  Pixel p of take k aims at combination (k + p) % 9 of its take's sign: over the takes
    every pixel meets every (channel, target)."""
    out = []
    for take in range(18):
        rng = _rng(c, take)
        sign = 1 if take < 9 else -1
        hue = int(rng.integers(-1000, 1001))
        px, g = _blank(c)
        # |Cb|, |Cr| after process(hue) in 1000..3000: past version 0's 512 in every channel
        g[:, :, -2:] = 16384 - hue + sign * rng.integers(1000, 3001, size=g[:, :, -2:].shape)
        d = _desc(c, (256, 256, 256), hue)
        f = model(d, px).pre.reshape(c.ysf * c.rows, -1, 3)
        low, high = TARGETS[:3], TARGETS[3:]
        # (channel, target): r and b follow the chroma's sign, g opposes it
        combos = [(ch, t) for ch in (0, 2) for t in (high if sign > 0 else low)] + \
                 [(1, t) for t in (low if sign > 0 else high)]
        p = np.arange(f.shape[1])[None, :] + 3 * np.arange(f.shape[0])[:, None]
        pick = (take + p) % 9
        ch = np.array([x[0] for x in combos])[pick]
        tg = np.array([x[1] for x in combos])[pick]
        Y = tg - np.take_along_axis(f, ch[:, :, None], axis=2)[:, :, 0]
        assert Y.min() >= 0 and Y.max() <= 65535
        Y = Y.reshape(c.ysf * c.rows, c.groups, 2)
        for mr in range(c.ysf):
            g[:, :, 2 * mr:2 * mr + 2] = Y[mr::c.ysf]
        out.append((d, px))
    return out


def _rounding(c):
    """Two takes, coefficients 256, Y around 30000, hue in -3..0.  Chroma after process(hue) is
    -(1 + (row + group) % 2 + 2 * u[group]), u in 0..2: neighbours differ in parity, so every
    two-term sum is negative and odd, every four-term sum negative and 2 mod 4.  Take 0: Cb and
    Cr both so (the >> 12 arguments of version 1's r and b are negative).  Take 1: Cr positive
    instead, 3..8 (2048 * 3 > 778 * 6): the >> 12 argument of every version's g is negative."""
    out = []
    for take in range(2):
        rng = _rng(c, take)
        hue = -int(rng.integers(0, 4))
        px, g = _blank(c)
        g[:, :, :-2] = rng.integers(29000, 31001, size=g[:, :, :-2].shape)
        par = (np.arange(c.rows)[:, None] + np.arange(c.groups)[None, :]) % 2
        for k in (0, 1):
            v = -(1 + par + 2 * rng.integers(0, 3, size=c.groups)[None, :])
            if take == 1 and k == 1:
                v = 2 - v
            g[:, :, -2 + k] = 16384 - hue + v
        out.append((_desc(c, (256, 256, 256), hue), px))
    return out


_BUILDERS = {"sensor": _sensor, "full": _full, "boundary": _boundary, "rounding": _rounding,
             "wrap": _wrap}


@functools.lru_cache(maxsize=None)
def images(c):
    """[(SrawDesc, input pixels)] of a case; shared between the tests: read-only"""
    out = _BUILDERS[c.cls](c)
    for _, px in out:
        px.flags.writeable = False
    return out


# ---- one plan's jobs in two buffers -------------------------------------------------------

def row_up(nbytes):
    return (nbytes + 15) // 16 * 16


class PlanLayout:
    """Jobs of one rsx_sraw_plan_create plan.  Every job has its own pitches (a multiple of 16
    unless a defect is asked for) and a gap before it; everything that is not a pixel of some
    job is 0xA5, in both buffers."""

    Entry = collections.namedtuple("Entry", "name desc px in_off in_pitch out_off out_pitch "
                                   "out_w out_h want_status")

    def __init__(self):
        self.entries = []
        self.in_end = self.out_end = 0

    def add(self, name, desc, px, ysf, in_extra=0, out_extra=0, gap=0, in_shift=0,
            out_shift=0, out_w=None, want_status=0):
        """in_extra / out_extra: bytes of row padding past roundUp(row bytes, 16); gap: unused
        bytes before the job in both buffers; in_shift / out_shift: what a defective job adds
        to its offsets; out_w: the output width in pixels the job claims, if not the right
        one"""
        rows, in_w = px.shape
        groups = in_w // (2 + 2 * ysf)
        e = self.Entry(name, desc, px, self.in_end + gap + in_shift, row_up(2 * in_w) + in_extra,
                       self.out_end + gap + out_shift, row_up(12 * groups) + out_extra,
                       2 * groups if out_w is None else out_w, ysf * rows, want_status)
        self.entries.append(e)
        self.in_end = row_up(e.in_off + e.in_pitch * rows)
        self.out_end = row_up(e.out_off + e.out_pitch * e.out_h)
        return e

    def jobs(self):
        out = []
        for e in self.entries:
            j = abi.SrawJob()
            j.desc = e.desc
            j.in_offset, j.img_offset = e.in_off, e.out_off
            for v, (w, h, cpp, pitch) in ((j.in_, (e.px.shape[1], e.px.shape[0], 1, e.in_pitch)),
                                          (j.img, (e.out_w, e.out_h, 3, e.out_pitch))):
                v.data = None
                v.pitch_bytes, v.dim_x, v.dim_y, v.cpp, v.is_cfa = pitch, w, h, cpp, 0
            out.append(j)
        return out

    @staticmethod
    def _put(buf, off, pitch, px):
        b = np.ascontiguousarray(px).view(np.uint8)
        for r in range(b.shape[0]):
            buf[off + r * pitch:off + r * pitch + b.shape[1]] = b[r]

    def in_host(self):
        a = np.full(self.in_end + 64, 0xA5, np.uint8)
        for e in self.entries:
            self._put(a, e.in_off, e.in_pitch, e.px)
        return a

    def out_bytes(self):
        return self.out_end + 64

    def render(self, answer):
        """The output buffer if every good job's pixels were answer(entry) (uint16, out_h x
        6 * groups) and nothing else had been written."""
        a = np.full(self.out_bytes(), 0xA5, np.uint8)
        for e in self.entries:
            if e.want_status == 0:
                self._put(a, e.out_off, e.out_pitch, answer(e))
        return a

    def check(self, got, status, want):
        """got: the output buffer after a run; status: the jobs' statuses; want: render() of
        the truth.  Every job's status; every good job's rectangle; then every other byte."""
        assert got.shape == want.shape
        assert list(status) == [e.want_status for e in self.entries]
        rest = got != want
        for e in self.entries:
            if e.want_status != 0:
                continue
            for r in range(e.out_h):
                lo = e.out_off + r * e.out_pitch
                hi = lo + 6 * e.out_w
                assert not rest[lo:hi].any(), \
                    "%s: output row %d differs at sample %d" % (e.name, r,
                                                                int(np.argmax(rest[lo:hi])) // 2)
                rest[lo:hi] = False
        assert not rest.any(), "byte %d outside every job's pixels was written: 0x%02x" % (
            int(np.argmax(rest)), int(got[int(np.argmax(rest))]))
