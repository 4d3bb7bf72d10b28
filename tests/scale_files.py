"""RawImageData::scaleBlackWhite (include/rsx.h section 6) as a numpy model, the cases every test
of the stage shares, and the case file the stand-alone programs read.

The model is written from the reference (common/RawImageDataU16.cpp:60-392,
common/RawImageDataFloat.cpp:120-170): the estimate, calculateBlackAreas with its 16-bit cells,
the plain variant in wrapping 32-bit arithmetic, the SSE2 variant lane by lane (eight 16-bit lanes
a block, the products split into mulhi and mullo halves as the intrinsics do), and the F32 pass in
numpy float32, one operation at a time.  tests/golden/scale_ref.json holds the reference's own
answers (scripts/record_scale_ref.cpp wrote them) for every case marked ref; to rebuild it:

    python tests/scale_files.py --write-cases /tmp/scale_cases.bin
    /tmp/record_scale_ref /tmp/scale_cases.bin > /tmp/scale_ref.jsonl
    python tests/scale_files.py --golden /tmp/scale_ref.jsonl

The last step refuses to write the file unless the model agrees with every recorded answer.  The
reference build has WITH_SSE2, so plain-variant cases with app_scale < 63 (host_sse2 = 0) and the
cases whose arithmetic leaves int32 (n_wrapped) cannot be recorded, nor can an empty crop, which
subFrame refuses: those are held against the model only (ref False).
"""
import functools
import hashlib
import json
import os
import struct
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scale_ref.json")
OK, INVALID_ARG, UNSUPPORTED = 0, 1, 7
PLAIN, SSE2, F32 = 0, 1, 2
CHK_BLOCKS = 8  # rsx_scale_core.h: blocks of eight pixels between two generator checkpoints
MWC_MOD = 18000 * 65536 - 1

f32 = np.float32


def _i32(v):
    """wrap to int32 (python int or int64 array)"""
    return ((v + (1 << 31)) % (1 << 32)) - (1 << 31)


def _trunc(f):
    """static_cast<int> of a binary32"""
    return int(np.trunc(f))


class Case:
    def __init__(self, name, img, cpp=1, cfa=True, crop=None, black=-1, white=None, sep=None,
                 areas=(), dither=True, sse2=True, ref=True):
        self.name, self.img, self.cpp, self.cfa = name, img, cpp, cfa
        h, ws = img.shape
        self.w, self.h = ws // cpp, h
        self.crop = (0, 0, self.w, self.h) if crop is None else crop
        self.black, self.white, self.sep = black, white, sep
        self.areas, self.dither, self.sse2, self.ref = list(areas), dither, sse2, ref
        self.is_f32 = img.dtype == np.float32


def mwc_step(v):
    return 18000 * (v & 65535) + (v >> 16)


def _estimate(c):
    ox, oy, cx, cy = c.crop
    if c.is_f32:
        r0, r1 = oy + 150 * c.cpp, oy + cy - 150
        c0, c1 = ox * c.cpp + 150, ox * c.cpp + (cx - 150) * c.cpp
        if r1 <= r0 or c1 <= c0:
            return f32(100000000.0), False
        win = c.img[r0:r1, c0:c1]
        return min(f32(100000000.0), win.min()), bool(np.isnan(win).any())
    r0, r1 = oy + 250, oy + cy - 250
    c0, c1 = ox * c.cpp + 500, ox * c.cpp + (cx - 250) * c.cpp + 250
    win = c.img[r0:r1, c0:c1] if r1 > r0 and c1 > c0 else np.zeros((0, 0), np.uint16)
    if win.size == 0:
        return 65536, 0
    return int(win.min()), int(win.max())


def _areas_levels(c, black):
    """calculateBlackAreas; None: an area past the image"""
    ox, oy, cx, cy = c.crop
    hist = np.zeros((4, 65536), np.int64)
    total = 0
    for off, size, vert in c.areas:
        size -= size & 1
        if not vert:
            if off + size > c.h:
                return None
            for y in range(off, off + size):
                xs = np.arange(ox, ox + cx)
                for par in (0, 1):
                    hist[2 * (y & 1) + par, c.img[y, ox]] += int(np.count_nonzero((xs & 1) == par))
            total += size * cx
        else:
            if off + size > c.w:
                return None
            for y in range(oy, oy + cy):
                for x in range(off, off + size):
                    hist[2 * (y & 1) + (x & 1), c.img[y, off]] += 1
            total += size * cy
    total = _i32(total)
    if total == 0:
        return [black] * 4
    hist &= 0xFFFF  # (the cells are uint16_t)
    total = int(total / 8)  # (C division)
    out = []
    for i in range(4):
        over = np.nonzero(np.cumsum(hist[i]) > total)[0]
        out.append(int(over[0]) if over.size else 65535)
    if not c.cfa:
        out = [(sum(out) + 2) >> 2] * 4
    return out


def _plain(c, img, white, bs):
    ox, oy, cx, cy = c.crop
    app = f32(65535.0) / f32(white - bs[0])
    full, half = _trunc(app * f32(4.0)), _trunc(app * f32(4095.0))
    mul, sub = [], []
    for i in range(4):
        v = i ^ (ox & 1) ^ ((oy & 1) << 1)
        mul.append(_trunc(f32(16384.0) * f32(65535.0) / f32(white - bs[v])))
        sub.append(bs[v])
    mul, sub = np.array(mul, np.int64), np.array(sub, np.int64)
    gw = cx * c.cpp
    ys = np.arange(cy, dtype=np.int64)
    v = cx + ys * 36969
    assert int(v.max(initial=0)) <= 0x7FFFFFFF
    view = img[oy:oy + cy, ox * c.cpp:ox * c.cpp + gw]
    n_wrapped = 0
    for x in range(gw):
        rand = 0
        if c.dither:
            v = mwc_step(v)
            rand = half - full * (v & 2047)
        par = 2 * (ys & 1) + (x & 1)
        d = view[:, x].astype(np.int64) - sub[par]
        prod = d * mul[par]
        t1 = prod + 8192
        t2 = _i32(t1) + rand
        bad = np.zeros(cy, bool)
        for q in (d, prod, t1, t2):
            bad |= q != _i32(q)
        n_wrapped += int(np.count_nonzero(bad))
        view[:, x] = np.clip(_i32(t2) >> 14, 0, 65535).astype(np.uint16)
    return n_wrapped


def _sse2(c, img, white, bs):
    ox, oy, cx, cy = c.crop
    app = f32(65535.0) / f32(white - bs[0])
    full, half = _trunc(app * f32(4.0)), _trunc(app * f32(4095.0))
    lanes = np.arange(8)
    words = []
    for r in (0, 1):
        b0, b1 = bs[2 * r + (ox & 1)], bs[2 * r + ((ox + 1) & 1)]
        m0 = _trunc(f32(1024.0) * f32(65535.0) / f32(white - b0))
        m1 = _trunc(f32(1024.0) * f32(65535.0) / f32(white - b1))
        b = ((b0 & 0xFFFFFFFF) | (b1 << 16)) & 0xFFFFFFFF
        m = ((m0 & 0xFFFFFFFF) | (m1 << 16)) & 0xFFFFFFFF
        words.append((np.where(lanes & 1, b >> 16, b & 0xFFFF), np.where(lanes & 1, m >> 16, m & 0xFFFF)))
    fsw = (full | (full << 16)) & 0xFFFFFFFF
    fs = np.where(lanes & 1, fsw >> 16, fsw & 0xFFFF).astype(np.int64)
    ys = np.arange(cy, dtype=np.int64)
    if c.dither:
        e = [(cx * a + ys * b) & 0xFFFFFFFF for a, b in ((1234, 23464), (4272, 12123), (2342, 34311),
                                                         (1676, 18000))]
        s = np.stack([(e[g >> 1] >> (16 * (g & 1))) & 0xFFFF for g in range(8)], axis=1)
        rmul = np.where(lanes & 1, 0x4d9f, 0x1d32).astype(np.int64)
    else:
        s = np.zeros((cy, 8), np.int64)
        rmul = np.zeros(8, np.int64)
    rowpar = (ys + oy) & 1
    sub = np.where(rowpar[:, None] == 0, words[0][0][None, :], words[1][0][None, :]).astype(np.int64)
    mul = np.where(rowpar[:, None] == 0, words[0][1][None, :], words[1][1][None, :]).astype(np.int64)
    for b in range(c.w // 8):
        blk = img[oy:oy + cy, 8 * b:8 * b + 8]
        d = np.maximum(blk.astype(np.int64) - sub, 0)  # subs_epu16
        prod = d * mul  # mulhi_epu16 : mullo_epi16
        t = _i32((prod & 0xFFFFFFFF) + 512)
        s16 = np.where(s >= 32768, s - 65536, s)
        sp = s16 * rmul  # signed 16 x 16
        s = ((sp >> 16) & 0xFFFF) ^ (sp & 0xFFFF)
        rm = ((s & 0xFF) * fs) & 0xFFFF  # mullo_epi16
        t = _i32(t + _i32((half >> 4) - rm))
        t = (t >> 10) - 32768
        t = np.clip(t, -32768, 32767)  # packs_epi32
        blk[:, :] = ((t & 0xFFFF) ^ 0x8000).astype(np.uint16)
    return 0


def apply(c):
    """(status, image, result): result = dict(black, white, sep, estimated, skipped, variant,
    n_wrapped), None unless OK"""
    ox, oy, cx, cy = c.crop
    img = c.img.copy()
    if ox < 0 or oy < 0 or cx < 0 or cy < 0 or ox + cx > c.w or oy + cy > c.h:
        return INVALID_ARG, img, None
    if c.w > 65536 or c.h > 65536 or c.cpp > 4:
        return UNSUPPORTED, img, None
    black, white = c.black, c.white
    no_levels = not c.areas and c.sep is None and black < 0
    estimated = False
    if c.is_f32:
        if white is None or c.areas:
            return UNSUPPORTED, img, None
        if no_levels:
            estimated = True
            b, nan = _estimate(c)
            if nan or b < f32(-2147483648.0):
                return UNSUPPORTED, img, None
            black = _trunc(b)
        bs = list(c.sep) if c.sep is not None else [black] * 4
        if any(white - v <= 0 for v in bs):
            return UNSUPPORTED, img, None
        res = dict(black=black, white=white, sep=tuple(bs), estimated=int(estimated), skipped=0,
                   variant=F32, n_wrapped=0)
        view = img[oy:oy + cy, ox * c.cpp:(ox + cx) * c.cpp]
        ys, xs = np.arange(cy)[:, None], np.arange(cx * c.cpp)[None, :]
        v = (2 * (ys & 1) + (xs & 1)) ^ (ox & 1) ^ ((oy & 1) << 1)
        mul = np.array([f32(65535.0) / f32(white - bs[i]) for i in range(4)], np.float32)[v]
        sub = np.array([f32(bs[i]) for i in range(4)], np.float32)[v]
        with np.errstate(all="ignore"):
            view[:, :] = (view - sub).astype(np.float32) * mul
        return OK, img, res
    if c.sep is None and cx and cy:
        for off, size, vert in c.areas:
            if off + (size - (size & 1)) > (c.w if vert else c.h):
                return INVALID_ARG, img, None
    if no_levels or white is None:
        estimated = True
        b, m = _estimate(c)
        if black < 0:
            black = b
        if white is None:
            white = m
    res = dict(black=black, white=white, sep=tuple(c.sep) if c.sep is not None else (0, 0, 0, 0),
               estimated=int(estimated), skipped=1, variant=0, n_wrapped=0)
    if (not c.areas and black == 0 and white == 65535 and c.sep is None) or cx * cy <= 0:
        return OK, img, res
    bs = list(c.sep) if c.sep is not None else _areas_levels(c, black)
    if any(white - v <= 0 for v in bs):
        return UNSUPPORTED, img, None
    app = f32(65535.0) / f32(white - bs[0])
    res.update(sep=tuple(bs), skipped=0)
    if c.sse2 and app < 63:
        res["variant"] = SSE2
        _sse2(c, img, white, bs)
    else:
        res["variant"] = PLAIN
        if cx + (cy - 1) * 36969 > 0x7FFFFFFF:
            return UNSUPPORTED, c.img.copy(), None
        res["n_wrapped"] = _plain(c, img, white, bs)
    return OK, img, res


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------
def _u16(seed, w, h, cpp=1, lo=0, hi=65536, top=65536):
    rng = np.random.default_rng(seed)
    img = rng.integers(lo, hi, (h, w * cpp), dtype=np.int64)
    # pixels below black and far above white: both ends saturate (top bounds the high ones where
    # a recorded plain-variant case must stay inside int32)
    k = rng.integers(0, 8, img.shape)
    img = np.where(k == 0, rng.integers(0, 200, img.shape), img)
    img = np.where(k == 1, rng.integers(top - top // 10, top, img.shape), img)
    return img.astype(np.uint16)


def _flt(seed, w, h, cpp=1):
    rng = np.random.default_rng(seed)
    return (rng.random((h, w * cpp)) * 70000.0 - 1000.0).astype(np.float32)


WIDE = 3 * CHK_BLOCKS * 8 + 8 + 3  # three checkpoint runs, one block, a remainder of 3


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    # the SSE2 variant: widths around the block of eight, heights 1, 2, 5, dither on and off
    for w in (8, 9, 15, 16, 17, 24):
        for h in (1, 2, 5):
            out.append(Case("sse2_%dx%d" % (w, h), _u16(w * 100 + h, w, h, lo=200, hi=17000), black=256,
                            white=16383, dither=bool((w + h) & 1)))
    out.append(Case("sse2_wide_dither", _u16(1, WIDE, 5, lo=100, hi=5000), black=64, white=4095))
    out.append(Case("sse2_wide_no_dither", _u16(2, WIDE, 2, lo=100, hi=5000), black=64, white=4095,
                    dither=False))
    # crops narrower than the image on both sides, every parity of the offset
    for ox in (1, 2):
        for oy in (1, 2):
            for sse2 in (True, False):
                # (the plain twin has app_scale >= 63, which the reference's build runs as plain too)
                out.append(Case("crop_%d_%d_%s" % (ox, oy, "sse2" if sse2 else "plain"),
                                _u16(ox * 10 + oy, 29, 7, lo=50, hi=(16000 if sse2 else 1500),
                                     top=(65536 if sse2 else 1800)),
                                crop=(ox, oy, 29 - ox - 3, 7 - oy - 1), white=(15000 if sse2 else 1000),
                                sep=(100, 110, 120, 90), sse2=True))
    out.append(Case("crop_cpp3_sse2", _u16(5, 21, 5, cpp=3, lo=0, hi=20000), cpp=3, cfa=False,
                    crop=(3, 1, 15, 3), white=16000, sep=(500, 500, 500, 500)))
    out.append(Case("crop_cpp3_plain", _u16(6, 21, 5, cpp=3, lo=0, hi=1200, top=1900), cpp=3, cfa=False,
                    crop=(3, 1, 15, 3), white=1000, sep=(20, 20, 20, 20)))
    # app_scale just under and at 63: 65535 / 1041 = 62.95.., 65535 / 1040 = 63.01..
    out.append(Case("app_scale_under_63", _u16(7, 40, 4, lo=0, hi=3000), black=100, white=1141))
    out.append(Case("app_scale_at_63", _u16(8, 40, 4, lo=0, hi=2100, top=2100), black=100, white=1140))
    # a second multiplier past 16 bits: white - level = 900 -> 1024 * 65535 / 900 = 74564
    out.append(Case("sse2_mul_spills", _u16(10, 33, 6, lo=0, hi=20000), crop=(1, 0, 31, 6),
                    white=16000, sep=(0, 15100, 15200, 100)))
    out.append(Case("sse2_levels_past_16_bits", _u16(11, 24, 4, lo=0, hi=65536), white=200000,
                    sep=(70000, 66000, 100, 65536)))
    out.append(Case("sse2_negative_level", _u16(12, 24, 4, lo=0, hi=65536), white=60000,
                    sep=(-5, 10, -70000, 0)))
    # the plain variant without SSE2 in the build: model only below app_scale 63
    out.append(Case("plain_no_sse2_dither", _u16(13, 37, 5, lo=0, hi=17000), crop=(3, 1, 30, 3),
                    black=256, white=16383, sse2=False, ref=False))
    out.append(Case("plain_no_sse2_no_dither", _u16(14, 37, 5, lo=0, hi=17000), crop=(2, 2, 30, 3),
                    sep=(256, 300, 200, 250), white=16383, sse2=False, dither=False, ref=False))
    out.append(Case("plain_wide", _u16(15, WIDE, 3, lo=0, hi=1200, top=1700), black=10, white=900))
    out.append(Case("plain_wrapped", _u16(16, 19, 3, lo=0, hi=65536), black=0, white=2, ref=False))
    # the estimate: a one-sample window, an empty window (white 0 - black 65536: refused), a window
    # (the reference goes on with a negative scale where the call refuses: not recorded)
    one = _u16(501, 501, 501, lo=300, hi=14000)
    one[250, 500] = 15000  # (the window)
    out.append(Case("estimate_one_sample", one, black=100))
    out.append(Case("estimate_empty", _u16(500, 500, 600, lo=300, hi=14000), ref=False))
    out.append(Case("estimate_window", _u16(520, 520, 515, lo=300, hi=14000)))
    out.append(Case("estimate_white_only", _u16(17, 520, 515, lo=300, hi=14000), black=200, dither=False))
    out.append(Case("estimate_cropped_cpp3", _u16(18, 342, 512, cpp=3, lo=300, hi=900), cpp=3, cfa=False,
                    crop=(4, 3, 336, 507)))
    # the skip rule
    out.append(Case("skip", _u16(19, 16, 4), black=0, white=65535))
    out.append(Case("skip_empty_crop", _u16(20, 16, 4), crop=(3, 1, 0, 2), black=10, white=1000, ref=False))
    out.append(Case("no_skip_with_levels", _u16(21, 16, 4), black=0, white=65535, sep=(0, 0, 0, 0)))
    # the areas
    a = _u16(22, 40, 30, lo=100, hi=400)
    out.append(Case("areas_horizontal", a, crop=(3, 2, 34, 26), white=4000, areas=[(0, 2, False), (27, 3, False)]))
    out.append(Case("areas_vertical", a, crop=(4, 1, 30, 27), white=4000, areas=[(0, 4, True), (35, 5, True)]))
    out.append(Case("areas_both_not_cfa", a, cfa=False, crop=(3, 2, 34, 26), white=4000,
                    areas=[(1, 2, False), (36, 4, True)]))
    out.append(Case("areas_odd_size_one", a, crop=(3, 2, 34, 26), black=77, white=4000, areas=[(0, 1, False)]))
    b = _u16(23, 40, 30, lo=100, hi=400)
    b[:, 0] = 0
    out.append(Case("areas_median_bin_0", b, crop=(0, 0, 40, 30), white=4000, areas=[(0, 4, True)]))
    b = b.copy()
    b[:, 0] = 65535
    out.append(Case("areas_median_bin_65535", b, crop=(0, 0, 40, 30), white=70000, areas=[(0, 4, True)]))
    out.append(Case("areas_past_image", a, crop=(3, 2, 34, 26), white=4000, areas=[(0, 2, False), (29, 2, False)]))
    out.append(Case("areas_past_image_vertical", a, crop=(3, 2, 34, 26), white=4000, areas=[(38, 4, True)]))
    # a count that wraps 65 536: 65535 columns are 32768 even and 32767 odd ones; rows 0 and 2 both
    # count 300, so the even columns' cell wraps to 0 (an empty histogram walks to 65535) and the
    # odd columns' holds 65534; rows 1 and 3 count 400 and 500: 32768 each in the even columns,
    # where the walk stops at 400, and 32767 each in the odd ones, where it must pass 400
    wrap = _u16(33, 65535, 4, lo=0, hi=65536)
    wrap[:, 0] = (300, 400, 300, 500)
    out.append(Case("areas_count_wraps", wrap, white=70000, areas=[(0, 4, False)], dither=False))
    # F32
    out.append(Case("f32_pass", _flt(24, 23, 5), crop=(1, 1, 20, 3), black=100, white=16000))
    out.append(Case("f32_pass_cpp3_levels", _flt(25, 11, 4, cpp=3), cpp=3, cfa=False, crop=(2, 0, 9, 4),
                    white=60000, sep=(1, 2, 3, 4)))
    out.append(Case("f32_estimate", _flt(26, 310, 305), white=65535))
    nan = _flt(27, 310, 305)
    nan[152, 155] = np.nan
    out.append(Case("f32_estimate_nan", nan, white=65535, ref=False))
    low = _flt(28, 310, 305)
    low[152, 155] = -3.0e9
    out.append(Case("f32_estimate_below_int", low, white=65535, ref=False))
    out.append(Case("f32_no_white", _flt(29, 16, 4), black=10, ref=False))
    out.append(Case("f32_areas", _flt(30, 16, 4), black=10, white=1000, areas=[(0, 2, False)], ref=False))
    # refusals common to both (the reference divides by zero or scales by a negative: not recorded)
    out.append(Case("white_equals_level", _u16(31, 16, 4), white=1000, sep=(10, 1000, 10, 10), ref=False))
    out.append(Case("white_below_level", _u16(32, 16, 4), black=2000, white=1000, ref=False))
    assert len({c.name for c in out}) == len(out)
    return out


def check_cases():
    """what the case list promises: a recorded case stays inside int32"""
    for c in cases():
        st, _, res = expected(c.name)
        assert not (c.ref and st == OK and res["n_wrapped"]), c.name


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """apply() of a case, computed once and shared: (status, image, result)"""
    st, img, res = apply(case(name))
    img.setflags(write=False)
    return st, img, res


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def load_golden():
    with open(GOLDEN) as f:
        return {e["name"]: e for e in json.load(f)}


def header(c, status):
    """the 22 int32 words of a case in the case file"""
    ox, oy, cx, cy = c.crop
    sep = c.sep if c.sep is not None else (0, 0, 0, 0)
    return [c.w, c.h, c.cpp, c.img.strides[0], int(c.cfa), ox, oy, cx, cy, int(c.is_f32), c.black,
            int(c.white is not None), c.white or 0, int(c.sep is not None), *sep, int(c.dither),
            int(c.sse2), len(c.areas), status]


def write_cases(path, only_ref=False):
    """the case file rsx_scale_host_check and scripts/record_scale_ref.cpp read"""
    cs = [c for c in cases() if c.ref or not only_ref]
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cs)))
        for c in cs:
            st, want, _ = expected(c.name)
            f.write(c.name.encode().ljust(64, b"\0"))
            f.write(struct.pack("<22i", *header(c, st)))
            for off, size, vert in c.areas:
                f.write(struct.pack("<IIii", off, size, int(vert), 0))
            f.write(np.ascontiguousarray(c.img).tobytes())
            f.write(np.ascontiguousarray(want).tobytes())


def write_golden(jsonl):
    recorded = [json.loads(line) for line in open(jsonl) if line.startswith("{")]
    names = [c.name for c in cases() if c.ref]
    assert [e["name"] for e in recorded if "name" in e] == names, "the recorder ran another case list"
    out = []
    for e in recorded:
        if "name" not in e:
            continue
        c = case(e["name"])
        st, img, res = expected(c.name)
        assert e["input"] == sha(c.img), e["name"]
        assert e["ok"] == (st == OK), (e["name"], e, st)
        assert e["image"] == sha(img), "the model disagrees with the reference on %s" % e["name"]
        if st == OK and not res["skipped"]:
            assert (e["black"], e["white"], tuple(e["sep"])) == (res["black"], res["white"], res["sep"]), \
                (e, res)
        out.append(e)
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    if sys.argv[1] == "--write-cases":
        write_cases(sys.argv[2], only_ref=True)
    elif sys.argv[1] == "--golden":
        write_golden(sys.argv[2])
