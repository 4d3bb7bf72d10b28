"""TEST INFRASTRUCTURE: DNG files with an OpcodeList1 and a LinearizationTable, an opcode-list
writer, and a numpy model of what DngDecoder does behind the tiles (include/rsx.h section 4d).

  dng_post_file()  an uncompressed DNG (16-bit tiles, or 32-bit float ones) on top of
                   rawfiles.Ifd / tiff_file with OPCODELIST1, LINEARIZATIONTABLE and ACTIVEAREA,
                   cpp 1 or 3; it goes through the reference's front door
  opcode_list()    the entry's bytes from a list of opcodes: the op_*() helpers, or raw()
  parse()          DngOpcodes::DngOpcodes restated: IOError_ for what throws IOException,
                   ListError for a RawDecoderException
  apply()          the whole stage: list (a pass per opcode, PixelOpcode::applyOP's loops), then
                   doLookup with a stepped generator.  Its switches select models that are NOT the
                   reference's (a test shows the golden file tells them apart).
  lut(), do_lookup(), dither_states()   TableLookUp::setTable with dither; doLookup
"""
import hashlib
import json
import os
import struct

import numpy as np

import rawfiles as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dng_post_ref.json")
OK, INVALID_ARG, IO, UNSUPPORTED = 0, 1, 2, 7
OPCODELIST1, LINEARIZATIONTABLE, SAMPLEFORMAT = 51008, 50712, 339
(REASON_NONE, REASON_ROI, REASON_PLANES, REASON_PITCH, REASON_DELTA_COUNT, REASON_DELTA_NOT_FINITE,
 REASON_TABLE_SIZE, REASON_POLY_DEGREE, REASON_UNKNOWN_OPCODE, REASON_UNSUPPORTED_OPCODE,
 REASON_INCONSISTENT_LENGTH, REASON_BAD_POINT, REASON_SETUP_NOT_U16, REASON_SETUP_CPP,
 REASON_SETUP_DELTA_RANGE, REASON_TRIM_EMPTY) = range(16)
f32 = np.float32


# ---------------------------------------------------------------------------------------
# the file
# ---------------------------------------------------------------------------------------
def dng_post_file(img, cpp=1, opcodes=None, table=None, active_area=None, tile=None):
    """img: (h, w * cpp) uint16 or float32.  opcodes: the entry's bytes (b"" writes an entry of
    count 0), table: the LinearizationTable's values, active_area: (top, left, bottom, right),
    tile: (tile_w, tile_h) in pixels (default: one tile)."""
    img = np.asarray(img)
    is_f32 = img.dtype == np.float32
    h, ws = img.shape
    w = ws // cpp
    tw, th = tile or (w, h)
    blobs = []
    for ty in range(0, h, th):
        for tx in range(0, w, tw):
            t = np.zeros((th, tw * cpp), img.dtype)
            part = img[ty:ty + th, tx * cpp:(tx + tw) * cpp]
            t[:part.shape[0], :part.shape[1]] = part
            blobs.append(t.view(np.uint8).reshape(-1))
    i = R.Ifd()
    i.add(R.NEWSUBFILETYPE, R.LONG, 0)
    i.add(R.IMAGEWIDTH, R.LONG, w).add(R.IMAGELENGTH, R.LONG, h)
    i.add(R.BITSPERSAMPLE, R.SHORT, [32 if is_f32 else 16] * cpp)
    i.add(R.COMPRESSION, R.SHORT, 1)
    i.add(R.PHOTOMETRIC, R.SHORT, 32803 if cpp == 1 else 34892)
    i.add(R.MAKE, R.ASCII, "RSX").add(R.MODEL, R.ASCII, "Synthetic")
    i.add(R.SAMPLESPERPIXEL, R.SHORT, cpp)
    if is_f32:
        i.add(SAMPLEFORMAT, R.SHORT, [3] * cpp)
    if cpp == 1:
        i.add(R.CFAREPEATPATTERNDIM, R.SHORT, [2, 2])
        i.add(R.CFAPATTERN, R.BYTE, [0, 1, 1, 2])
    i.add(R.DNGVERSION, R.BYTE, [1, 4, 0, 0])
    i.add(R.DNGBACKWARDVERSION, R.BYTE, [1, 1, 0, 0])
    i.add(R.UNIQUECAMERAMODEL, R.ASCII, "RSX Synthetic")
    if active_area:
        i.add(R.ACTIVEAREA, R.LONG, list(active_area))
    if opcodes is not None:
        i.add(OPCODELIST1, R.UNDEFINED, bytes(opcodes))
    if table is not None:
        i.add(LINEARIZATIONTABLE, R.SHORT, [int(v) for v in table])
    i.add(R.TILEWIDTH, R.LONG, tw).add(R.TILELENGTH, R.LONG, th)
    i.add_blobs(R.TILEOFFSETS, R.TILEBYTECOUNTS, blobs)
    return R.tiff_file(i)


# ---------------------------------------------------------------------------------------
# the list
# ---------------------------------------------------------------------------------------
def raw(code, payload=b"", flags=0, size=None):
    """an opcode with arbitrary bytes; size overrides the length field"""
    return (code, flags, bytes(payload), size)


def _pixel(roi, planes, pitch):
    top, left, bottom, right = roi
    return struct.pack(">8I", top, left, bottom, right, planes[0], planes[1], pitch[0], pitch[1])


def op_table(roi, table, planes=(0, 1), pitch=(1, 1), count=None):
    """MapTable; pitch = (rowPitch, colPitch); planes = (firstPlane, planes)"""
    t = [int(v) for v in table]
    return raw(7, _pixel(roi, planes, pitch) + struct.pack(">I", len(t) if count is None else count) +
               struct.pack(">%dH" % len(t), *t))


def op_poly(roi, coeffs, planes=(0, 1), pitch=(1, 1), degree=None):
    return raw(8, _pixel(roi, planes, pitch) +
               struct.pack(">I", len(coeffs) - 1 if degree is None else degree) +
               struct.pack(">%dd" % len(coeffs), *coeffs))


def op_delta(code, roi, deltas, planes=(0, 1), pitch=(1, 1), count=None):
    """10 DeltaPerRow, 11 DeltaPerColumn, 12 ScalePerRow, 13 ScalePerColumn"""
    d = np.asarray(deltas, dtype=">f4")
    return raw(code, _pixel(roi, planes, pitch) +
               struct.pack(">I", d.size if count is None else count) + d.tobytes())


def op_trim(roi):
    return raw(6, struct.pack(">4I", *roi))


def op_bad_constant(value):
    return raw(4, struct.pack(">II", value, 0))


def op_bad_list(points=(), rects=(), n_points=None, n_rects=None):
    """points: (y, x); rects: (top, left, bottom, right)"""
    b = struct.pack(">III", 0, len(points) if n_points is None else n_points,
                    len(rects) if n_rects is None else n_rects)
    for y, x in points:
        b += struct.pack(">II", y, x)
    for r in rects:
        b += struct.pack(">4I", *r)
    return raw(5, b)


def opcode_list(ops, count=None):
    out = struct.pack(">I", len(ops) if count is None else count)
    for code, flags, payload, size in ops:
        out += struct.pack(">4I", code, 0x01030000, flags, len(payload) if size is None else size)
        out += payload
    return out


# ---------------------------------------------------------------------------------------
# the parse
# ---------------------------------------------------------------------------------------
class IOError_(Exception):
    """what the reference throws as IOException: the file fails"""


class ListError(Exception):
    """a RawDecoderException: logged, the decode goes on"""

    def __init__(self, reason):
        Exception.__init__(self, reason)
        self.reason = reason


class _Stream:
    def __init__(self, data):
        self.d, self.pos = bytes(data), 0

    def check(self, n):
        if n < 0 or self.pos + n > len(self.d):
            raise IOError_()

    def skip(self, n):
        self.check(n)
        self.pos += n

    def get(self, fmt):
        n = struct.calcsize(fmt)
        self.check(n)
        v = struct.unpack_from(">" + fmt, self.d, self.pos)
        self.pos += n
        return v[0] if len(v) == 1 else v

    def u32(self):
        return self.get("I")

    def sub(self, n):
        self.check(n)
        s = _Stream(self.d[self.pos:self.pos + n])
        self.pos += n
        return s

    def remain(self):
        return len(self.d) - self.pos


def _roi(bs, dim_w, dim_h):
    top, left, bottom, right = (v - (1 << 32) if v >= (1 << 31) else v for v in bs.get("4I"))
    inside = lambda x, y: 0 <= x <= dim_w and 0 <= y <= dim_h  # noqa: E731
    if not (inside(left, top) and inside(right, bottom) and right >= left and bottom >= top):
        raise ListError(REASON_ROI)
    return top, left, bottom, right


def parse(data, cpp, crop, full):
    """[opcode dicts] in list order.  crop = (x, y, w, h), full = (w, h) of the uncropped image."""
    bs = _Stream(data)
    count = bs.u32()
    at = bs.pos
    for _ in range(count):
        bs.skip(12)
        bs.skip(bs.u32())
    bs.pos = at
    sub = list(crop)
    out = []
    for _ in range(count):
        code = bs.u32()
        bs.skip(4)
        flags = bs.u32()
        ob = bs.sub(bs.u32())
        op = {"code": code, "crop": tuple(sub)}
        if code == 0 or code > 13:
            raise ListError(REASON_UNKNOWN_OPCODE)
        if code in (1, 2, 3, 9):
            if not flags & 1:
                raise ListError(REASON_UNSUPPORTED_OPCODE)
        elif code == 4:
            op["value"] = ob.u32()
            ob.u32()
        elif code == 5:
            ob.u32()
            n_points, n_rects = ob.u32(), ob.u32()
            ob.check(8 * n_points + 16 * n_rects)
            if 8 * n_points >= 1 << 32 or 16 * n_rects >= 1 << 32:
                raise IOError_()
            pos = []
            for _ in range(n_points):
                y, x = ob.get("2I")
                if not (x < full[0] and y < full[1]):
                    raise ListError(REASON_BAD_POINT)
                pos.append(y << 16 | x)
            for _ in range(n_rects):
                top, left, bottom, right = _roi(ob, full[0], full[1])
                pos += [y << 16 | x for y in range(top, bottom) for x in range(left, right)]
            op["positions"] = pos
        elif code == 6:
            top, left, bottom, right = op["roi"] = _roi(ob, sub[2], sub[3])
            sub = [sub[0] + left, sub[1] + top, right - left, bottom - top]
        else:
            top, left, bottom, right = op["roi"] = _roi(ob, sub[2], sub[3])
            first, planes = ob.get("2I")
            if planes == 0 or first > cpp or planes > cpp or first + planes > cpp:
                raise ListError(REASON_PLANES)
            rp, cp = ob.get("2I")
            if rp < 1 or rp > bottom - top or cp < 1 or cp > right - left:
                raise ListError(REASON_PITCH)
            op.update(first=first, planes=planes, rp=rp, cp=cp)
            if code == 7:
                n = ob.u32()
                if n == 0 or n > 65536:
                    raise ListError(REASON_TABLE_SIZE)
                t = np.array(ob.get("%dH" % n), dtype=np.uint16).reshape(-1)
                op["table"] = np.concatenate([t, np.full(65536 - n, t[-1], np.uint16)])
            elif code == 8:
                n = ob.u32() + 1
                ob.check((8 * n) & 0xFFFFFFFF)
                if n > 9:
                    raise ListError(REASON_POLY_DEGREE)
                c = np.array(ob.get("%dd" % n), dtype=np.float64).reshape(-1)
                x = np.arange(65536, dtype=np.float64) / 65536.0
                val = np.full(65536, c[0])
                for j in range(1, n):
                    val = val + c[j] * np.power(x, float(j))
                val = val * 65535.5
                op["table"] = np.where(np.isnan(val), 0, np.clip(val, 0, 65535)).astype(np.uint16)
            else:
                n = ob.u32()
                if 4 * n >= 1 << 32:
                    raise IOError_()
                ob.check(4 * n)
                extent, pitch = (right - left, cp) if code in (11, 13) else (bottom - top, rp)
                if -(-extent // pitch) != n:
                    raise ListError(REASON_DELTA_COUNT)
                d = np.array(ob.get("%df" % n), dtype=f32).reshape(-1)
                bad = ~np.isfinite(d)
                if bad.any():
                    # (the values in front of the first bad one were read: a short opcode throws
                    # IOException only if it ends before that one)
                    raise ListError(REASON_DELTA_NOT_FINITE)
                op["deltas"] = d
        if ob.remain() != 0:
            raise ListError(REASON_INCONSISTENT_LENGTH)
        out.append(op)
    return out


# ---------------------------------------------------------------------------------------
# the look-up
# ---------------------------------------------------------------------------------------
def lut(table):
    """(base, delta), 65536 entries each: TableLookUp::setTable with dither"""
    t = np.asarray(table, dtype=np.int64)
    n = t.size
    lower = np.minimum(np.concatenate([t[:1], t[:-1]]), t)
    upper = np.maximum(np.concatenate([t[1:], t[-1:]]), t)
    base = np.full(65536, t[-1], np.int64)
    delta = np.zeros(65536, np.int64)
    base[:n] = np.clip(t - (upper - lower + 2) // 4, 0, 65535)
    delta[:n] = upper - lower
    return base, delta


def dither_states(dim_x, rows, n, use_then_step=False):
    """(len(rows), n): the generator's state when doLookup looks sample x of row y up"""
    v = ((dim_x + 13 * np.asarray(rows, dtype=np.uint64)) ^ np.uint64(0x45694584)) & np.uint64(0xFFFFFFFF)
    out = np.empty((v.size, n), np.uint64)
    for x in range(n):
        if use_then_step:
            out[:, x] = v
        v = (np.uint64(15700) * (v & np.uint64(65535)) + (v >> np.uint64(16))) & np.uint64(0xFFFFFFFF)
        if not use_then_step:
            out[:, x] = v
    return out


def do_lookup(img, dim_x, rows, table, use_then_step=False, wrap=False, row0=0):
    """rows row0 .. row0 + rows - 1 of img (h, ws) uint16, whole uncropped rows"""
    base, delta = lut(table)
    ys = np.arange(row0, row0 + rows)
    v = dither_states(dim_x, ys, img.shape[1], use_then_step).astype(np.int64)
    p = img[row0:row0 + rows].astype(np.int64)
    pix = base[p] + ((delta[p] * (v & 2047) + 1024) >> 12)
    pix = pix & 0xFFFF if wrap else np.minimum(pix, 65535)
    out = img.copy()
    out[row0:row0 + rows] = pix.astype(np.uint16)
    return out


# ---------------------------------------------------------------------------------------
# the stage
# ---------------------------------------------------------------------------------------
def apply(img, cpp, crop, opcodes=None, table=None, use_then_step=False, wrap=False,
          lookup_cropped=False):
    """(status, image, info).  status IO: the file fails (image = input).  info: list_status,
    reason, n_applied, crop (x, y, w, h), bad (positions, the reference's order)."""
    img = np.array(img)
    is_f32 = img.dtype == np.float32
    h, ws = img.shape
    info = {"list_status": OK, "reason": REASON_NONE, "n_applied": 0, "crop": tuple(crop), "bad": []}
    out = img.copy()
    ops = []
    if opcodes is not None and len(opcodes):
        try:
            ops = parse(opcodes, cpp, crop, (ws // cpp, h))
        except IOError_:
            return IO, img, info
        except ListError as e:
            info.update(list_status=INVALID_ARG, reason=e.reason)
    cx, cy, cw, ch = crop
    bad = []
    for k, op in enumerate(ops):
        code = op["code"]
        reason = REASON_NONE
        if code == 4:
            reason = REASON_SETUP_NOT_U16 if is_f32 else REASON_SETUP_CPP if cpp > 1 else REASON_NONE
        elif code in (7, 8) and is_f32:
            reason = REASON_SETUP_NOT_U16
        elif code >= 10 and not is_f32:
            d = op["deltas"].astype(np.float64)
            if code <= 11:
                ok = np.abs(d) <= 65535.0 / 65535.0
            else:
                ok = (d >= 0) & (d <= (2147483647 - 512) / 65535.0 / 1024.0)
            if not ok.all():
                reason = REASON_SETUP_DELTA_RANGE
        elif code == 6:
            top, left, bottom, right = op["roi"]
            if bottom == top or right == left:
                reason = REASON_TRIM_EMPTY
        if reason:
            info.update(list_status=INVALID_ARG, reason=reason)
            break
        if code == 4:
            view = out[cy:cy + ch, cx:cx + cw]
            rr, cc = np.nonzero(view == op["value"]) if op["value"] < 65536 else ((), ())
            off = cx | cy << 16
            bad += [(off + (int(r) << 16 | int(c))) & 0xFFFFFFFF for r, c in zip(rr, cc)]
        elif code == 5:
            bad = list(op["positions"]) + bad
        elif code == 6:
            top, left, bottom, right = op["roi"]
            cx, cy, cw, ch = cx + left, cy + top, right - left, bottom - top
        elif code in (7, 8, 10, 11, 12, 13):
            top, left, bottom, right = op["roi"]
            for y in range(-(-(bottom - top) // op["rp"])):
                row = out[cy + top + op["rp"] * y]
                for x in range(-(-(right - left) // op["cp"])):
                    s = cx * cpp + op["first"] + (left + op["cp"] * x) * cpp
                    sel = slice(s, s + op["planes"])
                    if code in (7, 8):
                        row[sel] = op["table"][row[sel]]
                        continue
                    f = op["deltas"][y if code in (10, 12) else x]
                    if is_f32:
                        row[sel] = (f + row[sel]) if code <= 11 else (f * row[sel])
                    elif code <= 11:
                        row[sel] = np.clip(int(f32(65535.0) * f) + row[sel].astype(np.int64), 0, 65535)
                    else:
                        row[sel] = np.clip((int(f32(1024.0) * f) * row[sel].astype(np.int64) + 512) >> 10,
                                           0, 65535)
        info["n_applied"] = k + 1
    info["crop"] = (cx, cy, cw, ch)
    info["bad"] = bad
    if table is not None and len(table) and not is_f32:
        # (every uncropped row: APPLY_LOOKUP carries FULL_IMAGE; lookup_cropped is the model that
        # believes startWorker's `cropped` argument)
        out = do_lookup(out, ws // cpp, ch if lookup_cropped else h, table, use_then_step, wrap)
    return OK, out, info


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


# ---------------------------------------------------------------------------------------
# the cases held against the reference (tests/test_dng_post_model.py, the golden file)
# ---------------------------------------------------------------------------------------
MAX_SCALE = (2147483647 - 512) / 65535.0 / 1024.0


def _f32_below(x):
    """the largest binary32 value <= x"""
    v = f32(x)
    return v if float(v) <= x else np.nextafter(v, f32(0))


def file_cases():
    """(name, image (h, w * cpp), cpp, opcodes or None, table or None, active_area or None)"""
    rng = np.random.default_rng(0xD46)
    a = rng.integers(0, 65536, size=(20, 70)).astype(np.uint16)
    a[::4, ::3] = 7
    small = rng.integers(0, 4096, size=(6, 8)).astype(np.uint16)
    rgb = rng.integers(0, 65536, size=(12, 22 * 3)).astype(np.uint16)
    ramp = (np.arange(20 * 70) % 4096).astype(np.uint16).reshape(20, 70)
    t256 = np.sort(rng.integers(0, 65536, size=256)).astype(np.uint16)
    t4096 = np.sort(rng.integers(0, 65536, size=4096)).astype(np.uint16)
    t64k = rng.integers(0, 65536, size=65536).astype(np.uint16)
    full = (0, 0, 20, 70)
    odd = (3, 5, 18, 64)  # top, left, bottom, right
    L = opcode_list
    row_d = lambda n, lo=-1.0, hi=1.0: rng.uniform(lo, hi, size=n).astype(f32)  # noqa: E731
    up = np.nextafter
    cases = [
        ("no_list_no_table", a, 1, None, None, None),
        ("empty_entry", a, 1, b"", None, None),
        ("count_zero", a, 1, L([]), None, None),
        ("table_full", a, 1, L([op_table(full, t64k)]), None, None),
        ("table_odd_roi_pitch2", a, 1, L([op_table(odd, t256, pitch=(2, 2))]), None, None),
        ("table_pitch3", a, 1, L([op_table(odd, t4096, pitch=(3, 3))]), None, None),
        ("poly", a, 1, L([op_poly(odd, [0.01, 0.5, 0.3, -0.1])]), None, None),
        ("poly_deg8_clamps", a, 1, L([op_poly(full, [-0.2, 2.5, 0, 0, 0, 0, 0, 0, -1.0])]), None, None),
        ("offset_row", a, 1, L([op_delta(10, odd, row_d(15))]), None, None),
        ("offset_col_pitch2", a, 1, L([op_delta(11, odd, row_d(30), pitch=(1, 2))]), None, None),
        ("scale_row_pitch3", a, 1, L([op_delta(12, odd, row_d(5, 0, 3), pitch=(3, 1))]), None, None),
        ("scale_col", a, 1, L([op_delta(13, odd, row_d(59, 0, 3))]), None, None),
        ("offset_plus_minus_one", a, 1, L([op_delta(10, (0, 0, 2, 70), [1.0, -1.0])]), None, None),
        ("offset_beyond_one", a, 1, L([op_table(odd, t256), op_delta(10, (0, 0, 2, 70), [up(f32(1), f32(2)), 0.0]),
                                       op_table(full, t64k)]), None, None),
        ("scale_at_max", a, 1, L([op_delta(12, (0, 0, 1, 70), [_f32_below(MAX_SCALE)])]), None, None),
        ("scale_beyond_max", a, 1, L([op_delta(10, odd, row_d(15)),
                                      op_delta(12, (0, 0, 1, 70), [up(_f32_below(MAX_SCALE), f32(99))])]),
         None, None),
        ("scale_negative", a, 1, L([op_delta(13, (0, 0, 20, 1), [-0.5])]), None, None),
        ("rgb_planes", rgb, 3, L([op_table((1, 3, 11, 20), t256, planes=(1, 2), pitch=(2, 3)),
                                  op_delta(11, (0, 1, 12, 22), row_d(11), planes=(1, 1), pitch=(1, 2)),
                                  op_delta(12, (2, 0, 9, 21), row_d(7, 0, 2), planes=(0, 3))]), None, None),
        ("rgb_first_plane_3", rgb, 3, L([op_table((0, 0, 12, 22), t256, planes=(3, 1))]), None, None),
        ("rgb_bad_constant", rgb, 3, L([op_table((0, 0, 12, 22), t256), op_bad_constant(7)]), t256, None),
        ("several", a, 1, L([op_delta(12, odd, row_d(15, 0, 2)), op_delta(11, full, row_d(70)),
                             op_table(odd, t4096, pitch=(2, 1)), op_bad_constant(7),
                             op_poly(full, [0.0, 1.0])]), t4096, None),
        ("trim_in_the_middle", a, 1, L([op_table(full, t64k), op_trim((2, 4, 12, 44)),
                                        op_delta(10, (0, 0, 10, 40), row_d(10)),
                                        op_bad_constant(7)]), t256, None),
        ("roi_only_valid_before_trim", a, 1, L([op_trim((2, 4, 12, 44)), op_table((0, 0, 11, 40), t256)]),
         t256, None),
        ("trim_empty", a, 1, L([op_table(full, t64k), op_trim((2, 4, 2, 44))]), t256, None),
        ("active_area_table", a, 1, None, t4096, (4, 6, 16, 60)),
        ("active_area_list", a, 1, L([op_delta(10, (1, 1, 11, 50), row_d(10)), op_bad_constant(7)]),
         t4096, (4, 6, 16, 60)),
        ("table_1", ramp, 1, None, [1234], None),
        ("table_2", ramp, 1, None, [100, 60000], None),
        ("table_256", ramp, 1, None, t256, None),
        ("table_4096", ramp, 1, None, t4096, None),
        ("table_65536", a, 1, None, t64k, None),
        ("table_non_monotonic", np.ones((6, 8), np.uint16), 1, None,
         [0, 65535, 0], None),
        ("table_small_image", small, 1, None, t4096, None),
        ("bad_roi", a, 1, L([op_table((0, 0, 21, 70), t256)]), t256, None),
        ("bad_planes", a, 1, L([op_table(full, t256, planes=(0, 2))]), None, None),
        ("bad_pitch", a, 1, L([op_table(odd, t256, pitch=(16, 1))]), None, None),
        ("bad_delta_count", a, 1, L([op_delta(10, odd, row_d(14))]), None, None),
        ("bad_delta_nan", a, 1, L([op_delta(10, odd, [0.5] * 14 + [float("nan")])]), None, None),
        ("bad_table_size", a, 1, L([op_table(odd, [], count=0)]), None, None),
        ("bad_poly_degree", a, 1, L([op_poly(odd, [0.0] * 10)]), None, None),
        ("unknown_opcode", a, 1, L([op_table(full, t64k), raw(14)]), t256, None),
        ("gainmap_required", a, 1, L([raw(9, b"\0" * 8)]), None, None),
        ("gainmap_optional_empty", a, 1, L([raw(9, b"", flags=1), op_table(odd, t256)]), None, None),
        ("gainmap_optional_payload", a, 1, L([raw(9, b"\0" * 8, flags=1), op_table(odd, t256)]), None, None),
        ("inconsistent_length", a, 1, L([op_bad_constant(7)[:2] + (op_bad_constant(7)[2] + b"\0", None)]),
         None, None),
        ("bad_list", a, 1, L([op_bad_constant(7), op_bad_list([(1, 2), (19, 69)], [(2, 3, 4, 6)]),
                              op_bad_list([(0, 0)])]), None, None),
        ("bad_point_outside", a, 1, L([op_bad_list([(20, 0)])]), None, None),
        ("truncated_list", a, 1, L([op_table(full, t256)])[:-3], t256, None),
        ("truncated_count", a, 1, L([op_table(full, t256)], count=2), None, None),
        ("short_opcode", a, 1, L([raw(10, op_delta(10, odd, row_d(15))[2][:-2])]), None, None),
        ("short_header", a, 1, b"\0\0", None, None),
    ]
    fa = rng.uniform(0, 1, size=(9, 14)).astype(f32)
    cases += [
        ("f32_offset_scale", fa, 1, L([op_delta(10, (1, 1, 8, 13), row_d(7)),
                                       op_delta(13, (0, 0, 9, 14), row_d(7, 0, 3), pitch=(1, 2))]), None, None),
        ("f32_beyond_u16_limits", fa, 1, L([op_delta(11, (0, 0, 9, 14), row_d(14, -5, 5)),
                                            op_delta(12, (0, 0, 9, 14), row_d(9, -3, 40000))]), None, None),
        ("f32_table_refused", fa, 1, L([op_delta(10, (0, 0, 9, 14), row_d(9)),
                                        op_table((0, 0, 9, 14), t256),
                                        op_delta(10, (0, 0, 9, 14), row_d(9))]), None, None),
    ]
    return cases


def case_crop(case):
    name, img, cpp, opcodes, table, aa = case
    h, ws = img.shape
    if aa:
        return (aa[1], aa[0], aa[3] - aa[1], aa[2] - aa[0])
    return (0, 0, ws // cpp, h)


def case_model(case, **kw):
    name, img, cpp, opcodes, table, aa = case
    return apply(img, cpp, case_crop(case), opcodes, table, **kw)


def case_file(case):
    name, img, cpp, opcodes, table, aa = case
    return dng_post_file(img, cpp, opcodes, table, aa)
