"""Lossy-JPEG DNG tiles (include/rsx.h section 4e): the fixtures of tests/golden/dng_jpeg_ref.json
(streams and the SHA-256 of what libjpeg-turbo's default decoder, through Pillow, made of them;
scripts/record_dng_jpeg_ref.py), marker surgery for the header tests, and a numpy model of
rawspeed_amd/csrc/rsx_jpeg_core.h: the header parse, the Huffman walk of a segment,
jpeg_idct_islow, the triangle-filter upsampling and the YCbCr conversion.  Nothing here needs
Pillow."""
import base64
import hashlib
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "dng_jpeg_ref.json")
BENCH_TILE = os.path.join(HERE, "golden", "dng_jpeg_bench_tile.json")

OK, INVALID_ARG, IO, BAD_CODE, RESTART, OVERFLOW, UNSUPPORTED, TILE_ERRORS = 0, 1, 2, 3, 4, 5, 7, 9
GREY, YCBCR, RGB = 0, 1, 2
OVERSHOOT = 16383

_golden = None


def golden():
    global _golden
    if _golden is None:
        with open(GOLDEN) as f:
            _golden = json.load(f)
        for group in ("cases", "forged"):
            for c in _golden[group]:
                c["stream"] = base64.b64decode(c["stream"])
        by = {c["name"]: c["stream"] for c in _golden["cases"]}
        for c in _golden["damaged"]:  # (kept as an edit of its base)
            b = by[c["base"]]
            byte, count = c.get("repeat", (0, 0))  # (a run of one byte in front of `insert`)
            c["stream"] = b[:c["head"]] + bytes([byte]) * count + bytes.fromhex(c["insert"]) + \
                b[len(b) - c["tail"]:]
    return _golden


def cases():
    """the undamaged fixtures: dicts with name, stream, width, height, cpp, sha256"""
    return golden()["cases"]


def case(name):
    return next(c for c in cases() if c["name"] == name)


def damaged():
    """damaged streams: name, stream, cpp, and Pillow's outcome: sha256 (with width, height) or None
    for an exception"""
    return golden()["damaged"]


def forged():
    """streams no encoder writes (coefficients that overshoot): as damaged()"""
    return golden()["forged"]


def bench_tile():
    with open(BENCH_TILE) as f:
        c = json.load(f)
    c["stream"] = base64.b64decode(c["stream"])
    return c


def sha(img):
    """SHA-256 of an image's 8-bit samples, row after row (what the recorder hashed)"""
    return hashlib.sha256(np.ascontiguousarray(img).astype(np.uint8).tobytes()).hexdigest()


# ------------------------------------------------------------------------------ marker surgery
def markers(stream):
    """[(marker, offset of its FF, total length with the FF xx)] up to and including SOS"""
    out, at = [], 2
    while at + 4 <= len(stream):
        assert stream[at] == 0xFF
        m = stream[at + 1]
        n = 2 + ((stream[at + 2] << 8) | stream[at + 3])
        out.append((m, at, n))
        at += n
        if m == 0xDA:
            break
    return out


def without_marker(stream, marker):
    for m, at, n in markers(stream):
        if m == marker:
            return stream[:at] + stream[at + n:]
    raise KeyError(marker)


def with_segment(stream, marker, payload, before=0xDB):
    """a new segment in front of the first `before` marker"""
    seg = bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)
    at = next(a for m, a, _ in markers(stream) if m == before)
    return stream[:at] + seg + stream[at:]


def with_ids(stream, ids):
    """the component ids of SOF and SOS replaced"""
    s = bytearray(stream)
    for m, at, n in markers(stream):
        if m in (0xC0, 0xC1):
            for c, v in enumerate(ids):
                s[at + 10 + 3 * c] = v
        if m == 0xDA:
            for c, v in enumerate(ids):
                s[at + 5 + 2 * c] = v
    return bytes(s)


def patched(stream, marker, offset, value):
    """byte `offset` of the first `marker` segment's payload (behind its length) replaced"""
    s = bytearray(stream)
    at = next(a for m, a, _ in markers(stream) if m == marker)
    s[at + 4 + offset] = value
    return bytes(s)


JFIF_APP0 = b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0"


def adobe_app14(transform):
    return b"Adobe\0\x64\0\0\0\0" + bytes([transform])


# ---------------------------------------------------------------------------------- the model
ZZ = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20,
      13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59,
      52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


class Refused(Exception):
    def __init__(self, status):
        super().__init__(status)
        self.status = status


def _codes(bits, vals, is_dc):
    """{(length, code): symbol}; Refused(IO) for counts that are no prefix code"""
    table, code, k = {}, 0, 0
    for l in range(1, 17):
        if k >= sum(bits):
            break
        for _ in range(bits[l]):
            table[(l, code)] = vals[k]
            if is_dc and vals[k] > 15:
                raise Refused(IO)
            code += 1
            k += 1
        if code >= (1 << l):
            raise Refused(IO)  # (jpeg_make_d_derived_tbl: the all-ones code is never assigned)
        code <<= 1
    return table


def parse_header(s):
    """the markers up to SOS -> a dict; Refused(IO / UNSUPPORTED)"""
    n = len(s)
    if n < 4 or s[0] != 0xFF or s[1] != 0xD8:
        raise Refused(IO)
    H = dict(jfif=False, adobe=None, q={}, huff={}, dri=0, sof=None)
    at = 2
    while True:
        if at + 2 > n or s[at] != 0xFF:
            raise Refused(IO)
        while at < n and s[at] == 0xFF:
            at += 1
        if at >= n:
            raise Refused(IO)
        m = s[at]
        at += 1
        if m in (0, 1, 0xD8, 0xD9) or 0xD0 <= m <= 0xD7 or at + 2 > n:
            raise Refused(IO)
        ln = (s[at] << 8) | s[at + 1]
        if ln < 2 or at + ln > n:
            raise Refused(IO)
        d = s[at + 2:at + ln]
        at += ln
        if m == 0xE0:
            if len(d) >= 14 and d[:5] == b"JFIF\0":
                H["jfif"] = True
        elif m == 0xEE:
            if len(d) >= 12 and d[:5] == b"Adobe":
                H["adobe"] = d[11]
        elif m == 0xDB:
            i = 0
            while i < len(d):
                prec, idx = d[i] >> 4, d[i] & 15
                i += 1
                size = 128 if prec else 64
                if idx > 3 or prec > 1 or i + size > len(d):
                    raise Refused(IO)
                q = np.zeros(64, np.int64)
                for k in range(64):
                    q[ZZ[k]] = ((d[i + 2 * k] << 8) | d[i + 2 * k + 1]) if prec else d[i + k]
                H["q"][idx] = q
                i += size
        elif m == 0xC4:
            i = 0
            while i < len(d):
                if i + 17 > len(d):
                    raise Refused(IO)
                tc, th = d[i] >> 4, d[i] & 15
                if tc > 1 or th > 3:
                    raise Refused(IO)
                bits = [0] + list(d[i + 1:i + 17])
                i += 17
                if sum(bits) > 256 or i + sum(bits) > len(d):
                    raise Refused(IO)
                H["huff"][(tc, th)] = (bits, list(d[i:i + sum(bits)]))
                i += sum(bits)
        elif m in (0xC0, 0xC1):
            if H["sof"] is not None or len(d) < 6:
                raise Refused(IO)
            prec, h, w, nc = d[0], (d[1] << 8) | d[2], (d[3] << 8) | d[4], d[5]
            H["sof"] = True
            if prec == 12:
                raise Refused(UNSUPPORTED)
            if prec != 8 or w == 0 or h == 0 or nc == 0 or len(d) != 6 + 3 * nc:
                raise Refused(IO)
            if nc not in (1, 3):
                raise Refused(UNSUPPORTED)
            H.update(width=w, height=h, ncomp=nc)
            H["comps"] = [(d[6 + 3 * c], d[7 + 3 * c] >> 4, d[7 + 3 * c] & 15, d[8 + 3 * c]) for c in range(nc)]
            for _, hh, vv, tq in H["comps"]:
                if not (1 <= hh <= 4 and 1 <= vv <= 4 and tq <= 3):
                    raise Refused(IO)
        elif 0xC2 <= m <= 0xCF and m not in (0xC8, 0xCC):
            raise Refused(UNSUPPORTED)
        elif m == 0xDD:
            if len(d) != 2:
                raise Refused(IO)
            H["dri"] = (d[0] << 8) | d[1]
        elif m == 0xDA:
            if H["sof"] is None or len(d) < 1:
                raise Refused(IO)
            ns = d[0]
            if not 1 <= ns <= 4 or len(d) != 4 + 2 * ns:
                raise Refused(IO)
            ids = [c[0] for c in H["comps"]]
            for i in range(ns):
                if d[1 + 2 * i] not in ids:
                    raise Refused(IO)
            if ns != H["ncomp"]:
                raise Refused(UNSUPPORTED)
            H["tabs"] = []
            for i in range(ns):
                if d[1 + 2 * i] != ids[i]:
                    raise Refused(UNSUPPORTED)
                td, ta = d[2 + 2 * i] >> 4, d[2 + 2 * i] & 15
                if td > 3 or ta > 3 or (0, td) not in H["huff"] or (1, ta) not in H["huff"] or \
                        H["comps"][i][3] not in H["q"]:
                    raise Refused(IO)
                H["tabs"].append((td, ta))
            if tuple(d[1 + 2 * ns:4 + 2 * ns]) != (0, 63, 0):
                raise Refused(UNSUPPORTED)
            H["scan"] = at
            break
    if H["ncomp"] == 1:
        H["colour"], H["hs"], H["vs"] = GREY, 1, 1
    else:
        ids = [c[0] for c in H["comps"]]
        if H["jfif"]:
            H["colour"] = YCBCR
        elif H["adobe"] is not None:
            H["colour"] = RGB if H["adobe"] == 0 else YCBCR
        elif ids == [ord("R"), ord("G"), ord("B")]:
            H["colour"] = RGB
        else:
            H["colour"] = YCBCR
        H["hs"], H["vs"] = H["comps"][0][1], H["comps"][0][2]
        chroma = all(c[1] == 1 and c[2] == 1 for c in H["comps"][1:])
        if not chroma or H["hs"] > 2 or H["vs"] > 2 or (H["hs"], H["vs"]) == (1, 2):
            raise Refused(UNSUPPORTED)
        if H["colour"] == RGB and (H["hs"], H["vs"]) != (1, 1):
            raise Refused(UNSUPPORTED)
    H["mcus_x"] = -(-H["width"] // (8 * H["hs"]))
    H["mcus_y"] = -(-H["height"] // (8 * H["vs"]))
    return H


def model_validate(s, cpp):
    """rsx_dng_jpeg_validate behind the argument checks -> (status, header or None)"""
    try:
        H = parse_header(s)
        if H["ncomp"] != cpp:
            return INVALID_ARG, None
        H["dc"] = [_codes(*H["huff"][(0, td)], True) for td, _ in H["tabs"]]
        H["ac"] = [_codes(*H["huff"][(1, ta)], False) for _, ta in H["tabs"]]
    except Refused as r:
        return r.status, None
    return OK, H


def segments(s, H):
    """[(first MCU, MCUs, start, end)]; Refused(RESTART / OVERFLOW)"""
    mcus = H["mcus_x"] * H["mcus_y"]
    per = H["dri"] or mcus
    n_seg = -(-mcus // per)
    out, seg, start, at, n = [], 0, H["scan"], H["scan"], len(s)
    while True:
        at = s.find(b"\xff", at)
        if at < 0:
            raise Refused(OVERFLOW)
        j = at + 1
        while j < n and s[j] == 0xFF:
            j += 1
        if j >= n:
            raise Refused(OVERFLOW)
        m = s[j]
        if m == 0:
            at = j + 1
            continue
        last = seg + 1 == n_seg
        if m == 0xD9:
            if not last:
                raise Refused(OVERFLOW)
        elif 0xD0 <= m <= 0xD7:
            if last or not H["dri"] or m != 0xD0 + (seg & 7):
                raise Refused(RESTART)
        else:
            raise Refused(RESTART)
        out.append((seg * per, mcus - seg * per if last else per, start, at))
        if last:
            return out
        seg += 1
        start = at = j + 1


class _Bits:
    def __init__(self, s, start, end):
        data, i = bytearray(), start
        while i < end:
            b = s[i]
            if b == 0xFF:
                j = i + 1
                while j < end and s[j] == 0xFF:
                    j += 1
                if j < end and s[j] == 0:
                    i = j + 1
                else:
                    break
            else:
                i += 1
            data.append(b)
        self.n = 8 * len(data)
        self.v = int.from_bytes(bytes(data) + b"\0\0\0\0", "big")
        self.total = self.n + 32
        self.at = 0

    def peek(self, k):
        return (self.v >> (self.total - self.at - k)) & ((1 << k) - 1)

    def symbol(self, table):
        for l in range(1, 17):
            sym = table.get((l, self.peek(l)))
            if sym is not None:
                if self.at + l > self.n:
                    raise Refused(OVERFLOW)
                self.at += l
                return sym
        raise Refused(BAD_CODE)

    def extend(self, k):
        if self.at + k > self.n:
            raise Refused(OVERFLOW)
        r = self.peek(k)
        self.at += k
        return r if r >= (1 << (k - 1)) else r - (1 << k) + 1


def _block(B, dc, ac, pred):
    coef = np.zeros(64, np.int64)
    k = B.symbol(dc)
    if k:
        pred += B.extend(k)
        if not -32768 <= pred <= 32767:
            raise Refused(UNSUPPORTED)
    coef[0] = pred
    k = 1
    while k < 64:
        rs = B.symbol(ac)
        r, size = rs >> 4, rs & 15
        if size:
            k += r
            if k > 63:
                raise Refused(BAD_CODE)
            coef[ZZ[k]] = B.extend(size)
        else:
            if r != 15:
                break
            k += 15
            if k > 63:
                raise Refused(BAD_CODE)
        k += 1
    return coef, pred


def _idct_pass(x, shift):
    """jpeg_idct_islow's one-dimensional pass over the last axis"""
    i = [x[..., k] for k in range(8)]
    z1 = (i[2] + i[6]) * 4433
    tmp2, tmp3 = z1 - i[6] * 15137, z1 + i[2] * 6270
    tmp0, tmp1 = (i[0] + i[4]) << 13, (i[0] - i[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    out = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0,
           tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
    return np.stack([(o + (1 << (shift - 1))) >> shift for o in out], axis=-1)


def idct(coef, q, limit="saturate"):
    """(n, 64) coefficients in natural order -> ((n, 8, 8) samples, whether all stayed inside
    +-OVERSHOOT).  limit: "saturate" (libjpeg-turbo's SIMD code) or "mask" (its C code's table)"""
    d = (coef * q).reshape(-1, 8, 8)
    ok = np.abs(d).max(initial=0) <= OVERSHOOT
    ws = _idct_pass(d.transpose(0, 2, 1), 11).transpose(0, 2, 1)  # columns
    ok = ok and np.abs(ws).max(initial=0) <= OVERSHOOT
    v = _idct_pass(ws, 18)
    if limit == "saturate":
        return np.clip(v + 128, 0, 255), ok
    x = v & 1023
    return np.where(x < 128, x + 128, np.where(x < 512, 255, np.where(x < 896, 0, x - 896))), ok


def _upsample(p, hs, vs, w, h):
    """plane p (its own size) to w x h: jdsample.c's fancy filters above two samples a row"""
    p = p.astype(np.int64)
    dh, dw = p.shape
    if hs == 1:
        return p[:h, :w]
    if dw <= 2:
        out = np.repeat(p, 2, axis=1)
        return (np.repeat(out, 2, axis=0) if vs == 2 else out)[:h, :w]
    if vs == 1:
        rows = [p]
    else:
        up = np.vstack([p[:1], p[:-1]])
        down = np.vstack([p[1:], p[-1:]])
        rows = [3 * p + up, 3 * p + down]
    outs = []
    for r in rows:
        left = np.hstack([r[:, :1], r[:, :-1]])
        right = np.hstack([r[:, 1:], r[:, -1:]])
        if vs == 1:
            even, odd = (3 * r + left + 1) >> 2, (3 * r + right + 2) >> 2
            even[:, 0], odd[:, -1] = r[:, 0], r[:, -1]
        else:
            even, odd = (3 * r + left + 8) >> 4, (3 * r + right + 7) >> 4
            even[:, 0], odd[:, -1] = (4 * r[:, 0] + 8) >> 4, (4 * r[:, -1] + 7) >> 4
        o = np.empty((dh, 2 * dw), np.int64)
        o[:, 0::2], o[:, 1::2] = even, odd
        outs.append(o)
    if vs == 1:
        return outs[0][:h, :w]
    full = np.empty((2 * dh, 2 * dw), np.int64)
    full[0::2], full[1::2] = outs[0], outs[1]
    return full[:h, :w]


def model_decode(s, cpp, limit="saturate"):
    """-> (status, the whole frame as (height, width * cpp) uint16 or None)"""
    st, H = model_validate(s, cpp)
    if st != OK:
        return st, None
    try:
        segs = segments(s, H)
    except Refused as r:
        return r.status, None
    nc, hs, vs = H["ncomp"], H["hs"], H["vs"]
    shape = [(H["mcus_y"] * 8 * (vs if c == 0 else 1), H["mcus_x"] * 8 * (hs if c == 0 else 1))
             for c in range(nc)]
    planes = [np.zeros(sh, np.int64) for sh in shape]
    layout = [(0, bx, by) for by in range(vs) for bx in range(hs)] if nc == 3 else [(0, 0, 0)]
    if nc == 3:
        layout += [(1, 0, 0), (2, 0, 0)]
    verdict = OK
    for first, count, start, end in segs:
        B = _Bits(s, start, end)
        pred = [0, 0, 0]
        coefs, where = [], []
        try:
            for mcu in range(first, first + count):
                mx, my = mcu % H["mcus_x"], mcu // H["mcus_x"]
                for c, bx, by in layout:
                    coef, pred[c] = _block(B, H["dc"][c], H["ac"][c], pred[c])
                    coefs.append(coef)
                    where.append((c, mx * (hs if c == 0 else 1) + bx, my * (vs if c == 0 else 1) + by))
        except Refused as r:
            verdict = max(verdict, r.status)
            continue
        for c in range(nc):
            sel = [k for k, w in enumerate(where) if w[0] == c]
            if not sel:
                continue
            px, ok = idct(np.stack([coefs[k] for k in sel]), H["q"][H["comps"][c][3]], limit)
            if not ok:
                verdict = max(verdict, UNSUPPORTED)
            for k, blk in zip(sel, px):
                _, bx, by = where[k]
                planes[c][8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = blk
    if verdict != OK:
        return verdict, None
    w, h = H["width"], H["height"]
    if nc == 1:
        return OK, planes[0][:h, :w].astype(np.uint16)
    y = planes[0][:h, :w]
    cw, ch = -(-w // hs), -(-h // vs)
    cb = _upsample(planes[1][:ch, :cw], hs, vs, w, h)
    cr = _upsample(planes[2][:ch, :cw], hs, vs, w, h)
    if H["colour"] == RGB:
        rgb = [y, cb, cr]
    else:
        cb, cr = cb - 128, cr - 128
        rgb = [y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb + 32768 - 46802 * cr) >> 16),
               y + ((116130 * cb + 32768) >> 16)]
    out = np.clip(np.stack(rgb, axis=-1), 0, 255).astype(np.uint16)
    return OK, out.reshape(h, 3 * w)


def paste(img, got, off_x, off_y, cpp):
    """the window JpegDecompressor::decode copies: frame `got` at (off_x, off_y) into img (rows of
    samples), cut at the image's right and bottom edge"""
    h = min(img.shape[0] - off_y, got.shape[0])
    w = min(img.shape[1] // cpp - off_x, got.shape[1] // cpp)
    img[off_y:off_y + h, cpp * off_x:cpp * (off_x + w)] = got[:h, :cpp * w]
    return w, h
