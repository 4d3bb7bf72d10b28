"""Baseline-DCT JPEG tile writer (include/rsx.h section 7e): the fixtures of
tests/golden/dctwrite_ref.json (inputs, the stream Pillow's encoder -- libjpeg-turbo -- wrote for
each, and the SHA-256 of Pillow's decode of it; scripts/record_dctwrite_ref.py), a numpy model of
rawspeed_amd/csrc/rsx_dctwrite_core.h (the checks, the container, jccolor, jcsample, jfdctint, the
quantiser, the scan order with its dummy blocks and the Huffman step), and the ctypes side of the
host build and the device calls.  Nothing here needs Pillow."""
import base64
import ctypes as C
import json
import os

import numpy as np

from rawspeed_amd import abi, build

import dng_jpeg_files as J

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "dctwrite_ref.json")

OK, INVALID_ARG, OVERFLOW, UNSUPPORTED, TILE_ERRORS, VALUE_RANGE = 0, 1, 5, 7, 9, 10
JFIF = abi.DCTWRITE_JFIF
SAMPLINGS = {0: (1, 1), 1: (2, 1), 2: (2, 2)}  # Pillow's subsampling= -> luma against chroma
COVERAGE = ("dc_category_11", "ac_size_10", "zrl", "no_eob", "stuffed_ff_in_data",
            "stuffed_ff_in_padding", "pad_0", "pad_1", "pad_2", "pad_3", "pad_4", "pad_5", "pad_6",
            "pad_7", "nine_intervals", "short_last_interval", "dummy_right_h2v1", "dummy_right_h2v2",
            "dummy_bottom_h2v2", "dummy_corner_h2v2")

ZZ = J.ZZ

# T.81 Annex K.1 and K.3
STD_LUMA_Q = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57,
              69, 56, 14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55,
              64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103,
              99]
STD_CHROMA_Q = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99,
                99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
DC_VALS = list(range(12))
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d],
           [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77])
AC_VALS = (bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728"
    "292a3435363738393a434445464748494a535455565758595a636465666768696a737475767778797a83848586878889"
    "8a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2"
    "e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"), bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a26"
    "2728292a35363738393a434445464748494a535455565758595a636465666768696a737475767778797a828384858687"
    "88898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9da"
    "e2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))


def _enc_table(bits, vals):
    """{symbol: (code, length)}"""
    out, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            out[vals[k]] = (code, l)
            code += 1
            k += 1
        code <<= 1
    return out


DC_ENC = [_enc_table(DC_BITS[t], DC_VALS) for t in (0, 1)]
AC_ENC = [_enc_table(AC_BITS[t], AC_VALS[t]) for t in (0, 1)]

_golden = None


def golden():
    global _golden
    if _golden is None:
        with open(GOLDEN) as f:
            _golden = json.load(f)
        for c in _golden["cases"]:
            c["stream"] = base64.b64decode(c["stream"])
            shape = (c["dim_y"], c["dim_x"]) if c["cpp"] == 1 else (c["dim_y"], c["dim_x"], 3)
            c["pixels"] = np.frombuffer(base64.b64decode(c["pixels"]), np.uint8).reshape(shape)
    return _golden


def cases():
    """the fixtures: dicts with name, pixels (dim_y, dim_x[, 3]) uint8, cpp, frame (off_x, off_y,
    width, height), subsampling (Pillow's 0 / 1 / 2), quality or qtables (two natural-order lists),
    restart (MCUs), stream (with APP0), sha256 (of Pillow's decode)"""
    return golden()["cases"]


def case(name):
    return next(c for c in cases() if c["name"] == name)


def quality_dqt(quality):
    """the payloads of the two DQT segments (zig-zag order) of Pillow's stream for quality="""
    raw = bytes.fromhex(golden()["quality_dqt"][quality - 1])
    return list(raw[:64]), list(raw[64:])


def tables_of(c):
    if c.get("qtables"):
        return [list(t) for t in c["qtables"]]
    return list(model_quality_tables(c["quality"]))


# ------------------------------------------------------------------------------------- the model
def model_quality_tables(quality):
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple([min(max((v * scale + 50) // 100, 1), 255) for v in t]
                 for t in (STD_LUMA_Q, STD_CHROMA_Q))


def model_validate(desc, img):
    """rsx_dctwrite_validate on dicts: desc has off_x, off_y, width, height, components, h_samp,
    v_samp, restart_interval, flags, reserved, qtables; img has dim_x, dim_y, cpp, pitch_bytes"""
    if desc is None or img is None:
        return INVALID_ARG
    if img["dim_x"] < 1 or img["dim_y"] < 1 or img["cpp"] < 1 or img["pitch_bytes"] % 2 or \
            img["pitch_bytes"] < 2 * img["cpp"] * img["dim_x"]:
        return INVALID_ARG
    if desc["components"] != img["cpp"]:
        return INVALID_ARG
    if desc["off_x"] >= img["dim_x"] or desc["off_y"] >= img["dim_y"]:
        return INVALID_ARG
    if not (1 <= desc["width"] <= 65535 and 1 <= desc["height"] <= 65535):
        return INVALID_ARG
    if desc["restart_interval"] > 65535:
        return INVALID_ARG
    if desc["flags"] & ~JFIF or desc["reserved"]:
        return INVALID_ARG
    for t in range(2 if desc["components"] > 1 else 1):
        if any(not 1 <= v <= 255 for v in desc["qtables"][t]):
            return INVALID_ARG
    if desc["components"] not in (1, 3):
        return UNSUPPORTED
    s = (desc["h_samp"], desc["v_samp"])
    if s not in ((1, 1), (2, 1), (2, 2)) or (desc["components"] == 1 and s != (1, 1)):
        return UNSUPPORTED
    return OK


def model_header(width, height, comps, hs, vs, tables, restart, jfif):
    o = bytearray(b"\xff\xd8")
    if jfif:
        o += b"\xff\xe0\x00\x10" + J.JFIF_APP0
    nt = 2 if comps > 1 else 1
    for t in range(nt):
        o += bytes([0xFF, 0xDB, 0, 67, t]) + bytes(tables[t][ZZ[i]] for i in range(64))
    o += bytes([0xFF, 0xC0, 0, 8 + 3 * comps, 8, height >> 8, height & 255, width >> 8, width & 255, comps])
    for c in range(comps):
        o += bytes([c + 1, (hs << 4 | vs) if c == 0 else 0x11, 0 if c == 0 else 1])
    for t in range(nt):
        o += bytes([0xFF, 0xC4, 0, 31, t]) + bytes(DC_BITS[t]) + bytes(DC_VALS)
        o += bytes([0xFF, 0xC4, 0, 181, 0x10 | t]) + bytes(AC_BITS[t]) + bytes(AC_VALS[t])
    if restart:
        o += bytes([0xFF, 0xDD, 0, 4, restart >> 8, restart & 255])
    o += bytes([0xFF, 0xDA, 0, 6 + 2 * comps, comps])
    for c in range(comps):
        o += bytes([c + 1, 0x00 if c == 0 else 0x11])
    return bytes(o + b"\x00\x3f\x00")


def model_frame(px, cpp, frame):
    """the frame's pixels (height, width, cpp) int64: a pixel outside the image is the nearest one"""
    off_x, off_y, w, h = frame
    a = np.asarray(px).astype(np.int64).reshape(px.shape[0], -1, cpp)
    ys = np.minimum(off_y + np.arange(h), a.shape[0] - 1)
    xs = np.minimum(off_x + np.arange(w), a.shape[1] - 1)
    return a[ys][:, xs]


def _planes(f, hs, vs):
    """the component planes, each edge-replicated to whole blocks: [(plane, width_in_blocks,
    height_in_blocks)]"""
    h, w, n = f.shape

    def whole(p):
        hb, wb = -(-p.shape[0] // 8), -(-p.shape[1] // 8)
        return np.pad(p, ((0, 8 * hb - p.shape[0]), (0, 8 * wb - p.shape[1])), mode="edge"), wb, hb

    if n == 1:
        return [whole(f[..., 0])]
    r, g, b = f[..., 0], f[..., 1], f[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16
    out = [whole(y)]
    for p in (cb, cr):
        if hs * vs > 1:
            cw, ch = -(-w // hs), -(-h // vs)
            wb = -(-cw // 8)
            # columns replicated at full resolution to 2 x 8 wb, rows to vs ch; rows of whole blocks
            # are replicated behind the filter (whole())
            p = np.pad(p, ((0, vs * ch - h), (0, 2 * 8 * wb - w)), mode="edge")
            if vs == 2:
                bias = np.tile([1, 2], 4 * wb)
                p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
            else:
                bias = np.tile([0, 1], 4 * wb)
                p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
        out.append(whole(p))
    return out


def _fdct_pass(d, first):
    """jfdctint over the last axis of d (..., 8), python-int exact in int64"""
    cb, p1 = 13, 2
    sh = cb - p1 if first else cb + p1

    def ds(x, n):
        return (x + (1 << (n - 1))) >> n

    t0, t7, t1, t6 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7], d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5, t3, t4 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5], d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = np.zeros_like(d)
    if first:
        o[..., 0], o[..., 4] = (t10 + t11) << p1, (t10 - t11) << p1
    else:
        o[..., 0], o[..., 4] = ds(t10 + t11, p1), ds(t10 - t11, p1)
    z1 = (t12 + t13) * 4433
    o[..., 2] = ds(z1 + t13 * 6270, sh)
    o[..., 6] = ds(z1 - t12 * 15137, sh)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[..., 7], o[..., 5] = ds(t4 + z1 + z3, sh), ds(t5 + z2 + z4, sh)
    o[..., 3], o[..., 1] = ds(t6 + z2 + z3, sh), ds(t7 + z1 + z4, sh)
    return o


def model_coefficients(f, hs, vs, tables):
    """[(coef (hb, wb, 64) zig-zag int64, wb, hb)] per component of frame f"""
    out = []
    for c, (p, wb, hb) in enumerate(_planes(f, hs, vs)):
        b = (p - 128).reshape(hb, 8, wb, 8).transpose(0, 2, 1, 3)  # (hb, wb, row, col)
        b = _fdct_pass(b, True)
        b = _fdct_pass(b.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)
        q = np.array(tables[1 if c else 0], np.int64).reshape(8, 8)
        v = np.sign(b) * ((np.abs(b) + 4 * q) // (8 * q))
        out.append((v.reshape(hb, wb, 64)[..., ZZ], wb, hb))
    return out


class _Writer:
    def __init__(self):
        self.out, self.acc, self.n, self.bits = bytearray(), 0, 0, 0

    def put(self, v, n):
        self.acc, self.n, self.bits = (self.acc << n) | v, self.n + n, self.bits + n
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 255
            self.out.append(b)
            if b == 255:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def close(self):
        pad = -self.n % 8
        if pad:
            self.put((1 << pad) - 1, pad)
            self.bits -= pad
        return pad


def _value(v, n):
    return (v - 1 if v < 0 else v) & ((1 << n) - 1)


def _put_block(W, t, diff, zz):
    n = abs(int(diff)).bit_length()
    W.put(*DC_ENC[t][n])
    if n:
        W.put(_value(int(diff), n), n)
    run = 0
    if zz is None:
        run = 63
    else:
        for k in range(1, 64):
            v = int(zz[k])
            if v == 0:
                run += 1
                continue
            while run > 15:
                W.put(*AC_ENC[t][0xF0])
                run -= 16
            n = abs(v).bit_length()
            W.put(*AC_ENC[t][run << 4 | n])
            W.put(_value(v, n), n)
            run = 0
    if run:
        W.put(*AC_ENC[t][0])


def model_stream(px, cpp, frame, hs, vs, tables, restart=0, jfif=True, stats=None):
    """the stream of section 7e for image px (dim_y, dim_x[, 3]); stats (a dict) gets symbol_bits,
    scan_bytes, pads (the 1-bits that close each interval) and dummies (a set of 'right' / 'bottom' /
    'corner')"""
    f = model_frame(px, cpp, frame)
    h, w, _ = f.shape
    comp = model_coefficients(f, hs, vs, tables)
    mcus_x, mcus_y = -(-w // (8 * hs)), -(-h // (8 * vs))
    n_mcu = mcus_x * mcus_y
    per = restart or n_mcu
    layout = [(0, bx, by) for by in range(vs) for bx in range(hs)] if cpp == 3 else [(0, 0, 0)]
    if cpp == 3:
        layout += [(1, 0, 0), (2, 0, 0)]
    head = model_header(w, h, cpp, hs, vs, tables, restart, jfif)
    W = _Writer()
    pads, dummies, pred = [], set(), [0, 0, 0]
    for m in range(n_mcu):
        if m % per == 0:
            if m:
                pads.append(W.close())
                W.out += bytes([0xFF, 0xD0 + (m // per - 1) % 8])
            pred = [0, 0, 0]
        mx, my = m % mcus_x, m // mcus_x
        for c, kx, ky in layout:
            coef, wb, hb = comp[c]
            bx, by = mx * (hs if c == 0 else 1) + kx, my * (vs if c == 0 else 1) + ky
            t = 1 if c else 0
            if bx >= wb or by >= hb:
                dummies.add("corner" if bx >= wb and by >= hb else "right" if bx >= wb else "bottom")
                _put_block(W, t, 0, None)
                continue
            zz = coef[by, bx]
            _put_block(W, t, zz[0] - pred[c], zz)
            pred[c] = zz[0]
    pads.append(W.close())
    if stats is not None:
        stats.update(symbol_bits=W.bits, scan_bytes=len(W.out), pads=pads, dummies=dummies)
    return head + bytes(W.out) + b"\xff\xd9"


def model_case(c, jfif=True, restart=None, stats=None):
    hs, vs = SAMPLINGS[c["subsampling"]]
    return model_stream(c["pixels"], c["cpp"], c["frame"], hs, vs, tables_of(c),
                        c["restart"] if restart is None else restart, jfif, stats)


def model_bound(frame, cpp, hs, vs, restart, jfif):
    w, h = frame[2], frame[3]
    n_mcu = -(-w // (8 * hs)) * -(-h // (8 * vs))
    blocks = n_mcu * (1 if cpp == 1 else hs * vs + 2)
    n_int = -(-n_mcu // (restart or n_mcu))
    head = len(model_header(w, h, cpp, hs, vs, ([1] * 64, [1] * 64), restart, jfif))
    return head + 416 * blocks + 4 * n_int + 2


# ------------------------------------------------------------------------------ the ctypes side
class Img:
    """a uint16 image in host memory with `pad` samples behind every row"""

    def __init__(self, px, cpp, pad=0):
        a = np.asarray(px).astype(np.uint16).reshape(np.asarray(px).shape[0], -1)
        self.cpp, self.dim_y, self.dim_x = cpp, a.shape[0], a.shape[1] // cpp
        self.buf = np.full((self.dim_y, a.shape[1] + pad), 0x5A5A, np.uint16)
        self.buf[:, :a.shape[1]] = a
        self.pitch_bytes = 2 * self.buf.shape[1]

    def view(self, data=None):
        return abi.Image(self.buf.ctypes.data if data is None else data, self.pitch_bytes, self.dim_x,
                         self.dim_y, self.cpp, 0)

    def as_dict(self):
        return dict(dim_x=self.dim_x, dim_y=self.dim_y, cpp=self.cpp, pitch_bytes=self.pitch_bytes)


def desc_of(c, jfif=True, restart=None):
    hs, vs = SAMPLINGS[c["subsampling"]]
    lu, ch = tables_of(c)
    return abi.dctwrite_desc(*c["frame"], c["cpp"], hs, vs, lu, ch,
                             c["restart"] if restart is None else restart, JFIF if jfif else 0)


def desc_dict(d):
    return dict(off_x=d.off_x, off_y=d.off_y, width=d.width, height=d.height,
                components=d.components, h_samp=d.h_samp, v_samp=d.v_samp,
                restart_interval=d.restart_interval, flags=d.flags, reserved=d.reserved,
                qtables=[list(d.qtables[0]), list(d.qtables[1])])


_host = None


def host_lib():
    global _host
    if _host is None:
        build.build_dctwrite_host()
        L = C.CDLL(build.LIB_DCTWRITE_HOST)
        L.rsx_dctwrite_host_bound.restype = C.c_uint64
        L.rsx_dctwrite_host_bound.argtypes = [C.c_void_p, C.c_void_p]
        L.rsx_dctwrite_host_validate.argtypes = [C.c_void_p, C.c_void_p]
        L.rsx_dctwrite_host_quality_tables.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
        L.rsx_dctwrite_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        _host = L
    return _host


def host_encode(desc, img, cap=None, guard=16):
    """the host build's stream -> (status, bytes written as np.uint8, abi.DctWriteResult, whether the
    `guard` bytes behind `cap` are untouched)"""
    L = host_lib()
    view = img.view()
    if cap is None:
        cap = int(L.rsx_dctwrite_host_bound(C.byref(desc), C.byref(view)))
    out = np.full(cap + guard, 0xA5, np.uint8)
    r = abi.DctWriteResult()
    st = L.rsx_dctwrite_host(C.byref(desc), C.byref(view), C.c_void_p(out.ctypes.data), cap, C.byref(r))
    return st, out[:r.bytes].copy(), r, bool(np.all(out[cap:] == 0xA5))


def tiled(c, nx, ny):
    """fixture c's image repeated nx x ny times, as a case over the whole of it (no recorded stream:
    the model supplies the bytes)"""
    reps = (ny, nx) if c["cpp"] == 1 else (ny, nx, 1)
    px = np.tile(c["pixels"], reps)
    return dict(c, name="%s_x%dx%d" % (c["name"], nx, ny), pixels=px, dim_x=c["dim_x"] * nx,
                dim_y=c["dim_y"] * ny, frame=[0, 0, c["dim_x"] * nx, c["dim_y"] * ny], stream=None,
                sha256=None)
