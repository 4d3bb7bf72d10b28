"""The writers of F32 images (include/rsx.h section 7d): the numpy model of the exact narrowing
and of the packed stream, the host build of the core (rawspeed_amd/librsx_fpwrite_host.so), and
the case lists the CPU and GPU tests share.

The model narrows by search, not by arithmetic: the images of all patterns of a narrow format,
widened by model_widen, form a strictly increasing table per sign; a binary32 sample has a narrow
pattern iff its magnitude is in the table, and the pattern is its index.  model_widen restates
extendBinaryFloatingPoint (common/FloatingPoint.h:109-145) with the subnormals taken through
float64 arithmetic, and tests/test_fpwrite_model.py holds it against the oracle's F32 unpack."""
import ctypes as C
import zlib

import numpy as np

from rawspeed_amd import abi, build

OK, INVALID_ARG, IO = abi.RSX_OK, abi.RSX_ERR_INVALID_ARG, abi.RSX_ERR_IO
VALUE_RANGE = abi.RSX_ERR_VALUE_RANGE
BPS = (16, 24, 32)
FORMAT = {16: (10, 5), 24: (16, 7)}  # fraction bits, exponent bits
ORDERS = (abi.ORDER_LSB, abi.ORDER_MSB)

_host = None


def host():
    global _host
    if _host is None:
        lib, _ = build.build_fpwrite_host()
        L = C.CDLL(lib)
        L.rsx_fpwrite_host_narrow.argtypes = [C.c_uint32, C.c_int, C.c_void_p]
        L.rsx_fpwrite_host_widen.argtypes = [C.c_uint32, C.c_int]
        L.rsx_fpwrite_host_widen.restype = C.c_uint32
        L.rsx_fpwrite_host_widen_range.argtypes = [C.c_uint32, C.c_size_t, C.c_int, C.c_void_p]
        L.rsx_fpwrite_host_widen_range.restype = None
        L.rsx_fpwrite_host_fit_class_many.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
        L.rsx_fpwrite_host_fit_class_many.restype = None
        L.rsx_fpwrite_host_narrow_many.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p,
                                                   C.c_void_p]
        L.rsx_fpwrite_host_narrow_many.restype = None
        L.rsx_fpwrite_host_pack_validate.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.rsx_fpwrite_host_pack.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                            C.c_void_p]
        L.rsx_fpwrite_host_fit.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _host = L
    return _host


def pack_block_bytes():
    """output bytes a workgroup of the pack kernel covers"""
    return host().rsx_fpwrite_host_pack_block_bytes()


def fit_block_samples():
    """samples of a piece of the fit kernel"""
    return host().rsx_fpwrite_host_fit_block_samples()


def seed_of(name):
    return zlib.crc32(name.encode())


def round_up4(n):
    return (n + 3) // 4 * 4


# ---------------------------------------------------------------------------------------------
# the model of the narrowing
# ---------------------------------------------------------------------------------------------
def model_widen(narrow, bps):
    """narrow patterns (uint32, any shape) -> binary32 patterns"""
    n = np.asarray(narrow, dtype=np.uint32)
    if bps == 32:
        return n.copy()
    frac, expw = FORMAT[bps]
    bias, emax = (1 << (expw - 1)) - 1, (1 << expw) - 1
    sign = (n >> np.uint32(frac + expw)) & np.uint32(1)
    ne = (n >> np.uint32(frac)) & np.uint32(emax)
    nf = n & np.uint32((1 << frac) - 1)
    normal = ((ne + np.uint32(127 - bias)) << np.uint32(23)) | (nf << np.uint32(23 - frac))
    special = np.uint32(0x7F800000) | (nf << np.uint32(23 - frac))
    # a subnormal is nf 2^(1 - bias - frac): a binary32 normal, exact through float64
    sub = (nf.astype(np.float64) * 2.0 ** (1 - bias - frac)).astype(np.float32).view(np.uint32)
    mag = np.where(ne == emax, special, np.where(ne == 0, sub, normal)).astype(np.uint32)
    return (mag | (sign << np.uint32(31))).astype(np.uint32)


_tables = {}


def magnitude_table(bps):
    """the images of the non-negative patterns of the narrow format, in pattern order"""
    if bps not in _tables:
        t = model_widen(np.arange(1 << (bps - 1), dtype=np.uint32), bps)
        assert (np.diff(t.astype(np.int64)) > 0).all()  # one image a pattern, in order
        _tables[bps] = t
    return _tables[bps]


def model_narrow(x, bps):
    """binary32 patterns -> (narrow patterns, exact): exact[i] iff x[i] is an image of the widening;
    the pattern of an inexact sample is 0"""
    x = np.asarray(x, dtype=np.uint32)
    if bps == 32:
        return x.copy(), np.ones(x.shape, dtype=bool)
    t = magnitude_table(bps)
    mag = x & np.uint32(0x7FFFFFFF)
    idx = np.minimum(np.searchsorted(t, mag), len(t) - 1)
    exact = t[idx] == mag
    n = idx.astype(np.uint32) | ((x >> np.uint32(31)) << np.uint32(bps - 1))
    return np.where(exact, n, 0).astype(np.uint32), exact


def model_fit(x):
    """the least of 16 / 24 / 32 under which every sample narrows exactly"""
    for bps in (16, 24):
        if model_narrow(x, bps)[1].all():
            return bps
    return 32


def specials(bps):
    """narrow patterns at the edges: zeros, subnormals, the least and greatest normals, infinities,
    NaN payloads"""
    if bps == 32:
        return np.array([0, 1 << 31, 1, 0x7FFFFF, 0x800000, 0x7F7FFFFF, 0x7F800000, 0xFF800000,
                         0x7F800001, 0x7FC00000, 0xFFFFFFFF], dtype=np.uint32)
    frac, expw = FORMAT[bps]
    top = ((1 << expw) - 1) << frac
    mags = [0, 1, 2, (1 << frac) - 1, 1 << frac, top - 1, top, top | 1, top | (1 << (frac - 1)),
            top | ((1 << frac) - 1)]
    return np.array(mags + [m | (1 << (bps - 1)) for m in mags], dtype=np.uint32)


def exact_samples(name, bps, rows, cols):
    """(rows, cols) binary32 patterns that all narrow exactly under bps, the specials planted"""
    rng = np.random.default_rng(seed_of(name))
    n = rng.integers(0, 1 << bps, (rows, cols), dtype=np.uint64).astype(np.uint32)
    flat = n.reshape(-1)
    for k, v in enumerate(specials(bps)):
        flat[(k * 7919) % flat.size] = v
    return model_widen(n, bps)


# ---------------------------------------------------------------------------------------------
# images and packed streams
# ---------------------------------------------------------------------------------------------
class Img32:
    """An F32 image of dim_y rows of dim_x * cpp 4-byte samples in a buffer of pitch bytes a row"""

    def __init__(self, px, cpp=1, pad=0):
        px = np.ascontiguousarray(px, dtype=np.uint32)
        self.dim_y, n = px.shape
        assert n % cpp == 0 and pad % 4 == 0
        self.dim_x, self.cpp = n // cpp, cpp
        self.pitch = 4 * n + pad
        self.buf = np.full(self.pitch * self.dim_y, 0xA5, dtype=np.uint8)
        self.buf.reshape(self.dim_y, self.pitch)[:, :4 * n] = px.view(np.uint8)
        self.px = px

    def view(self, ptr=None):
        return abi.Image(self.buf.ctypes.data if ptr is None else ptr, self.pitch, self.dim_x,
                         self.dim_y, self.cpp, 0)


def pack_desc(crop_x, crop_y, w, h, pitch, bps, order):
    return abi.UnpackDesc(crop_x, crop_y, w, h, pitch, bps, order)


def first_sample(desc, cpp):
    """copyPixels starts at offset.x * cpp, decodePackedFP at offset.x"""
    return desc.crop_x * cpp if desc.bits_per_pixel == 32 else desc.crop_x


def window_of(desc, img):
    """the samples a descriptor writes: (crop_h, crop_w cpp) binary32 patterns"""
    x0 = first_sample(desc, img.cpp)
    return img.px[desc.crop_y:desc.crop_y + desc.crop_h, x0:x0 + desc.crop_w * img.cpp]


def model_pack(desc, img):
    """-> (the stream, roundUp(crop_h pitch, 4) bytes, and the count of inexact samples)"""
    bps, pitch = desc.bits_per_pixel, desc.input_pitch_bytes
    n, exact = model_narrow(window_of(desc, img), bps)
    bytesps = bps // 8
    big = bps != 32 and desc.bit_order == abi.ORDER_MSB
    shifts = [8 * (bytesps - 1 - j) if big else 8 * j for j in range(bytesps)]
    data = np.stack([(n >> np.uint32(s)) & np.uint32(0xFF) for s in shifts], axis=2).astype(np.uint8)
    h = desc.crop_h
    stream = np.zeros(round_up4(h * pitch), dtype=np.uint8)
    stream[:h * pitch].reshape(h, pitch)[:, :n.shape[1] * bytesps] = data.reshape(h, -1)
    return stream, int((~exact).sum())


def host_pack(desc, img, cap=None, guard=16):
    """rsx_fpwrite_host_pack -> (status, the whole guarded buffer, abi.FpWritePackResult)"""
    need = round_up4(max(desc.crop_h, 0) * max(desc.input_pitch_bytes, 0))
    cap = need if cap is None else cap
    out = np.full(cap + guard, 0x5A, dtype=np.uint8)
    r = abi.FpWritePackResult()
    v = img.view()
    st = host().rsx_fpwrite_host_pack(C.byref(desc), C.byref(v), out.ctypes.data, cap, C.byref(r))
    return st, out, r


def host_fit(img, windows):
    v = img.view()
    arr = (abi.FpWriteWindow * len(windows))(*[abi.FpWriteWindow(*w) for w in windows])
    out = (C.c_int32 * len(windows))()
    st = host().rsx_fpwrite_host_fit(C.byref(v), len(windows), arr, out)
    return st, list(out)


def host_widen_all(bps):
    """the host core's widening of every pattern of the narrow format"""
    out = np.zeros(1 << bps, np.uint32)
    host().rsx_fpwrite_host_widen_range(0, out.size, bps, out.ctypes.data)
    return out


def host_fit_bps(x):
    """the least of 16 / 24 / 32 for every sample by itself, by the core's predicate"""
    x = np.ascontiguousarray(x, dtype=np.uint32).reshape(-1)
    out = np.zeros(x.size, np.uint8)
    host().rsx_fpwrite_host_fit_class_many(x.ctypes.data, x.size, out.ctypes.data)
    return np.array([16, 24, 32])[out]


def host_narrow(x, bps):
    """rsx_fpwrite_host_narrow_many -> (patterns, exact)"""
    x = np.ascontiguousarray(x, dtype=np.uint32).reshape(-1)
    out = np.zeros(x.size, np.uint32)
    exact = np.zeros(x.size, np.uint8)
    host().rsx_fpwrite_host_narrow_many(x.ctypes.data, x.size, bps, out.ctypes.data,
                                        exact.ctypes.data)
    return out, exact.astype(bool)


def pack_cases():
    """(name, bps, order, cpp, crop_w, crop_h, crop_x, crop_y, stream padding, image padding): the
    smallest shapes at which the gather can go wrong -- a row shorter than a lane's 16 bytes (a
    lane spans rows), samples of 3 bytes straddling lanes, pitches that are no multiple of 4 (the
    tail), cpp 2 and 3 with a crop_x that counts samples (16 / 24) or pixels (32), and a stream of
    more than one workgroup."""
    block = pack_block_bytes()
    out = []
    for bps in BPS:
        b = bps // 8
        for order in ORDERS:
            if bps == 32 and order == abi.ORDER_MSB:
                continue  # (copyPixels ignores the order; one MSB case below)
            tag = "%d%s" % (bps, "m" if order == abi.ORDER_MSB else "l")
            out += [("one" + tag, bps, order, 1, 2, 1, 0, 0, 0, 0),
                    ("short" + tag, bps, order, 1, 3, 5, 1, 1, 1, 4),
                    ("odd" + tag, bps, order, 1, 37, 3, 2, 0, 3, 0),
                    ("cpp2" + tag, bps, order, 2, 9, 4, 3, 2, 0, 8),
                    ("cpp3" + tag, bps, order, 3, 7, 2, 1, 0, 2, 4),
                    ("block" + tag, bps, order, 1, block // b + 5, 2, 0, 1, 1, 0)]
    out.append(("copy_msb", 32, abi.ORDER_MSB, 1, 6, 2, 1, 0, 0, 0))
    return out


def pack_case(case):
    """-> (desc, Img32 of samples that narrow exactly)"""
    name, bps, order, cpp, w, h, crop_x, crop_y, pad, img_pad = case
    dim_x = crop_x + w + 1
    px = exact_samples(name, bps, crop_y + h + 1, dim_x * cpp)
    img = Img32(px, cpp=cpp, pad=img_pad)
    pitch = w * cpp * bps // 8 + pad
    return pack_desc(crop_x, crop_y, w, h, pitch, bps, order), img


def validate_model(d, img, out_cap):
    """rsx_fpwrite_pack_validate restated: rsx_unpack_f32_validate's verdicts in its order, then the
    writer's own"""
    need = (d.crop_h & 0xFFFFFFFF) * (d.input_pitch_bytes & 0xFFFFFFFF)
    if need > 0xFFFFFFFF:
        return IO
    if d.crop_w <= 0 or d.crop_h <= 0 or d.input_pitch_bytes < 1:
        return INVALID_ARG
    if not abi.ORDER_LSB <= d.bit_order <= abi.ORDER_MSB32:
        return INVALID_ARG
    if not 1 <= img.cpp <= 3 or not 1 <= d.bits_per_pixel <= 32:
        return INVALID_ARG
    bits = d.crop_w * img.cpp * d.bits_per_pixel
    if bits % 8 or d.input_pitch_bytes < bits // 8:
        return INVALID_ARG
    u64 = lambda v: v & 0xFFFFFFFFFFFFFFFF  # (the reader compares unsigned: a negative size passes)
    if d.crop_x < 0 or d.crop_y < 0 or d.crop_y > u64(img.dim_y) or \
            d.crop_x + d.crop_w > u64(img.dim_x):
        return INVALID_ARG
    if d.bits_per_pixel != 32:
        if d.bit_order not in ORDERS or d.bits_per_pixel not in (16, 24):
            return INVALID_ARG
        if need < 4:
            return IO
    if img.dim_x < 1 or img.dim_y < 1:
        return INVALID_ARG
    if d.crop_y + d.crop_h > img.dim_y:
        return INVALID_ARG
    x0 = d.crop_x * img.cpp if d.bits_per_pixel == 32 else d.crop_x
    if img.pitch_bytes % 4 or img.pitch_bytes < (x0 + d.crop_w * img.cpp) * 4:
        return INVALID_ARG
    if out_cap < round_up4(need):
        return INVALID_ARG
    return OK


# ---------------------------------------------------------------------------------------------
# deflate tiles
# ---------------------------------------------------------------------------------------------
import dng_deflate_files as DF  # noqa: E402

BLOCK = abi.FPWRITE_BLOCK
INPUT_OVERFLOW, UNSUPPORTED = abi.RSX_ERR_INPUT_OVERFLOW, abi.RSX_ERR_UNSUPPORTED
_dfl = None


def dfl():
    global _dfl
    if _dfl is None:
        L = host()
        L.rsx_fpwrite_host_deflate.argtypes = [C.c_void_p] * 4
        L.rsx_fpwrite_host_deflate_bound.argtypes = [C.c_void_p] * 3
        L.rsx_fpwrite_host_deflate_bound.restype = C.c_uint64
        L.rsx_fpwrite_host_limit.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.rsx_fpwrite_host_block_stats.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        L.rsx_fpwrite_host_block_stats.restype = None
        L.rsx_fpwrite_host_deflate_bytes.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.rsx_fpwrite_host_deflate_bytes.restype = C.c_uint64
        _dfl = L
    return _dfl


def bound_model(n_bytes):
    """the closed form of rsx_fpwrite_deflate_bound"""
    return n_bytes + 6 * ((n_bytes + BLOCK - 1) // BLOCK) + 6


def host_deflate_bytes(data):
    """raw bytes as one tile's bytes -> (the stream, abi.FpWriteDeflateResult)"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    out = np.zeros(bound_model(data.size) + 8, np.uint8)
    r = abi.FpWriteDeflateResult()
    n = dfl().rsx_fpwrite_host_deflate_bytes(data.ctypes.data, data.size, out.ctypes.data, C.byref(r))
    return out[:n].copy(), r


def host_block_stats(data):
    data = np.ascontiguousarray(data, dtype=np.uint8)
    out = (C.c_uint32 * 2)()
    dfl().rsx_fpwrite_host_block_stats(data.ctypes.data, data.size, out)
    return out[0], out[1]


def host_limit(freq, maxbits):
    f = np.ascontiguousarray(freq, dtype=np.uint32)
    out = np.zeros(f.size, np.uint8)
    used = dfl().rsx_fpwrite_host_limit(f.ctypes.data, f.size, maxbits, out.ctypes.data)
    return used, out


def deflate_tile(geom, out_ptr=None, out_cap=0):
    return abi.FpWriteDeflateTile(out_ptr, out_cap, *geom)


def host_deflate(desc, geom, img, cap=None, guard=16):
    """rsx_fpwrite_host_deflate -> (status, the whole guarded buffer, abi.FpWriteDeflateResult)"""
    v = img.view()
    t = deflate_tile(geom)
    bound = int(dfl().rsx_fpwrite_host_deflate_bound(C.byref(desc), C.byref(t), C.byref(v)))
    cap = bound if cap is None else cap
    out = np.full(cap + guard, 0x5A, dtype=np.uint8)
    t = deflate_tile(geom, out.ctypes.data, cap)
    r = abi.FpWriteDeflateResult()
    st = dfl().rsx_fpwrite_host_deflate(C.byref(desc), C.byref(t), C.byref(v), C.byref(r))
    return st, out, r


def samples_from_tile_bytes(data, tile_w, pf):
    """bps 32: the (tile_h, tile_w) samples whose tile_bytes are `data` (the predictor undone)"""
    rows = np.asarray(data, dtype=np.uint8).reshape(-1, 4 * tile_w).astype(np.uint32)
    if rows.shape[1] > pf:
        for c in range(pf, rows.shape[1]):
            rows[:, c] = (rows[:, c] + rows[:, c - pf]) & 0xFF
    p = rows.reshape(rows.shape[0], 4, tile_w)
    return (p[:, 0] << 24 | p[:, 1] << 16 | p[:, 2] << 8 | p[:, 3]).astype(np.uint32)


def de_bruijn(k, n):
    """every word of length n over k letters exactly once (cyclic)"""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return np.array(seq, dtype=np.uint8)


LIMITER_COUNTS = [1, 1, 3, 5, 9, 15, 25, 41, 67, 109, 177, 287, 465, 753, 1219, 1973, 3193]


def crafted_bytes(name):
    """tile bytes built to reach one rule each; all a multiple of 512 bytes (bps 32, tile_w 128)"""
    rng = np.random.default_rng(seed_of(name))
    if name == "all256":
        d = np.repeat(np.arange(256, dtype=np.uint8), BLOCK // 256)
        rng.shuffle(d)
        return d
    if name == "nomatch":  # no three bytes twice, no run: every match finder comes back empty
        return (de_bruijn(21, 3)[:9216] * 3 + 7).astype(np.uint8)
    if name == "limiter":  # a plain Huffman tree over these counts is 16 deep
        d = np.concatenate([np.full(c, 40 + i, np.uint8) for i, c in enumerate(LIMITER_COUNTS)])
        rng.shuffle(d)
        return np.concatenate([d, np.zeros(-d.size % 512, np.uint8)])
    if name in ("period64", "period65"):  # rows of 512 bytes repeat at 32768 / 32768 + 512 bytes
        rows = 64 if name == "period64" else 65
        one = rng.integers(0, 256, rows * 512, dtype=np.uint64).astype(np.uint8)
        return np.concatenate([one, one[:8 * 512]])
    raise KeyError(name)


def deflate_cases():
    """(name, bps, predictor, cpp, geom, kind): geom = (tile_w, tile_h, off_x, off_y, width, height)
    in samples; kind is a kind of DF.random_samples, 'zero', or 'crafted' (crafted_bytes(name)).
    The smallest shapes at which each rule can go wrong (ISSUE: the shape list)."""
    out = []
    for bps in BPS:
        out.append(("one%d" % bps, bps, 3, 1, (1, 1, 0, 0, 1, 1), "bits"))
        out.append(("bits%d" % bps, bps, 34894, 1, (40, 70, 1, 2, 40, 70), "bits"))  # stored blocks
        out.append(("mixed%d" % bps, bps, 3, 1, (128, 128, 0, 0, 128, 128), "mixed"))
        for w in (2, 4, 5):  # rows of at most predFactor bytes, and one sample more
            out.append(("narrow%d_%d" % (bps, w), bps, 34895, 1, (w, 9, 3, 1, w, 9), "mixed"))
    for cpp in (1, 2, 3, 4):
        for pred in (3, 34894, 34895):
            bps = BPS[(cpp + pred) % 3]
            out.append(("cpp%d_p%d" % (cpp, pred), bps, pred, cpp,
                        (12 * cpp, 11, 2 * cpp, 1, 12 * cpp, 11), "mixed"))
    out.append(("ragged_right", 16, 3, 1, (32, 20, 4, 0, 21, 20), "smooth"))
    out.append(("ragged_bottom", 24, 34894, 1, (32, 20, 0, 3, 32, 13), "smooth"))
    out.append(("ragged_both", 32, 34895, 2, (32, 20, 2, 3, 18, 7), "mixed"))
    # a tile of exactly RSX_FPWRITE_BLOCK bytes, one less (3 x 5461) and two more (2 x 8193); one
    # more has no tile (16385 is no multiple of 2, 3 or 4): host_deflate_bytes covers it
    assert BLOCK == 16384
    out.append(("block_exact", 16, 3, 1, (128, 64, 0, 0, 128, 64), "smooth"))
    out.append(("block_minus1", 24, 3, 1, (5461, 1, 0, 0, 5461, 1), "smooth"))
    out.append(("block_plus2", 16, 3, 1, (8193, 1, 0, 0, 8193, 1), "smooth"))
    out.append(("zero", 32, 3, 1, (128, 40, 0, 0, 128, 40), "zero"))
    for name in ("all256", "nomatch", "limiter", "period64", "period65"):
        n = crafted_bytes(name).size
        out.append((name, 32, 3, 1, (128, n // 512, 0, 0, 128, n // 512), "crafted"))
    return out


def deflate_case(case):
    """-> (desc, geom, Img32, the tile's narrow samples (tile_h, tile_w), zero outside the window)"""
    name, bps, pred, cpp, geom, kind = case
    tile_w, tile_h, off_x, off_y, width, height = geom
    rng = np.random.default_rng(seed_of(name))
    if kind == "zero":
        win = np.zeros((height, width), np.uint32)
    elif kind == "crafted":
        win = samples_from_tile_bytes(crafted_bytes(name), tile_w, DF.PREDICTORS[pred] * cpp)
    else:
        win = DF.random_samples(rng, bps, height, width, kind)
    cols = -(-(off_x + width + 1) // cpp) * cpp
    px = exact_samples(name + "_bg", bps, off_y + height + 1, cols)
    px[off_y:off_y + height, off_x:off_x + width] = model_widen(win, bps)
    tile = np.zeros((tile_h, tile_w), np.uint32)
    tile[:height, :width] = win
    return abi.DngDeflateDesc(bps, pred), geom, Img32(px, cpp=cpp, pad=4 * (len(name) % 3)), tile


def write_deflate_cases(path):
    """the shape list as the file rsx_fpwrite_host_check takes (its format is described there)"""
    with open(path, "wb") as f:
        for case in deflate_cases():
            d, geom, img, _ = deflate_case(case)
            f.write(np.array([d.bps, d.predictor, img.cpp, *geom, img.pitch, img.dim_x, img.dim_y],
                             dtype=np.uint32).tobytes())
            f.write(img.buf.tobytes())
    return len(deflate_cases())


def deflate_validate_model(bps, pred, geom, img):
    """rsx_fpwrite_deflate_validate restated: rsx_dng_deflate_validate's verdicts in its order"""
    tile_w, tile_h, off_x, off_y, width, height = geom
    if bps not in BPS or pred not in DF.PREDICTORS:
        return INVALID_ARG
    if not 1 <= img.cpp <= 4 or img.dim_x <= 0 or img.dim_y <= 0 or img.pitch_bytes % 4:
        return INVALID_ARG
    if 0 in (tile_w, tile_h, width, height) or width > tile_w or height > tile_h:
        return INVALID_ARG
    if off_x + width > img.dim_x * img.cpp or off_y + height > img.dim_y:
        return INVALID_ARG
    if img.pitch_bytes < img.dim_x * img.cpp * 4:
        return INVALID_ARG
    if bps // 8 * tile_w * tile_h >= 1 << 28:
        return UNSUPPORTED
    return OK
