"""RafDecoder::applyCorrections' 45 degree rotation (decoders/RafDecoder.cpp:228-270): a numpy model
transcribed from the cited lines, the validation of include/rsx.h section 3y as a model, and the
case lists the CPU and the device tests share.

The reference cannot be run for this path here (it sits behind the fuji_rotate camera hint, which
needs the camera database), so the yardstick is this transcription, the host build of the core
header, and the hand-worked answers in tests/test_fuji_rotate_model.py."""
import ctypes as C

import numpy as np

from rawspeed_amd import abi, build

OK, INVALID_ARG, UNSUPPORTED = abi.RSX_OK, abi.RSX_ERR_INVALID_ARG, abi.RSX_ERR_UNSUPPORTED

TILE_W, TILE_H = 64, 32  # the destination tile of the shipped kernel (rsx_fuji_rotate.hip)


class OutOfBounds(Exception):
    """the reference's ThrowRDE("Trying to write out of bounds")"""


def rotated_size(W, H, alt):
    """-> (rotatedsize, rotationPos), :236-242"""
    return (H + W // 2, W // 2 - 1) if alt else (W + H // 2, W - 1)


def forward(W, H, alt, x, y):
    """-> (h, w), :257-263; works on ints and on numpy arrays"""
    R = rotated_size(W, H, alt)[0]
    if alt:
        return R - (H + 1 - y + (x >> 1)), ((x + 1) >> 1) + y
    return W - 1 - x + (y >> 1), ((y + 1) >> 1) + x


def inverse(W, alt, h, w):
    """-> (x, y) of the one point of the plane that lands on (h, w)"""
    if alt:
        x = w - h + (W // 2 - 1)
        return x, w - ((x + 1) >> 1)
    return (w - h + W - 1) >> 1, w + h - (W - 1)


def rotate_literal(src, cx, cy, W, H, alt):
    """The loop of :253-269 as it stands, on a 2-D uint16 array.  A negative row is an IndexError
    here (the reference writes in front of its row); the reference's own check raises OutOfBounds."""
    R = rotated_size(W, H, alt)[0]
    dim_x, dim_y = R, R - 1
    dst = np.zeros((dim_y, dim_x), np.uint16)  # clearArea
    for y in range(H):
        for x in range(W):
            h, w = forward(W, H, alt, x, y)
            if h < dim_y and w < dim_x:
                if h < 0 or w < 0:
                    raise IndexError((h, w))
                dst[h, w] = src[cy + y, cx + x]
            else:
                raise OutOfBounds((x, y, h, w))
    return dst


def rotate_scatter(src, cx, cy, W, H, alt):
    """the same scatter in one numpy assignment (valid geometries only)"""
    R = rotated_size(W, H, alt)[0]
    y, x = np.mgrid[0:H, 0:W]
    h, w = forward(W, H, alt, x, y)
    dst = np.zeros((R - 1, R), np.uint16)
    dst[h, w] = src[cy:cy + H, cx:cx + W]
    return dst


def rotate_gather(src, cx, cy, W, H, alt):
    """every destination sample from the inverse map: what the device runs"""
    R = rotated_size(W, H, alt)[0]
    h, w = np.mgrid[0:R - 1, 0:R]
    x, y = inverse(W, alt, h, w)
    inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
    dst = np.zeros((R - 1, R), np.uint16)
    dst[inside] = src[cy + y[inside], cx + x[inside]]
    return dst


def refusal(W, H, alt):
    """what the descriptor alone is refused with (rsx_raf_rotate_geometry), or OK"""
    if W < 1 or H < 1:
        return INVALID_ARG
    R = rotated_size(W, H, alt)[0]
    if R < 2 or R > 65535:
        return INVALID_ARG
    if not alt and H % 2:
        return INVALID_ARG  # the reference throws "Trying to write out of bounds"
    if alt and W % 2:
        return UNSUPPORTED  # the reference writes row -1
    return OK


def source(dim_x, dim_y, seed=1):
    """a source image whose every sample is distinct from its neighbours and never 0 or 0xA5A5"""
    rng = np.random.default_rng(seed)
    a = rng.integers(1, 0xA000, (dim_y, dim_x), dtype=np.uint16)
    return a


def src_pitch(dim_x):
    return (2 * dim_x + 15) // 16 * 16 + 32


# (W, H) of the issue's list; the normal layout refuses odd H (the reference throws there), so the
# odd-H entries are refusal cases under it and each has an even-H neighbour for the pixels
SIZES = [(1, 2), (2, 1), (2, 2), (7, 5), (8, 8), (9, 16), (63, 65), (64, 64), (65, 63), (130, 67),
         (3, 200), (200, 3)]
SIZES_EVEN_H = [(7, 6), (63, 66), (65, 64), (130, 68), (200, 4)]


def _edge_sizes():
    """R - 1 (rows) around TILE_H and R (columns) around TILE_W: T - 1, T, T + 1, 2 T + 1"""
    rs = sorted({TILE_W - 1, TILE_W, TILE_W + 1, 2 * TILE_W + 1} |
                {t + 1 for t in (TILE_H - 1, TILE_H, TILE_H + 1, 2 * TILE_H + 1)})
    normal, alt = [], []
    for R in rs:
        H = 2 * (R // 3)
        normal.append((R - H // 2, H))
        W = 2 * (R // 3)
        alt.append((W, R - W // 2))
    return normal, alt


EDGE_NORMAL, EDGE_ALT = _edge_sizes()
CROPS = [(0, 0), (1, 0), (0, 1), (3, 5)]


def cases():
    """[(W, H, alt)]: every size under the normal layout, the even-W ones under alt as well"""
    out = []
    for W, H in SIZES + SIZES_EVEN_H + EDGE_NORMAL:
        out.append((W, H, 0))
    for W, H in SIZES + SIZES_EVEN_H + EDGE_ALT:
        if W % 2 == 0:
            out.append((W, H, 1))
    return out


# ---------------------------------------------------------------------------------------------
# the host build of the core header
# ---------------------------------------------------------------------------------------------
_host = None


def host_lib():
    global _host
    if _host is None:
        L = C.CDLL(build.LIB_FUJI_ROTATE_HOST)
        L.rsx_fuji_rotate_host_geometry.argtypes = [C.c_void_p] * 4
        L.rsx_fuji_rotate_host_validate.argtypes = [C.c_void_p] * 3
        L.rsx_fuji_rotate_host_scatter.argtypes = [C.c_void_p] * 3
        L.rsx_fuji_rotate_host_gather.argtypes = [C.c_void_p] * 3
        L.rsx_fuji_rotate_host_forward.argtypes = [C.c_int32] * 5 + [C.c_void_p] * 2
        L.rsx_fuji_rotate_host_inverse.argtypes = [C.c_int32] * 4 + [C.c_void_p] * 2
        L.rsx_fuji_rotate_host_forward.restype = None
        L.rsx_fuji_rotate_host_inverse.restype = None
        _host = L
    return _host


def image_of(arr2d_bytes, pitch, dim_x, dim_y):
    """an abi.Image over a uint8 numpy buffer"""
    return abi.Image(arr2d_bytes.ctypes.data, pitch, dim_x, dim_y, 1, 1)


def padded(src, pitch):
    """the rows of a 2-D uint16 array in a uint8 buffer of `pitch` bytes a row, 0x5A between them"""
    h, w = src.shape
    buf = np.full(pitch * h, 0x5A, np.uint8)
    buf.reshape(h, pitch)[:, :2 * w] = src.view(np.uint8).reshape(h, 2 * w)
    return buf


def host_rotate(which, src, cx, cy, W, H, alt, dst_pad=6):
    """through librsx_fuji_rotate_host.so (`which`: "scatter", the reference's loop restated, or
    "gather") -> (status, rows or None); the destination's padding must keep its 0xA5"""
    R = rotated_size(W, H, alt)[0]
    sp = src_pitch(src.shape[1])
    sbuf = padded(src, sp)
    dp = 2 * R + dst_pad
    dbuf = np.full(dp * max(R - 1, 1), 0xA5, np.uint8)
    d = abi.fuji_rotate_desc((cx, cy), (W, H), alt)
    fn = getattr(host_lib(), "rsx_fuji_rotate_host_" + which)
    st = fn(C.byref(d), C.byref(image_of(sbuf, sp, src.shape[1], src.shape[0])),
            C.byref(image_of(dbuf, dp, R, R - 1)))
    if st != OK:
        assert (dbuf == 0xA5).all()
        return st, None
    rows = dbuf.reshape(R - 1, dp)
    assert (rows[:, 2 * R:] == 0xA5).all()
    return st, rows[:, :2 * R].copy().view(np.uint16)
