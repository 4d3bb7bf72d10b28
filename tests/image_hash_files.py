"""What the image-hash tests share (include/rsx.h section 4g): the expectation from hashlib and
numpy, image layouts with a lead-in and padded pitches, and the host build of the core
(rawspeed_amd/librsx_image_hash_host.so)."""
import ctypes as C
import hashlib

import numpy as np

from rawspeed_amd import abi, build

OK, INVALID_ARG, UNSUPPORTED = abi.RSX_OK, abi.RSX_ERR_INVALID_ARG, abi.RSX_ERR_UNSUPPORTED

# u16, cpp 1: row_bytes mod 64 = 2, 54, 56, 58, 62, 0 (56 and above need the second padding block),
# and the same behind one whole block
WIDTHS_U16 = [1, 27, 28, 29, 31, 32] + [w + 64 for w in (1, 27, 28, 29, 31, 32)]
WIDTHS_U16_CPP3 = [9, 20]
WIDTHS_F32 = [13, 14, 15, 16]
WIDTHS_LONG = [4099, 32768]
# the wavefront's tail; remainders 16, 48, 0, 16 and 32 of the chain over the digests
HEIGHTS = [1, 63, 64, 65, 130]

_host = None


def host():
    global _host
    if _host is None:
        lib, _ = build.build_image_hash_host()
        L = C.CDLL(lib)
        L.rsx_image_hash_host_validate.argtypes = [C.c_void_p, C.c_int32]
        L.rsx_image_hash_host_md5.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
        L.rsx_image_hash_host_md5.restype = None
        L.rsx_image_hash_host_md5_pieces.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
        L.rsx_image_hash_host_md5_pieces.restype = None
        L.rsx_image_hash_host_tables.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rsx_image_hash_host_tables.restype = None
        L.rsx_image_hash_host.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int]
        _host = L
    return _host


def host_md5(buf, offset, n):
    """md5 of buf[offset:offset + n] (a numpy uint8 array: the address is the array's plus offset)"""
    out = (C.c_uint8 * 16)()
    host().rsx_image_hash_host_md5(C.c_void_p(buf.ctypes.data + offset), n, out)
    return bytes(out)


def view_of(buf, offset, pitch, dim_x, dim_y, cpp):
    return abi.Image(buf.ctypes.data + offset, pitch, dim_x, dim_y, cpp, 0)


def host_hash(view, sample_bytes, threads=1, lines=True):
    """rsx_image_hash_host -> (status, abi.ImageHashResult, the line digests or None); the outputs
    start as 0xA5"""
    r = abi.ImageHashResult()
    C.memset(C.byref(r), 0xA5, C.sizeof(r))
    buf = np.full(16 * max(1, view.dim_y), 0xA5, np.uint8)
    st = host().rsx_image_hash_host(C.byref(view), sample_bytes, buf.ctypes.data if lines else None,
                                    C.byref(r), threads)
    return st, r, (buf.tobytes() if lines else None)


def expect(rows, sample_bytes):
    """rows: (dim_y, row_bytes) uint8 -> (line digests, md5, byte_sum, sample_sum)"""
    rows = np.ascontiguousarray(rows)
    lines = b"".join(hashlib.md5(r.tobytes()).digest() for r in rows)
    samples = int(rows.view(np.uint16).sum(dtype=np.uint64)) if sample_bytes == 2 else 0
    return lines, hashlib.md5(lines).digest(), int(rows.sum(dtype=np.uint64)), samples


def result_bytes(md5, byte_sum, sample_sum):
    """the 32 bytes of an rsx_image_hash_result"""
    return md5 + int(byte_sum).to_bytes(8, "little") + int(sample_sum).to_bytes(8, "little")


def same(result, want):
    """an abi.ImageHashResult against expect()'s tuple"""
    return (result.digest(), result.byte_sum, result.sample_sum) == want[1:]


class Layout:
    """An image of random (or constant) samples in a buffer of exactly lead + pitch (dim_y - 1) +
    row_bytes bytes: no padding behind the last row.  Lead-in and padding are random bytes."""

    def __init__(self, rng, dim_x, dim_y, cpp, sample_bytes, pad=0, lead=0, value=None):
        self.dim_x, self.dim_y, self.cpp, self.sample_bytes = dim_x, dim_y, cpp, sample_bytes
        self.row_bytes = dim_x * cpp * sample_bytes
        self.pitch, self.lead = self.row_bytes + pad, lead
        self.size = lead + self.pitch * (dim_y - 1) + self.row_bytes
        self.buf = rng.integers(0, 256, self.size, dtype=np.uint8)
        if value is not None:
            for y in range(dim_y):
                self.row(y)[:] = value
        self.rng = rng

    def row(self, y):
        at = self.lead + y * self.pitch
        return self.buf[at:at + self.row_bytes]

    def rows(self):
        return np.stack([self.row(y) for y in range(self.dim_y)])

    def rewrite_padding(self):
        """new random bytes in the lead-in and between the rows"""
        keep = self.rows()
        self.buf[:] = self.rng.integers(0, 256, self.size, dtype=np.uint8)
        for y in range(self.dim_y):
            self.row(y)[:] = keep[y]

    def want(self):
        return expect(self.rows(), self.sample_bytes)

    def view(self, base=None):
        """the image at `base` (an address; default: the host buffer's) + lead"""
        base = self.buf.ctypes.data if base is None else base
        return abi.Image(base + self.lead, self.pitch, self.dim_x, self.dim_y, self.cpp, 0)
