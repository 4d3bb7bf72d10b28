"""TEST INFRASTRUCTURE: the compiled reference's answers, stored.

The cross-checks against the unmodified reference (oracle_lib.Ref, oracle/_ref) run
live only where the reference sources were at hand when oracle/_ref was built.
Everywhere else they replay what the reference answered, from
tests/golden/ref_vectors.json.gz:

  StoredRef     -- the calls of Ref the CPU tests make, answered from the file: the
                   status (and consumed bytes), last_error(), and a SHA-256 digest of
                   every view of the image the reference left behind.  A call is looked
                   up by a digest of everything it was given (method, descriptor bytes,
                   stream bytes, the image's geometry and contents before the call), so
                   a test whose inputs changed finds no answer and fails: regenerate.
  StoredArray   -- what a stored image's u16() / u32() / pixels() return: the shape,
                   dtype and digest of the reference's array.  np.array_equal against
                   it compares every element (through the digest of the other array's
                   bytes); any other use of it raises.
  RecordingRef  -- a live Ref that remembers every call it answers; the recording is
                   merged into RSX_REF_RECORD=<file> at the end of the session.

Regenerate where oracle/_ref is built:
    RSX_REF_RECORD=tests/golden/ref_vectors.json.gz python -m pytest tests -m "not gpu"
"""
import gzip
import hashlib
import json
import os

import numpy as np

VECTORS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                       "ref_vectors.json.gz")


def _pitch(dim_x, cpp, f32):
    """RawImageData::createData: roundUp(dim.x * bpp, 16)."""
    return (dim_x * cpp * (4 if f32 else 2) + 15) // 16 * 16


def digest(arr):
    return hashlib.sha256(np.ascontiguousarray(arr).tobytes()).hexdigest()[:32]


class StoredArray:
    """An array of the reference's that only its digest stands for (see the module docstring)."""

    def __init__(self, shape, dtype, dig):
        self.shape, self.dtype, self.digest = tuple(shape), np.dtype(dtype), dig

    def equals(self, other):
        if isinstance(other, StoredArray):
            return (other.shape, other.dtype, other.digest) == (self.shape, self.dtype,
                                                                self.digest)
        o = np.asarray(other)
        if o.shape != self.shape:
            return False
        c = o.astype(self.dtype)
        return bool(np.array_equal(c, o)) and digest(c) == self.digest

    def __array_function__(self, func, types, args, kwargs):
        if func is np.array_equal and len(args) == 2 and not kwargs:
            a, b = args
            return (b if a is self else a) is not None and \
                (self.equals(b) if a is self else self.equals(a))
        raise TypeError("a stored reference array (a digest) supports np.array_equal only, "
                        "not %s" % func.__name__)

    def __array__(self, *a, **k):
        raise TypeError("a stored reference array is a digest: compare it with np.array_equal")


def _views(u16, dim_x, cpp):
    """The views the tests read of an image (u32 is u16's bytes, so its digest)."""
    return {"u16": digest(u16), "pixels": digest(u16[:, :dim_x * cpp])}


def _feed(h, x):
    """Everything a call is given, into the key's digest."""
    from oracle_lib import RefImage
    if isinstance(x, (RefImage, StoredImage)):
        h.update(b"img")
        h.update(np.array([x.dim_x, x.dim_y, x.cpp, x.pitch], np.int64).tobytes())
        h.update((x.contents() if isinstance(x, StoredImage) else digest(x.u16())).encode())
    elif isinstance(x, np.ndarray):
        h.update(("nd%s%s" % (x.dtype.str, x.shape)).encode())
        h.update(np.ascontiguousarray(x).tobytes())
    elif isinstance(x, (bytes, bytearray)):
        h.update(b"b")
        h.update(bytes(x))
    elif isinstance(x, (list, tuple)):
        h.update(b"[%d" % len(x))
        for y in x:
            _feed(h, y)
    elif x is None or isinstance(x, (bool, int, float, str, np.integer)):
        h.update(repr(x if not isinstance(x, np.integer) else int(x)).encode())
    else:  # a ctypes descriptor
        h.update(type(x).__name__.encode())
        h.update(bytes(x))


def call_key(method, args, kwargs):
    h = hashlib.sha256(method.encode())
    _feed(h, list(args))
    for k in sorted(kwargs):
        h.update(k.encode())
        _feed(h, kwargs[k])
    return h.hexdigest()[:32]


# the calls answered as (result, the images they were given); decode_file is apart
IMAGE_CALLS = ("unpack", "unpack_variant", "decode8bit_lookup", "samsung_v1", "samsung_v2",
               "sony_arw1", "hasselblad", "pentax", "sraw", "nikon", "ljpeg", "cr2")
FILE_INFO = ("full_w", "full_h", "cpp", "pitch", "w", "h_px", "off_x", "off_y", "is_f32",
             "is_cfa")


def _images(args):
    from oracle_lib import RefImage
    return [a for a in args if isinstance(a, (RefImage, StoredImage))]


def load(path=VECTORS):
    with gzip.open(path, "rt") as f:
        return json.load(f)


class RecordingRef:
    """A live Ref that remembers what it answered (see the module docstring)."""

    def __init__(self, ref, path):
        self.ref, self.path, self.lib = ref, path, ref.lib
        self.entries = {}

    def __getattr__(self, name):
        f = getattr(self.ref, name)
        if name in IMAGE_CALLS:
            return lambda *a, **k: self._image_call(name, f, a, k)
        return f

    def image(self, dim_x, dim_y, cpp=1, is_cfa=True, fill=0xA5, f32=False):
        img = self.ref.image(dim_x, dim_y, cpp, is_cfa, fill, f32)
        assert img.pitch == _pitch(dim_x, cpp, f32), (img.pitch, dim_x, cpp, f32)
        return img

    def _image_call(self, name, f, args, kwargs):
        key = call_key(name, args, kwargs)
        res = f(*args, **kwargs)
        self.entries[key] = {"result": list(res) if isinstance(res, tuple) else res,
                             "last_error": self.ref.last_error(),
                             "images": [_views(i.u16(), i.dim_x, i.cpp) for i in _images(args)]}
        return res

    def decode_file(self, blob, uncorrected=False, threads=1):
        key = call_key("decode_file", (blob, uncorrected, threads), {})
        st, img = self.ref.decode_file(blob, uncorrected=uncorrected, threads=threads)
        e = {"result": st, "last_error": self.ref.last_error(), "file": None}
        if img is not None:
            errors = [img.errors()]  # (reading the log empties it: handed on once)
            e["file"] = {k: int(getattr(img, k)) for k in FILE_INFO}
            e["file"].update(errors=errors[0], raw=digest(img.raw()), u16=digest(img.u16()))
            img.errors = lambda: errors.pop() if errors else ""
        self.entries[key] = e
        return st, img

    def save(self):
        """Merged into self.path (calls recorded by other runs are kept)."""
        entries = load(self.path) if os.path.exists(self.path) else {}
        entries.update(self.entries)
        with gzip.GzipFile(self.path, "wb", mtime=0) as f:
            f.write(json.dumps(entries, sort_keys=True, indent=0).encode())


class StoredImage:
    """The stand-in for a RefImage: same geometry; the bytes the test put in, then the
    digests of what the reference left behind."""

    def __init__(self, dim_x, dim_y, cpp=1, is_cfa=True, fill=0xA5, f32=False):
        self.dim_x, self.dim_y, self.cpp = dim_x, dim_y, cpp
        self.pitch = _pitch(dim_x, cpp, f32)
        self.buf = np.full(self.pitch * dim_y, fill, dtype=np.uint8)
        self.views = None

    def contents(self):
        return self.views["u16"] if self.views else digest(self.buf)

    def u16(self):
        if self.views:
            return StoredArray((self.dim_y, self.pitch // 2), np.uint16, self.views["u16"])
        return self.buf.view(np.uint16).reshape(self.dim_y, self.pitch // 2)

    def u32(self):
        if self.views:
            return StoredArray((self.dim_y, self.pitch // 4), np.uint32, self.views["u16"])
        return self.u16().view(np.uint32)

    def pixels(self):
        if self.views:
            return StoredArray((self.dim_y, self.dim_x * self.cpp), np.uint16,
                               self.views["pixels"])
        return self.u16()[:, :self.dim_x * self.cpp]

    def set_pixels(self, px):
        assert self.views is None, "the reference already wrote this image"
        self.u16()[:, :px.shape[1]] = px

    def close(self):
        pass


class StoredFile:
    """The stand-in for oracle_lib.DecodedFile."""

    def __init__(self, info):
        for k in FILE_INFO:
            setattr(self, k, info[k])
        self._info = info
        self._errors = info["errors"]

    def raw(self):
        return StoredArray((self.full_h, self.pitch), np.uint8, self._info["raw"])

    def u16(self):
        return StoredArray((self.full_h, self.full_w * self.cpp), np.uint16, self._info["u16"])

    def errors(self):
        e, self._errors = self._errors, ""  # (moved out of the log, as the reference does)
        return e


class StoredRef:
    """Ref's answers replayed from tests/golden/ref_vectors.json.gz (see the module docstring)."""

    def __init__(self, path=VECTORS):
        self.path = path
        self.entries = load(path)
        self._last_error = ""

    def _entry(self, key, what):
        e = self.entries.get(key)
        if e is None:
            raise AssertionError(
                "no stored reference answer for this %s call (its inputs differ from the "
                "recorded ones): regenerate %s where oracle/_ref is built (tests/ref_vectors.py)"
                % (what, os.path.basename(self.path)))
        self._last_error = e["last_error"]
        return e

    def __getattr__(self, name):
        if name in IMAGE_CALLS:
            return lambda *a, **k: self._image_call(name, a, k)
        raise AttributeError("%s: not among the stored reference calls" % name)

    def _image_call(self, name, args, kwargs):
        e = self._entry(call_key(name, args, kwargs), name)
        for img, views in zip(_images(args), e["images"]):
            img.views = views
        r = e["result"]
        return tuple(r) if isinstance(r, list) else r

    def image(self, dim_x, dim_y, cpp=1, is_cfa=True, fill=0xA5, f32=False):
        return StoredImage(dim_x, dim_y, cpp, is_cfa, fill, f32)

    def last_error(self):
        return self._last_error

    def decode_file(self, blob, uncorrected=False, threads=1):
        e = self._entry(call_key("decode_file", (blob, uncorrected, threads), {}),
                        "decode_file")
        return e["result"], (StoredFile(e["file"]) if e["file"] else None)
