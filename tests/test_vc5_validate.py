"""rsx_vc5_validate: every refusal include/rsx.h section 4c lists, in its documented order (the
constructor's checks, VC5Decompressor.cpp:384-424, then what the tag parse would have thrown),
and the accepted corners.  Host code only: no GPU needed."""
import numpy as np
import pytest

import vc5_files as V
from rawspeed_amd import abi, capi

OK, INV, IO, UNS = abi.RSX_OK, abi.RSX_ERR_INVALID_ARG, abi.RSX_ERR_IO, abi.RSX_ERR_UNSUPPORTED
TABLE = np.zeros(4096, np.uint16)


def _bands(w, h, precision=16):
    """bands of the least size, one after the other: (bands, bytes in all)"""
    w3, h3 = V.dims(w, h)[3]
    low = 8 * (-(-w3 * h3 * precision // 64))
    bands, at = [], 0
    for c in range(4):
        row = []
        for s in range(10):
            n = low if s == 0 else 4
            row.append((at, n, 1 if s else 0, precision if s == 0 else 0))
            at += n
        bands.append(row)
    return bands, at


def _v(w=48, h=40, cpp=1, pitch=None, phase=0, table=TABLE, codes="book", bands=None, n=None,
       precision=16):
    b, total = _bands(max(w, 34), max(h, 34), precision)
    d, keep = abi.vc5_desc(phase, table, V.book() if codes == "book" else codes,
                           b if bands is None else bands, [[0, 0, 0]] * 4)
    img = abi.Image(None, 2 * w if pitch is None else pitch, w, h, cpp, 1)
    return capi.vc5_validate(d, img, total if n is None else n)


def _with(bands, c, s, **kw):
    out = [list(r) for r in bands]
    off, n, q, p = out[c][s]
    out[c][s] = (kw.get("offset", off), kw.get("bytes", n), q, kw.get("precision", p))
    return out


def test_accepted_corners():
    assert _v(34, 34) == OK and _v(65534, 34) == OK and _v(34, 65534) == OK
    assert _v(48, 40, pitch=2 * 48 + 10) == OK and _v(phase=1) == OK
    assert _v(precision=8) == OK
    b, total = _bands(48, 40)
    assert _v(bands=b, n=total + 7) == OK                       # bytes behind the bands
    assert _v(bands=_with(b, 3, 9, bytes=4 + 3), n=total + 3) == OK


def test_null_pointers():
    img = abi.Image(None, 96, 48, 40, 1, 1)
    assert capi.vc5_validate(None, img, 1 << 20) == INV
    assert _v(table=None) == INV and _v(codes=None) == INV
    assert capi.lib().rsx_vc5_validate(None, None, 0) == INV


@pytest.mark.parametrize("kw", [
    dict(cpp=2), dict(cpp=3), dict(cpp=0),
    dict(w=0), dict(h=0), dict(w=-2, pitch=64), dict(h=-4),
    dict(w=47), dict(h=39), dict(w=65536), dict(h=65536), dict(w=33), dict(h=35),
    dict(pitch=2 * 48 - 2), dict(pitch=0),
    dict(phase=2), dict(phase=3), dict(phase=-1),
])
def test_geometry_and_phase_are_invalid_arguments(kw):
    assert _v(n=1 << 30, **kw) == INV
    assert _v(n=0, **kw) == INV        # in front of the bands


@pytest.mark.parametrize("codes", [
    [], V.book() + [(26, 0, 1, 0)], V.book()[:5] + V.book()[:1], [(1, 0, 1, 0), (2, 1, 1, 1)],
    [(0, 0, 1, 0)], [(27, 0, 1, 0)], [(2, 4, 1, 0)], [(2, 1, 512, 0)], [(2, 1, 1, 1024)],
    [(2, 1, 1, -1024)],
])
def test_code_books_that_are_refused(codes):
    assert _v(codes=codes) == INV
    assert _v(codes=codes, w=32) == INV  # in front of the size rule


def test_accepted_code_books():
    assert _v(codes=[(1, 0, 1, 0), (2, 2, 511, -1023), (2, 3, 0, 1023)]) == OK
    assert _v(codes=V.book_with_hole()[0]) == OK


def test_small_images_are_unsupported():
    """a level narrower or shorter than 3: behind the constructor's checks and the book, in
    front of precision and bands"""
    for w, h in ((32, 48), (48, 32), (2, 2), (32, 32)):
        assert _v(w, h) == UNS
        assert _v(w, h, n=0) == UNS and _v(w, h, precision=7) == UNS
    assert _v(32, 48, cpp=2) == INV and _v(32, 47) == INV and _v(32, 48, phase=2) == INV


def test_precision_and_bands():
    b, total = _bands(48, 40)
    for p in (7, 17, 0):
        assert _v(bands=_with(b, 2, 0, precision=p)) == INV
    assert _v(bands=_with(b, 0, 0, precision=7), n=0) == INV   # the first band's precision first
    assert _v(n=total - 1) == IO and _v(n=0) == IO
    assert _v(bands=_with(b, 1, 4, offset=total - 3)) == IO     # reaches past the tile
    assert _v(bands=_with(b, 1, 4, offset=1 << 40)) == IO
    assert _v(bands=_with(b, 2, 7, bytes=3)) == IO              # the bit reader's minimum
    assert _v(bands=_with(b, 2, 7, bytes=0)) == IO
    low = b[0][0][1]
    assert _v(bands=_with(b, 3, 0, bytes=low - 1)) == IO        # shorter than its fields
    # a band's precision is looked at in front of the band before it? no: bands go in order
    assert _v(bands=_with(_with(b, 0, 5, bytes=1), 1, 0, precision=3)) == IO
    assert _v(bands=_with(_with(b, 1, 5, bytes=1), 1, 0, precision=3)) == INV
