"""The image-hash core (rawspeed_amd/csrc/rsx_image_hash_core.h) as host C++ against hashlib and
numpy: MD5 over every length around the padding edge at every alignment, the tables against RFC
1321's formulas, images of both sample sizes with tight and padded pitches, the two sums, and the
hex-joined form of the hash against hashes recorded from the unmodified reference
(tests/golden/golden_hashes.json).  No GPU."""
import hashlib
import json
import math
import os

import numpy as np
import pytest

import golden_cases as G
import image_hash_files as F
from oracle_lib import HostImage
from rawspeed_amd import abi

with open(os.path.join(os.path.dirname(__file__), "golden", "golden_hashes.json")) as f:
    GOLD = json.load(f)


def test_md5_of_every_length_and_alignment():
    rng = np.random.default_rng(1)
    buf = rng.integers(0, 256, 256, dtype=np.uint8)
    assert buf.ctypes.data % 4 == 0
    for n in range(201):
        for a in range(4):
            assert F.host_md5(buf, a, n) == hashlib.md5(buf[a:a + n].tobytes()).digest(), (n, a)


def test_md5_in_pieces():
    import ctypes as C
    rng = np.random.default_rng(2)
    buf = rng.integers(0, 256, 1000, dtype=np.uint8)
    for n in (0, 1, 55, 56, 63, 64, 65, 119, 120, 128, 999):
        want = hashlib.md5(buf[:n].tobytes()).digest()
        for piece in (1, 3, 63, 64, 65, 1000):
            out = (C.c_uint8 * 16)()
            F.host().rsx_image_hash_host_md5_pieces(buf.ctypes.data, n, piece, out)
            assert bytes(out) == want, (n, piece)


def test_tables_are_rfc_1321s():
    sines = np.zeros(64, np.uint32)
    shifts = np.zeros(64, np.int32)
    words = np.zeros(64, np.int32)
    F.host().rsx_image_hash_host_tables(sines.ctypes.data, shifts.ctypes.data, words.ctypes.data)
    assert [int(v) for v in sines] == [int(abs(math.sin(i + 1)) * 2 ** 32) for i in range(64)]
    rows = ([7, 12, 17, 22], [5, 9, 14, 20], [4, 11, 16, 23], [6, 10, 15, 21])
    assert [int(v) for v in shifts] == [rows[i // 16][i % 4] for i in range(64)]
    assert [int(v) for v in words] == [i if i < 16 else (5 * i + 1) % 16 if i < 32 else
                                       (3 * i + 5) % 16 if i < 48 else (7 * i) % 16
                                       for i in range(64)]


SHAPES = [(w, 1, 2) for w in F.WIDTHS_U16] + [(w, 3, 2) for w in F.WIDTHS_U16_CPP3] + \
         [(w, 1, 4) for w in F.WIDTHS_F32] + [(5, 3, 4), (4099, 1, 2), (1028, 3, 4)]


@pytest.mark.parametrize("w,cpp,sb", SHAPES)
def test_images_tight_and_padded(w, cpp, sb):
    rng = np.random.default_rng([3, w, cpp, sb])
    for h in (1, 5):
        for pad, lead in ((0, 0), (2 * sb, sb), (16, 0), (2 * sb + 64, 3 * sb)):
            L = F.Layout(rng, w, h, cpp, sb, pad=pad, lead=lead)
            want = L.want()
            for threads in (1, 3):
                st, r, lines = F.host_hash(L.view(), sb, threads)
                assert st == F.OK and lines == want[0] and F.same(r, want), (h, pad, lead, threads)
            L.rewrite_padding()
            st, r, lines = F.host_hash(L.view(), sb, 2, lines=False)
            assert st == F.OK and lines is None and F.same(r, want), (h, pad, lead)


@pytest.mark.parametrize("sb", (2, 4))
def test_sums(sb):
    rng = np.random.default_rng(4)
    w, h = 2056, 130
    for value in (0xFF, None):
        L = F.Layout(rng, w, h, 1, sb, pad=16, value=value)
        st, r, _ = F.host_hash(L.view(), sb, 4)
        want = L.want()
        assert st == F.OK and F.same(r, want)
        if value is not None:
            assert r.byte_sum == 255 * 2056 * sb * h
            assert r.sample_sum == (0xFFFF * 2056 * h if sb == 2 else 0)
        assert (r.sample_sum != 0) == (sb == 2)


def test_refusals_write_nothing():
    rng = np.random.default_rng(5)
    L = F.Layout(rng, 8, 2, 1, 2)
    v = L.view()
    v.pitch_bytes = 14
    st, r, lines = F.host_hash(v, 2)
    assert st == F.INVALID_ARG and bytes(r) == b"\xa5" * 32 and lines == b"\xa5" * 32
    assert F.host_hash(L.view(), 3)[0] == F.INVALID_ARG
    v = L.view()
    v.data = None
    assert F.host_hash(v, 2)[0] == F.INVALID_ARG


UNPACK_2056 = [i for i, c in enumerate(G.UNPACK_CASES) if c["w"] == 2056]


@pytest.mark.parametrize("i", UNPACK_2056)
def test_hex_joined_hash_of_the_unpack_cases(oracle, i):
    """the core's line digests of the oracle's image, hex-joined, are the reference's hash"""
    d, data, (w, h, cpp) = G.build_unpack(G.UNPACK_CASES[i])
    img = HostImage(w, h, cpp)
    g = GOLD["unpack"][str(i)]
    assert oracle.unpack(d, data, img) == g["status"]
    st, r, lines = F.host_hash(img.view(), 2)
    assert st == F.OK
    assert abi.hex_joined_hash(lines) == g["hash"]
    assert r.digest() == hashlib.md5(lines).digest()


@pytest.mark.parametrize("i", range(len(G.F32_CASES)))
def test_hex_joined_hash_of_the_f32_cases(oracle, i):
    d, data, (w, h, cpp) = G.build_f32(G.F32_CASES[i])
    img = HostImage(w, h, cpp, bpc=4)
    g = GOLD["f32"][str(i)]
    assert oracle.unpack_f32(d, data, img) == g["status"] == 0
    st, r, lines = F.host_hash(img.view(), 4)
    assert st == F.OK and r.sample_sum == 0
    assert abi.hex_joined_hash(lines) == g["hash"]
