"""rsx_crw_core.h as host C++ (rawspeed_amd/librsx_crw_host.so): every case of tests/crw_files.py
with and without low bits against the model and the reference's recorded hashes, pixels and
verdicts, with canaries; with a padded pitch; and the case file through rsx_crw_host_check, the
same source built as a program with AddressSanitizer and UBSan where g++ has them.  The host build
decodes with the closed forms the kernels use (the overflow read as a threshold on the bit a symbol
starts at), the model with the reference's reader: their agreement on the streams that end early
and on the markers is the check of those forms."""
import struct
import subprocess

import numpy as np
import pytest

import crw_files as F
from rawspeed_amd import build

NAMES = F.case_names()


@pytest.mark.parametrize("name", NAMES)
def test_case(name):
    c = F.build_case(name)
    g = F.golden()["cases"][name]
    for lowbits in (True, False):
        st, px, buf = F.host_decode(c["data"], c["low"] if lowbits else None, c["width"],
                                    c["height"], c["table"])
        want_st, want = F.expected(name, lowbits)
        assert st == want_st == g["lowbits"][0]
        if st == F.OK:
            assert np.array_equal(px, want)
            if lowbits:
                assert F.sha_rows(px) == g["lowbits"][1]
        else:
            assert (buf == 0xA5).all(), "a failing decode wrote into the image"


@pytest.mark.parametrize("name", ["geom_68x16", "geom_4x16", "geom_2672x4_plus2"])
@pytest.mark.parametrize("pad", [2, 10, 16])
def test_padded_pitch(name, pad):
    c = F.build_case(name)
    w, h = c["width"], c["height"]
    st, px, buf = F.host_decode(c["data"], c["low"], w, h, c["table"], pitch=2 * w + pad)
    assert st == F.OK
    assert np.array_equal(px, F.expected(name, True)[1])
    assert (buf.reshape(h, 2 * w + pad)[:, 2 * w:] == 0xA5).all(), "the pitch padding was written"


def test_refusals_at_their_boundaries():
    data = bytes(64)
    for name, w, h, table, low_short, cpp, pitch, want in F.VALIDATION:
        if want == F.OK:
            continue
        low = bytes(max(0, w * h // 4 - low_short))
        st, px, buf = F.host_decode(data, low, w, h, table, pitch=pitch, cpp=cpp)
        assert st == want, name
        assert (buf == 0xA5).all(), name
    st, _, buf = F.host_decode(bytes(7), bytes(16), 8, 8, 0)
    assert st == F.ERR_IO and (buf == 0xA5).all()


def _fnv(px):
    h = 0xcbf29ce484222325
    for b in np.ascontiguousarray(px, "<u2").tobytes():
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def test_the_check_program_on_the_case_file(tmp_path):
    """every stream and every low-bit array from a heap block of exactly its size: a read past
    either is the sanitizer's to report"""
    names = [n for n in NAMES if F.build_case(n)["width"] * F.build_case(n)["height"] <= 40000]
    path = tmp_path / "cases.bin"
    want = []
    with open(path, "wb") as f:
        f.write(b"RSXC" + struct.pack("<I", len(names)))
        for k, name in enumerate(names):
            c = F.build_case(name)
            lowbits = k % 3 != 2
            low = c["low"] if lowbits else b""
            pitch = 2 * c["width"] + 2 * (k % 4)
            f.write(struct.pack("<7I", c["width"], c["height"], pitch, c["table"], int(lowbits),
                                len(low), len(c["data"])))
            f.write(low)
            f.write(c["data"])
            st, px = F.expected(name, lowbits)
            vst = F.validate(c["width"], c["height"], c["table"], lowbits, len(low),
                             len(c["data"]), 1, pitch)
            want.append("%d %d %016x" % (vst, -1 if vst != F.OK else st,
                                         _fnv(px) if st == F.OK else 0))
    r = subprocess.run([build.BIN_CRW_CHECK, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split("\n")[:-1] == want
