"""rsx_kodak_core.h as host C++ (rawspeed_amd/librsx_kodak_host.so): every case of
tests/kodak_files.py under each table mode against the model and the reference's recorded hashes,
pixels and verdicts; with a padded pitch; the closed forms; and the case file through
rsx_kodak_host_check, the same source built as a program with AddressSanitizer and UBSan where g++
has them."""
import struct
import subprocess

import numpy as np
import pytest

import kodak_files as F
from rawspeed_amd import abi, build

NAMES = F.names()
ROUTE = {F.NONE: "uncorrected", F.DITHER: "corrected"}


@pytest.mark.parametrize("name", NAMES)
def test_case(name):
    c, b = F.case(name), F.build_case(name)
    g = F.golden()[name]
    for mode in (F.NONE, F.PLAIN, F.DITHER):
        st, px, buf, consumed = F.host_decode(b["data"], c["width"], c["height"], c["bps"], mode,
                                              F.table_for(mode, b["curve"]))
        want_st, want = F.expected(name, mode)
        assert st == want_st
        if mode in ROUTE:
            assert st == g[ROUTE[mode]][0]
        if st == F.OK:
            assert np.array_equal(px, want)
            assert consumed == F.model_values(name)[2]
            if mode in ROUTE:
                assert F.sha_rows(px) == g[ROUTE[mode]][1]
        else:
            assert (buf == 0xA5).all(), "a failing decode wrote into the image"


@pytest.mark.parametrize("name", ["g_260x65", "g_4x2", "g_516x2"])
@pytest.mark.parametrize("pad", [2, 10, 16])
def test_padded_pitch(name, pad):
    c, b = F.case(name), F.build_case(name)
    w, h = c["width"], c["height"]
    st, px, buf, _ = F.host_decode(b["data"], w, h, c["bps"], F.DITHER,
                                   F.dither_table(b["curve"]), pitch=2 * w + pad)
    assert st == F.OK
    assert np.array_equal(px, F.expected(name, F.DITHER)[1])
    assert (buf.reshape(h, 2 * w + pad)[:, 2 * w:] == 0xA5).all(), "the pitch padding was written"


def test_refusals_at_their_boundaries():
    """what the whole-file route cannot express: the constructor's refusals, held against the core"""
    data = bytes(1 << 16)
    for w, h, bps, cpp in ((4520, 1, 12, 1), (4, 3013, 12, 1), (6, 2, 12, 1), (8, 2, 11, 1),
                           (8, 2, 12, 2)):
        st, px, buf, _ = F.host_decode(data, w, h, bps, F.NONE, None, cpp=cpp)
        assert st == F.ERR_INVALID_ARG == F.validate(w, h, bps, len(data), cpp=cpp)
        assert (buf == 0xA5).all()
    st, px, _, _ = F.host_decode(bytes(4516 // 4 * 610), 4516, 1, 12, F.NONE, None)
    assert st == F.OK and not px.any()


def test_closed_forms():
    L = F.host_lib()
    for length in (4, 8, 12, 252, 256):
        for total in range(0, 15 * length + 1, 1 if length < 16 else 7):
            assert L.rsx_kodak_host_segment_bytes(length, total) == F.segment_bytes(length, total)
    for w, h in ((4, 1), (260, 3), (4516, 3012), (256, 7)):
        assert L.rsx_kodak_host_image_bound(w, h) == F.image_bound(w, h)
    assert abi.kodak_table_entries(10, F.PLAIN) == 1024 and abi.kodak_table_entries(10, F.DITHER) == 2048
    assert abi.kodak_table_entries(12, F.PLAIN) == 4096 and abi.kodak_table_entries(12, F.DITHER) == 8192
    assert abi.kodak_table_entries(12, F.NONE) == 0


def _fnv(px):
    h = 0xcbf29ce484222325
    for b in np.ascontiguousarray(px, "<u2").tobytes():
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def test_the_check_program_on_the_case_file(tmp_path):
    """every stream and table from a heap block of exactly its size: a read past either is the
    sanitizer's to report"""
    names = [n for n in NAMES if F.case(n)["width"] * F.case(n)["height"] <= 40000]
    path = tmp_path / "cases.bin"
    want = []
    with open(path, "wb") as f:
        f.write(b"RSXK" + struct.pack("<I", len(names)))
        for k, name in enumerate(names):
            c, b = F.case(name), F.build_case(name)
            mode = (F.NONE, F.PLAIN, F.DITHER)[k % 3]
            table = F.table_for(mode, b["curve"])
            entries = 0 if table is None else table.size
            pitch = 2 * c["width"] + 2 * (k % 4)
            f.write(struct.pack("<7I", c["width"], c["height"], pitch, c["bps"], mode, entries,
                                len(b["data"])))
            if entries:
                f.write(table.astype("<u2").tobytes())
            f.write(b["data"])
            st, px = F.expected(name, mode)
            vst = F.validate(c["width"], c["height"], c["bps"], len(b["data"]), pitch)
            want.append("%d %d %016x" % (vst, -1 if vst != F.OK else st,
                                         _fnv(px) if st == F.OK else 0))
    r = subprocess.run([build.BIN_KODAK_CHECK, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split("\n")[:-1] == want
