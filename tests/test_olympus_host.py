"""rsx_olympus_core.h as host C++ (rawspeed_amd/librsx_olympus_host.so): every case of
tests/olympus_files.py against the model and the reference's recorded hashes, statuses included;
with a padded pitch; and the case file through rsx_olympus_host_check, the same source built as a
program with AddressSanitizer and UBSan where g++ has them."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import olympus_files as F
from rawspeed_amd import abi

CASES = F.case_list()
NAMES = [c["name"] for c in CASES]


@pytest.mark.parametrize("name", NAMES)
def test_case(name):
    c = F.case(name)
    rc, px = F.expected(name)
    hrc, got = F.host_expected(name)
    assert hrc == rc
    g = F.golden()[name]
    assert g["ok"] == (hrc == F.OK)
    if g["ok"]:
        assert np.array_equal(got, px)
        assert F.sha_rows(got) == g["sha256"]


@pytest.mark.parametrize("name", ["g_130x6_noise12", "g_4x130_noise12", "c_6x6_checker"])
@pytest.mark.parametrize("pad", [1, 5, 8])
def test_padded_pitch(name, pad):
    c = F.case(name)
    w, h = c["width"], c["height"]
    rc, buf = F.host_decode(F.build_case(name)["data"], w, h, pad=pad)
    assert rc == F.OK
    assert np.array_equal(buf[:, :w], F.expected(name)[1])
    assert (buf[:, w:] == 0xA5A5).all(), "the pitch padding was written"


def test_a_failing_decode_leaves_the_image():
    for name in ("r_cut_3", "r_2x2_10_bytes", "x_3x2"):
        c = F.case(name)
        rc, buf = F.host_decode(F.build_case(name)["data"], c["width"], c["height"])
        assert rc == F.expected(name)[0] != F.OK
        assert (buf == 0xA5A5).all()


def test_validate():
    v = F.host_lib().rsx_olympus_host_validate

    def img(w, h, pitch=None, cpp=1):
        return abi.Image(None, 2 * max(w, 0) if pitch is None else pitch, w, h, cpp, 1)
    assert v(100, C.byref(img(4, 4))) == F.OK
    assert v(100, None) == F.ERR_INVALID_ARG
    for w, h in F.REFUSED:
        assert v(100, C.byref(img(w, h))) == F.ERR_INVALID_ARG
    assert v(100, C.byref(img(F.MAX_X, F.MAX_Y))) == F.OK
    assert v(100, C.byref(img(4, 4, pitch=6))) == F.ERR_INVALID_ARG
    assert v(100, C.byref(img(4, 4, cpp=3))) == F.ERR_INVALID_ARG
    # the constructor comes before the reader
    assert v(3, C.byref(img(3, 2))) == F.ERR_INVALID_ARG
    assert [v(n, C.byref(img(2, 2))) for n in (0, 6, 7, 10, 11)] == [F.ERR_IO] * 4 + [F.OK]
    for w, h in ((4, 4), (3, 2), (0, 2), (10402, 2)):
        for n in (6, 10, 11):
            assert v(n, C.byref(img(w, h))) == F.validate(n, w, h)


def test_check_program_on_the_case_file(tmp_path):
    from rawspeed_amd import build
    build.build_olympus_host()
    path = str(tmp_path / "cases.bin")
    names = F.write_cases(path, pad=6)
    r = subprocess.run([build.BIN_OLYMPUS_CHECK, path], capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(names)
    for name, line in zip(names, lines):
        c = F.case(name)
        rc, px = F.expected(name)
        vst = F.validate(len(F.build_case(name)["data"]), c["width"], c["height"])
        want = [vst, rc if vst == F.OK else -1, F.fnv_rows(px) if rc == F.OK else 0]
        got = line.split()
        assert [int(got[0]), int(got[1]), int(got[2], 16)] == want, name
