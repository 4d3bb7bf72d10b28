"""rsx_fuji_core.h as host C++ (rawspeed_amd/librsx_fuji_host.so): every case of
tests/fuji_files.py against the model and the reference's recorded hashes, statuses included; on
threads; with a padded pitch; and the case file through rsx_fuji_host_check, the same source built
as a program with AddressSanitizer and UBSan where g++ has them."""
import os
import subprocess

import numpy as np
import pytest

import fuji_files as F

NAMES = [c["name"] for c in F.case_list()]


@pytest.mark.parametrize("name", NAMES)
def test_case(name):
    b = F.build_case(name)
    rc, sts, px = F.expected(name)
    hrc, hs, got = F.host_decode(b["data"], pad=name.count("1") % 3)
    assert (hrc, hs) == (rc, sts)
    F.check_pixels(name, got, 0xA5A5)
    g = F.golden()[name]
    assert g["ok"] == (hrc == F.OK)
    if g["ok"]:
        assert F.sha_rows(got) == g["sha256"]


def test_strips_on_threads():
    for name in (n for n in NAMES if "12288x6" in n or n.endswith("_multi")):
        b = F.build_case(name)
        one = F.host_decode(b["data"], threads=1)
        many = F.host_decode(b["data"], threads=5)
        assert one[:2] == many[:2] == F.expected(name)[:2]
        assert np.array_equal(one[2], many[2])


def test_strips_outside_the_input():
    import ctypes as C
    from rawspeed_amd import abi
    b = F.build_case("b14_768x6_flat")
    st, d = F.host_parse(b["data"])
    buf = np.zeros((6, 768), np.uint16)
    view = abi.Image(buf.ctypes.data, 2 * 768, 768, 6, 1, 1)
    a = np.frombuffer(b["data"], np.uint8)
    assert F.host_lib().rsx_fuji_host_decode(C.byref(d), a.ctypes.data, len(b["data"]) - 1,
                                             C.byref(view), None, 1) == F.ERR_IO


def test_check_program_on_the_case_file(tmp_path):
    from rawspeed_amd import build
    build.build_fuji_host()
    path = str(tmp_path / "cases.bin")
    names = F.write_cases(path)
    r = subprocess.run([build.BIN_FUJI_CHECK, path], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(names)
    for name, line in zip(names, lines):
        rc, sts, _ = F.expected(name)
        assert [int(v) for v in line.split()] == [0, 0, rc] + sts, name
