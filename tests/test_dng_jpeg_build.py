"""The lossy-JPEG tile decode builds: rsx_dng_jpeg.hip for gfx950 (hipcc cross-compiles; no GPU
needed), the host library, the symbols the package binds, the struct layouts of rawspeed_amd/abi.py
against include/rsx.h (a C program prints them), and the stand-alone program rsx_jpeg_host_check
-- its own main, AddressSanitizer and UBSan where g++ has them, run as a plain child process --
which decodes every fixture, every damaged stream and 2000 seeded corruptions through the host
core."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess
import tempfile

import pytest

import dng_jpeg_files as J
from rawspeed_amd import abi, build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rawspeed_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")

EXPORTS = ["rsx_dng_jpeg_validate", "rsx_dng_decompress_jpeg", "rsx_dng_jpeg_plan_create",
           "rsx_dng_jpeg_plan_tile_status"]


def test_the_kernels_compile_for_gfx950():
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc"))
                  if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.skip("hipcc not found")
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", "-Wall",
                            "-Wno-unused-function", "-Werror", "-I" + INCLUDE, "-I" + CSRC,
                            os.path.join(CSRC, "rsx_dng_jpeg.hip"), "-o", os.path.join(d, "jpeg.o")],
                           capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr


def test_sources_are_part_of_the_core_library():
    assert "rsx_dng_jpeg.hip" in build.CORE_SOURCES
    assert "rsx_dng_jpeg.h" in build.CORE_HEADERS and "rsx_jpeg_core.h" in build.CORE_HEADERS
    for name in ("rsx_dng_jpeg.hip", "rsx_dng_jpeg.h", "rsx_jpeg_core.h", "rsx_jpeg_host.cpp"):
        assert os.path.exists(os.path.join(CSRC, name))


def test_host_library_builds_and_exports():
    lib_path, prog = build.build_jpeg_host()
    assert os.path.exists(lib_path) and os.access(prog, os.X_OK)
    L = C.CDLL(lib_path)
    for name in ("rsx_jpeg_host_validate", "rsx_jpeg_host_decode"):
        assert hasattr(L, name), name


def test_exports_are_declared_in_the_header_and_bound():
    header = open(os.path.join(INCLUDE, "rsx.h")).read()
    src = open(os.path.join(CSRC, "rsx_api.hip")).read()
    assert sorted(n for n in capi.EXPORTS if "_jpeg" in n and "ljpeg" not in n) == sorted(EXPORTS)
    for n in EXPORTS:
        assert re.search(r"\bint %s\(" % n, header), n
        assert re.search(r'extern "C" int %s\(' % n, src), n
        getattr(capi.lib(), n)


def test_struct_layouts_match_the_header():
    fields = {"rsx_dng_jpeg_tile": (abi.DngJpegTile, {"in": "in_", "in_bytes": "in_bytes",
                                                      "off_x": "off_x", "off_y": "off_y"}),
              "rsx_dng_jpeg_info": (abi.DngJpegInfo, {f: f for f in (
                  "width", "height", "components", "h_samp", "v_samp", "colour_space",
                  "restart_interval", "n_segments")}),
              "rsx_dng_jpeg_job": (abi.DngJpegJob, {f: f for f in (
                  "n_tiles", "tiles", "in_offsets", "img_offset", "img")})}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rsx.h"', "int main(void) {"]
    for c_name, (_, names) in fields.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (c_name, c_name))
        for f in names:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (c_name, f, c_name, f))
    lines.append("return 0; }")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as f:
            f.write("\n".join(lines))
        subprocess.run(["gcc", "-I" + INCLUDE, src, "-o", exe], check=True, capture_output=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    got = dict(line.split() for line in out.splitlines())
    for c_name, (t, names) in fields.items():
        assert int(got[c_name]) == C.sizeof(t), c_name
        for c_field, py_field in names.items():
            assert int(got["%s.%s" % (c_name, c_field)]) == getattr(t, py_field).offset, (c_name, c_field)


def test_the_model_and_the_core_agree_on_the_overshoot_bound():
    core = open(os.path.join(CSRC, "rsx_jpeg_core.h")).read()
    assert re.search(r"OVERSHOOT = %d;" % J.OVERSHOOT, core)


def test_the_check_program_carries_the_sanitizers_where_the_compiler_has_them():
    if not build._links_with_sanitizers():
        pytest.skip("g++ has no sanitizer runtimes here")
    _, prog = build.build_jpeg_host()
    data = open(prog, "rb").read()
    assert b"__asan_init" in data and b"__ubsan_handle" in data


def test_the_check_program_decodes_every_stream_and_2000_corruptions_clean():
    _, prog = build.build_jpeg_host()
    streams = [c["stream"] for c in J.cases() + J.damaged() + J.forged()]
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "corpus.bin")
        with open(path, "wb") as f:
            f.write(b"RSXJ" + struct.pack("<I", len(streams)))
            for s in streams:
                f.write(struct.pack("<I", len(s)) + s)
        r = subprocess.run([prog, path, "2000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"corpus: (\d+) decoded, (\d+) refused; corruptions: (\d+) decoded, (\d+) refused",
                  r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) + int(m.group(2)) == len(streams)
    assert int(m.group(1)) >= len(J.cases())  # (every undamaged fixture decodes)
    assert int(m.group(3)) + int(m.group(4)) == 2000 and int(m.group(4)) > 0
