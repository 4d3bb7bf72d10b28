"""The bad-pixel stage builds: the host library and its program (which passes, on its built-in cases
and on the model's), the symbols the package binds, the struct layouts of rawspeed_amd/abi.py
against include/rsx.h (a C program prints them), and the compiled kernels -- no scratch, at most
128 vector registers, every memory access global.  hipcc cross-compiles gfx950; no GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import bad_pixels_files as B
from rawspeed_amd import abi, build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rawspeed_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")

EXPORTS = ["rsx_bad_pixels_validate", "rsx_bad_pixels_fix", "rsx_bad_pixels_plan_create",
           "rsx_bad_pixels_plan_result", "rsx_panasonic_v4_decompress_fixed", "rsx_dng_finish",
           "rsx_dng_decompress_ljpeg_finish", "rsx_dng_decompress_uncompressed_finish"]


def test_host_library_and_program_build():
    lib_path, prog = build.build_bad_pixels_host()
    assert os.path.exists(lib_path) and os.access(prog, os.X_OK)
    L = C.CDLL(lib_path)
    for name in ("rsx_bad_pixels_host_validate", "rsx_bad_pixels_host_fix"):
        assert hasattr(L, name), name


def test_the_check_program_passes_on_its_own_cases_and_on_the_models():
    _, prog = build.build_bad_pixels_host()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "cases.bin")
        B.write_case_file(path)
        r = subprocess.run([prog, path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d file cases" % len(B.cases()) in r.stdout
    assert "rsx_bad_pixels_host_check OK" in r.stdout


def test_the_check_program_carries_the_sanitizers_where_the_compiler_has_them():
    """build_bad_pixels_host() builds plain only where an empty program does not link with the
    sanitizer flags; where one does, the check program must be the instrumented one"""
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
             "-static-libubsan"]
    assert flags == build.SANITIZE
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        with open(src, "w") as f:
            f.write("int main() { return 0; }\n")
        can = subprocess.run(["g++", src, "-o", os.path.join(d, "t")] + flags,
                             capture_output=True).returncode == 0
    if not can:
        pytest.skip("g++ has no sanitizer runtimes here")
    _, prog = build.build_bad_pixels_host()
    data = open(prog, "rb").read()
    assert b"__asan_init" in data and b"__ubsan_handle" in data


def test_sources_are_part_of_the_core_library():
    assert "rsx_bad_pixels.hip" in build.CORE_SOURCES
    assert "rsx_bad_pixels.h" in build.CORE_HEADERS and "rsx_bad_pixels_core.h" in build.CORE_HEADERS
    for name in ("rsx_bad_pixels.hip", "rsx_bad_pixels.h", "rsx_bad_pixels_core.h",
                 "rsx_bad_pixels_host.cpp"):
        assert os.path.exists(os.path.join(CSRC, name))


def test_exports_are_declared_in_the_header():
    header = open(os.path.join(INCLUDE, "rsx.h")).read()
    src = open(os.path.join(CSRC, "rsx_api.hip")).read()
    names = [n for n in capi.EXPORTS if "bad_pixels" in n and "dng_post" not in n and
             not n.startswith("rsx_panasonic_v4_plan")] + ["rsx_panasonic_v4_decompress_fixed"] + \
        [n for n in capi.EXPORTS if n.endswith("_finish")]
    assert sorted(names) == sorted(EXPORTS)
    for n in EXPORTS:
        assert n in capi.EXPORTS, n
        assert re.search(r"\bint %s\(" % n, header), n
        assert re.search(r'extern "C" int %s\(' % n, src), n
    assert re.search(r"#define RSX_ABI_VERSION 4\b", header)


def test_struct_layouts_match_the_header():
    fields = {"rsx_bad_pixels_desc": (abi.BadPixelsDesc, ["positions", "n_positions", "map_pitch",
                                                          "map_in", "map_out", "is_f32"]),
              "rsx_bad_pixels_result": (abi.BadPixelsResult, ["n_bad", "n_fixed", "map_made"]),
              "rsx_bad_pixels_job": (abi.BadPixelsJob, ["in_offset", "n_positions", "map_pitch",
                                                        "map_in", "is_f32", "img_offset", "img"])}
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
        for f in names:
            assert int(got["%s.%s" % (c_name, f)]) == getattr(t, f).offset, (c_name, f)


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not found")


@pytest.fixture(scope="module")
def kernels():
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "bad_pixels.s")
        subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S",
                        "--cuda-device-only", "-I" + INCLUDE, "-I" + CSRC,
                        os.path.join(CSRC, "rsx_bad_pixels.hip"), "-o", out],
                       check=True, capture_output=True, timeout=300)
        asm = open(out).read()
    found = {}
    for name, body in re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, re.S):
        code = re.search(r"^%s:(.*?)^\.Lfunc_end" % re.escape(name), asm, re.S | re.M).group(1)
        get = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, body).group(1))  # noqa: E731
        found[name] = dict(scratch=get("private_segment_fixed_size"), vgpr=get("next_free_vgpr"),
                           lds=get("group_segment_fixed_size"), code=code)
    return asm, found


def test_kernels_without_scratch_and_flat_accesses(kernels):
    asm, found = kernels
    for stem, count in (("bp_init_kernel", 1), ("bp_zero_kernel", 1), ("bp_mark_kernel", 1),
                        ("bp_columns_kernel", 1), ("bp_fix_kernel", 2)):  # (uint16 and F32)
        hits = [v for k, v in found.items() if stem in k]
        assert len(hits) == count, (stem, list(found))
        for k in hits:
            assert k["scratch"] == 0 and k["lds"] == 0
            assert k["vgpr"] <= 128, (stem, k["vgpr"])  # (4 waves a SIMD at the least)
    assert len(found) == 6
    assert not re.search(r"\bscratch_", asm)
    assert not re.search(r"\bflat_(load|store|atomic)", asm)
    fix = [v for k, v in found.items() if "bp_fix_kernel" in k]
    for k in fix:
        assert "global_store_short" in k["code"] or "global_store_dword " in k["code"]
