"""The compiled F32 writers (rsx_fpwrite_pack.hip): the kernels compile for gfx950 without scratch
or spills and a lane's 16 bytes go out in one store; the core headers compile as strict host
C++17; the check program runs (a stand-alone program with AddressSanitizer and UBSan where g++ has
them: nothing is loaded into Python) and walks every binary16 and binary24 pattern; the library
binds the section's symbols; the struct layouts of rawspeed_amd/abi.py are include/rsx.h's.
hipcc cross-compiles gfx950; no GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from rawspeed_amd import abi, build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "rawspeed_amd", "csrc")
EXPORTS = ["rsx_fpwrite_fit", "rsx_fpwrite_pack_validate", "rsx_fpwrite_pack",
           "rsx_fpwrite_pack_plan_create", "rsx_fpwrite_pack_plan_result",
           "rsx_fpwrite_deflate_validate", "rsx_fpwrite_deflate_bound", "rsx_fpwrite_deflate",
           "rsx_fpwrite_deflate_plan_create", "rsx_fpwrite_deflate_plan_result"]
KERNELS = ["fpwrite_pack_kernel", "fpwrite_fit_kernel"]
DEFLATE_KERNELS = ["fpwrite_deflate_planes_kernel", "fpwrite_deflate_block_kernel",
                   "fpwrite_deflate_scan_kernel", "fpwrite_deflate_emit_kernel"]
NEW_SOURCES = ("rsx_fpwrite_pack.hip", "rsx_fpwrite_core.h", "rsx_fp_narrow.h", "rsx_fpwrite.h",
               "rsx_fpwrite_host.cpp", "rsx_fpwrite_deflate.hip", "rsx_deflate_core.h")


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not found")


def test_kernels_have_no_scratch_and_no_spills():
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S",
                        "--cuda-device-only", "-I" + INCLUDE, "-I" + CSRC,
                        os.path.join(CSRC, "rsx_fpwrite_pack.hip"), "-o", out], check=True,
                       capture_output=True, timeout=300)
        text = open(out).read()
    bodies = dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S))
    assert len(bodies) == len(KERNELS)
    for name in KERNELS:
        (body,) = [b for n, b in bodies.items() if name in n]
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) == 0, name
    assert len(re.findall(r"\.vgpr_spill_count:\s+0\b", text)) == len(KERNELS)
    assert len(re.findall(r"\.sgpr_spill_count:\s+0\b", text)) == len(KERNELS)
    assert "global_store_dwordx4" in text  # a lane's 16 bytes in one store


def test_deflate_kernels_compile_and_report_their_scratch():
    """the four kernels compile for gfx950 without spills; the block kernel's private segment (the
    code counts of the canonical code) is reported, not hidden: it stays small"""
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S",
                        "--cuda-device-only", "-I" + INCLUDE, "-I" + CSRC,
                        os.path.join(CSRC, "rsx_fpwrite_deflate.hip"), "-o", out], check=True,
                       capture_output=True, timeout=300)
        text = open(out).read()
    bodies = dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S))
    assert len(bodies) == len(DEFLATE_KERNELS)
    for name in DEFLATE_KERNELS:
        (body,) = [b for n, b in bodies.items() if name in n]
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
        print(name, "private segment", scratch)
        assert scratch == 0 or (name == "fpwrite_deflate_block_kernel" and scratch <= 256), name
    assert len(re.findall(r"\.vgpr_spill_count:\s+0\b", text)) == len(DEFLATE_KERNELS)
    assert len(re.findall(r"\.sgpr_spill_count:\s+0\b", text)) == len(DEFLATE_KERNELS)


def test_check_program_walks_the_deflate_shape_list():
    """every tile of the shape list through the host core as a stand-alone program under the
    sanitizers: into the bound, into exactly its size, one byte short, and with an inexact sample"""
    import fpwrite_files as F
    build.build_fpwrite_host()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "tiles.bin")
        n = F.write_deflate_cases(path)
        r = subprocess.run([build.BIN_FPWRITE_CHECK, path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "deflate: %d tiles" % n in r.stdout and "ERROR" not in r.stderr
    assert r.stdout.strip().endswith("rsx_fpwrite_host_check OK")


def test_core_headers_compile_as_strict_host_cxx():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        open(src, "w").write('#include "rsx_fpwrite_core.h"\n'
                             "int main() { uint32_t n = 0;\n"
                             "  const bool half = narrow_fp<10, 5>(0x3F800000u, &n) && n == 0x3C00u;\n"
                             "  const bool not24 = !narrow_fp<16, 7>(0x3F800001u, &n);\n"
                             "  return half && not24 && fp_fit_class(0x3F800080u) == 1 &&\n"
                             "         widen_fp_plain<10, 5>(1) == 0x33800000u &&\n"
                             "         rsx_fpwrite::round_up4(5) == 8 ? 0 : 1; }\n")
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + INCLUDE,
                        "-I" + CSRC, src, "-o", os.path.join(d, "t")], check=True,
                       capture_output=True)
        assert subprocess.run([os.path.join(d, "t")]).returncode == 0


def test_check_program_runs():
    build.build_fpwrite_host()
    r = subprocess.run([build.BIN_FPWRITE_CHECK], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("rsx_fpwrite_host_check OK") and "ERROR" not in r.stderr
    assert "narrow 16: 65536 patterns" in r.stdout and "narrow 24: 16777216 patterns" in r.stdout
    assert re.search(r"pack: \d+ geometries round-trip", r.stdout)


def test_the_library_is_built_from_the_sources():
    assert "rsx_fpwrite_pack.hip" in build.CORE_SOURCES
    assert "rsx_fpwrite_deflate.hip" in build.CORE_SOURCES
    for name in ("rsx_fpwrite.h", "rsx_fpwrite_core.h", "rsx_fp_narrow.h", "rsx_deflate_core.h"):
        assert name in build.CORE_HEADERS
    for name in build.CORE_SOURCES + build.CORE_HEADERS:
        assert os.path.exists(os.path.join(build.CSRC, name)), name
    assert os.path.exists(os.path.join(build.CSRC, "rsx_fpwrite_host.cpp"))
    assert os.path.basename(build.LIB_FPWRITE_HOST) == "librsx_fpwrite_host.so"
    assert "build_fpwrite_host()" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "rawspeed_amd/rsx_fpwrite_host_check" in open(os.path.join(ROOT, ".gitignore")).read()
    # plain HIP C++: no inline assembly in the writers
    for name in NEW_SOURCES:
        assert "asm" not in open(os.path.join(CSRC, name)).read()


def test_symbols_and_layouts():
    header = open(os.path.join(INCLUDE, "rsx.h")).read()
    assert "7d. Floating-point images" in header
    assert "#define RSX_ABI_VERSION 4" in header and abi.RSX_ABI_VERSION == 4
    assert sorted(n for n in capi.EXPORTS if n.startswith("rsx_fpwrite_")) == sorted(EXPORTS)
    lib = capi.lib()
    assert lib.rsx_abi_version() == 4
    for n in EXPORTS:
        assert re.search(r"\b%s\(" % n, header), n
        getattr(lib, n)
    structs = {"rsx_fpwrite_window": (abi.FpWriteWindow, ("x", "y", "w", "h")),
               "rsx_fpwrite_pack_result": (abi.FpWritePackResult,
                                           ("bytes_written", "stream_bytes", "inexact")),
               "rsx_fpwrite_pack_job": (abi.FpWritePackJob, ("desc", "reserved", "img_offset",
                                                             "out_offset", "out_cap", "img")),
               "rsx_fpwrite_deflate_tile": (abi.FpWriteDeflateTile,
                                            ("out", "out_cap", "tile_w", "tile_h", "off_x", "off_y",
                                             "width", "height")),
               "rsx_fpwrite_deflate_result": (abi.FpWriteDeflateResult,
                                              ("status", "adler", "bytes", "blocks", "stored_blocks")),
               "rsx_fpwrite_deflate_job": (abi.FpWriteDeflateJob,
                                           ("desc", "tile_w", "tile_h", "off_x", "off_y", "width",
                                            "height", "img_offset", "out_offset", "out_cap", "img"))}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rsx.h"', "int main(void) {"]
    for s, (_, fields) in structs.items():
        lines.append('printf("%%zu", sizeof(%s));' % s)
        for f in fields:
            lines.append('printf(" %%zu", offsetof(%s, %s));' % (s, f))
        lines.append('printf("\\n");')
    lines.append('printf("%d\\n", RSX_FPWRITE_BLOCK);')
    lines.append("return 0; }")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", "-I" + INCLUDE, src, "-o", os.path.join(d, "t")],
                       check=True, capture_output=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True).stdout.split("\n")
    for line, (s, (cls, fields)) in zip(out, structs.items()):
        want = [C.sizeof(cls)] + [getattr(cls, f).offset for f in fields]
        assert [int(v) for v in line.split()] == want, s
    assert int(out[len(structs)]) == abi.FPWRITE_BLOCK
