"""The compiled baseline-DCT JPEG writer (rsx_dctwrite.hip): it compiles for gfx950 with -Werror,
its kernels use no scratch and spill nothing; the core header compiles as strict host C++17; the
check program runs (a stand-alone program with AddressSanitizer and UBSan where g++ has them:
nothing is loaded into Python) and proves the reciprocal quantiser; the library is built from the
sources and binds the section's symbols, none of which falls under another section's pinned prefix;
the struct layouts of rawspeed_amd/abi.py are include/rsx.h's.  hipcc cross-compiles gfx950; no GPU
needed."""
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
EXPORTS = ["rsx_dctwrite_quality_tables", "rsx_dctwrite_validate", "rsx_dctwrite_bound",
           "rsx_dctwrite", "rsx_dctwrite_plan_create", "rsx_dctwrite_plan_result"]
KERNELS = ["dctwrite_transform_kernel", "dctwrite_length_kernel", "dctwrite_scan_kernel",
           "dctwrite_offsets_kernel", "dctwrite_zero_kernel", "dctwrite_emit_kernel",
           "dctwrite_count_kernel", "dctwrite_place_kernel", "dctwrite_stuff_kernel"]
NEW_SOURCES = ("rsx_dctwrite.hip", "rsx_dctwrite.h", "rsx_dctwrite_core.h", "rsx_dctwrite_host.cpp")


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not found")


def test_hip_file_compiles_for_gfx950_without_warnings():
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c",
                            "-Wall", "-Wno-unused-function", "-Werror", "-I" + INCLUDE, "-I" + CSRC,
                            os.path.join(CSRC, "rsx_dctwrite.hip"), "-o", os.path.join(d, "w.o")],
                           capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr


def test_kernels_have_no_scratch_and_no_spills():
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S",
                        "--cuda-device-only", "-I" + INCLUDE, "-I" + CSRC,
                        os.path.join(CSRC, "rsx_dctwrite.hip"), "-o", out], check=True,
                       capture_output=True, timeout=600)
        text = open(out).read()
    bodies = dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S))
    assert len(bodies) == len(KERNELS)
    for name in KERNELS:
        (body,) = [b for n, b in bodies.items() if name in n]
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) == 0, name
    assert len(re.findall(r"\.vgpr_spill_count:\s+0\b", text)) == len(KERNELS)
    assert len(re.findall(r"\.sgpr_spill_count:\s+0\b", text)) == len(KERNELS)
    assert "global_store_dwordx4" in text  # a lane's eight coefficients in one store
    assert "global_atomic_or" in text      # the words two blocks share


def test_core_header_compiles_as_strict_host_cxx():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        open(src, "w").write('#include "rsx_dctwrite_core.h"\n'
                             "int main() { using namespace rsx_dctw;\n"
                             "  uint16_t lu[64], ch[64];\n"
                             "  int d[8] = {1, 1, 1, 1, 1, 1, 1, 1};\n"
                             "  fdct_pass<true>(d);\n"
                             "  HuffEnc h; build_huff(&h);\n"
                             "  return quality_tables(50, lu, ch) == RSX_OK && lu[0] == 16 && ch[63] == 99 &&\n"
                             "         d[0] == 32 && d[1] == 0 && quantise(-12, 1, recip_of(1)) == -2 &&\n"
                             "         h.dc_len[0][0] == 2 && h.ac_code[0][0] == 10 && h.ac_len[1][0xF0] == 10 &&\n"
                             "         bit_length(1023) == 10 && value_bits(-3, 2) == 0 ? 0 : 1; }\n")
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + INCLUDE,
                        "-I" + CSRC, src, "-o", os.path.join(d, "t")], check=True,
                       capture_output=True)
        assert subprocess.run([os.path.join(d, "t")]).returncode == 0


def test_check_program_runs():
    build.build_dctwrite_host()
    r = subprocess.run([build.BIN_DCTWRITE_CHECK], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("rsx_dctwrite_host_check OK") and "ERROR" not in r.stderr
    assert "quantise: 32768 x 255 pairs equal the division" in r.stdout
    assert re.search(r"frames: \d+ written, bounded and refused", r.stdout)


def test_the_library_is_built_from_the_sources():
    assert "rsx_dctwrite.hip" in build.CORE_SOURCES
    for name in ("rsx_dctwrite.h", "rsx_dctwrite_core.h"):
        assert name in build.CORE_HEADERS
    for name in build.CORE_SOURCES + build.CORE_HEADERS:
        assert os.path.exists(os.path.join(build.CSRC, name)), name
    assert os.path.exists(os.path.join(build.CSRC, "rsx_dctwrite_host.cpp"))
    assert os.path.basename(build.LIB_DCTWRITE_HOST) == "librsx_dctwrite_host.so"
    assert "build_dctwrite_host()" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "rawspeed_amd/rsx_dctwrite_host_check" in open(os.path.join(ROOT, ".gitignore")).read()
    # plain HIP C++: no inline assembly, no kernel kept in a string
    for name in NEW_SOURCES:
        text = open(os.path.join(CSRC, name)).read()
        assert "asm" not in text and "hiprtc" not in text, name


def test_symbols_and_layouts():
    header = open(os.path.join(INCLUDE, "rsx.h")).read()
    assert "7e. Lossy (baseline DCT) JPEG tiles" in header
    assert "#define RSX_ABI_VERSION 4" in header and abi.RSX_ABI_VERSION == 4
    assert sorted(n for n in capi.EXPORTS if n.startswith("rsx_dctwrite")) == sorted(EXPORTS)
    for n in EXPORTS:  # (the names other sections pin)
        assert "_jpeg" not in n and not n.startswith(("rsx_encode_", "rsx_fpwrite_", "rsx_dng_lossy"))
    lib = capi.lib()
    assert lib.rsx_abi_version() == 4
    for n in EXPORTS:
        assert re.search(r"\b%s\(" % n, header), n
        getattr(lib, n)
    structs = {"rsx_dctwrite_desc": (abi.DctWriteDesc,
                                     ("off_x", "off_y", "width", "height", "components", "h_samp",
                                      "v_samp", "restart_interval", "flags", "reserved", "qtables")),
               "rsx_dctwrite_tile": (abi.DctWriteTile, ("desc", "out", "out_cap")),
               "rsx_dctwrite_result": (abi.DctWriteResult, ("status", "reserved", "bytes",
                                                            "scan_bytes", "symbol_bits")),
               "rsx_dctwrite_job": (abi.DctWriteJob, ("desc", "img_offset", "out_offset", "out_cap",
                                                      "img"))}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rsx.h"', "int main(void) {"]
    for s, (_, fields) in structs.items():
        lines.append('printf("%%zu", sizeof(%s));' % s)
        for f in fields:
            lines.append('printf(" %%zu", offsetof(%s, %s));' % (s, f))
        lines.append('printf("\\n");')
    lines.append('printf("%u\\n", RSX_DCTWRITE_JFIF);')
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
    assert int(out[len(structs)]) == abi.DCTWRITE_JFIF


def test_quality_tables_export_is_the_models():
    import dctwrite_files as D
    for q in range(1, 101):
        st, lu, ch = capi.dctwrite_quality_tables(q)
        assert st == 0 and (lu, ch) == D.model_quality_tables(q), q
    assert capi.dctwrite_quality_tables(0)[0] == D.INVALID_ARG
    assert capi.dctwrite_quality_tables(101)[0] == D.INVALID_ARG
