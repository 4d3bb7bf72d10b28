"""The compiled image-hash kernels (rsx_image_hash.hip): the two row kernels and the finishing one compile for gfx950, use no scratch and
spill nothing; the core header compiles as host C++17 with -Wall -Wextra -Werror; the check program
runs (with AddressSanitizer and UBSan where g++ has them: a stand-alone program, nothing is loaded
into Python); the library is built from the sources, binds the section's symbols, and the struct
layouts of rawspeed_amd/abi.py are include/rsx.h's.  hipcc cross-compiles gfx950; no GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "rawspeed_amd", "csrc")
SRC = os.path.join(CSRC, "rsx_image_hash.hip")
EXPORTS = ["rsx_image_hash_validate", "rsx_image_hash", "rsx_image_hash_plan_create"]
# a lane of the row kernel: the state, two blocks of sixteen words, the sums, addresses
MAX_VGPRS = 64


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not found")


def test_kernels_have_no_scratch_and_no_spills():
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "ih.s")
        subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S",
                        "--cuda-device-only", "-I" + INCLUDE, "-I" + CSRC, SRC, "-o", out],
                       check=True, capture_output=True, timeout=300)
        text = open(out).read()
    bodies = dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S))
    assert len(bodies) == 3
    lds = {"image_hash_rows_kernelILb0E": 0, "image_hash_rows_kernelILb1E": 64 * 80,
           "image_hash_finish_kernel": 0}
    for name, want_lds in lds.items():
        (body,) = [b for n, b in bodies.items() if name in n]
        get = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, body).group(1))  # noqa: E731
        assert get("private_segment_fixed_size") == 0
        assert get("group_segment_fixed_size") == want_lds
        assert get("next_free_vgpr") <= MAX_VGPRS, get("next_free_vgpr")
    assert len(re.findall(r"\.private_segment_fixed_size:\s+0\b", text)) == 3
    assert len(re.findall(r"\.vgpr_spill_count:\s+0\b", text)) == 3
    assert len(re.findall(r"\.sgpr_spill_count:\s+0\b", text)) == 3
    # 16-byte loads of the rows and of the digests, a 16-byte store of a digest; the rotation and
    # the sums are one instruction each
    assert "global_load_dwordx4" in text and "global_store_dwordx4" in text
    assert "v_alignbit_b32" in text and "v_sad_u8" in text and "v_sad_u16" in text
    assert "ds_write_b128" in text and "ds_read_b128" in text


def test_core_header_compiles_as_strict_host_cxx():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        open(src, "w").write('#include "rsx_image_hash_core.h"\n'
                             "int main() { rsx_imghash::Md5 m; uint8_t d[16];\n"
                             '  m.update(reinterpret_cast<const uint8_t*>("abc"), 3);\n'
                             "  m.final(d);\n"
                             "  uint32_t s[4]; uint64_t b, v;\n"
                             '  rsx_imghash::hash_row(reinterpret_cast<const uint8_t*>("abc"), 3, s, &b, &v);\n'
                             "  rsx_image img = {nullptr, 16, 8, 1, 1, 0};\n"
                             "  return d[0] == 0x90 && d[15] == 0x72 && s[0] == 0x98500190u && b == 294 &&\n"
                             "         rsx_imghash::validate(&img, 2) == RSX_OK ? 0 : 1; }\n")
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + INCLUDE,
                        "-I" + CSRC, src, "-o", os.path.join(d, "t")], check=True,
                       capture_output=True)
        assert subprocess.run([os.path.join(d, "t")]).returncode == 0


def test_check_program_runs():
    from rawspeed_amd import build
    build.build_image_hash_host()
    r = subprocess.run([build.BIN_IMAGE_HASH_CHECK], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().split("\n") == ["suite 7", "lengths 804 804", "images 30 30", "ok"]


def test_check_program_runs_under_the_sanitizers():
    """the same source, built here with -fsanitize=address,undefined as a program of its own"""
    from rawspeed_amd import build
    if not build._links_with_sanitizers():
        pytest.skip("g++ has no sanitizer runtimes")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "check")
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-pthread",
                        "-I" + INCLUDE, "-I" + CSRC, "-DRSX_IMAGE_HASH_HOST_MAIN",
                        os.path.join(CSRC, "rsx_image_hash_host.cpp"), "-o", exe] + build.SANITIZE,
                       check=True, capture_output=True, timeout=300)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok") and "ERROR" not in r.stderr


def test_the_library_is_built_from_the_sources():
    from rawspeed_amd import build
    assert "rsx_image_hash.hip" in build.CORE_SOURCES
    assert "rsx_image_hash.h" in build.CORE_HEADERS and "rsx_image_hash_core.h" in build.CORE_HEADERS
    for name in build.CORE_SOURCES + build.CORE_HEADERS:
        assert os.path.exists(os.path.join(build.CSRC, name)), name
    assert os.path.exists(os.path.join(build.CSRC, "rsx_image_hash_host.cpp"))
    assert os.path.basename(build.LIB_IMAGE_HASH_HOST) == "librsx_image_hash_host.so"
    assert os.path.basename(build.BIN_IMAGE_HASH_CHECK) == "rsx_image_hash_host_check"
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "build_image_hash_host()" in entry
    ignore = open(os.path.join(ROOT, ".gitignore")).read()
    assert "rawspeed_amd/rsx_image_hash_host_check" in ignore


def test_the_md5_text_names_its_source():
    core = open(os.path.join(CSRC, "rsx_image_hash_core.h")).read()
    assert "RFC 1321" in core and "floor(2^32 |sin(i + 1)|)" in core


def test_symbols_and_layouts():
    from rawspeed_amd import abi, capi
    header = open(os.path.join(INCLUDE, "rsx.h")).read()
    assert "4g. The image hash of rstest" in header
    assert header.index("4f. DngDecoder's branch") < header.index("4g. The image hash of rstest")
    assert "#define RSX_ABI_VERSION 4" in header
    assert sorted(n for n in capi.EXPORTS if n.startswith("rsx_image_hash")) == sorted(EXPORTS)
    lib = capi.lib()
    for n in EXPORTS:
        assert re.search(r"\b%s\(" % n, header), n
        getattr(lib, n)
    structs = {"rsx_image_hash_result": (abi.ImageHashResult, ("md5", "byte_sum", "sample_sum")),
               "rsx_image_hash_job": (abi.ImageHashJob, ("img_offset", "lines_offset",
                                                         "result_offset", "sample_bytes",
                                                         "reserved", "img"))}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rsx.h"', "int main(void) {"]
    for name, (_, fields) in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        for f in fields:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f))
    lines += ["return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-I" + INCLUDE, src, "-o", exe], check=True)
        got = dict(l.split() for l in subprocess.run([exe], capture_output=True, text=True,
                                                     check=True).stdout.splitlines())
    for name, (cls, fields) in structs.items():
        assert int(got[name]) == C.sizeof(cls), name
        for f in fields:
            assert int(got["%s.%s" % (name, f)]) == getattr(cls, f).offset, (name, f)
    assert C.sizeof(abi.ImageHashResult) == 32
