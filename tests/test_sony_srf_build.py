"""The compiled Sony SRF kernel (rsx_sony_srf.hip): it compiles for gfx950, uses no scratch and
spills nothing; the core header compiles as host C++ with -Wall -Wextra -Werror; the check program
runs; the library is built from the sources, binds the section's symbols, and the struct layout of
rawspeed_amd/abi.py is include/rsx.h's.  hipcc cross-compiles gfx950; no GPU needed."""
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
SRC = os.path.join(CSRC, "rsx_sony_srf.hip")
EXPORTS = ["rsx_sony_decrypt", "rsx_sony_srf_validate", "rsx_sony_srf_decompress",
           "rsx_sony_srf_plan_create"]
MAX_VGPRS = 64
LDS_BYTES = 9728  # the table (256 words) and the chunk's 127 + 2048 words, rounded up to 16


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not found")


def test_kernel_has_no_scratch_and_moves_16_bytes():
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "srf.s")
        subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S",
                        "--cuda-device-only", "-I" + INCLUDE, "-I" + CSRC, SRC, "-o", out],
                       check=True, capture_output=True, timeout=300)
        text = open(out).read()
    bodies = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)
    assert len(bodies) == 1 and "sony_srf_kernel" in bodies[0][0]
    body = bodies[0][1]
    get = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, body).group(1))  # noqa: E731
    assert get("private_segment_fixed_size") == 0
    assert get("next_free_vgpr") <= MAX_VGPRS, get("next_free_vgpr")
    assert 0 < get("group_segment_fixed_size") <= LDS_BYTES
    assert len(re.findall(r"\.vgpr_spill_count:\s+0\b", text)) == 1
    assert len(re.findall(r"\.sgpr_spill_count:\s+0\b", text)) == 1
    assert "global_load_dwordx4" in text and "global_store_dwordx4" in text


def test_core_header_compiles_as_strict_host_cxx():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        open(src, "w").write('#include "rsx_sony_srf_core.h"\n'
                             "int main() { uint32_t t[rsx_sony_srf::TABLE];\n"
                             "  rsx_sony_srf::table_from_key(1u, t, rsx_sony_srf::TABLE);\n"
                             "  const rsx_sony_srf::Poly c = rsx_sony_srf::x_pow(127);\n"
                             "  return rsx_sony_srf::jump_word(c, t, 0) == t[127] ? 0 : 1; }\n")
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + INCLUDE,
                        "-I" + CSRC, src, "-o", os.path.join(d, "t")], check=True,
                       capture_output=True)
        assert subprocess.run([os.path.join(d, "t")]).returncode == 0


def test_check_program_runs():
    from rawspeed_amd import build
    build.build_sony_srf_host()
    r = subprocess.run([build.BIN_SONY_SRF_CHECK], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "ok" and lines[-2] == "decode 0 1"
    assert len(lines) == 16 * 4 + 2 and all(l.endswith(" 1 1") for l in lines[:-2])


def test_the_library_is_built_from_the_sources():
    from rawspeed_amd import build
    assert "rsx_sony_srf.hip" in build.CORE_SOURCES
    assert "rsx_sony_srf.h" in build.CORE_HEADERS and "rsx_sony_srf_core.h" in build.CORE_HEADERS
    for name in build.CORE_SOURCES + build.CORE_HEADERS:
        assert os.path.exists(os.path.join(build.CSRC, name)), name
    assert os.path.exists(os.path.join(build.CSRC, "rsx_sony_srf_host.cpp"))
    assert os.path.basename(build.LIB_SONY_SRF_HOST) == "librsx_sony_srf_host.so"
    assert os.path.basename(build.BIN_SONY_SRF_CHECK) == "rsx_sony_srf_host_check"
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "build_sony_srf_host()" in entry
    ignore = open(os.path.join(ROOT, ".gitignore")).read()
    assert "rawspeed_amd/rsx_sony_srf_host_check" in ignore


def test_symbols_and_layouts():
    from rawspeed_amd import abi, capi
    import sony_srf_files as F
    header = open(os.path.join(INCLUDE, "rsx.h")).read()
    assert "3z. ArwDecoder::SonyDecrypt" in header
    assert "#define RSX_ABI_VERSION 4" in header
    assert sorted(n for n in capi.EXPORTS if n.startswith("rsx_sony_srf") or
                  n == "rsx_sony_decrypt") == sorted(EXPORTS)
    lib = capi.lib()
    for n in EXPORTS:
        assert re.search(r"\b%s\(" % n, header), n
        getattr(lib, n)
    core = open(os.path.join(CSRC, "rsx_sony_srf_core.h")).read()
    assert "constexpr int CHUNK = %d;" % F.CHUNK in core
    fields = ("in_offset", "in_bytes", "img_offset", "key", "reserved", "img")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rsx.h"', "int main(void) {",
             'printf("job %zu\\n", sizeof(rsx_sony_srf_job));']
    for f in fields:
        lines.append('printf("job.%s %%zu\\n", offsetof(rsx_sony_srf_job, %s));' % (f, f))
    lines += ["return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-I" + INCLUDE, src, "-o", exe], check=True)
        got = dict(l.split() for l in subprocess.run([exe], capture_output=True, text=True,
                                                     check=True).stdout.splitlines())
    assert int(got["job"]) == C.sizeof(abi.SonySrfJob)
    for f in fields:
        assert int(got["job." + f]) == getattr(abi.SonySrfJob, f).offset, f
