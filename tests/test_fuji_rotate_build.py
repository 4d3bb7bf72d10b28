"""The compiled SuperCCD rotation kernels (rsx_fuji_rotate.hip): both compile for gfx950, use no
scratch and spill nothing; the core header compiles as host C++ with -Wall -Wextra -Werror; the
check program runs; the library is built from the sources, binds the section's symbols, and the
struct layouts of rawspeed_amd/abi.py are include/rsx.h's.  hipcc cross-compiles gfx950; no GPU
needed."""
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
SRC = os.path.join(CSRC, "rsx_fuji_rotate.hip")
EXPORTS = ["rsx_raf_rotate_geometry", "rsx_raf_rotate_validate", "rsx_raf_rotate",
           "rsx_raf_rotate_plan_create"]
KERNELS = ["fuji_rotate_kernel", "fuji_rotate_lds_kernel"]
MAX_VGPRS = 64
LDS_BYTES = 96 * 50 * 2  # the bounding box of a tile's diamond


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not found")


def test_kernels_have_no_scratch_and_store_16_bytes():
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "fr.s")
        subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S",
                        "--cuda-device-only", "-I" + INCLUDE, "-I" + CSRC, SRC, "-o", out],
                       check=True, capture_output=True, timeout=300)
        text = open(out).read()
    bodies = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)
    assert len(bodies) == len(KERNELS)
    get = lambda b, k: int(re.search(r"\.amdhsa_%s (\d+)" % k, b).group(1))  # noqa: E731
    for kernel in KERNELS:
        (body,) = [b for n, b in bodies if kernel + "E" in n]
        assert get(body, "private_segment_fixed_size") == 0, kernel
        assert get(body, "next_free_vgpr") <= MAX_VGPRS, (kernel, get(body, "next_free_vgpr"))
        lds = LDS_BYTES if "lds" in kernel else 0
        assert get(body, "group_segment_fixed_size") == lds, kernel
    assert len(re.findall(r"\.vgpr_spill_count:\s+0\b", text)) == len(KERNELS)
    assert len(re.findall(r"\.sgpr_spill_count:\s+0\b", text)) == len(KERNELS)
    assert "global_store_dwordx4" in text  # (eight samples of a row leave as one store)


def test_core_header_compiles_as_strict_host_cxx():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        open(src, "w").write('#include "rsx_fuji_rotate_core.h"\n'
                             "int main() { rsx_raf_rotate_desc d{0, 0, 2, 2, 0, 0}; int32_t a, b, c;\n"
                             "  return rsx_fujirot::geometry(&d, &a, &b, &c); }\n")
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + INCLUDE,
                        "-I" + CSRC, src, "-o", os.path.join(d, "t")], check=True,
                       capture_output=True)
        assert subprocess.run([os.path.join(d, "t")]).returncode == 0


def test_check_program_runs():
    from rawspeed_amd import build
    build.build_fuji_rotate_host()
    r = subprocess.run([build.BIN_FUJI_ROTATE_CHECK], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    assert lines[0] == "ran 576 refused 576" and lines[1] == "ok"


def test_the_library_is_built_from_the_sources():
    from rawspeed_amd import build
    assert "rsx_fuji_rotate.hip" in build.CORE_SOURCES
    assert "rsx_fuji_rotate.h" in build.CORE_HEADERS
    assert "rsx_fuji_rotate_core.h" in build.CORE_HEADERS
    for name in build.CORE_SOURCES + build.CORE_HEADERS:
        assert os.path.exists(os.path.join(build.CSRC, name)), name
    assert os.path.exists(os.path.join(build.CSRC, "rsx_fuji_rotate_host.cpp"))
    assert os.path.basename(build.LIB_FUJI_ROTATE_HOST) == "librsx_fuji_rotate_host.so"
    assert os.path.basename(build.BIN_FUJI_ROTATE_CHECK) == "rsx_fuji_rotate_host_check"
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "build_fuji_rotate_host()" in entry
    ignore = open(os.path.join(ROOT, ".gitignore")).read()
    assert "rawspeed_amd/rsx_fuji_rotate_host_check" in ignore


def test_symbols_and_layouts():
    from rawspeed_amd import abi, capi
    header = open(os.path.join(INCLUDE, "rsx.h")).read()
    assert "3y. RafDecoder::applyCorrections" in header
    assert "#define RSX_ABI_VERSION 4" in header
    assert sorted(n for n in capi.EXPORTS if n.startswith("rsx_raf_rotate")) == sorted(EXPORTS)
    lib = capi.lib()
    for n in EXPORTS:
        assert re.search(r"\b%s\(" % n, header), n
        getattr(lib, n)
    job_f = ("desc", "in_offset", "img_offset", "in", "img")
    desc_f = ("crop_x", "crop_y", "size_x", "size_y", "alt_layout", "reserved")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rsx.h"', "int main(void) {",
             'printf("job %zu\\n", sizeof(rsx_raf_rotate_job));',
             'printf("desc %zu\\n", sizeof(rsx_raf_rotate_desc));']
    for f in job_f:
        lines.append('printf("job.%s %%zu\\n", offsetof(rsx_raf_rotate_job, %s));' % (f, f))
    for f in desc_f:
        lines.append('printf("desc.%s %%zu\\n", offsetof(rsx_raf_rotate_desc, %s));' % (f, f))
    lines += ["return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-I" + INCLUDE, src, "-o", exe], check=True)
        got = dict(l.split() for l in subprocess.run([exe], capture_output=True, text=True,
                                                     check=True).stdout.splitlines())
    assert int(got["job"]) == C.sizeof(abi.FujiRotateJob)
    assert int(got["desc"]) == C.sizeof(abi.FujiRotateDesc)
    for f in job_f:
        assert int(got["job." + f]) == getattr(abi.FujiRotateJob, "in_" if f == "in" else f).offset
    for f in desc_f:
        assert int(got["desc." + f]) == getattr(abi.FujiRotateDesc, f).offset, f
