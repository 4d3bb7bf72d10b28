"""The compiled compressed-RAF kernel (rsx_fuji.hip): fuji_strip_kernel compiles for gfx950, uses
no scratch, and stays within what DESIGN.md 4.19 states: 192 VGPRs (two waves a SIMD, which the
five workgroups a CU of its LDS need) and 28.7 KB of LDS.  The library is built from the source,
binds the section's symbols, and the struct layouts of rawspeed_amd/abi.py are include/rsx.h's.
hipcc cross-compiles gfx950; no GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
SRC = os.path.join(ROOT, "rawspeed_amd", "csrc", "rsx_fuji.hip")
EXPORTS = ["rsx_fuji_parse", "rsx_fuji_validate", "rsx_fuji_decompress", "rsx_fuji_plan_create",
           "rsx_fuji_plan_strip_status"]
VGPRS, LDS_BYTES = 192, 28 * 1024 + 768


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not found")


def test_kernel_has_no_scratch_and_stays_within_its_budget():
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "fuji.s")
        subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S",
                        "--cuda-device-only", "-I" + INCLUDE,
                        "-I" + os.path.join(ROOT, "rawspeed_amd", "csrc"), SRC, "-o", out],
                       check=True, capture_output=True, timeout=300)
        text = open(out).read()
    kernels = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)
    (name, body), = kernels
    assert "fuji_strip_kernel" in name
    get = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, body).group(1))  # noqa: E731
    assert get("private_segment_fixed_size") == 0
    assert get("next_free_vgpr") <= VGPRS, get("next_free_vgpr")
    assert get("group_segment_fixed_size") <= LDS_BYTES, get("group_segment_fixed_size")
    assert 160 * 1024 // get("group_segment_fixed_size") == 5  # (strips a CU)
    assert "global_store_dwordx4" in text  # (the image rows go as 16-byte stores)
    assert re.search(r"\.vgpr_spill_count:\s+0\b", text)


def test_design_states_the_budget():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 4.19"):]
    assert "%d VGPRs" % VGPRS in sec and "28.7 KB" in sec


def test_the_library_is_built_from_the_fuji_source():
    from rawspeed_amd import build
    assert "rsx_fuji.hip" in build.CORE_SOURCES
    assert "rsx_fuji.h" in build.CORE_HEADERS and "rsx_fuji_core.h" in build.CORE_HEADERS
    for name in build.CORE_SOURCES + build.CORE_HEADERS:
        assert os.path.exists(os.path.join(build.CSRC, name)), name
    assert os.path.exists(os.path.join(build.CSRC, "rsx_fuji_host.cpp"))


def test_symbols_and_layouts():
    from rawspeed_amd import abi, capi
    header = open(os.path.join(INCLUDE, "rsx.h")).read()
    assert sorted(n for n in capi.EXPORTS if n.startswith("rsx_fuji_")) == sorted(EXPORTS)
    lib = capi.lib()
    for n in EXPORTS:
        assert re.search(r"\b%s\(" % n, header), n
        getattr(lib, n)
    types = {"rsx_fuji_desc": abi.FujiDesc, "rsx_fuji_job": abi.FujiJob}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rsx.h"', "int main(void) {"]
    for c_name in types:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (c_name, c_name))
    lines.append('printf("strip_offset %zu\\n", offsetof(rsx_fuji_desc, strip_offset));')
    lines.append('printf("img %zu\\n", offsetof(rsx_fuji_job, img));')
    lines += ["return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-I" + INCLUDE, src, "-o", exe], check=True)
        got = dict(l.split() for l in subprocess.run([exe], capture_output=True, text=True,
                                                     check=True).stdout.splitlines())
    for c_name, t in types.items():
        assert int(got[c_name]) == C.sizeof(t), c_name
    assert int(got["strip_offset"]) == abi.FujiDesc.strip_offset.offset
    assert int(got["img"]) == abi.FujiJob.img.offset
    assert abi.FUJI_MAX_STRIPS == int(re.search(r"#define RSX_FUJI_MAX_STRIPS (\d+)", header).group(1))
