"""The compiled compressed-ORF kernels (rsx_olympus.hip): olympus_parse_kernel and
olympus_recon_kernel compile for gfx950, use no scratch and spill nothing, and stay within what
DESIGN.md 4.20 states: 32 VGPRs and no LDS for the walk, 192 VGPRs and 26.2 KB of LDS for the
reconstruction.  The library is built from the source, binds the section's symbols, and the struct
layout of rawspeed_amd/abi.py is include/rsx.h's.  hipcc cross-compiles gfx950; no GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
SRC = os.path.join(ROOT, "rawspeed_amd", "csrc", "rsx_olympus.hip")
EXPORTS = ["rsx_olympus_validate", "rsx_olympus_decompress", "rsx_olympus_plan_create",
           "rsx_olympus_plan_job_status"]
PARSE_VGPRS, PARSE_LDS = 32, 0
RECON_VGPRS, RECON_LDS = 192, 26784


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not found")


def test_kernels_have_no_scratch_and_stay_within_their_budgets():
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "olympus.s")
        subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S",
                        "--cuda-device-only", "-I" + INCLUDE,
                        "-I" + os.path.join(ROOT, "rawspeed_amd", "csrc"), SRC, "-o", out],
                       check=True, capture_output=True, timeout=300)
        text = open(out).read()
    kernels = dict((("parse" if "parse" in n else "recon"), b) for n, b in
                   re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S))
    names = re.findall(r"\.amdhsa_kernel (\S+)", text)
    assert len(names) == 2
    assert any("olympus_parse_kernel" in n for n in names)
    assert any("olympus_recon_kernel" in n for n in names)
    get = lambda b, k: int(re.search(r"\.amdhsa_%s (\d+)" % k, b).group(1))  # noqa: E731
    for key, vgprs, lds in (("parse", PARSE_VGPRS, PARSE_LDS), ("recon", RECON_VGPRS, RECON_LDS)):
        body = kernels[key]
        assert get(body, "private_segment_fixed_size") == 0, key
        assert get(body, "next_free_vgpr") <= vgprs, (key, get(body, "next_free_vgpr"))
        assert get(body, "group_segment_fixed_size") <= lds, (key, get(body, "group_segment_fixed_size"))
    assert len(re.findall(r"\.vgpr_spill_count:\s+0\b", text)) == 2
    assert len(re.findall(r"\.sgpr_spill_count:\s+0\b", text)) == 2
    assert "v_readlane_b32" in text     # (the window's words come out of the lanes' registers)
    assert "wave_shr:1" in text         # (U: the lane above's value, one shift a step)


def test_design_states_the_budgets():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 4.20"):]
    assert "%d VGPRs" % PARSE_VGPRS in sec and "%d VGPRs" % RECON_VGPRS in sec and "26.2 KB" in sec


def test_the_library_is_built_from_the_olympus_source():
    from rawspeed_amd import build
    assert "rsx_olympus.hip" in build.CORE_SOURCES
    assert "rsx_olympus.h" in build.CORE_HEADERS and "rsx_olympus_core.h" in build.CORE_HEADERS
    for name in build.CORE_SOURCES + build.CORE_HEADERS:
        assert os.path.exists(os.path.join(build.CSRC, name)), name
    assert os.path.exists(os.path.join(build.CSRC, "rsx_olympus_host.cpp"))
    assert os.path.basename(build.LIB_OLYMPUS_HOST) == "librsx_olympus_host.so"
    assert os.path.basename(build.BIN_OLYMPUS_CHECK) == "rsx_olympus_host_check"


def test_symbols_and_layouts():
    from rawspeed_amd import abi, capi, synth
    header = open(os.path.join(INCLUDE, "rsx.h")).read()
    assert sorted(n for n in capi.EXPORTS if n.startswith("rsx_olympus_")) == sorted(EXPORTS)
    lib = capi.lib()
    for n in EXPORTS:
        assert re.search(r"\b%s\(" % n, header), n
        getattr(lib, n)
    for n in ("rsx_synth_olympus_encode", "rsx_synth_olympus_plant"):
        getattr(synth.lib(), n)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rsx.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(rsx_olympus_job));']
    for f in ("in_offset", "in_bytes", "img_offset", "img"):
        lines.append('printf("%s %%zu\\n", offsetof(rsx_olympus_job, %s));' % (f, f))
    lines += ["return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-I" + INCLUDE, src, "-o", exe], check=True)
        got = dict(l.split() for l in subprocess.run([exe], capture_output=True, text=True,
                                                     check=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(abi.OlympusJob)
    for f in ("in_offset", "in_bytes", "img_offset", "img"):
        assert int(got[f]) == getattr(abi.OlympusJob, f).offset, f
