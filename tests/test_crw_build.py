"""The compiled Canon CRW kernels (rsx_crw.hip): they compile for gfx950, use no scratch and spill
nothing, and stay within what DESIGN.md 4.22 states.  The library is built from the source, binds
the section's symbols, the shipped segment and window sizes are the ones the case list was cut
for, and the struct layouts of rawspeed_amd/abi.py are include/rsx.h's.  hipcc cross-compiles
gfx950; no GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import crw_files as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
SRC = os.path.join(ROOT, "rawspeed_amd", "csrc", "rsx_crw.hip")
EXPORTS = ["rsx_crw_validate", "rsx_crw_decompress", "rsx_crw_plan_create", "rsx_crw_plan_stats"]
KERNELS = ["crw_zero_kernel", "crw_count_kernel", "crw_compact_kernel", "crw_parse_kernel",
           "crw_settle_kernel", "crw_scan_kernel", "crw_write_kernel", "crw_carry_kernel",
           "crw_recon_kernel"]
MAX_VGPRS = 64
# DESIGN 4.22's 34.7 KB: a window of 256 rows of 33 words (33 792 bytes), the tables (532), the
# entries (514) and the flags (257), each aligned
WINDOW_LDS = int(34.7 * 1024)
OTHER_LDS = 1024


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not found")


def test_kernels_have_no_scratch_and_stay_within_their_budgets():
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "crw.s")
        subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S",
                        "--cuda-device-only", "-I" + INCLUDE,
                        "-I" + os.path.join(ROOT, "rawspeed_amd", "csrc"), SRC, "-o", out],
                       check=True, capture_output=True, timeout=300)
        text = open(out).read()
    bodies = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)
    assert len(bodies) == len(KERNELS)
    counts = dict(re.findall(r"\.symbol:\s+(\S+)\.kd\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text))
    get = lambda b, k: int(re.search(r"\.amdhsa_%s (\d+)" % k, b).group(1))  # noqa: E731
    for kernel in KERNELS:
        (name, body), = [(n, b) for n, b in bodies if kernel in n]
        assert get(body, "private_segment_fixed_size") == 0, kernel
        assert int(counts[name]) <= MAX_VGPRS, (kernel, counts[name])
        windowed = kernel in ("crw_parse_kernel", "crw_settle_kernel", "crw_write_kernel")
        assert get(body, "group_segment_fixed_size") <= (WINDOW_LDS if windowed else OTHER_LDS), kernel
    assert len(re.findall(r"\.vgpr_spill_count:\s+0\b", text)) == len(KERNELS)
    assert len(re.findall(r"\.sgpr_spill_count:\s+0\b", text)) == len(KERNELS)
    assert "global_store_dwordx4" in text  # (eight pixels leave as one store where the row allows)


def test_design_states_the_budgets_and_the_macros_are_the_case_list_s():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 4.22"):]
    assert "%d VGPRs" % MAX_VGPRS in sec and "34.7 KB" in sec
    src = open(SRC).read()
    assert int(re.search(r"#define RSX_CRW_SEG_BITS (\d+)", src).group(1)) == F.SEG_BITS
    assert int(re.search(r"#define RSX_CRW_WIN_SEGS (\d+)", src).group(1)) == F.WIN_SEGS
    assert WINDOW_LDS <= 34.7 * 1024


def test_the_library_is_built_from_the_crw_source():
    from rawspeed_amd import build
    assert "rsx_crw.hip" in build.CORE_SOURCES
    assert "rsx_crw.h" in build.CORE_HEADERS and "rsx_crw_core.h" in build.CORE_HEADERS
    for name in build.CORE_SOURCES + build.CORE_HEADERS:
        assert os.path.exists(os.path.join(build.CSRC, name)), name
    assert os.path.exists(os.path.join(build.CSRC, "rsx_crw_host.cpp"))
    assert os.path.basename(build.LIB_CRW_HOST) == "librsx_crw_host.so"
    assert os.path.basename(build.BIN_CRW_CHECK) == "rsx_crw_host_check"
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "build_crw_host()" in entry


def test_symbols_and_layouts():
    from rawspeed_amd import abi, capi, synth
    header = open(os.path.join(INCLUDE, "rsx.h")).read()
    assert "3x. CrwDecompressor" in header
    assert sorted(n for n in capi.EXPORTS if n.startswith("rsx_crw_")) == sorted(EXPORTS)
    lib = capi.lib()
    for n in EXPORTS:
        assert re.search(r"\b%s\(" % n, header), n
        getattr(lib, n)
    getattr(synth.lib(), "rsx_synth_crw_encode")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rsx.h"', "int main(void) {",
             'printf("job %zu\\n", sizeof(rsx_crw_job));',
             'printf("desc %zu\\n", sizeof(rsx_crw_desc));']
    job_fields = ("desc", "in_offset", "in_bytes", "low_offset", "low_bytes", "img_offset", "img")
    for f in job_fields:
        lines.append('printf("job.%s %%zu\\n", offsetof(rsx_crw_job, %s));' % (f, f))
    for f in ("dec_table", "has_lowbits"):
        lines.append('printf("desc.%s %%zu\\n", offsetof(rsx_crw_desc, %s));' % (f, f))
    lines += ["return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-I" + INCLUDE, src, "-o", exe], check=True)
        got = dict(l.split() for l in subprocess.run([exe], capture_output=True, text=True,
                                                     check=True).stdout.splitlines())
    assert int(got["job"]) == C.sizeof(abi.CrwJob)
    assert int(got["desc"]) == C.sizeof(abi.CrwDesc)
    for f in job_fields:
        assert int(got["job." + f]) == getattr(abi.CrwJob, f).offset, f
    for f in ("dec_table", "has_lowbits"):
        assert int(got["desc." + f]) == getattr(abi.CrwDesc, f).offset, f


def test_the_c_writer_is_the_case_list_s_encoder():
    from rawspeed_amd import synth
    for table in range(3):
        px = F.noise_image(256, 16, 90 + table, 20.0)
        assert synth.crw_encode(px, table) == F.encode_image(px, table)
