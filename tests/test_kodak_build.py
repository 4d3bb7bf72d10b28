"""The compiled Kodak DCR kernels (rsx_kodak.hip): the map kernels and the decode kernel compile
for gfx950, use no scratch and spill nothing, and stay within what DESIGN.md 4.21 states.  The
library is built from the source, binds the section's symbols, and the struct layouts of
rawspeed_amd/abi.py are include/rsx.h's.  hipcc cross-compiles gfx950; no GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
SRC = os.path.join(ROOT, "rawspeed_amd", "csrc", "rsx_kodak.hip")
EXPORTS = ["rsx_kodak_validate", "rsx_kodak_decompress", "rsx_kodak_plan_create"]
KERNELS = ["kodak_succ_kernel", "kodak_row_map_kernel", "kodak_row_double_kernel",
           "kodak_row_walk_kernel", "kodak_seg_kernel", "kodak_decode_kernel"]
MAX_VGPRS = 32
SUCC_LDS, DECODE_LDS = 4128, 2464  # 1025 + 4 words; four segments of 154 words


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not found")


def test_kernels_have_no_scratch_and_stay_within_their_budgets():
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "kodak.s")
        subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S",
                        "--cuda-device-only", "-I" + INCLUDE,
                        "-I" + os.path.join(ROOT, "rawspeed_amd", "csrc"), SRC, "-o", out],
                       check=True, capture_output=True, timeout=300)
        text = open(out).read()
    bodies = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)
    assert len(bodies) == len(KERNELS)
    get = lambda b, k: int(re.search(r"\.amdhsa_%s (\d+)" % k, b).group(1))  # noqa: E731
    for kernel in KERNELS:
        (body,) = [b for n, b in bodies if kernel in n]
        assert get(body, "private_segment_fixed_size") == 0, kernel
        assert get(body, "next_free_vgpr") <= MAX_VGPRS, (kernel, get(body, "next_free_vgpr"))
        lds = {"kodak_succ_kernel": SUCC_LDS, "kodak_decode_kernel": DECODE_LDS}.get(kernel, 0)
        assert get(body, "group_segment_fixed_size") <= lds, kernel
    assert len(re.findall(r"\.vgpr_spill_count:\s+0\b", text)) == len(KERNELS)
    assert len(re.findall(r"\.sgpr_spill_count:\s+0\b", text)) == len(KERNELS)
    assert "global_store_dwordx2" in text  # (four pixels a lane leave as one store)


def test_design_states_the_budgets():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 4.21"):]
    assert "%d VGPRs" % MAX_VGPRS in sec and "4.0 KB" in sec and "2.4 KB" in sec


def test_the_library_is_built_from_the_kodak_source():
    from rawspeed_amd import build
    assert "rsx_kodak.hip" in build.CORE_SOURCES
    assert "rsx_kodak.h" in build.CORE_HEADERS and "rsx_kodak_core.h" in build.CORE_HEADERS
    for name in build.CORE_SOURCES + build.CORE_HEADERS:
        assert os.path.exists(os.path.join(build.CSRC, name)), name
    assert os.path.exists(os.path.join(build.CSRC, "rsx_kodak_host.cpp"))
    assert os.path.basename(build.LIB_KODAK_HOST) == "librsx_kodak_host.so"
    assert os.path.basename(build.BIN_KODAK_CHECK) == "rsx_kodak_host_check"
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "build_kodak_host()" in entry


def test_symbols_and_layouts():
    from rawspeed_amd import abi, capi, synth
    header = open(os.path.join(INCLUDE, "rsx.h")).read()
    assert "3w. KodakDecompressor" in header
    assert sorted(n for n in capi.EXPORTS if n.startswith("rsx_kodak_")) == sorted(EXPORTS)
    lib = capi.lib()
    for n in EXPORTS:
        assert re.search(r"\b%s\(" % n, header), n
        getattr(lib, n)
    getattr(synth.lib(), "rsx_synth_kodak_encode")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rsx.h"', "int main(void) {",
             'printf("job %zu\\n", sizeof(rsx_kodak_job));',
             'printf("desc %zu\\n", sizeof(rsx_kodak_desc));',
             'printf("modes %d\\n", RSX_KODAK_TABLE_NONE + 10 * RSX_KODAK_TABLE_PLAIN + '
             '100 * RSX_KODAK_TABLE_DITHER);']
    for f in ("desc", "in_offset", "in_bytes", "img_offset", "img"):
        lines.append('printf("job.%s %%zu\\n", offsetof(rsx_kodak_job, %s));' % (f, f))
    for f in ("bps", "table_mode", "table"):
        lines.append('printf("desc.%s %%zu\\n", offsetof(rsx_kodak_desc, %s));' % (f, f))
    lines += ["return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-I" + INCLUDE, src, "-o", exe], check=True)
        got = dict(l.split() for l in subprocess.run([exe], capture_output=True, text=True,
                                                     check=True).stdout.splitlines())
    assert int(got["job"]) == C.sizeof(abi.KodakJob)
    assert int(got["desc"]) == C.sizeof(abi.KodakDesc)
    assert int(got["modes"]) == (abi.RSX_KODAK_TABLE_NONE + 10 * abi.RSX_KODAK_TABLE_PLAIN +
                                 100 * abi.RSX_KODAK_TABLE_DITHER)
    for f in ("desc", "in_offset", "in_bytes", "img_offset", "img"):
        assert int(got["job." + f]) == getattr(abi.KodakJob, f).offset, f
    for f in ("bps", "table_mode", "table"):
        assert int(got["desc." + f]) == getattr(abi.KodakDesc, f).offset, f
