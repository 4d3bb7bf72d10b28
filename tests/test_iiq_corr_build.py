"""The compiled IIQ correction kernels (rsx_iiq_corr.hip): no scratch, no LDS, the fused pass within
64 VGPRs (8 waves a SIMD) with a 16-byte load and a 16-byte store, the row and column walks within 32; every
memory access global.  hipcc cross-compiles gfx950; no GPU needed."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from rawspeed_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rawspeed_amd", "csrc")
KERNELS = ("iiq_ff_rows_kernel", "iiq_ff_cols_kernel", "iiq_correct_kernel")


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not found")


@pytest.fixture(scope="module")
def kernels():
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "iiq_corr.s")
        subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S",
                        "--cuda-device-only", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                        os.path.join(CSRC, "rsx_iiq_corr.hip"), "-o", out],
                       check=True, capture_output=True, timeout=300)
        asm = open(out).read()
    found = {}
    for name, body in re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, re.S):
        code = re.search(r"^%s:(.*?)s_endpgm" % re.escape(name), asm, re.S | re.M).group(1)
        get = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, body).group(1))  # noqa: E731
        found[name] = dict(scratch=get("private_segment_fixed_size"), vgpr=get("next_free_vgpr"),
                           lds=get("group_segment_fixed_size"), code=code)
    return asm, found


def _one(found, part):
    hits = [v for k, v in found.items() if part in k]
    assert len(hits) == 1, (part, list(found))
    return hits[0]


def test_the_kernels_are_there_without_scratch_or_lds(kernels):
    asm, found = kernels
    for part in KERNELS:
        k = _one(found, part)
        assert k["scratch"] == 0 and k["lds"] == 0, part
        assert k["vgpr"] <= (64 if part == "iiq_correct_kernel" else 32), (part, k["vgpr"])
    assert not re.search(r"\bscratch_", asm)


def test_fused_pass_moves_16_bytes_and_memory_accesses_stay_global(kernels):
    asm, found = kernels
    code = _one(found, "iiq_correct_kernel")["code"]
    assert "global_load_dwordx4" in code and "global_store_dwordx4" in code
    assert "global_store_short" in code  # the halves path
    assert not re.search(r"\bflat_(load|store)", asm)


def test_sources_are_part_of_the_core_library():
    assert "rsx_iiq_corr.hip" in build.CORE_SOURCES
    assert "rsx_iiq_corr.h" in build.CORE_HEADERS and "rsx_iiq_corr_core.h" in build.CORE_HEADERS
    for name in ("rsx_iiq_corr.hip", "rsx_iiq_corr.h", "rsx_iiq_corr_core.h", "rsx_iiq_corr_host.cpp"):
        assert os.path.exists(os.path.join(CSRC, name))
