"""The compiled VC-5 kernels (rsx_vc5.hip): no scratch, and the register and LDS budget DESIGN.md
4.13 states -- the band kernel within 128 VGPRs (its 16 waves are four a SIMD) and, for its table,
window and exits, 44 KiB of LDS, the other kernels within 64 VGPRs (8 waves a SIMD), the merge
kernel's log table 8 KiB -- and 16-byte stores in the merge kernel.  hipcc cross-compiles gfx950; no GPU needed."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from rawspeed_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rawspeed_amd", "csrc")
KERNELS = ("vc5_lowpass_kernel", "vc5_band_kernel", "vc5_level_kernel", "vc5_merge_kernel")


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not found")


@pytest.fixture(scope="module")
def kernels():
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "vc5.s")
        subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S",
                        "--cuda-device-only", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                        os.path.join(CSRC, "rsx_vc5.hip"), "-o", out],
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


def test_all_four_kernels_are_there_without_scratch(kernels):
    asm, found = kernels
    for part in KERNELS:
        k = _one(found, part)
        assert k["scratch"] == 0, part
        assert k["vgpr"] <= (128 if part == "vc5_band_kernel" else 64), (part, k["vgpr"])
    assert not re.search(r"\bscratch_", asm)


def test_lds_budgets(kernels):
    _, found = kernels
    assert 40 * 1024 <= _one(found, "vc5_band_kernel")["lds"] <= 44 * 1024
    assert _one(found, "vc5_merge_kernel")["lds"] == 8192
    assert _one(found, "vc5_level_kernel")["lds"] == 0 and _one(found, "vc5_lowpass_kernel")["lds"] == 0


def test_merge_stores_16_bytes_and_memory_accesses_stay_global(kernels):
    asm, found = kernels
    assert "global_store_dwordx4" in _one(found, "vc5_merge_kernel")["code"]
    assert "global_store_dwordx4" in _one(found, "vc5_band_kernel")["code"]  # the zeroing
    assert not re.search(r"\bflat_(load|store)", asm)


def test_sources_are_part_of_the_core_library():
    assert "rsx_vc5.hip" in build.CORE_SOURCES
    assert "rsx_vc5.h" in build.CORE_HEADERS and "rsx_vc5_core.h" in build.CORE_HEADERS
    for name in ("rsx_vc5.hip", "rsx_vc5.h", "rsx_vc5_core.h", "rsx_vc5_host.cpp"):
        assert os.path.exists(os.path.join(CSRC, name))
