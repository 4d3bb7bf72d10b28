"""The compiled bad-column kernel (rsx_iiq_defects.hip): in the library, no scratch, no LDS, within
32 VGPRs, 2-byte gathers and one 2-byte store, every memory access global.  hipcc cross-compiles
gfx950; no GPU needed."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from rawspeed_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rawspeed_amd", "csrc")
KERNEL = "iiq_bad_columns_kernel"


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not found")


@pytest.fixture(scope="module")
def kernels():
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "iiq_defects.s")
        subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S",
                        "--cuda-device-only", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                        os.path.join(CSRC, "rsx_iiq_defects.hip"), "-o", out],
                       check=True, capture_output=True, timeout=300)
        asm = open(out).read()
    found = {}
    for name, body in re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, re.S):
        code = re.search(r"^%s:(.*?)s_endpgm" % re.escape(name), asm, re.S | re.M).group(1)
        get = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, body).group(1))  # noqa: E731
        found[name] = dict(scratch=get("private_segment_fixed_size"), vgpr=get("next_free_vgpr"),
                           lds=get("group_segment_fixed_size"), code=code)
    return asm, found


def test_one_kernel_without_scratch_or_lds(kernels):
    asm, found = kernels
    assert len(found) == 1 and KERNEL in list(found)[0], list(found)
    k = list(found.values())[0]
    assert k["scratch"] == 0 and k["lds"] == 0 and k["vgpr"] <= 32, k["vgpr"]
    assert not re.search(r"\bscratch_", asm)
    # (tests/test_iiq_corr_build.py counts the kernels of rsx_iiq_corr.hip by these names)
    for other in ("iiq_correct_kernel", "iiq_ff_rows_kernel", "iiq_ff_cols_kernel"):
        assert other not in list(found)[0]


def test_two_byte_gathers_one_two_byte_store_all_global(kernels):
    asm, found = kernels
    code = list(found.values())[0]["code"]
    assert "global_load_ushort" in code or "global_load_short" in code
    assert len(re.findall(r"\bglobal_store_short\b", code)) >= 1
    assert not re.search(r"\bglobal_store_(dword|byte)", code)
    assert not re.search(r"\bflat_(load|store)", asm)
    assert not re.search(r"\bds_(read|write|load|store)", code)


def test_source_is_part_of_the_core_library():
    assert "rsx_iiq_defects.hip" in build.CORE_SOURCES
    assert os.path.exists(os.path.join(CSRC, "rsx_iiq_defects.hip"))
    lib = build.build_core()
    with open(lib, "rb") as f:
        assert KERNEL.encode() in f.read()
