"""The compiled sNEF kernel (rsx_nikon_snef.hip): no scratch, the register and LDS budget DESIGN.md
4.12 states -- at most 64 VGPRs (8 waves a SIMD) and the 16 KiB table in LDS (8 workgroups a CU)
-- 16-byte stores, and colour arithmetic in separate binary64 multiplications and additions: a
fused multiply-add changes the green expression for 34 chroma pairs (tests/test_snef_model.py).
hipcc cross-compiles gfx950; no GPU needed."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from rawspeed_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rawspeed_amd", "csrc")


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not found")


@pytest.fixture(scope="module")
def asm():
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "snef.s")
        subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S",
                        "--cuda-device-only", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                        os.path.join(CSRC, "rsx_nikon_snef.hip"), "-o", out],
                       check=True, capture_output=True, timeout=300)
        return open(out).read()


def test_kernel_has_no_scratch_and_keeps_eight_waves_per_simd(asm):
    kernels = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, re.S)
    assert [n for n, _ in kernels if "nikon_snef_kernel" in n], [n for n, _ in kernels]
    for name, body in kernels:
        get = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, body).group(1))  # noqa: E731
        assert get("private_segment_fixed_size") == 0, name
        assert get("next_free_vgpr") <= 64, (name, get("next_free_vgpr"))
        assert get("group_segment_fixed_size") <= 20 * 1024, (name, get("group_segment_fixed_size"))
    assert not re.search(r"\bscratch_", asm)


def test_stores_are_16_bytes_wide_and_loads_stay_global(asm):
    assert "global_store_dwordx4" in asm
    assert "global_load_dwordx4" in asm
    assert not re.search(r"\bflat_(load|store)", asm)


def test_colour_expressions_are_not_contracted(asm):
    assert "v_mul_f64" in asm and "v_add_f64" in asm
    assert "v_fma_f64" not in asm and "v_fmac_f64" not in asm


def test_sources_are_part_of_the_core_library():
    assert "rsx_nikon_snef.hip" in build.CORE_SOURCES
    assert "rsx_nikon_snef.h" in build.CORE_HEADERS and "rsx_dither_dev.h" in build.CORE_HEADERS
    for name in ("rsx_nikon_snef.hip", "rsx_nikon_snef.h", "rsx_dither_dev.h"):
        assert os.path.exists(os.path.join(CSRC, name))
