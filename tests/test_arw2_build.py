"""The compiled SonyArw2Decompressor kernel (rsx_sony_arw2.hip): no scratch, and registers and
LDS that allow the occupancy DESIGN.md 4.7 claims -- 8 waves a SIMD (two 256-lane workgroups
a SIMD's worth: at most 64 VGPRs) and 8 workgroups a CU in LDS (at most 20 KiB each).
hipcc cross-compiles gfx950; no GPU needed."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not found")


def test_arw2_kernel_has_no_scratch_and_keeps_eight_waves_per_simd():
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "a2.s")
        subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S",
                        "--cuda-device-only", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "rawspeed_amd", "csrc"),
                        os.path.join(ROOT, "rawspeed_amd", "csrc", "rsx_sony_arw2.hip"),
                        "-o", out], check=True, capture_output=True, timeout=300)
        text = open(out).read()
    kernels = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)
    assert [n for n, _ in kernels if "arw2_kernel" in n], [n for n, _ in kernels]
    for name, body in kernels:
        get = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, body).group(1))  # noqa: E731
        assert get("private_segment_fixed_size") == 0, name
        assert get("next_free_vgpr") <= 64, (name, get("next_free_vgpr"))
        assert get("group_segment_fixed_size") <= 20 * 1024, (name, get("group_segment_fixed_size"))
    # the lanes of a block pair swap their halves through DPP, not through LDS
    assert "ds_bpermute" not in text
