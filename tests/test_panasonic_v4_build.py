"""The compiled Panasonic V4 kernel (rsx_panasonic_v4.hip): no scratch (pred and nonz per column
parity are scalars, every field is cut from the packet's four dwords by shifts), at most 64 VGPRs
(8 waves a SIMD) and at most 20 KiB of LDS (8 workgroups a CU), 16-byte stores,
and the name the plans' kernel tables and the profiles show.  hipcc cross-compiles gfx950; no GPU
needed."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "rawspeed_amd", "csrc", "rsx_panasonic_v4.hip")


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not found")


def test_panasonic_v4_kernel_has_no_scratch_and_keeps_eight_waves_per_simd():
    assert os.path.exists(SOURCE)
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "p4.s")
        subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S",
                        "--cuda-device-only", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "rawspeed_amd", "csrc"), SOURCE, "-o", out],
                       check=True, capture_output=True, timeout=300)
        text = open(out).read()
    kernels = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)
    names = [n for n, _ in kernels]
    assert len(kernels) == 1 and "panasonic_v4_kernel" in names[0], names
    for name, body in kernels:
        get = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, body).group(1))  # noqa: E731
        assert get("private_segment_fixed_size") == 0, name
        assert get("next_free_vgpr") <= 64, (name, get("next_free_vgpr"))
        assert get("group_segment_fixed_size") <= 20 * 1024, (name, get("group_segment_fixed_size"))
    # the packets come in as 16-byte loads, the image goes out as 16-byte stores, and a
    # workgroup takes its slice of the list with one atomic add
    assert "global_load_dwordx4" in text and "global_store_dwordx4" in text
    assert len(re.findall(r"\bglobal_atomic_add\w*", text)) == 1


def test_the_library_is_built_from_the_panasonic_v4_source():
    from rawspeed_amd import build
    assert "rsx_panasonic_v4.hip" in build.CORE_SOURCES
    assert "rsx_panasonic_v4.h" in build.CORE_HEADERS and "rsx_panasonic_dev.h" in build.CORE_HEADERS
    for name in build.CORE_SOURCES + build.CORE_HEADERS:
        assert os.path.exists(os.path.join(build.CSRC, name)), name
