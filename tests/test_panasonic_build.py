"""The compiled Panasonic kernels (rsx_panasonic.hip): every instantiation of panasonic_kernel
uses no scratch, at most 64 VGPRs (8 waves a SIMD) and at most 20 KiB of LDS (8 workgroups a CU
of 160 KiB; the bound asked for was 4 workgroups, 40 KiB), and carries the name
the plans' kernel tables and the profiles show.  hipcc cross-compiles gfx950; no GPU needed."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INSTANCES = ["ILi5ELi12EE", "ILi5ELi14EE", "ILi6ELi12EE", "ILi6ELi14EE", "ILi7ELi14EE"]


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not found")


def test_panasonic_kernels_have_no_scratch_and_keep_eight_waves_per_simd():
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "pn.s")
        subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S",
                        "--cuda-device-only", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "rawspeed_amd", "csrc"),
                        os.path.join(ROOT, "rawspeed_amd", "csrc", "rsx_panasonic.hip"),
                        "-o", out], check=True, capture_output=True, timeout=300)
        text = open(out).read()
    kernels = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)
    names = [n for n, _ in kernels]
    # one instantiation per layout, each under the stable name
    assert len(kernels) == 5 and all("panasonic_kernel" in n for n in names), names
    for inst in INSTANCES:
        assert [n for n in names if "panasonic_kernel" + inst in n], (inst, names)
    for name, body in kernels:
        get = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, body).group(1))  # noqa: E731
        assert get("private_segment_fixed_size") == 0, name
        assert get("next_free_vgpr") <= 64, (name, get("next_free_vgpr"))
        assert get("group_segment_fixed_size") <= 20 * 1024, (name, get("group_segment_fixed_size"))
    # the image goes out as 16-byte stores
    assert "global_store_dwordx4" in text


def test_the_library_is_built_from_the_panasonic_source():
    from rawspeed_amd import build
    assert "rsx_panasonic.hip" in build.CORE_SOURCES and "rsx_panasonic.h" in build.CORE_HEADERS
