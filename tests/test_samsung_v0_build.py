"""The compiled SamsungV0 kernels (rsx_samsung_v0.hip): sv0_parse_kernel and sv0_recon_kernel
compile for gfx950, use no scratch and no static LDS (their LDS is what the launch asks for:
the row's words and the per-block records, resp. three pre-swap rows), and stay within the
registers DESIGN.md 4.9 states: 64 VGPRs for the parse (8 waves a SIMD) and 160 for the
reconstruction (its one workgroup a frame is 6 waves, two on a SIMD at the most).  The launches' LDS follows from the widest
row, 347 blocks, for the parse: 17.4 KB; the reconstruction takes 36 KB.  hipcc cross-compiles gfx950; no GPU needed."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "rawspeed_amd", "csrc", "rsx_samsung_v0.hip")
VGPR = {"sv0_parse_kernel": 64, "sv0_recon_kernel": 160}


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not found")


def test_samsung_v0_kernels_have_no_scratch_and_stay_within_their_registers():
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "sv0.s")
        subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S",
                        "--cuda-device-only", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "rawspeed_amd", "csrc"), SRC, "-o", out],
                       check=True, capture_output=True, timeout=300)
        text = open(out).read()
    kernels = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)
    names = [n for n, _ in kernels]
    assert len(kernels) == 2, names
    for want, vgprs in VGPR.items():
        (name, body), = [(n, b) for n, b in kernels if want in n]
        get = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, body).group(1))  # noqa: E731
        assert get("private_segment_fixed_size") == 0, name
        assert get("group_segment_fixed_size") == 0, name
        assert get("next_free_vgpr") <= vgprs, (name, get("next_free_vgpr"))
    # local values and the image go as 16-byte accesses
    assert "global_store_dwordx4" in text and "global_load_dwordx4" in text


def test_launch_lds_of_the_widest_row():
    """the constants the launches size their LDS with, read from the source"""
    src = open(SRC).read()
    threads = int(re.search(r"SV0_THREADS = (\d+);", src).group(1))
    assert threads == 384 >= (5546 + 15) // 16
    assert int(re.search(r"SV0_PARSE_THREADS = (\d+);", src).group(1)) * 2 == threads
    assert "SV0_LDS_LUT = 2 * SV0_THREADS + 16;" in src and "SV0_LDS_HEAD = SV0_LDS_LUT + 512;" in src
    assert "SV0_BLOCK_BITS = 281;" in src
    nblk = (5546 + 15) // 16
    parse = (2 * threads + 16 + 512 + nblk * 281 // 32 + 3) * 4
    recon = 3 * 8 * threads * 4
    assert parse <= 17.5 * 1024 and recon == 36 * 1024


def test_the_library_is_built_from_the_samsung_v0_source():
    from rawspeed_amd import build
    assert "rsx_samsung_v0.hip" in build.CORE_SOURCES and "rsx_samsung_v0.h" in build.CORE_HEADERS
