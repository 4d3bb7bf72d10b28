"""The compiled deflate DNG kernels (rsx_dng_deflate.hip): dfl_inflate_kernel and dfl_row_kernel
compile for gfx950 and use no scratch.  The inflate's LDS is the decoder's state, 40 KB a wave --
the 32 KiB window, the tables, the code lengths -- so that four waves share the 160 KiB of a CU
(DESIGN.md 4.11); with one wave a SIMD its registers (DESIGN: below 128 vector registers) do not
bound the occupancy.  The row kernel takes no LDS and at most 64 registers.  hipcc cross-compiles
gfx950; no GPU needed."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rawspeed_amd", "csrc")
SRC = os.path.join(CSRC, "rsx_dng_deflate.hip")
VGPR = {"dfl_inflate_kernel": 128, "dfl_row_kernel": 64}
LDS = {"dfl_inflate_kernel": 40 * 1024, "dfl_row_kernel": 0}


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not found")


def test_deflate_kernels_have_no_scratch_and_stay_within_their_registers_and_lds():
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "dfl.s")
        subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S",
                        "--cuda-device-only", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, SRC,
                        "-o", out], check=True, capture_output=True, timeout=300)
        text = open(out).read()
    kernels = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)
    assert len(kernels) == 2, [n for n, _ in kernels]
    meta = text[text.index("amdhsa.kernels:"):]
    for want in VGPR:
        (name, body), = [(n, b) for n, b in kernels if want in n]
        get = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, body).group(1))  # noqa: E731
        assert get("private_segment_fixed_size") == 0, name
        assert get("group_segment_fixed_size") <= LDS[want], (name, get("group_segment_fixed_size"))
        (entry,) = [e for e in meta.split("\n  - .") if name + "\n" in e]
        vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", entry).group(1))
        assert vgprs <= VGPR[want], (name, vgprs)
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", entry).group(1)) == 0, name
    # four decoders in a CU
    (name, body), = [(n, b) for n, b in kernels if "dfl_inflate_kernel" in n]
    assert 4 * int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1)) <= 160 * 1024
    # the window goes out in 16-byte stores, the input is taken from its lane
    assert "global_store_dwordx4" in text and "v_readlane_b32" in text


def test_the_decoder_state_is_what_the_design_says():
    core = open(os.path.join(CSRC, "rsx_inflate_core.h")).read()
    assert "RING = 32768" in core and "LEN_CAP = 852, DIST_CAP = 592, CL_CAP = 128" in core
    assert "LEN_ROOT = 9, DIST_ROOT = 6, CL_ROOT = 7" in core
    shared = 32768 + 4 * (852 + 592 + 128) + 2 * 320 + 3 * 2 * 16 + 320
    assert shared == 40112 <= 40 * 1024


def test_the_library_is_built_from_the_deflate_sources():
    from rawspeed_amd import build
    assert "rsx_dng_deflate.hip" in build.CORE_SOURCES
    for h in ("rsx_dng_deflate.h", "rsx_inflate_core.h", "rsx_fp_widen.h"):
        assert h in build.CORE_HEADERS
    assert "widen_fp" not in open(os.path.join(CSRC, "rsx_unpack.hip")).read().split("#include")[0]
    assert "uint32_t widen_fp(uint32_t narrow)" in open(os.path.join(CSRC, "rsx_fp_widen.h")).read()
