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


def test_the_test_material_mirrors_the_launch_geometry():
    """tests/vc5_files.py names the sizes the device tests place their edges by -- the window and
    the words behind it, the merge, level and low-pass decompositions, the image sides -- and the
    tests assert from them that an input reaches its path.  Read here out of the sources, so that
    a retuned kernel cannot move an edge away from its test unnoticed."""
    import vc5_files as V
    hip = open(os.path.join(CSRC, "rsx_vc5.hip")).read()
    core = open(os.path.join(CSRC, "rsx_vc5_core.h")).read()

    def const(name, text=hip):
        return re.search(r"constexpr \w+ (?:\w+ = [^,;]+, )*%s = ([^,;]+)[,;]" % name, text).group(1).strip()

    assert const("SEG_BITS", core) == "RSX_VC5_SEG_BITS"
    assert int(re.search(r"#define RSX_VC5_SEG_BITS (\d+)", core).group(1)) == V.SEG_BITS
    assert const("VC_THREADS") == "RSX_VC5_THREADS"
    assert int(re.search(r"#define RSX_VC5_THREADS (\d+)", hip).group(1)) == V.LANES
    assert const("VC_WIN_BITS") == "VC_THREADS * SEG_BITS" and V.WIN_BITS == V.LANES * V.SEG_BITS
    assert const("VC_WIN_WORDS") == "VC_WIN_BITS / 32"
    assert const("VC_WIN_LOAD") == "VC_WIN_WORDS + %d" % V.WIN_EXTRA_WORDS
    assert (int(const("VC_TILE_X")), int(const("VC_TILE_Y"))) == (V.LEVEL_X, V.LEVEL_Y)
    assert int(const("VC_MERGE_ROWS")) == V.MERGE_ROWS
    assert (int(const("VC_MIN_DIM")), int(const("VC_MAX_DIM"))) == (V.MIN_DIM, V.MAX_DIM)
    # the low-pass band: VC_LP_SPLIT workgroups of 256 lanes, and the loop's stride
    split = int(const("VC_LP_SPLIT"))
    assert "__launch_bounds__(256) vc5_lowpass_kernel" in hip and "i += 256u * VC_LP_SPLIT" in hip
    assert "dim3(n_lp * VC_LP_SPLIT), dim3(256)" in hip and split * 256 == V.LP_STRIDE
    # the merge: 64 lanes of 4 cells a row (the kernel and the plan's tile count write them out)
    lanes, cells = re.search(r"c0 = (\d+)u \* \(I\.tx \* (\d+)u \+ \(threadIdx\.x & 63u\)\)", hip).group(2, 1)
    assert int(cells) == V.MERGE_LANE_CELLS and int(lanes) * int(cells) == V.MERGE_CELLS
    assert "tx < (M.w2 + %du) / %du" % (V.MERGE_CELLS - 1, V.MERGE_CELLS) in hip


def test_sources_are_part_of_the_core_library():
    assert "rsx_vc5.hip" in build.CORE_SOURCES
    assert "rsx_vc5.h" in build.CORE_HEADERS and "rsx_vc5_core.h" in build.CORE_HEADERS
    for name in ("rsx_vc5.hip", "rsx_vc5.h", "rsx_vc5_core.h", "rsx_vc5_host.cpp"):
        assert os.path.exists(os.path.join(CSRC, name))
