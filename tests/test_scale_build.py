"""The black/white scaling stage builds: the host library and its program (which passes, on its
built-in cases and on the model's, with AddressSanitizer and UBSan where g++ has them), the
symbols the package binds, the struct layouts of rawspeed_amd/abi.py against include/rsx.h (a C
program prints them), and the compiled kernels.  hipcc cross-compiles gfx950; no GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import scale_files as S
from rawspeed_amd import abi, build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rawspeed_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")

EXPORTS = ["rsx_scale_validate", "rsx_scale_black_white", "rsx_scale_plan_create",
           "rsx_scale_plan_result"]


def test_host_library_and_program_build():
    lib_path, prog = build.build_scale_host()
    assert os.path.exists(lib_path) and os.access(prog, os.X_OK)
    L = C.CDLL(lib_path)
    for name in ("rsx_scale_host_validate", "rsx_scale_host_black_white", "rsx_scale_host_jump"):
        assert hasattr(L, name), name


def test_the_check_program_passes_on_its_own_cases_and_on_the_models():
    _, prog = build.build_scale_host()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "cases.bin")
        S.write_cases(path)
        r = subprocess.run([prog, path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d file cases" % len(S.cases()) in r.stdout
    assert "rsx_scale_host_check OK" in r.stdout


def test_the_check_program_carries_the_sanitizers_where_the_compiler_has_them():
    if not build._links_with_sanitizers():
        pytest.skip("g++ has no sanitizer runtimes here")
    _, prog = build.build_scale_host()
    data = open(prog, "rb").read()
    assert b"__asan_init" in data and b"__ubsan_handle" in data


def test_sources_are_part_of_the_core_library():
    assert "rsx_scale.hip" in build.CORE_SOURCES
    assert "rsx_scale.h" in build.CORE_HEADERS and "rsx_scale_core.h" in build.CORE_HEADERS
    for name in ("rsx_scale.hip", "rsx_scale.h", "rsx_scale_core.h", "rsx_scale_host.cpp"):
        assert os.path.exists(os.path.join(CSRC, name))


def test_exports_are_declared_in_the_header_and_bound():
    header = open(os.path.join(INCLUDE, "rsx.h")).read()
    src = open(os.path.join(CSRC, "rsx_api.hip")).read()
    assert sorted(n for n in capi.EXPORTS if n.startswith("rsx_scale_")) == sorted(EXPORTS)
    for n in EXPORTS:
        assert re.search(r"\bint %s\(" % n, header), n
        assert re.search(r'extern "C" int %s\(' % n, src), n
        # (the names the other stages' build tests pick their exports by)
        assert not any(s in n for s in ("bad_pixels", "dng_post", "_finish"))
        getattr(capi.lib(), n)


def test_struct_layouts_match_the_header():
    fields = {"rsx_scale_area": (abi.ScaleArea, ["offset", "size", "is_vertical"]),
              "rsx_scale_desc": (abi.ScaleDesc, ["off_x", "off_y", "crop_x", "crop_y", "is_f32",
                                                 "black_level", "has_white", "white_point",
                                                 "has_separate", "black_separate", "n_areas", "areas",
                                                 "dither", "host_sse2"]),
              "rsx_scale_result": (abi.ScaleResult, ["black_level", "white_point", "black_separate",
                                                     "estimated", "skipped", "variant", "n_wrapped"]),
              "rsx_scale_job": (abi.ScaleJob, ["desc", "img_offset", "img"])}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rsx.h"', "int main(void) {"]
    for c_name, (_, names) in fields.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (c_name, c_name))
        for f in names:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (c_name, f, c_name, f))
    lines.append("return 0; }")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as f:
            f.write("\n".join(lines))
        subprocess.run(["gcc", "-I" + INCLUDE, src, "-o", exe], check=True, capture_output=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    got = dict(line.split() for line in out.splitlines())
    for c_name, (t, names) in fields.items():
        assert int(got[c_name]) == C.sizeof(t), c_name
        for f in names:
            assert int(got["%s.%s" % (c_name, f)]) == getattr(t, f).offset, (c_name, f)


def test_the_model_and_the_core_agree_on_the_checkpoint_distance():
    core = open(os.path.join(CSRC, "rsx_scale_core.h")).read()
    assert re.search(r"CHK_BLOCKS = %d;" % S.CHK_BLOCKS, core)


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not found")


@pytest.fixture(scope="module")
def kernels():
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "scale.s")
        subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S",
                        "--cuda-device-only", "-I" + INCLUDE, "-I" + CSRC,
                        os.path.join(CSRC, "rsx_scale.hip"), "-o", out],
                       check=True, capture_output=True, timeout=300)
        asm = open(out).read()
    found = {}
    for name, body in re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, re.S):
        code = re.search(r"^%s:(.*?)^\.Lfunc_end" % re.escape(name), asm, re.S | re.M).group(1)
        get = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, body).group(1))  # noqa: E731
        found[name] = dict(scratch=get("private_segment_fixed_size"), vgpr=get("next_free_vgpr"),
                           lds=get("group_segment_fixed_size"), code=code)
    return asm, found


def test_kernels_without_scratch_and_flat_accesses(kernels):
    asm, found = kernels
    stems = ("sc_init_kernel", "sc_estimate_kernel", "sc_hist_kernel", "sc_levels_kernel",
             "sc_chain_kernel", "sc_pass_kernel")
    for stem in stems:
        hits = [v for k, v in found.items() if stem in k]
        assert len(hits) == 1, (stem, list(found))
        assert hits[0]["scratch"] == 0
        assert hits[0]["vgpr"] <= 128, (stem, hits[0]["vgpr"])  # (4 waves a SIMD at the least)
        assert (hits[0]["lds"] != 0) == (stem == "sc_levels_kernel")
    assert len(found) == len(stems)
    assert not re.search(r"\bscratch_", asm)
    assert not re.search(r"\bflat_(load|store|atomic)", asm)
    # the pass moves 16 bytes a lane where a run lies on the grid
    code = next(v for k, v in found.items() if "sc_pass_kernel" in k)["code"]
    assert "global_load_dwordx4" in code and "global_store_dwordx4" in code
    # the F32 pass rounds twice: no fused multiply-add in the kernel
    assert not re.search(r"\bv_fma(c|ak|mk)?_f32", code)
