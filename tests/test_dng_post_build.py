"""The DNG opcode / look-up stage builds: the host library and its program, the symbols the package
binds, the struct layouts of rawspeed_amd/abi.py against include/rsx.h (a C program prints them),
and the compiled kernel -- no scratch, 16-byte loads and stores, every memory access global.
hipcc cross-compiles gfx950; no GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from rawspeed_amd import abi, build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rawspeed_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")


def test_host_library_and_program_build():
    lib_path, prog = build.build_dng_post_host()
    assert os.path.exists(lib_path) and os.access(prog, os.X_OK)
    L = C.CDLL(lib_path)
    for name in ("rsx_dng_post_host_validate", "rsx_dng_post_host_apply", "rsx_dng_post_host_dither_state"):
        assert hasattr(L, name), name


def test_the_check_program_carries_the_sanitizers_where_the_compiler_has_them():
    """build_dng_post_host() falls back to a plain build when the sanitizer link fails; where a
    one-line program links with the same flags, the check program must be the instrumented one"""
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
             "-static-libubsan"]
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        with open(src, "w") as f:
            f.write("int main() { return 0; }\n")
        can = subprocess.run(["g++", src, "-o", os.path.join(d, "t")] + flags,
                             capture_output=True).returncode == 0
    if not can:
        pytest.skip("g++ has no sanitizer runtimes here")
    _, prog = build.build_dng_post_host()
    data = open(prog, "rb").read()
    assert b"__asan_init" in data and b"__ubsan_handle" in data


def test_sources_are_part_of_the_core_library():
    assert "rsx_dng_post.hip" in build.CORE_SOURCES
    assert "rsx_dng_post.h" in build.CORE_HEADERS and "rsx_dng_post_core.h" in build.CORE_HEADERS
    for name in ("rsx_dng_post.hip", "rsx_dng_post.h", "rsx_dng_post_core.h", "rsx_dng_post_host.cpp"):
        assert os.path.exists(os.path.join(CSRC, name))


def test_exports_are_declared_in_the_header():
    header = open(os.path.join(INCLUDE, "rsx.h")).read()
    names = [n for n in capi.EXPORTS if "dng_post" in n or n.endswith("_post")]
    assert sorted(names) == sorted([
        "rsx_dng_post_validate", "rsx_dng_post", "rsx_dng_decompress_ljpeg_post",
        "rsx_dng_decompress_uncompressed_post", "rsx_dng_post_plan_create",
        "rsx_dng_post_plan_result", "rsx_dng_post_plan_bad_pixels"])
    for n in names:
        assert re.search(r"\bint %s\(" % n, header), n
    src = open(os.path.join(CSRC, "rsx_api.hip")).read()
    for n in names:
        assert re.search(r'extern "C" int %s\(' % n, src), n


def test_struct_layouts_match_the_header():
    fields = {"rsx_dng_post_desc": (abi.DngPostDesc, ["opcodes", "opcodes_bytes", "table_count", "table",
                                                      "is_f32", "crop_x", "crop_h"]),
              "rsx_dng_post_result": (abi.DngPostResult, ["list_status", "n_applied", "crop_x", "n_bad"]),
              "rsx_dng_post_job": (abi.DngPostJob, ["desc", "img_offset", "img", "bad_cap"])}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rsx.h"', "int main(void) {"]
    for c_name, (_, names) in fields.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (c_name, c_name))
        for f in names:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (c_name, f, c_name, f))
    lines.append('printf("max_ops %d\\n", RSX_DNG_POST_MAX_PIXEL_OPS);')
    lines.append('printf("reason_last %d\\n", (int)RSX_DNG_POST_REASON_TRIM_EMPTY);')
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
    assert int(got["max_ops"]) == abi.RSX_DNG_POST_MAX_PIXEL_OPS
    assert int(got["reason_last"]) == abi.DNG_POST_REASON_TRIM_EMPTY


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not found")


@pytest.fixture(scope="module")
def kernels():
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "dng_post.s")
        subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S",
                        "--cuda-device-only", "-I" + INCLUDE, "-I" + CSRC,
                        os.path.join(CSRC, "rsx_dng_post.hip"), "-o", out],
                       check=True, capture_output=True, timeout=300)
        asm = open(out).read()
    found = {}
    for name, body in re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, re.S):
        code = re.search(r"^%s:(.*?)s_endpgm" % re.escape(name), asm, re.S | re.M).group(1)
        get = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, body).group(1))  # noqa: E731
        found[name] = dict(scratch=get("private_segment_fixed_size"), vgpr=get("next_free_vgpr"),
                           lds=get("group_segment_fixed_size"), code=code)
    return asm, found


def test_both_kernels_without_scratch(kernels):
    asm, found = kernels
    hits = [v for k, v in found.items() if "dng_post_kernel" in k]
    assert len(hits) == 2, list(found)  # (uint16 and F32)
    for k in hits:
        assert k["scratch"] == 0 and k["lds"] <= 16
        assert k["vgpr"] <= 128, k["vgpr"]  # (4 waves a SIMD at the least)
        assert "global_load_dwordx4" in k["code"] and "global_store_dwordx4" in k["code"]
    assert not re.search(r"\bscratch_", asm)
    assert not re.search(r"\bflat_(load|store)", asm)
