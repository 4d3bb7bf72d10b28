"""The compiled writers (rsx_encode_pack.hip, rsx_encode_ljpeg.hip): the kernels compile for gfx950
without scratch or spills; the core header compiles as strict host C++17; the check program runs
(a stand-alone program with AddressSanitizer and UBSan where g++ has them: nothing is loaded into
Python); the library binds the section's symbols; the struct layouts of rawspeed_amd/abi.py are
include/rsx.h's; and the table made from a histogram (T.81 Annex K.2) is a valid one that never
costs more than the Nikon tree on its own histogram.  hipcc cross-compiles gfx950; no GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from rawspeed_amd import abi, build, capi

import encode_files as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "rawspeed_amd", "csrc")
EXPORTS = ["rsx_encode_pack_validate", "rsx_encode_pack_u16", "rsx_encode_pack_plan_create",
           "rsx_encode_ljpeg_validate", "rsx_encode_ljpeg_bound", "rsx_encode_ljpeg",
           "rsx_encode_ljpeg_plan_create", "rsx_encode_ljpeg_plan_result",
           "rsx_encode_ljpeg_container", "rsx_encode_ljpeg_histogram",
           "rsx_encode_huff_from_histogram"]
KERNELS = {"rsx_encode_pack.hip": ["encode_pack_kernel"],
           "rsx_encode_ljpeg.hip": ["encode_ljpeg_clear_kernel", "encode_ljpeg_length_kernelILb0E",
                                    "encode_ljpeg_length_kernelILb1E", "encode_ljpeg_scan_kernel",
                                    "encode_ljpeg_emit_kernel", "encode_ljpeg_count_kernel",
                                    "encode_ljpeg_place_kernel", "encode_ljpeg_stuff_kernel"]}


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not found")


@pytest.mark.parametrize("src", sorted(KERNELS))
def test_kernels_have_no_scratch_and_no_spills(src):
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S",
                        "--cuda-device-only", "-I" + INCLUDE, "-I" + CSRC, os.path.join(CSRC, src),
                        "-o", out], check=True, capture_output=True, timeout=300)
        text = open(out).read()
    bodies = dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S))
    assert len(bodies) == len(KERNELS[src])
    for name in KERNELS[src]:
        (body,) = [b for n, b in bodies.items() if name in n]
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) == 0, name
    n = len(bodies)
    assert len(re.findall(r"\.vgpr_spill_count:\s+0\b", text)) == n
    assert len(re.findall(r"\.sgpr_spill_count:\s+0\b", text)) == n
    if src == "rsx_encode_pack.hip":
        assert "global_store_dwordx4" in text  # a lane's 16 bytes in one store


def test_core_header_compiles_as_strict_host_cxx():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        open(src, "w").write('#include "rsx_encode_core.h"\n'
                             "int main() { uint32_t diff, ssss, n;\n"
                             "  rsx_encode::reduce(-32768, &diff, &ssss);\n"
                             "  const uint16_t code[17] = {2}; const uint8_t len[17] = {2};\n"
                             "  const uint32_t w = rsx_encode::symbol(code, len, 0, 0, &n);\n"
                             "  return ssss == 16 && w == 2 && n == 2 &&\n"
                             "         rsx_encode::round_up4(5) == 8 ? 0 : 1; }\n")
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + INCLUDE,
                        "-I" + CSRC, src, "-o", os.path.join(d, "t")], check=True,
                       capture_output=True)
        assert subprocess.run([os.path.join(d, "t")]).returncode == 0


def test_check_program_runs():
    build.build_encode_host()
    r = subprocess.run([build.BIN_ENCODE_CHECK], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("rsx_encode_host_check OK") and "ERROR" not in r.stderr


def test_check_program_walks_the_case_list():
    """the case list of tests/encode_files.py handed to the program as a file: the difference lists
    (the all-ones code, the 16-bit codes, the FF tails) in both tail modes, the pack lists"""
    build.build_encode_host()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "cases.txt")
        F._write_cases(path)
        r = subprocess.run([build.BIN_ENCODE_CHECK, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    n_pack = sum(1 for c in F.pack_cases() if c[4] == 1)
    assert "cases: %d pack, %d ljpeg" % (n_pack, len(F.difference_lists())) in r.stdout
    assert "container: 96 layouts" in r.stdout and "ERROR" not in r.stderr


def test_the_library_is_built_from_the_sources():
    for name in ("rsx_encode_pack.hip", "rsx_encode_ljpeg.hip"):
        assert name in build.CORE_SOURCES
    assert "rsx_encode.h" in build.CORE_HEADERS and "rsx_encode_core.h" in build.CORE_HEADERS
    for name in build.CORE_SOURCES + build.CORE_HEADERS:
        assert os.path.exists(os.path.join(build.CSRC, name)), name
    assert os.path.exists(os.path.join(build.CSRC, "rsx_encode_host.cpp"))
    assert os.path.basename(build.LIB_ENCODE_HOST) == "librsx_encode_host.so"
    assert "build_encode_host()" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "rawspeed_amd/rsx_encode_host_check" in open(os.path.join(ROOT, ".gitignore")).read()
    # plain HIP C++: no inline assembly in the writers
    for name in ("rsx_encode_pack.hip", "rsx_encode_ljpeg.hip", "rsx_encode_core.h"):
        assert "asm" not in open(os.path.join(CSRC, name)).read()


def test_symbols_and_layouts():
    header = open(os.path.join(INCLUDE, "rsx.h")).read()
    assert "7. Writers: BitVacuumer* and PrefixCodeVectorEncoder" in header
    assert "#define RSX_ABI_VERSION 4" in header and abi.RSX_ABI_VERSION == 4
    assert sorted(n for n in capi.EXPORTS if n.startswith("rsx_encode_")) == sorted(EXPORTS)
    lib = capi.lib()
    assert lib.rsx_abi_version() == 4
    for n in EXPORTS:
        assert re.search(r"\b%s\(" % n, header), n
        getattr(lib, n)
    structs = {"rsx_encode_pack_result": (abi.EncodePackResult, ("bytes_written", "stream_bytes")),
               "rsx_encode_result": (abi.EncodeResult, ("status", "reserved", "bytes", "symbol_bits")),
               "rsx_encode_pack_job": (abi.EncodePackJob, ("desc", "reserved", "img_offset",
                                                           "out_offset", "out_cap", "img")),
               "rsx_encode_ljpeg_job": (abi.EncodeLJpegJob, ("desc", "flags", "reserved", "img_offset",
                                                             "out_offset", "out_cap", "img"))}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rsx.h"', "int main(void) {"]
    for s, (_, fields) in structs.items():
        lines.append('printf("%%zu", sizeof(%s));' % s)
        for f in fields:
            lines.append('printf(" %%zu", offsetof(%s, %s));' % (s, f))
        lines.append('printf("\\n");')
    lines.append('printf("%d %d %d\\n", RSX_ENCODE_TAIL_JPEG, RSX_ENCODE_TAIL_VACUUMER, '
                 'RSX_ENCODE_TABLE_ALL_CATEGORIES);')
    lines.append("return 0; }")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", "-I" + INCLUDE, src, "-o", os.path.join(d, "t")],
                       check=True, capture_output=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True).stdout.split("\n")
    for line, (s, (cls, fields)) in zip(out, structs.items()):
        want = [C.sizeof(cls)] + [getattr(cls, f).offset for f in fields]
        assert [int(v) for v in line.split()] == want, s
    assert out[len(structs)].split() == [str(abi.ENCODE_TAIL_JPEG), str(abi.ENCODE_TAIL_VACUUMER),
                                         str(abi.ENCODE_TABLE_ALL_CATEGORIES)]


def _histograms():
    """200 seeded histograms: one category, all 17, sparse and dense ones, small and huge counts"""
    out = []
    for k in range(200):
        rng = np.random.default_rng(k)
        h = np.zeros(17, np.uint64)
        if k < 17:
            h[k] = 1 + k * 1000
        elif k < 40:
            h[:] = rng.integers(1, 1 << rng.integers(1, 40), 17, dtype=np.uint64)
        else:
            n = int(rng.integers(1, 18))
            cats = rng.choice(17, n, replace=False)
            scale = 2.0 ** rng.uniform(0, 30)
            h[cats] = (rng.exponential(scale, n) + 1).astype(np.uint64)
        out.append(h)
    return out


def _kraft_with_reserved_point(counts):
    """the code space used, in units of 2^-16, with one more code of the longest length"""
    top = max(l for l in range(16) if counts[l])
    return sum(c << (15 - l) for l, c in enumerate(counts)) + (1 << (15 - top))


@pytest.mark.parametrize("flags", (0, abi.ENCODE_TABLE_ALL_CATEGORIES))
def test_table_from_histogram(flags):
    lib = capi.lib()
    img = F.Img(np.zeros((2, 4), np.uint16))
    v = img.view()
    for k, h in enumerate(_histograms()):
        st, t = capi.encode_huff_from_histogram(h, flags)
        hst, ht = F.host_huff(h, flags)
        assert st == hst == F.OK and bytes(t) == bytes(ht), k
        counts, values = F.table_of(t)
        present = set(range(17)) if flags else {c for c in range(17) if h[c]}
        assert set(values) == present and len(values) == len(present), k
        assert not any(counts[16:]) and sum(counts) == len(values)
        assert _kraft_with_reserved_point(counts) <= 1 << 16, k
        d = F.ljpeg_desc((0, 0, 4, 2), img, 1, [(counts, values)], [0], [0], None)
        assert lib.rsx_ljpeg_validate(C.byref(d), C.byref(v), 64) == F.OK, k
        own, nikon = F.cost_bits((counts, values), h), F.cost_bits(F.NIKON14, h)
        assert own is not None
        if not flags and nikon is not None:
            assert own <= nikon, (k, own, nikon)
    empty = np.zeros(17, np.uint64)
    assert capi.encode_huff_from_histogram(empty)[0] == F.INVALID_ARG
    assert capi.encode_huff_from_histogram(empty, abi.ENCODE_TABLE_ALL_CATEGORIES)[0] == F.OK
    assert capi.encode_huff_from_histogram(empty, 2)[0] == F.INVALID_ARG
