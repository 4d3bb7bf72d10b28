"""The lossy-DNG chain builds: the symbols the package binds, their names against the patterns the
other stages' build tests pick their exports by, and the struct layouts of rawspeed_amd/abi.py
against include/rsx.h (a C program prints them).  No GPU needed."""
import ctypes as C
import os
import re
import subprocess
import tempfile

from rawspeed_amd import abi, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rawspeed_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")

EXPORTS = ["rsx_dng_lossy_validate", "rsx_dng_lossy_decompress"]


def test_exports_are_declared_in_the_header_and_bound():
    header = open(os.path.join(INCLUDE, "rsx.h")).read()
    src = open(os.path.join(CSRC, "rsx_api.hip")).read()
    assert sorted(n for n in capi.EXPORTS if n.startswith("rsx_dng_lossy")) == sorted(EXPORTS)
    for n in EXPORTS:
        assert re.search(r"\bint %s\(" % n, header), n
        assert re.search(r'extern "C" int %s\(' % n, src), n
        getattr(capi.lib(), n)


def test_names_stay_out_of_the_other_stages_patterns():
    for n in EXPORTS:
        assert "_jpeg" not in n or "ljpeg" in n
        assert not any(s in n for s in ("dng_post", "bad_pixels"))
        assert not n.startswith("rsx_scale_")
        assert not n.endswith(("_post", "_finish"))


def test_the_abi_version_stays():
    header = open(os.path.join(INCLUDE, "rsx.h")).read()
    assert re.search(r"#define RSX_ABI_VERSION 4\b", header)
    assert capi.lib().rsx_abi_version() == 4


def test_struct_layouts_match_the_header():
    fields = {"rsx_dng_lossy_desc": (abi.DngLossyDesc, ["stage1", "has_list2", "opcodes2_bytes",
                                                        "opcodes2", "scale", "fix", "reserved"]),
              "rsx_dng_lossy_result": (abi.DngLossyResult, ["list1", "list2", "scale", "fixed",
                                                            "stages", "reserved"])}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rsx.h"', "int main(void) {"]
    for c_name, (_, names) in fields.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (c_name, c_name))
        for f in names:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (c_name, f, c_name, f))
    for k in ("STAGE1", "SCALED", "LIST2", "FIXED"):
        lines.append('printf("%s %%d\\n", RSX_DNG_LOSSY_%s);' % (k, k))
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
    assert [int(got[k]) for k in ("STAGE1", "SCALED", "LIST2", "FIXED")] == \
        [abi.DNG_LOSSY_STAGE1, abi.DNG_LOSSY_SCALED, abi.DNG_LOSSY_LIST2, abi.DNG_LOSSY_FIXED]
