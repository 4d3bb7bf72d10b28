"""The compiled PhaseOneDecompressor kernel (rsx_phase_one.hip) keeps its 64 pixels a lane in
registers: no scratch, and no static LDS (the row's words, checkpoints and scan totals are
the dynamic LDS the launch asks for).  hipcc cross-compiles gfx950; no GPU needed."""
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


def test_phase_one_kernel_has_no_scratch():
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "p1.s")
        subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S",
                        "--cuda-device-only", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "rawspeed_amd", "csrc"),
                        os.path.join(ROOT, "rawspeed_amd", "csrc", "rsx_phase_one.hip"),
                        "-o", out], check=True, capture_output=True, timeout=300)
        text = open(out).read()
    kernels = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)
    assert any("p1_row_kernel" in name for name, _ in kernels), [n for n, _ in kernels]
    for name, body in kernels:
        get = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, body).group(1))  # noqa: E731
        assert get("private_segment_fixed_size") == 0, name
        assert get("group_segment_fixed_size") == 0, name
        assert get("next_free_vgpr") <= 128, (name, get("next_free_vgpr"))
