"""bench.py end to end on one GPU: a plain run carries the headline and nothing that takes
runs of its own; --full adds the rest (here: the copy ceiling, the cheapest of its legs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _bench(*flags):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
           "--warmup", "1", "--frames", "2"] + list(flags)
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def test_plain_run_is_the_headline(tmp_path):
    res = _bench("--dump-outputs", str(tmp_path))
    assert res["metric"] == "MPix/s decoded (bit-exact)" and res["unit"] == "MPix/s"
    assert res["higher_is_better"] is True and res["dtype"] == "u16"
    assert res["bit_exact"] is True and res["value"] > 0 and res["ms_per_step"] > 0
    assert res["steps"] == 3 and res["warmup"] == 1 and res["n_gpus"] == 1
    # the in-run kernel time of the timed launches, but no copy probe of its own
    assert res["roofline"]["launches_timed"] == 3
    assert "copy_ceiling" not in res["roofline"]
    for k in ("cpu_baseline", "ljpeg", "extra_file"):
        assert k not in res, k
    st = np.load(str(tmp_path / "unpack_status.npy"))
    assert st.tolist() == [0.0, 0.0, 0.0]
    assert np.load(str(tmp_path / "unpack_rows.npy")).shape[1] == 8192


def test_full_run_adds_the_copy_ceiling():
    res = _bench("--full", "--no-extra", "--no-cfg5", "--no-cpu-baseline")
    assert res["bit_exact"] is True and res["value"] > 0
    assert res["roofline"]["copy_ceiling"]["gbps"] > 0
