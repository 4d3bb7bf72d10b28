"""Helpers for the -m gpu parity tests: device buffers come from torch
(plumbing only); every decode goes through the C-ABI (rawspeed_amd/librsx.so)."""
import ctypes
import os

import numpy as np
import torch

from rawspeed_amd import abi, capi

_ctx = None


def ctx():
    global _ctx
    if _ctx is None:
        _ctx = capi.Context(0)
    return _ctx


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def image_job_view(dim_x, dim_y, cpp, pitch, is_cfa=True):
    v = abi.Image()
    v.data = None
    v.pitch_bytes = pitch
    v.dim_x, v.dim_y, v.cpp = dim_x, dim_y, cpp
    v.is_cfa = 1 if is_cfa else 0
    return v


def plan_row_status(plan, job, n):
    """After results(): (status, the n row or strip statuses of job `job` of the last run) as the
    plan's row_status gives them.  Phase One, Samsung V0 and ARW2 plans have no getter under their
    own name; rsx_fuji_plan_strip_status hands the call to the plan whichever decoder made it
    (decoder_plan_get, rsx_api.hip)."""
    st = (ctypes.c_int32 * max(1, n))()
    rc = capi.lib().rsx_fuji_plan_strip_status(plan._h, job, st)
    return rc, list(st)[:n]


class env:
    """Names set to "1" in the environment for the block (read when a plan is made)."""

    def __init__(self, names):
        self.names = names

    def __enter__(self):
        for n in self.names:
            os.environ[n] = "1"

    def __exit__(self, *a):
        for n in self.names:
            os.environ.pop(n, None)


def run_plan(make_plan, jobs, in_host, out_bytes, route=()):
    """A plan made under `route` (environment names), run twice into 0xA5-filled outputs of
    out_bytes + 16 bytes.  Returns (statuses, first output, second output, kernel names of the
    runs, the consumed bytes of each run)."""
    with env(route):
        plan = make_plan(jobs)
    d_in = to_dev(in_host)
    d_out = torch.full((out_bytes + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    plan.set_timing(True)
    plan.run(d_in.data_ptr(), d_out.data_ptr())
    rc, status, consumed = plan.results()
    tab = plan.kernel_table()
    plan.kernel_time()  # (resets the totals: the next table is the next run's)
    names = [n for n, _ in tab[0]] if tab else []
    # a second run of the same plan: the steady-state instantiation, the cached level -- and the pass
    # that redoes what the single-pass kernel gave up on is launched by the run itself (the first
    # run's is launched when the results are fetched, outside the timed launches): its kernels are
    # in THIS run's table
    d_out2 = torch.full((out_bytes + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    plan.run(d_in.data_ptr(), d_out2.data_ptr())
    rc2, status2, consumed2 = plan.results()
    tab = plan.kernel_table()
    names += ["run 2: " + n for n, _ in tab[0]] if tab else []
    plan.set_timing(False)
    plan.close()
    assert rc == rc2 and status == status2  # (rc: the first failing job's status)
    return status, d_out.cpu().numpy(), d_out2.cpu().numpy(), names, (consumed, consumed2)
