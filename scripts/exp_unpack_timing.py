"""GPU experiment: where does the time of an unpack step go?

The headline workload (8 frames of BASELINE configs[1] per step), timing off and on: host
enqueue time against total time per step, and the in-run kernel time where it is on.  Then the
single-frame launch.  RSX_LIB=<path> runs another build of the library (A/B).

  python scripts/exp_unpack_timing.py [--steps 50] [--json OUT]
"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import bench
from rawspeed_amd import capi
import __graft_entry__ as ge

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--json", default=None, help="also write the figures to this file")
args = ap.parse_args()
if not os.environ.get("RSX_LIB"):
    ge.build()
ctx = capi.Context(0)
F, cfg = 8, bench.CFG2
jobs = bench.unpack_jobs(cfg, F)
packed, _ = bench.make_frames(cfg, 1, 1)
inp = torch.from_numpy(np.tile(packed, F)).cuda()
h, opitch = cfg["h"], bench.out_pitch(cfg["w"])
out = torch.empty(F * h * opitch, dtype=torch.uint8, device="cuda")
plan = ctx.unpack_plan(jobs)
s = torch.cuda.current_stream().cuda_stream
N = min(args.steps, 64)  # (the event pool times 64 launches)
rows = []
for timing in (False, True, False, True, False, True):
    plan.set_timing(timing)
    for _ in range(5): plan.run(inp.data_ptr(), out.data_ptr(), s)
    torch.cuda.synchronize()
    if timing:
        plan.kernel_time()  # (drop the warm-up launches)
    t0 = time.perf_counter()
    ts = []
    for _ in range(N):
        t1 = time.perf_counter(); plan.run(inp.data_ptr(), out.data_ptr(), s); ts.append(time.perf_counter() - t1)
    t_enq = time.perf_counter() - t0
    torch.cuda.synchronize()
    t_all = time.perf_counter() - t0
    kt = plan.kernel_time() if timing else None
    rows.append({"timing": timing, "enqueue_ms_per_step": round(t_enq / N * 1e3, 4),
                 "total_ms_per_step": round(t_all / N * 1e3, 4),
                 "max_call_ms": round(max(ts) * 1e3, 4),
                 "kernel_ms": round(kt[1], 5) if kt else None, "launches": kt[2] if kt else None})
    print("timing", timing, "enqueue %.4f ms/step" % (t_enq / N * 1e3), "total %.4f ms/step" % (t_all / N * 1e3),
          "max call %.3f ms" % (max(ts) * 1e3), "ktime", kt, flush=True)
plan.set_timing(False)
# single-frame latency
plan1 = ctx.unpack_plan(bench.unpack_jobs(cfg, 1))
for _ in range(3): plan1.run(inp.data_ptr(), out.data_ptr(), s)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(50): plan1.run(inp.data_ptr(), out.data_ptr(), s)
torch.cuda.synchronize()
single_us = (time.perf_counter() - t0) / 50 * 1e6
print("single frame (L3-resident) %.1f us/frame" % single_us)
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump({"lib": os.environ.get("RSX_LIB") or "in-tree", "steps": N, "runs": rows,
                   "single_frame_us": round(single_us, 1)}, f, indent=1)
