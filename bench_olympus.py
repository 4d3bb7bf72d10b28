"""OlympusDecompressor (compressed ORF) benchmark.  One frame of 5240 x 3912 (the E-M1 II/III and
OM-1 raw size) of seeded 12-bit noise from the C writer (rsx_synth_olympus_encode), decoded with
the input and the output resident in HBM: plans of 1, 8, 64 and 256 frames in one launch each (the
two kernels' hipEvent times from rsx_plan_kernel_table; the jobs of a plan read the same input
bytes, their outputs are their own), the host-pointer call, and the host build of the same core
(librsx_olympus_host.so) on one thread and as --threads frames at once on --threads threads (the
codec's loop is serial, so threads only help across frames).  Every leg's output is hashed against
the host build's before it is timed.  Prints one JSON line and, with --out, writes it;
--write-frame FILE writes the stream for scripts/record_olympus_ref.cpp --time."""
import argparse
import hashlib
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 5240, 3912


def make_frame(seed=1):
    from rawspeed_amd import synth
    img = np.random.default_rng([0x01, seed]).integers(0, 4096, (H, W), dtype=np.uint16)
    return synth.olympus_encode(img), img


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def host_once(data):
    import olympus_files as F
    t0 = time.perf_counter()
    rc, buf = F.host_decode(data, W, H, fill=0)
    dt = (time.perf_counter() - t0) * 1e3
    assert rc == 0, rc
    return dt, buf


def host_build(data, threads, reps=3):
    """-> (best ms of one frame on one thread, best ms of `threads` frames at once, sha)"""
    one, digest = None, None
    for _ in range(reps):
        dt, buf = host_once(data)
        one = dt if one is None else min(one, dt)
        digest = sha(buf)
    many = None
    for _ in range(reps):
        pool = [threading.Thread(target=host_once, args=(data,)) for _ in range(threads)]
        t0 = time.perf_counter()
        for t in pool:
            t.start()
        for t in pool:
            t.join()
        dt = (time.perf_counter() - t0) * 1e3
        many = dt if many is None else min(many, dt)
    return round(one, 2), round(many, 2), digest


def device_leg(ctx, torch, data, n_frames, want_sha, steps, warmup):
    from rawspeed_amd import abi
    jobs = []
    for k in range(n_frames):
        j = abi.OlympusJob()
        j.in_offset, j.in_bytes, j.img_offset = 0, len(data), k * 2 * W * H
        j.img = abi.Image(None, 2 * W, W, H, 1, 1)
        jobs.append(j)
    inp = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    out = torch.zeros(n_frames * 2 * W * H, dtype=torch.uint8, device="cuda")
    plan = ctx.olympus_plan(jobs)
    s = torch.cuda.current_stream().cuda_stream
    plan.run(inp.data_ptr(), out.data_ptr(), s)
    rc, _, _ = plan.results()
    exact = rc == 0
    for k in sorted({0, n_frames - 1}):
        exact &= sha(out[k * 2 * W * H:(k + 1) * 2 * W * H].cpu().numpy()) == want_sha
    for _ in range(warmup):
        plan.run(inp.data_ptr(), out.data_ptr(), s)
    plan.results()
    plan.set_timing(True)
    t0 = time.perf_counter()
    for _ in range(steps):
        plan.run(inp.data_ptr(), out.data_ptr(), s)
    plan.results()
    wall = (time.perf_counter() - t0) / steps * 1e3
    table, runs = plan.kernel_table()
    plan.close()
    k = dict(table)
    parse, recon = k["olympus_parse_kernel"], k["olympus_recon_kernel"]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    # one wavefront a job walks: the jobs beyond one a SIMD (4 a CU) share a SIMD's scalar unit
    return {"frames": n_frames, "parse_ms": round(parse, 3), "recon_ms": round(recon, 3),
            "kernel_ms": round(parse + recon, 3),
            "kernel_ms_per_frame": round((parse + recon) / n_frames, 3),
            "walk_ns_per_symbol": round(parse * 1e6 / (W * H), 2),
            "wall_ms_per_step": round(wall, 3), "compute_units": cus,
            "gpix_s": round(n_frames * W * H / ((parse + recon) * 1e-3) / 1e9, 4),
            "runs": runs, "bit_exact": bool(exact)}


def host_pointer_leg(ctx, data, want_sha, reps=3):
    from oracle_lib import HostImage
    best, exact = None, True
    for _ in range(reps):
        out = HostImage(W, H)
        t0 = time.perf_counter()
        st = ctx.olympus_decompress(data, out.view())
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
        exact &= st == 0 and sha(out.pixels()) == want_sha
    return {"host_call_ms": round(best, 2), "bit_exact": bool(exact)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--plans", default="1,8,64,256")
    ap.add_argument("--write-frame")
    ap.add_argument("--out")
    args = ap.parse_args()
    data, img = make_frame()
    if args.write_frame:
        with open(args.write_frame, "wb") as f:
            f.write(data)
        return
    import torch
    from rawspeed_amd import capi
    ctx = capi.Context(0)
    res = {"metric": "olympus_decode", "width": W, "height": H, "stream_bytes": len(data),
           "bits_per_pixel": round((len(data) - 7) * 8 / (W * H), 3), "threads": args.threads}
    one, many, digest = host_build(data, args.threads)
    exact = digest == sha(img)
    res["host_build"] = {"ms_1_frame_1_thread": one,
                         "ms_%d_frames_%d_threads" % (args.threads, args.threads): many,
                         "ms_per_frame_threads": round(many / args.threads, 2)}
    for n in [int(v) for v in args.plans.split(",")]:
        leg = device_leg(ctx, torch, data, n, digest, args.steps if n < 64 else 2, args.warmup)
        exact &= leg["bit_exact"]
        res["plan%d" % n] = leg
    leg = host_pointer_leg(ctx, data, digest)
    exact &= leg["bit_exact"]
    res["host_pointers"] = leg
    # frames a plan needs before a frame costs less than on the host's threads
    per_frame_host = many / args.threads
    for n in [int(v) for v in args.plans.split(",")]:
        if res["plan%d" % n]["kernel_ms_per_frame"] < per_frame_host:
            res["first_plan_ahead_of_host_threads"] = n
            break
    res["break_even_frames"] = round(res["plan1"]["kernel_ms"] / per_frame_host, 1)
    res["bit_exact"] = bool(exact)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
