"""FujiDecompressor (compressed RAF) benchmark.  Frames of 6240 x 4158 (9 strips; 4160 is no
multiple of the 6 rows of a strip line, which the header check refuses) as X-Trans and as Bayer,
14 bit, and a 16-strip frame of 12288 x 4158, decoded with the input and the output resident in
HBM: one frame, and plans of 8 and 64 X-Trans frames in one launch (the kernel's hipEvent time
from rsx_plan_kernel_table); the host-pointer call; and the host build of the same core
(librsx_fuji_host.so) on 1 and on --threads threads in the same run.  The frames come from the C
writer (rsx_synth_fuji_encode_strip) over a sensor-like image; ONE encoded strip is reused for all
strips of a frame, and the frames of a plan read the same input bytes (their outputs are their
own).  Every leg's output is hashed against the host build's before it is timed.  Prints one JSON
line; --write-frame FILE writes the X-Trans container for scripts/record_fuji_ref.cpp --time."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LDS_PER_CU = 160 * 1024
KERNEL_LDS = 28680  # fuji_strip_kernel's static LDS (tests/test_fuji_build.py holds the bound)


def make_frame(raw_type, raw_bits, w, h, seed=1):
    """-> (container bytes, coded samples of the frame)"""
    import fuji_files as F
    from rawspeed_amd import synth
    lines = h // 6
    rng = np.random.default_rng([0xF0, raw_type, raw_bits, seed])
    y, x = np.mgrid[0:h, 0:F.BLOCK]
    q4 = (1 << raw_bits) - 1
    img = np.clip(q4 // 8 + 3 * x + y + rng.normal(0, 24, (h, F.BLOCK)), 0, q4).astype(np.uint16)
    strip, _, _ = synth.fuji_encode_strip(raw_type, raw_bits, lines, img)
    n = (w + F.BLOCK - 1) // F.BLOCK
    hd = F.header(raw_type, raw_bits, w, h)
    half = (512 if raw_type == 16 else 384) // 2
    coded = 0
    for row in range(6):
        for comp in range(2):
            coded += half  # (the odd phase)
            coded += sum(1 for i in range(half)
                         if not (raw_type == 16 and F.Strip.no_bits(row, i, comp)))
    return F.container(hd, [strip] * n), coded * lines * n


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def host_build(data, threads, reps=3):
    """-> (best ms, sha of the rows)"""
    import ctypes as C
    import fuji_files as F
    from rawspeed_amd import abi
    st, d = F.host_parse(data)
    w, h = d.raw_width, d.raw_height
    a = np.frombuffer(data, np.uint8)
    best, digest = None, None
    for _ in range(reps):
        buf = np.zeros((h, w), np.uint16)
        view = abi.Image(buf.ctypes.data, 2 * w, w, h, 1, 1)
        t0 = time.perf_counter()
        rc = F.host_lib().rsx_fuji_host_decode(C.byref(d), a.ctypes.data, len(data), C.byref(view),
                                               None, threads)
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0, rc
        best = dt if best is None else min(best, dt)
        digest = sha(buf)
    return round(best, 2), digest


def device_leg(ctx, torch, data, n_frames, want_sha, coded, steps, warmup):
    from rawspeed_amd import abi, capi
    st, d = capi.fuji_parse(data)
    w, h = d.raw_width, d.raw_height
    jobs = []
    for k in range(n_frames):
        j = abi.FujiJob()
        j.desc = d
        j.in_offset, j.in_bytes, j.img_offset = 0, len(data), k * 2 * w * h
        j.img = abi.Image(None, 2 * w, w, h, 1, 1)
        jobs.append(j)
    inp = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    out = torch.zeros(n_frames * 2 * w * h, dtype=torch.uint8, device="cuda")
    plan = ctx.fuji_plan(jobs)
    s = torch.cuda.current_stream().cuda_stream
    plan.run(inp.data_ptr(), out.data_ptr(), s)
    rc, _, _ = plan.results()
    exact = rc == 0
    for k in sorted({0, n_frames - 1}):
        exact &= sha(out[k * 2 * w * h:(k + 1) * 2 * w * h].cpu().numpy()) == want_sha
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
    kms = sum(ms for _, ms in table)
    strips = d.n_strips * n_frames
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    resident = min(strips, cus * (LDS_PER_CU // KERNEL_LDS))
    # the strips that are resident walk side by side: a strip's chain takes the kernel's time
    # divided by the rounds of residency
    rounds = -(-strips // resident)
    return {"frames": n_frames, "strips": strips, "strips_resident": resident,
            "kernel_ms": round(kms, 3), "kernel_ms_per_frame": round(kms / n_frames, 3),
            "wall_ms_per_step": round(wall, 3),
            "gpix_s": round(n_frames * w * h / (kms * 1e-3) / 1e9, 3),
            "walk_ns_per_coded_sample": round(kms * 1e6 / rounds / (coded / d.n_strips), 2),
            "runs": runs, "bit_exact": bool(exact)}


def host_pointer_leg(ctx, data, want_sha, reps=3):
    from oracle_lib import HostImage
    from rawspeed_amd import capi
    st, d = capi.fuji_parse(data)
    best, exact = None, True
    for _ in range(reps):
        out = HostImage(d.raw_width, d.raw_height)
        t0 = time.perf_counter()
        st, _ = ctx.fuji_decompress(d, data, out.view())
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
        exact &= st == 0 and sha(out.pixels()) == want_sha
    return {"host_call_ms": round(best, 2), "bit_exact": bool(exact)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--write-frame")
    args = ap.parse_args()
    W, H = 6240, 4158
    if args.write_frame:
        with open(args.write_frame, "wb") as f:
            f.write(make_frame(16, 14, W, H)[0])
        return
    import torch
    from rawspeed_amd import capi
    ctx = capi.Context(0)
    res = {"metric": "fuji_decode", "threads": args.threads}
    exact = True
    frames = {"xtrans14": make_frame(16, 14, W, H), "bayer14": make_frame(0, 14, W, H),
              "xtrans14_16strips": make_frame(16, 14, 12288, H)}
    cpu = {}
    for name, (data, coded) in frames.items():
        one, digest = host_build(data, 1)
        many, digest_n = host_build(data, args.threads)
        exact &= digest == digest_n
        cpu[name] = digest
        res["host_build_" + name] = {"ms_1_thread": one, "ms_threads": many,
                                     "container_bytes": len(data), "coded_samples": coded}
    for name, (data, coded) in frames.items():
        leg = device_leg(ctx, torch, data, 1, cpu[name], coded, args.steps, args.warmup)
        exact &= leg["bit_exact"]
        res[name] = leg
    data, coded = frames["xtrans14"]
    for n in (8, 64):
        leg = device_leg(ctx, torch, data, n, cpu["xtrans14"], coded, max(2, args.steps // 2),
                         args.warmup)
        exact &= leg["bit_exact"]
        res["xtrans14_plan%d" % n] = leg
    leg = host_pointer_leg(ctx, data, cpu["xtrans14"])
    exact &= leg["bit_exact"]
    res["xtrans14_host_pointers"] = leg
    res["bit_exact"] = bool(exact)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
