"""CrwDecompressor (Canon CRW) benchmark.  One frame of 3152 x 2068 (the EOS 10D / 300D raw size)
with low bits: a seeded smooth scene with shot noise on a Bayer pattern, its upper 10 bits through
the C writer (rsx_synth_crw_encode), its lower two as the low-bit array, decoded with the input and
the output resident in HBM:
  plan1, plan8, plan64  plans of that many frames, the kernels' hipEvent times from
                        rsx_plan_kernel_table (the jobs of a plan read the same input bytes; their
                        buffers and their outputs are their own); plan1 with the whole table and
                        the split compact (with the run's zero fills) / parse rounds / settle /
                        write / reconstruct, and the stats of rsx_crw_plan_stats
  plan1_no_rounds       plan1 on a context created with RSX_CRW_SPEC_ROUNDS=0: every window behind
                        the first is left to the settling kernel, so the difference is what the
                        speculation over the windows is worth
  variants              plan1 under other builds of the library (--variant NAME=PATH, made with
                        rawspeed_amd.build.build_variant and -DRSX_CRW_SEG_BITS / _WIN_SEGS)
  copy_probe            rsx_probe_stream_copy over the stream's bytes in and the image's bytes out,
                        in the same run; both buffers fit the Infinity Cache, so this is a
                        cache-resident figure below what any decode of the frame can reach
  host_pointers         rsx_crw_decompress through host pointers
  host_build            librsx_crw_host.so, one thread
  reference             the unmodified reference's time for the same file on one thread, as
                        scripts/record_crw_ref.py recorded it (tests/golden/crw_ref.json) -- on
                        the recorder's CPU, not on this machine's
Every leg's output is hashed against the host build's before it is timed.  Prints one JSON line
and, with --out, writes it."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, TABLE = 3152, 2068, 0
SPLIT = {"compact": ("crw_zero_kernel", "crw_count_kernel", "crw_compact_kernel"),
         "parse_rounds": ("crw_parse_kernel",), "settle": ("crw_settle_kernel",),
         "write": ("crw_scan_kernel", "crw_write_kernel"),
         "reconstruct": ("crw_carry_kernel", "crw_recon_kernel")}


def make_frame(seed=1):
    """-> (the scan, the low bits, the 12-bit values the frame decodes to)"""
    from rawspeed_amd import synth
    rng = np.random.default_rng([0x0C, seed])
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    scene = (0.45 + 0.3 * np.sin(x / 311.0) * np.cos(y / 173.0) + 0.15 * np.sin((x + 2 * y) / 37.0)
             + 0.08 * np.sin(x / 5.0) * np.sin(y / 7.0))
    gain = np.array([[0.6, 1.0], [1.0, 0.75]], np.float32)[(y.astype(np.int32) & 1),
                                                           (x.astype(np.int32) & 1)]
    signal = np.clip(scene * gain, 0.01, 0.98) * 4095.0
    noisy = signal + rng.standard_normal((H, W), dtype=np.float32) * np.sqrt(signal + 16.0) * 0.5
    img = np.clip(np.round(noisy), 0, 4095).astype(np.uint16)
    two = (img & 3).reshape(-1, 4).astype(np.uint8)
    low = (two[:, 0] | two[:, 1] << 2 | two[:, 2] << 4 | two[:, 3] << 6).astype(np.uint8).tobytes()
    return synth.crw_encode(img >> 2, TABLE), low, img


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def host_build(data, low, reps=3):
    import crw_files as F
    best, digest = None, None
    for _ in range(reps):
        t0 = time.perf_counter()
        st, px, _ = F.host_decode(data, low, W, H, TABLE)
        dt = (time.perf_counter() - t0) * 1e3
        assert st == 0, st
        best = dt if best is None else min(best, dt)
        digest = sha(px)
    return round(best, 2), digest


def device_leg(ctx, torch, data, low, n_frames, want_sha, steps, warmup):
    from rawspeed_amd import abi
    low_off = (len(data) + 15) // 16 * 16
    jobs = []
    for k in range(n_frames):
        j = abi.CrwJob()
        j.desc = abi.crw_desc(TABLE, True)
        j.in_offset, j.in_bytes, j.low_offset, j.low_bytes = 0, len(data), low_off, len(low)
        j.img_offset = k * 2 * W * H
        j.img = abi.Image(None, 2 * W, W, H, 1, 1)
        jobs.append(j)
    both = np.zeros(low_off + len(low), np.uint8)
    both[:len(data)] = np.frombuffer(data, np.uint8)
    both[low_off:] = np.frombuffer(low, np.uint8)
    inp = torch.from_numpy(both).cuda()
    out = torch.zeros(n_frames * 2 * W * H, dtype=torch.uint8, device="cuda")
    plan = ctx.crw_plan(jobs)
    s = torch.cuda.current_stream().cuda_stream
    plan.run(inp.data_ptr(), out.data_ptr(), s)
    rc, _, _ = plan.results()
    exact = rc == 0
    for k in sorted({0, n_frames - 1}):
        exact &= sha(out[k * 2 * W * H:(k + 1) * 2 * W * H].cpu().numpy()) == want_sha
    stats = plan.stats(0)
    for _ in range(warmup):
        plan.run(inp.data_ptr(), out.data_ptr(), s)
    plan.results()
    plan.set_timing(True)
    t0 = time.perf_counter()
    for _ in range(steps):
        plan.run(inp.data_ptr(), out.data_ptr(), s)
    plan.results()
    wall = (time.perf_counter() - t0) / steps * 1e3
    table_ms, runs = plan.kernel_table()
    plan.close()
    k = {}
    # (the table has one row a kernel name: the launches of the parse rounds are summed in theirs)
    for name, ms in table_ms:
        k[name] = k.get(name, 0.0) + ms
    total = sum(k.values())
    leg = {"frames": n_frames, "kernel_ms": round(total, 4),
           "kernel_ms_per_frame": round(total / n_frames, 4),
           "split_ms": {part: round(sum(k.get(n, 0.0) for n in names), 4)
                        for part, names in SPLIT.items()},
           "wall_ms_per_step": round(wall, 3),
           "mpix_s": round(n_frames * W * H / (total * 1e-3) / 1e6, 1),
           "stats": dict(zip(("windows", "inner_rounds", "outer_rounds", "settle_work"), stats)),
           "runs": runs, "bit_exact": bool(exact)}
    if n_frames == 1:
        leg["kernels_ms"] = {name: round(ms, 4) for name, ms in k.items()}
    return leg


def copy_probe(ctx, torch, data, steps):
    inp = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    out = torch.zeros(2 * W * H, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    ms = [ctx.probe_stream_copy(inp.data_ptr(), inp.numel(), out.data_ptr(), out.numel(), s,
                                reps=max(steps, 5)) for _ in range(3)]
    return round(float(np.median(ms)), 4)


def host_pointer_leg(ctx, data, low, want_sha, reps=3):
    from oracle_lib import HostImage
    best, exact = None, True
    for _ in range(reps):
        out = HostImage(W, H)
        t0 = time.perf_counter()
        st = ctx.crw_decompress(TABLE, data, low, out.view())
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
        exact &= st == 0 and sha(out.pixels()) == want_sha
    return {"host_call_ms": round(best, 2), "bit_exact": bool(exact)}


def child_plan1(args, env):
    """plan1 in a child process: the library reads RSX_CRW_SPEC_ROUNDS when a context is made, and
    RSX_LIB names another build of it"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only-plan1", "--steps",
                        str(args.steps), "--warmup", str(args.warmup)],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        return {"error": r.stderr[-400:]}
    return json.loads(r.stdout.strip().split("\n")[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--plans", default="1,8,64")
    ap.add_argument("--only-plan1", action="store_true")
    ap.add_argument("--variant", action="append", default=[], help="NAME=PATH of another build")
    ap.add_argument("--out")
    args = ap.parse_args()
    import crw_files as F
    data, low, img = make_frame()
    want = sha(img)
    import torch
    from rawspeed_amd import capi
    ctx = capi.Context(0)
    if args.only_plan1:
        print(json.dumps(device_leg(ctx, torch, data, low, 1, want, args.steps, args.warmup)))
        return
    res = {"metric": "crw_decode", "width": W, "height": H, "table": TABLE,
           "stream_bytes": len(data), "bits_per_pixel": round(len(data) * 8 / (W * H), 3),
           "segment_bits": F.SEG_BITS, "window_segments": F.WIN_SEGS}
    one, digest = host_build(data, low)
    exact = digest == want
    res["host_build"] = {"ms_1_frame_1_thread": one}
    for n in [int(v) for v in args.plans.split(",")]:
        leg = device_leg(ctx, torch, data, low, n, want, args.steps if n < 64 else 3, args.warmup)
        exact &= leg["bit_exact"]
        res["plan%d" % n] = leg
    res["copy_probe_ms"] = copy_probe(ctx, torch, data, args.steps)
    leg = host_pointer_leg(ctx, data, low, want)
    exact &= leg["bit_exact"]
    res["host_pointers"] = leg
    res["plan1_no_rounds"] = child_plan1(args, {"RSX_CRW_SPEC_ROUNDS": "0"})
    res["variants"] = {}
    for v in args.variant:
        name, path = v.split("=", 1)
        res["variants"][name] = child_plan1(args, {"RSX_LIB": os.path.abspath(path)})
    try:
        with open(F.GOLDEN) as f:
            ref = json.load(f).get("reference_timing")
    except OSError:
        ref = None
    if ref and ref.get("stream_sha256") == hashlib.sha256(data).hexdigest():
        res["reference"] = ref
        res["reference_over_plan1_kernels"] = round(ref["ms_1_thread"] / res["plan1"]["kernel_ms"], 2)
    res["bit_exact"] = bool(exact)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
