"""KodakDecompressor (Kodak DCR) benchmark.  One frame of 4516 x 3012 at 12 bits (the DCS Pro 14n
raw size): a seeded smooth scene with shot noise on a Bayer pattern, through the C writer
(rsx_synth_kodak_encode), decoded through a camera-like curve (the dither table, as DcrDecoder
installs it) with the input and the output resident in HBM:
  plan1, plan8, plan64  plans of that many frames, the kernels' hipEvent times from
                        rsx_plan_kernel_table (the jobs of a plan read the same input bytes; their
                        maps and their outputs are their own); plan1 with the whole table
  plan1_row_walk        plan1 with the row starts by one dependent load a row
                        (RSX_KODAK_ROW_WALK=1) instead of by doubling
  copy_probe            rsx_probe_stream_copy over the stream's bytes in and the image's bytes out,
                        in the same run: the floor of any decode
  host_pointers         rsx_kodak_decompress through host pointers
  host_build            librsx_kodak_host.so, one thread
  reference             the unmodified reference's time for the same file on one thread, as
                        scripts/record_kodak_ref.py recorded it (tests/golden/kodak_ref.json) -- on
                        the recorder's CPU, not on this machine's
Every leg's output is hashed against the host build's before it is timed.  Prints one JSON line
and, with --out, writes it."""
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

W, H, BPS = 4516, 3012, 12
FIND = ("kodak_succ_kernel", "kodak_row_map_kernel", "kodak_row_double_kernel",
        "kodak_row_walk_kernel", "kodak_seg_kernel")


def make_frame(seed=1):
    """-> (the stream, the values it decodes to, the curve)"""
    from rawspeed_amd import synth
    rng = np.random.default_rng([0x0D, seed])
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    scene = (0.45 + 0.3 * np.sin(x / 311.0) * np.cos(y / 173.0) + 0.15 * np.sin((x + 2 * y) / 37.0)
             + 0.08 * np.sin(x / 5.0) * np.sin(y / 7.0))
    gain = np.array([[0.6, 1.0], [1.0, 0.75]], np.float32)[(y.astype(np.int32) & 1),
                                                           (x.astype(np.int32) & 1)]
    signal = np.clip(scene * gain, 0.01, 0.98) * 4095.0
    noisy = signal + rng.standard_normal((H, W), dtype=np.float32) * np.sqrt(signal + 16.0) * 0.5
    img = np.clip(np.round(noisy), 0, 4095).astype(np.uint16)
    n = 1 << BPS
    curve = np.minimum(65535, np.round(65535 * (np.arange(n) / (n - 1.0)) ** 0.6)).astype(np.uint16)
    return synth.kodak_encode(img), img, curve


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def host_build(data, table, reps=3):
    import kodak_files as F
    best, digest = None, None
    for _ in range(reps):
        t0 = time.perf_counter()
        st, px, _, _ = F.host_decode(data, W, H, BPS, F.DITHER, table)
        dt = (time.perf_counter() - t0) * 1e3
        assert st == 0, st
        best = dt if best is None else min(best, dt)
        digest = sha(px)
    return round(best, 2), digest


def device_leg(ctx, torch, data, table, n_frames, want_sha, steps, warmup):
    from rawspeed_amd import abi
    jobs, keep = [], []
    for k in range(n_frames):
        j = abi.KodakJob()
        j.desc, arr = abi.kodak_desc(BPS, abi.RSX_KODAK_TABLE_DITHER, table)
        keep.append(arr)
        j.in_offset, j.in_bytes, j.img_offset = 0, len(data), k * 2 * W * H
        j.img = abi.Image(None, 2 * W, W, H, 1, 1)
        jobs.append(j)
    inp = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    out = torch.zeros(n_frames * 2 * W * H, dtype=torch.uint8, device="cuda")
    plan = ctx.kodak_plan(jobs)
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
    table_ms, runs = plan.kernel_table()
    plan.close()
    k = {}
    for name, ms in table_ms:  # (one entry a launch: the doubling levels add up)
        k[name] = k.get(name, 0.0) + ms
    find = sum(ms for name, ms in k.items() if name in FIND)
    total = sum(k.values())
    leg = {"frames": n_frames, "kernel_ms": round(total, 4),
           "kernel_ms_per_frame": round(total / n_frames, 4),
           "find_starts_ms": round(find, 4), "decode_ms": round(k["kodak_decode_kernel"], 4),
           "find_starts_share": round(find / total, 3),
           "wall_ms_per_step": round(wall, 3),
           "gpix_s": round(n_frames * W * H / (total * 1e-3) / 1e9, 3),
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


def host_pointer_leg(ctx, data, table, want_sha, reps=3):
    from oracle_lib import HostImage
    from rawspeed_amd import abi
    best, exact = None, True
    for _ in range(reps):
        out = HostImage(W, H)
        t0 = time.perf_counter()
        st = ctx.kodak_decompress(BPS, abi.RSX_KODAK_TABLE_DITHER, table, data, out.view())
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
        exact &= st == 0 and sha(out.pixels()) == want_sha
    return {"host_call_ms": round(best, 2), "bit_exact": bool(exact)}


def row_walk_leg(args):
    """plan1 in a child process whose library reads RSX_KODAK_ROW_WALK at plan creation"""
    import subprocess
    env = dict(os.environ, RSX_KODAK_ROW_WALK="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only-plan1", "--steps",
                        str(args.steps), "--warmup", str(args.warmup)], env=env,
                       capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        return {"error": r.stderr[-400:]}
    return json.loads(r.stdout.strip().split("\n")[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--plans", default="1,8,64")
    ap.add_argument("--only-plan1", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    import kodak_files as F
    data, img, curve = make_frame()
    table = F.dither_table(curve)
    want = sha(F.apply_table(img.astype(np.int32), F.DITHER, curve))
    import torch
    from rawspeed_amd import capi
    ctx = capi.Context(0)
    if args.only_plan1:
        print(json.dumps(device_leg(ctx, torch, data, table, 1, want, args.steps, args.warmup)))
        return
    res = {"metric": "kodak_decode", "width": W, "height": H, "bps": BPS,
           "stream_bytes": len(data), "bits_per_pixel": round(len(data) * 8 / (W * H), 3),
           "segments": H * ((W + 255) // 256)}
    one, digest = host_build(data, table)
    exact = digest == want
    res["host_build"] = {"ms_1_frame_1_thread": one}
    for n in [int(v) for v in args.plans.split(",")]:
        leg = device_leg(ctx, torch, data, table, n, want, args.steps if n < 64 else 3, args.warmup)
        exact &= leg["bit_exact"]
        res["plan%d" % n] = leg
    res["copy_probe_ms"] = copy_probe(ctx, torch, data, args.steps)
    leg = host_pointer_leg(ctx, data, table, want)
    exact &= leg["bit_exact"]
    res["host_pointers"] = leg
    res["plan1_row_walk"] = row_walk_leg(args)
    try:
        with open(F.GOLDEN) as f:
            ref = json.load(f).get("reference_timing")
    except OSError:
        ref = None
    if ref and ref.get("stream_sha256") == hashlib.sha256(data).hexdigest():
        res["reference"] = ref
        res["reference_over_plan1_kernels"] = round(ref["ms_1_thread"] / res["plan1"]["kernel_ms"], 1)
    res["bit_exact"] = bool(exact)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
