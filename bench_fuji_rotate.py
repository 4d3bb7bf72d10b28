"""SuperCCD rotation benchmark (RafDecoder::applyCorrections, rsx_fuji_rotate.hip).  Two
camera-sized frames, seeded noise: 4000 x 3000 under the normal layout (5500 x 5499 out) and
4352 x 1446 under the alt layout (3622 x 3621 out), source and destination resident in HBM:
  plan              a plan of the one frame, the kernel's hipEvent time from rsx_plan_kernel_table,
                    once per kernel: the direct gather and the one staged through LDS
                    (RSX_FUJI_ROTATE_KERNEL=direct|lds, each in a child process; "default" is
                    what a plan made without the variable runs)
  copy_probe        rsx_probe_stream_copy over the crop's bytes in and the rotated image's bytes
                    out, in the same run: the floor of any rotation
  host_pointers     rsx_raf_rotate through host pointers (the rows go up, about twice the bytes
                    come back)
  host_build        librsx_fuji_rotate_host.so on one thread: the reference's loop restated (clear,
                    then scatter); the reference itself cannot be run for this path here
Every leg's output is hashed against the model's before it is timed.  Prints one JSON line and,
with --out, writes it."""
import argparse
import ctypes as C
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

FRAMES = {"normal_4000x3000": (4000, 3000, 0), "alt_4352x1446": (4352, 1446, 1)}
CROP = (4, 2)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def make(W, H):
    import fuji_rotate_files as F
    src = F.source(W + CROP[0] + 4, H + CROP[1] + 2, 5)
    pitch = (2 * src.shape[1] + 15) // 16 * 16
    return src, F.padded(src, pitch), pitch


def plan_leg(ctx, torch, name, steps, warmup):
    import fuji_rotate_files as F
    from rawspeed_amd import abi
    W, H, alt = FRAMES[name]
    src, sbytes, sp = make(W, H)
    want = sha(F.rotate_scatter(src, CROP[0], CROP[1], W, H, alt))
    R = F.rotated_size(W, H, alt)[0]
    pitch = (2 * R + 15) // 16 * 16
    j = abi.FujiRotateJob()
    j.desc = abi.fuji_rotate_desc(CROP, (W, H), alt)
    j.in_ = abi.Image(None, sp, src.shape[1], src.shape[0], 1, 1)
    j.img = abi.Image(None, pitch, R, R - 1, 1, 1)
    inp = torch.from_numpy(sbytes).cuda()
    out = torch.full((pitch * (R - 1),), 0xA5, dtype=torch.uint8, device="cuda")
    plan = ctx.fuji_rotate_plan([j])
    s = torch.cuda.current_stream().cuda_stream
    plan.run(inp.data_ptr(), out.data_ptr(), s)
    rc = plan.results()[0]
    got = out.cpu().numpy().reshape(R - 1, pitch)[:, :2 * R]
    exact = rc == 0 and sha(got) == want
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
    (kname, ms), = table
    crop_bytes, out_bytes = 2 * W * H, 2 * R * (R - 1)
    probe = [ctx.probe_stream_copy(inp.data_ptr(), crop_bytes, out.data_ptr(), out_bytes, s,
                                   reps=max(steps, 5)) for _ in range(3)]
    return {"kernel": kname, "kernel_ms": round(ms, 4), "wall_ms_per_step": round(wall, 3),
            "runs": runs, "in_bytes": crop_bytes, "out_bytes": out_bytes,
            "gb_s": round((crop_bytes + out_bytes) / (ms * 1e-3) / 1e9, 1),
            "copy_probe_ms": round(float(np.median(probe)), 4), "bit_exact": bool(exact)}


def host_pointer_leg(ctx, name, reps=3):
    import fuji_rotate_files as F
    from oracle_lib import HostImage
    from rawspeed_amd import abi
    W, H, alt = FRAMES[name]
    src, sbytes, sp = make(W, H)
    want = sha(F.rotate_scatter(src, CROP[0], CROP[1], W, H, alt))
    R = F.rotated_size(W, H, alt)[0]
    best, exact = None, True
    for _ in range(reps):
        out = HostImage(R, R - 1)
        t0 = time.perf_counter()
        st = ctx.fuji_rotate(abi.fuji_rotate_desc(CROP, (W, H), alt),
                             F.image_of(sbytes, sp, src.shape[1], src.shape[0]), out.view())
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
        exact &= st == 0 and sha(out.pixels()) == want
    return {"host_call_ms": round(best, 2), "bit_exact": bool(exact)}


def host_build_leg(name, reps=3):
    import fuji_rotate_files as F
    from rawspeed_amd import abi
    W, H, alt = FRAMES[name]
    src, sbytes, sp = make(W, H)
    want = sha(F.rotate_scatter(src, CROP[0], CROP[1], W, H, alt))
    R = F.rotated_size(W, H, alt)[0]
    d = abi.fuji_rotate_desc(CROP, (W, H), alt)
    out = {}
    for which in ("scatter", "gather"):
        fn = getattr(F.host_lib(), "rsx_fuji_rotate_host_" + which)
        best = None
        for _ in range(reps):
            dbuf = np.full(2 * R * (R - 1), 0xA5, np.uint8)
            t0 = time.perf_counter()
            st = fn(C.byref(d), C.byref(F.image_of(sbytes, sp, src.shape[1], src.shape[0])),
                    C.byref(F.image_of(dbuf, 2 * R, R, R - 1)))
            dt = (time.perf_counter() - t0) * 1e3
            assert st == 0 and sha(dbuf) == want
            best = dt if best is None else min(best, dt)
        out[which + "_ms_1_thread"] = round(best, 2)
    return out


def child(which, args):
    env = dict(os.environ)
    env.pop("RSX_FUJI_ROTATE_KERNEL", None)
    if which != "default":
        env["RSX_FUJI_ROTATE_KERNEL"] = which
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only-plans", "--steps",
                        str(args.steps), "--warmup", str(args.warmup)], env=env,
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        return {"error": r.stderr[-400:]}
    return json.loads(r.stdout.strip().split("\n")[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only-plans", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.only_plans:
        import torch
        from rawspeed_amd import capi
        ctx = capi.Context(0)
        print(json.dumps({n: plan_leg(ctx, torch, n, args.steps, args.warmup) for n in FRAMES}))
        return
    res = {"metric": "fuji_rotate", "crop": list(CROP)}
    for which in ("default", "direct", "lds"):
        res["plan_" + which] = child(which, args)
    from rawspeed_amd import capi
    ctx = capi.Context(0)
    res["host_pointers"] = {n: host_pointer_leg(ctx, n) for n in FRAMES}
    res["host_build"] = {n: host_build_leg(n) for n in FRAMES}
    plans = [res["plan_" + which] for which in ("default", "direct", "lds")]
    exact = all("error" not in p and all(leg["bit_exact"] for leg in p.values()) for p in plans)
    exact &= all(leg["bit_exact"] for leg in res["host_pointers"].values())
    res["bit_exact"] = bool(exact)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
