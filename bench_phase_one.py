"""PhaseOneDecompressor benchmark: IIQ "L" frames of 11976 x 8854 (the largest the reference
accepts) and 8192 x 5464, decoded with the input and output resident in HBM (one plan launch
per step, the kernel's hipEvent time from rsx_plan_kernel_table), through the host-pointer
call, and by the unmodified reference (oracle/_ref, whole-file decode) on one and on all host
threads.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_BPS = 8.0e12  # MI355X HBM3E


def make_frame(w, h, seed):
    import iiq_files as I
    rng = np.random.default_rng([0xBE7C, w, h, seed])
    img = I.sample_image(rng, w, h)
    rows = I.encode(img, seed, (0.0, 0.0, 0.0))  # (a plain encoder: shortest lengths)
    blob = I.iiq_file(rows, w, rng, gap_max=0)
    raw, strips, _, _ = I.iiq_strips(blob)
    return img, blob, raw, strips


def device_leg(ctx, torch, img, raw, strips, steps, warmup):
    from rawspeed_amd import abi
    h, w = img.shape
    pitch = (2 * w + 15) // 16 * 16
    arr = abi.phase_one_strips(strips)
    j = abi.PhaseOneJob()
    j.strips, j.n_strips = arr, len(strips)
    j.in_offset, j.in_bytes, j.img_offset = 0, len(raw), 0
    j.img = abi.Image(None, pitch, w, h, 1, 1)
    inp = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).cuda()
    out = torch.zeros(pitch * h, dtype=torch.uint8, device="cuda")
    plan = ctx.phase_one_plan([j])
    s = torch.cuda.current_stream().cuda_stream
    for _ in range(warmup):
        plan.run(inp.data_ptr(), out.data_ptr(), s)
    plan.results()
    plan.set_timing(True)
    t0 = time.perf_counter()
    for _ in range(steps):
        plan.run(inp.data_ptr(), out.data_ptr(), s)
    rc, st, _ = plan.results()
    wall = (time.perf_counter() - t0) / steps * 1e3
    table, runs = plan.kernel_table()
    plan.close()
    kms = sum(ms for _, ms in table)
    got = out.cpu().numpy().view(np.uint16).reshape(h, pitch // 2)[:, :w]
    exact = rc == 0 and np.array_equal(got, img)
    alg = len(raw) + 2 * w * h
    return {"kernel_ms": round(kms, 4), "wall_ms_per_step": round(wall, 4),
            "gpix_s": round(w * h / (kms * 1e-3) / 1e9, 2), "alg_bytes": alg,
            "roofline_frac": round(alg / (kms * 1e-3) / PEAK_BPS, 4), "kernels": table,
            "runs": runs, "bit_exact": bool(exact)}


def host_leg(ctx, img, raw, strips, reps=3):
    from oracle_lib import HostImage
    h, w = img.shape
    best, exact = None, True
    a = np.frombuffer(raw, np.uint8)
    for _ in range(reps):
        out = HostImage(w, h)
        t0 = time.perf_counter()
        st, _ = ctx.phase_one_decompress(a, strips, out.view())
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
        exact &= st == 0 and np.array_equal(out.pixels(), img)
    return round(best, 3), bool(exact)


def ref_leg(blob, img, threads, reps=2):
    from oracle_lib import Ref
    if not Ref.available():
        return None, None
    ref = Ref()
    h, w = img.shape
    best, exact = None, True
    for _ in range(reps):
        t0 = time.perf_counter()
        st, dec = ref.decode_file(blob, threads=threads)
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
        exact &= st == 0 and np.array_equal(dec.u16()[:h, :w], img)
        dec.close()
    return round(best, 2), bool(exact)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    args = ap.parse_args()
    import torch
    from rawspeed_amd import capi
    ctx = capi.Context(0)
    res = {"metric": "phase_one_decode", "threads": args.threads}
    exact = True
    for name, (w, h) in (("L", (11976, 8854)), ("cfg2", (8192, 5464))):
        img, blob, raw, strips = make_frame(w, h, 1)
        leg = device_leg(ctx, torch, img, raw, strips, args.steps, args.warmup)
        exact &= leg["bit_exact"]
        res[name] = leg
        if name == "L":
            hms, hex_ = host_leg(ctx, img, raw, strips)
            r1, e1 = ref_leg(blob, img, 1)
            rn, en = ref_leg(blob, img, args.threads)
            exact &= hex_ and e1 is not False and en is not False
            res["L"].update({"host_call_ms": hms, "ref_1t_ms": r1, "ref_all_ms": rn})
            if rn:
                res["L"]["speedup_vs_ref_all"] = round(rn / leg["kernel_ms"], 1)
    res["bit_exact"] = bool(exact)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
