"""SonyArw2Decompressor benchmark: ARW2 frames of 9600 x 6376 (the largest the reference
accepts, 61 MPix) and 6048 x 4024, decoded with the input and output resident in HBM (one plan
launch per step, the kernel's hipEvent time from rsx_plan_kernel_table) with the dithering
table and with none; a batched plan of 16 frames of 6048 x 4024; the host-pointer call next
to the time of its PCIe copies alone; and the unmodified reference (oracle/_ref, whole-file
decode) on one and on --threads host threads.  Every device output is compared bit for bit
with the model tests/arw2_files.py (pinned against the reference by
tests/test_arw2_model.py).  Prints one JSON line."""
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
    import arw2_files as A
    data = A.random_stream(np.random.default_rng([0xA2B, w, h, seed]), w, h)
    table = A.table_dither(A.decode_curve(A.REALISTIC_CURVE))
    return data, table


def alg_bytes(w, h, mode):
    # 1 byte in and 2 bytes out per pixel, plus the table the kernel reads
    return 3 * w * h + (8192 * 2 if mode else 0)


def device_leg(ctx, torch, frames, mode, steps, warmup):
    """frames: [(w, h, data, table)] decoded by one plan; returns the leg's dict"""
    import arw2_files as A
    from rawspeed_amd import abi
    jobs, keep, parts, layout = [], [], [], []
    in_off = out_off = 0
    for w, h, data, table in frames:
        d, arr = abi.sony_arw2_desc(mode, table if mode else None)
        keep.append(arr)
        j = abi.SonyArw2Job()
        j.desc = d
        j.in_offset, j.in_bytes, j.img_offset = in_off, w * h, out_off
        j.img = abi.Image(None, 2 * w, w, h, 1, 1)
        jobs.append(j)
        parts.append(data)
        layout.append((out_off, w, h))
        in_off += w * h
        out_off += 2 * w * h
    inp = torch.from_numpy(np.concatenate(parts)).cuda()
    out = torch.zeros(out_off, dtype=torch.uint8, device="cuda")
    plan = ctx.sony_arw2_plan(jobs)
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
    host = out.cpu().numpy()
    exact = rc == 0
    for (off, w, h), (_, _, data, tab) in list(zip(layout, frames))[:2]:
        _, img, _ = A.model_decode(data, w, h, mode, tab if mode else None)
        exact &= np.array_equal(host[off:off + 2 * w * h].view(np.uint16).reshape(h, w), img)
    px = sum(w * h for w, h, _, _ in frames)
    alg = sum(alg_bytes(w, h, mode) for w, h, _, _ in frames)
    return {"kernel_ms": round(kms, 4), "wall_ms_per_step": round(wall, 4),
            "gpix_s": round(px / (kms * 1e-3) / 1e9, 2), "alg_bytes": alg,
            "roofline_frac": round(alg / (kms * 1e-3) / PEAK_BPS, 4), "kernels": table,
            "runs": runs, "bit_exact": bool(exact)}


def host_leg(ctx, torch, w, h, data, table, reps=5):
    import arw2_files as A
    from oracle_lib import HostImage
    from rawspeed_amd import abi
    _, img, _ = A.model_decode(data, w, h, A.DITHER, table)
    best, exact = None, True
    for _ in range(reps):
        out = HostImage(w, h)
        t0 = time.perf_counter()
        st, _ = ctx.sony_arw2_decompress(abi.ARW2_TABLE_DITHER, table, data, out.view(), rows=False)
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
        exact &= st == 0 and np.array_equal(out.pixels(), img)
    # the PCIe copies alone: w * h bytes up and 2 w h bytes down, pageable host memory
    src = torch.from_numpy(np.asarray(data))
    dst = torch.empty(2 * w * h, dtype=torch.uint8)
    dev_in = torch.empty(w * h, dtype=torch.uint8, device="cuda")
    dev_out = torch.empty(2 * w * h, dtype=torch.uint8, device="cuda")
    up = down = None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev_in.copy_(src)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        dst.copy_(dev_out)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        up = (t1 - t0) * 1e3 if up is None else min(up, (t1 - t0) * 1e3)
        down = (t2 - t1) * 1e3 if down is None else min(down, (t2 - t1) * 1e3)
    return {"host_call_ms": round(best, 3), "pcie_up_ms": round(up, 3),
            "pcie_down_ms": round(down, 3)}, bool(exact)


def ref_leg(w, h, data, threads, reps=2):
    import arw2_files as A
    from oracle_lib import Ref
    if not Ref.available():
        return None, None
    ref = Ref()
    blob = A.arw2_file(w, h, data, A.REALISTIC_CURVE)
    _, img, _ = A.model_decode(data, w, h, A.DITHER, A.table_dither(A.decode_curve(A.REALISTIC_CURVE)))
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
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--batch", type=int, default=16)
    args = ap.parse_args()
    import torch
    from rawspeed_amd import abi, capi
    ctx = capi.Context(0)
    res = {"metric": "sony_arw2_decode", "threads": args.threads, "peak_bps": PEAK_BPS}
    exact = True
    frames = {}
    for name, (w, h) in (("max", (9600, 6376)), ("cfg2", (6048, 4024))):
        data, table = make_frame(w, h, 1)
        frames[name] = (w, h, data, table)
        for mname, mode in (("dither", abi.ARW2_TABLE_DITHER), ("none", abi.ARW2_TABLE_NONE)):
            leg = device_leg(ctx, torch, [frames[name]], mode, args.steps, args.warmup)
            exact &= leg["bit_exact"]
            res["%s_%s" % (name, mname)] = leg
    batch = [(6048, 4024) + make_frame(6048, 4024, 100 + k) for k in range(args.batch)]
    leg = device_leg(ctx, torch, batch, abi.ARW2_TABLE_DITHER, max(5, args.steps // 5),
                     args.warmup)
    exact &= leg["bit_exact"]
    res["batch%d_dither" % args.batch] = leg
    w, h, data, table = frames["max"]
    hl, hex_ = host_leg(ctx, torch, w, h, data, table)
    exact &= hex_
    r1, e1 = ref_leg(w, h, data, 1)
    rn, en = ref_leg(w, h, data, args.threads)
    exact &= e1 is not False and en is not False
    res["max_host"] = dict(hl, ref_1t_ms=r1, ref_threads_ms=rn)
    if rn:
        res["max_host"]["speedup_kernel_vs_ref_threads"] = round(
            rn / res["max_dither"]["kernel_ms"], 1)
    res["bit_exact"] = bool(exact)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
