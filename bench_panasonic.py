"""Panasonic RW2 V5 / V6 / V7 benchmark: frames of about 24 MP and about 47 MP in each of the five
layouts, decoded with the input and output resident in HBM (one plan launch per step, the
kernel's hipEvent time from rsx_plan_kernel_table, the images at the RawImage's pitch; --repeats timed rounds of --steps, the median
round and the spread between the rounds); a batched plan of 16 frames; and two yardsticks from
the same run: (a) the project's 14-bit rsx_unpack_plan on the same pixel count, (b) the
unmodified reference (oracle/_ref, whole-file decode) on one and on --threads host threads,
together with the host-pointer call next to the time of its PCIe copies alone.  Every device
output is compared bit for bit with the model tests/rw2_files.py (pinned against the reference
by tests/test_panasonic_model.py) before it is timed.  Prints one JSON line."""
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


def out_pitch(w):
    """the RawImage's own pitch (RawImageData::createData): rows on the 16-byte grid"""
    return (2 * w + 15) // 16 * 16

# (version, bps): the ~24 MP and the ~47 MP frame; widths divisible by the layout's n
SIZES = {
    (7, 14): ((6012, 4008), (8316, 5640)),
    (5, 14): ((6012, 4008), (8316, 5640)),
    (5, 12): ((6000, 4000), (8320, 5640)),
    (6, 14): ((6006, 4004), (8316, 5640)),
    (6, 12): ((6006, 4004), (8316, 5640)),
}


def make_frame(version, bps, w, h, seed):
    import rw2_files as P
    rng = np.random.default_rng([0x9A2, version, bps, w, h, seed])
    return P.random_stream(rng, version, bps, w, h, zero_half=version == 6 and seed % 2 == 1)


def alg_bytes(version, bps, w, h):
    # 16 bytes in and 2 n bytes out per packet
    import rw2_files as P
    n = P.PIXELS[(version, bps)]
    return (w * h // n) * (16 + 2 * n)


def timed_rounds(plan, run, steps, warmup, repeats):
    """[kernel ms per run] of `repeats` rounds of `steps` runs, and the kernel table of the last"""
    for _ in range(warmup):
        run()
    plan.results()
    plan.set_timing(True)
    rounds, table = [], None
    for _ in range(repeats):
        for _ in range(steps):
            run()
        rc, _, _ = plan.results()
        assert rc == 0, rc
        tab = plan.kernel_table()
        if tab:
            table = tab[0]
            rounds.append(sum(ms for _, ms in table))
            plan.kernel_time()  # (resets the totals)
        else:
            name, ms, _ = plan.kernel_time()
            table = [(name, ms)]
            rounds.append(ms)
    plan.set_timing(False)
    return rounds, table


def summary(rounds, px, alg):
    kms = float(np.median(rounds))
    return {"kernel_ms": round(kms, 4), "rounds_ms": [round(r, 4) for r in rounds],
            "spread": round((max(rounds) - min(rounds)) / kms, 4),
            "gpix_s": round(px / (kms * 1e-3) / 1e9, 2), "alg_bytes": alg,
            "roofline_frac": round(alg / (kms * 1e-3) / PEAK_BPS, 4)}


def device_leg(ctx, torch, frames, steps, warmup, repeats, check=2):
    """frames: [(version, bps, w, h, data)] decoded by one plan"""
    import rw2_files as P
    from rawspeed_amd import abi
    jobs, parts, layout = [], [], []
    in_off = out_off = 0
    for version, bps, w, h, data in frames:
        j = abi.PanasonicJob()
        j.desc = abi.PanasonicDesc(version, bps)
        j.in_offset, j.in_bytes, j.img_offset = in_off, data.size, out_off
        j.img = abi.Image(None, out_pitch(w), w, h, 1, 1)
        jobs.append(j)
        parts.append(data)
        layout.append((out_off, w, h))
        in_off += data.size
        out_off += (out_pitch(w) * h + 255) // 256 * 256
    inp = torch.from_numpy(np.concatenate(parts)).cuda()
    out = torch.zeros(out_off, dtype=torch.uint8, device="cuda")
    plan = ctx.panasonic_plan(jobs)
    s = torch.cuda.current_stream().cuda_stream
    # bit-exactness of what is about to be timed
    plan.run(inp.data_ptr(), out.data_ptr(), s)
    rc, st, cons = plan.results()
    host = out.cpu().numpy()
    exact = rc == 0 and cons == [f[4].size for f in frames]
    for (off, w, h), (version, bps, _, _, data) in list(zip(layout, frames))[:check]:
        img = P.model_decode(version, bps, w, h, data)
        got = host[off:off + out_pitch(w) * h].view(np.uint16).reshape(h, out_pitch(w) // 2)
        exact &= np.array_equal(got[:, :w], img)
    del host
    rounds, table = timed_rounds(plan, lambda: plan.run(inp.data_ptr(), out.data_ptr(), s),
                                 steps, warmup, repeats)
    plan.close()
    leg = summary(rounds, sum(f[2] * f[3] for f in frames), sum(alg_bytes(*f[:4]) for f in frames))
    leg.update(kernels=table, bit_exact=bool(exact))
    return leg


def unpack_leg(ctx, torch, w, h, steps, warmup, repeats):
    """yardstick (a): rsx_unpack_plan, 14 bits packed, the same pixel count and the same output
    pitch (1.75 bytes in and 2 bytes out per pixel)"""
    from rawspeed_amd import abi
    assert w % 4 == 0
    pitch = w * 14 // 8
    rng = np.random.default_rng([14, w, h])
    data = rng.integers(0, 256, size=pitch * h, dtype=np.uint8)
    j = abi.UnpackJob()
    j.desc = abi.UnpackDesc(0, 0, w, h, pitch, 14, abi.ORDER_MSB)
    j.in_offset, j.in_bytes, j.img_offset = 0, pitch * h, 0
    j.img = abi.Image(None, out_pitch(w), w, h, 1, 1)
    inp = torch.from_numpy(data).cuda()
    out = torch.zeros(out_pitch(w) * h, dtype=torch.uint8, device="cuda")
    plan = ctx.unpack_plan([j])
    s = torch.cuda.current_stream().cuda_stream
    rounds, table = timed_rounds(plan, lambda: plan.run(inp.data_ptr(), out.data_ptr(), s),
                                 steps, warmup, repeats)
    plan.close()
    leg = summary(rounds, w * h, pitch * h + 2 * w * h)
    leg["kernels"] = table
    return leg


def host_leg(ctx, torch, version, bps, w, h, data, reps=5):
    import rw2_files as P
    from oracle_lib import HostImage
    img = P.model_decode(version, bps, w, h, data)
    best, exact = None, True
    for _ in range(reps):
        out = HostImage(w, h)
        t0 = time.perf_counter()
        st = ctx.panasonic_decompress(version, bps, data, out.view())
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
        exact &= st == 0 and np.array_equal(out.pixels(), img)
    # the PCIe copies alone: the consumed bytes up and the image down, pageable host memory
    down_bytes = HostImage(w, 1).pitch * h
    src = torch.from_numpy(np.asarray(data))
    dst = torch.empty(down_bytes, dtype=torch.uint8)
    dev_in = torch.empty(data.size, dtype=torch.uint8, device="cuda")
    dev_out = torch.empty(down_bytes, dtype=torch.uint8, device="cuda")
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


def ref_leg(version, bps, w, h, data, threads, reps=2):
    """yardstick (b): "not measured" without oracle/_ref"""
    import rw2_files as P
    from oracle_lib import Ref
    if not Ref.available():
        return "not measured", None
    ref = Ref()
    blob = P.rw2_file(w, h, version, bps, data)
    img = P.model_decode(version, bps, w, h, data)
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
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--layouts", default="7/14,5/14,5/12,6/14,6/12")
    args = ap.parse_args()
    import torch
    from rawspeed_amd import capi
    ctx = capi.Context(0)
    res = {"metric": "panasonic_decode", "threads": args.threads, "peak_bps": PEAK_BPS,
           "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats}
    exact = True
    layouts = [tuple(int(x) for x in s.split("/")) for s in args.layouts.split(",")]
    for version, bps in layouts:
        for tag, (w, h) in zip(("24mp", "47mp"), SIZES[(version, bps)]):
            data = make_frame(version, bps, w, h, 1)
            name = "v%d_%d_%s" % (version, bps, tag)
            leg = device_leg(ctx, torch, [(version, bps, w, h, data)], args.steps, args.warmup,
                             args.repeats)
            leg.update(w=w, h=h)
            hl, hex_ = host_leg(ctx, torch, version, bps, w, h, data)
            leg.update(hl)
            r1, e1 = ref_leg(version, bps, w, h, data, 1)
            rn, en = ref_leg(version, bps, w, h, data, args.threads)
            leg.update(ref_1t_ms=r1, ref_threads_ms=rn)
            if isinstance(rn, float):
                leg["speedup_kernel_vs_ref_threads"] = round(rn / leg["kernel_ms"], 1)
            exact &= leg["bit_exact"] and hex_ and e1 is not False and en is not False
            if w % 4 == 0 and bps == 14 and version != 6:
                # yardstick (a): 3.75 bytes a pixel there, 3.78 here
                u = unpack_leg(ctx, torch, w, h, args.steps, args.warmup, args.repeats)
                leg["unpack14"] = u
                leg["vs_unpack14"] = round(leg["kernel_ms"] / u["kernel_ms"], 3)
            res[name] = leg
    # one plan of 16 frames, the layouts in turn
    batch = []
    for k in range(args.batch):
        version, bps = layouts[k % len(layouts)]
        w, h = SIZES[(version, bps)][0]
        batch.append((version, bps, w, h, make_frame(version, bps, w, h, 100 + k)))
    leg = device_leg(ctx, torch, batch, max(5, args.steps // 5), args.warmup, args.repeats)
    exact &= leg["bit_exact"]
    res["batch%d_24mp" % args.batch] = leg
    res["bit_exact"] = bool(exact)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
