"""NefDecoder::DecodeNikonSNef benchmark: sNEF frames of 3680 x 2456 (the largest the reference
accepts, 9 MPix; 3 bytes in and 6 bytes out per pixel) decoded with the input and output resident
in HBM -- one frame and --batch frames in one plan, the kernel's hipEvent time from
rsx_plan_kernel_table -- next to rsx_probe_stream_copy over the same byte counts in the same run;
the host-pointer call next to the time of its PCIe copies alone; and, where oracle/_ref is built,
the unmodified reference's whole-file decode of the same frame (its loop is single-threaded by
construction).  Every device output is compared bit for bit with the model tests/snef_files.py
(pinned against the reference by tests/test_snef_model.py).  Prints one JSON line."""
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
W, H = 3680, 2456
WB = ((2, 1), (3, 2))  # inv_wb 512 and 682


def make_frame(seed):
    return np.random.default_rng([0x5EF0, seed]).integers(0, 256, 3 * W * H, dtype=np.uint8)


_MODEL = {}


def model(data, table, inv_wb):
    """the model's image of a frame (computed once per frame: it takes seconds)"""
    import snef_files as S
    if id(data) not in _MODEL:
        _MODEL[id(data)] = S.model_decode(data, W, H, inv_wb[0], inv_wb[1], table)
    return _MODEL[id(data)]


def device_leg(ctx, torch, frames, table, inv_wb, steps, warmup, repeats):
    """frames: the inputs decoded by one plan; returns the leg's dict"""
    from rawspeed_amd import abi
    jobs, keep, layout = [], [], []
    in_off = out_off = 0
    for data in frames:
        d, arr = abi.nikon_snef_desc(inv_wb[0], inv_wb[1], table)
        keep.append(arr)
        j = abi.NikonSnefJob()
        j.desc = d
        j.in_offset, j.in_bytes, j.img_offset = in_off, 3 * W * H, out_off
        j.img = abi.Image(None, 6 * W, W, H, 3, 0)
        jobs.append(j)
        layout.append(out_off)
        in_off += 3 * W * H
        out_off += 6 * W * H
    inp = torch.from_numpy(np.concatenate(frames)).cuda()
    out = torch.zeros(out_off, dtype=torch.uint8, device="cuda")
    plan = ctx.nikon_snef_plan(jobs)
    s = torch.cuda.current_stream().cuda_stream
    for _ in range(warmup):
        plan.run(inp.data_ptr(), out.data_ptr(), s)
    rc, _, _ = plan.results()
    host = out.cpu().numpy()
    exact = rc == 0
    for off, data in list(zip(layout, frames))[:2]:
        img = model(data, table, inv_wb)
        exact &= np.array_equal(host[off:off + 6 * W * H].view(np.uint16).reshape(H, 3 * W), img)
    # kernel and copy probe take turns, `repeats` times, so that both see the same machine
    kernel, probe, walls = [], [], []
    for _ in range(repeats):
        plan.set_timing(True)
        t0 = time.perf_counter()
        for _ in range(steps):
            plan.run(inp.data_ptr(), out.data_ptr(), s)
        plan.results()
        walls.append((time.perf_counter() - t0) / steps * 1e3)
        table_ms, runs = plan.kernel_table()
        plan.set_timing(False)
        kernel.append(sum(ms for _, ms in table_ms))
        probe.append(ctx.probe_stream_copy(inp.data_ptr(), in_off, out.data_ptr(), out_off, s, reps=steps))
    plan.close()
    kms, pms = float(np.median(kernel)), float(np.median(probe))
    px = len(frames) * W * H
    alg = 9 * px + 16384  # 3 bytes in and 6 bytes out per pixel, plus the table
    return {"kernel_ms": round(kms, 4), "kernel_ms_all": [round(x, 4) for x in kernel],
            "copy_probe_ms": round(pms, 4), "copy_probe_ms_all": [round(x, 4) for x in probe],
            "kernel_frac_of_probe": round(pms / kms, 3),
            "wall_ms_per_step": round(float(np.median(walls)), 4),
            "gpix_s": round(px / (kms * 1e-3) / 1e9, 2), "alg_bytes": alg,
            "tb_s": round(alg / (kms * 1e-3) / 1e12, 3),
            "roofline_frac": round(alg / (kms * 1e-3) / PEAK_BPS, 4), "bit_exact": bool(exact)}


def host_leg(ctx, torch, data, table, inv_wb, reps=5):
    from oracle_lib import HostImage
    img = model(data, table, inv_wb)
    best, exact = None, True
    for _ in range(reps):
        out = HostImage(W, H, cpp=3, is_cfa=False)
        t0 = time.perf_counter()
        st = ctx.nikon_snef_decompress(inv_wb, table, data, out.view())
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
        exact &= st == 0 and np.array_equal(out.pixels(), img)
    # the PCIe copies alone: 3 w h bytes up and 6 w h bytes down, pageable host memory
    src = torch.from_numpy(np.asarray(data))
    dst = torch.empty(6 * W * H, dtype=torch.uint8)
    dev_in = torch.empty(3 * W * H, dtype=torch.uint8, device="cuda")
    dev_out = torch.empty(6 * W * H, dtype=torch.uint8, device="cuda")
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


def ref_leg(data, table, inv_wb, reps=2):
    import snef_files as S
    from oracle_lib import Ref
    if not Ref.available():
        return None, None
    ref = Ref()
    blob = S.snef_file(W, H, data, *WB)
    img = model(data, table, inv_wb)
    best, exact = None, True
    for _ in range(reps):
        t0 = time.perf_counter()
        st, dec = ref.decode_file(blob)
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
        exact &= st == 0 and np.array_equal(dec.u16()[:H, :3 * W], img)
        dec.close()
    return round(best, 2), bool(exact)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    args = ap.parse_args()
    import torch
    import snef_files as S
    from rawspeed_amd import capi
    ctx = capi.Context(0)
    # the curve the reference agreed with (tests/golden/snef_ref.json): no libm in the way
    table = S.host_table(S.load_golden()[0])
    inv_wb = (S.inv_wb(WB[0]), S.inv_wb(WB[1]))
    res = {"metric": "nikon_snef_decode", "frame": [W, H], "peak_bps": PEAK_BPS}
    one = make_frame(1)
    res["one_frame"] = device_leg(ctx, torch, [one], table, inv_wb, args.steps, args.warmup, args.repeats)
    batch = [make_frame(100 + k) for k in range(args.batch)]
    res["batch%d" % args.batch] = device_leg(ctx, torch, batch, table, inv_wb, max(5, args.steps // 2),
                                             args.warmup, args.repeats)
    exact = res["one_frame"]["bit_exact"] and res["batch%d" % args.batch]["bit_exact"]
    hl, hex_ = host_leg(ctx, torch, one, table, inv_wb)
    exact &= hex_
    r1, e1 = ref_leg(one, table, inv_wb)
    exact &= e1 is not False
    res["host"] = dict(hl, ref_1t_ms=r1)
    if r1:
        res["host"]["speedup_kernel_vs_ref"] = round(r1 / res["one_frame"]["kernel_ms"], 1)
        res["host"]["speedup_host_call_vs_ref"] = round(r1 / hl["host_call_ms"], 2)
    res["bit_exact"] = bool(exact)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
