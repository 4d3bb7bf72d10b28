"""F32 writer benchmark (rsx_fpwrite_pack.hip; include/rsx.h section 7d).

  python bench_fpwrite.py [--steps K] [--warmup W] [--small]

  pack  an 8192 x 5464 one-component F32 image that narrows exactly, packed at 16 / 24 / 32 bits
        (MSB): the hipEvent time of fpwrite_pack_kernel from a plan of one image, next to the bare
        copy probe over the same bytes in the same run (rsx_probe_stream_copy: 16-byte loads of the
        image, 16-byte stores of the stream), and the host-pointer call.  Every timed launch takes
        the next buffers of a ring several times the last-level cache.
  fit   rsx_fpwrite_fit over the same image as one window and as 256 x 256 windows, device-resident
        (the call's wall time, the same call over windows of one sample, whose difference
        estimates fpwrite_fit_kernel's own time, and a probe that only reads) and through a host
        pointer.
  deflate  the same image in 256 x 256 and 512 x 512 tiles at 16 / 24 / 32 bits (predictor 3),
        device-resident as one plan (hipEvent times per kernel) and through host pointers; next to
        them, in the same run, zlib.compress at levels 1 and 6 over the same tile bytes on 1 and on
        16 host threads (libz releases the interpreter lock), and the sizes.  A sample of the tiles
        is compared with the host build's streams and every stream's length with its bound.
Every device result is compared with the host build's.  One JSON line on stdout; --out FILE writes
it as well."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LAST_LEVEL_CACHE = 256 << 20


def best_of(fn, reps):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best


def pack_leg(ctx, torch, F, abi, px, bps, steps, warmup):
    h, w = px.shape
    img = F.Img32(px)
    d = F.pack_desc(0, 0, w, h, w * bps // 8, bps, abi.ORDER_MSB)
    st, want, hr = F.host_pack(d, img, guard=0)
    written = int(hr.bytes_written)
    moved = img.buf.size + written
    ring = max(2, -(-3 * LAST_LEVEL_CACHE // moved))
    s = torch.cuda.current_stream().cuda_stream
    dimgs = [torch.from_numpy(img.buf).cuda() for _ in range(ring)]
    douts = [torch.zeros(written + 64, dtype=torch.uint8, device="cuda") for _ in range(ring)]
    ip, op = ([t.data_ptr() for t in ts] for ts in (dimgs, douts))
    plan = ctx.fpwrite_pack_plan([abi.fpwrite_pack_job(d, 0, 0, written, w, h, 1, img.pitch)])
    for k in range(ring):
        plan.run(ip[k], op[k], s)
    exact = st == 0 and plan.results()[0] == 0 and all(
        np.array_equal(t[:written].cpu().numpy(), want) for t in douts)
    for i in range(warmup):
        plan.run(ip[i % ring], op[i % ring], s)
    plan.results()
    plan.set_timing(True)
    for i in range(steps):
        plan.run(ip[i % ring], op[i % ring], s)
    plan.results()
    table, runs = plan.kernel_table()
    k = dict(table)["fpwrite_pack_kernel"]
    plan.close()
    probe = np.mean([ctx.probe_stream_copy(ip[i % ring], img.buf.size, op[(i + 1) % ring], written, s, 1)
                     for i in range(warmup + steps)][warmup:])
    call_out = np.empty(written, np.uint8)
    call = best_of(lambda: ctx.fpwrite_pack(d, img.view(), call_out.ctypes.data, written), 3)
    exact = exact and np.array_equal(call_out, want)
    return {"width": w, "height": h, "bits": bps, "bytes_moved": int(moved), "ring_of_buffers": ring,
            "pack_kernel_ms": round(k, 4), "pack_gb_s": round(moved / k / 1e6, 1),
            "probe_ms": round(float(probe), 4), "pack_share_of_probe": round(float(probe) / k, 3),
            "host_pointer_call_ms": round(call, 2), "runs": runs, "bit_exact": bool(exact)}


def fit_leg(ctx, torch, F, px, tile, steps):
    h, w = px.shape
    img = F.Img32(px)
    wins = [(0, 0, w, h)] if tile is None else [
        (x, y, min(tile, w - x), min(tile, h - y)) for y in range(0, h, tile) for x in range(0, w, tile)]
    dimg = torch.from_numpy(img.buf).cuda()
    st, got = ctx.fpwrite_fit(img.view(dimg.data_ptr()), wins)
    hst, want = F.host_fit(img, wins)
    dev = best_of(lambda: ctx.fpwrite_fit(img.view(dimg.data_ptr()), wins), steps)
    # the same call over as many windows of one sample: the plan, the uploads, the launch and the
    # copy back without the reading; the difference estimates the kernel's own time
    tiny = [(x, y, 1, 1) for x, y, _, _ in wins]
    over = best_of(lambda: ctx.fpwrite_fit(img.view(dimg.data_ptr()), tiny), steps)
    hostp = best_of(lambda: ctx.fpwrite_fit(img.view(), wins), 3)
    s = torch.cuda.current_stream().cuda_stream
    sink = torch.zeros(64, dtype=torch.uint8, device="cuda")
    probe = ctx.probe_stream_copy(dimg.data_ptr(), img.buf.size, sink.data_ptr(), 0, s, steps)
    return {"windows": len(wins), "window": tile or "image", "device_call_ms": round(dev, 3),
            "device_call_one_sample_windows_ms": round(over, 3),
            "kernel_estimate_ms": round(dev - over, 3),
            "read_probe_ms": round(float(probe), 4), "host_pointer_call_ms": round(hostp, 2),
            "host_core_one_thread_ms": round(best_of(lambda: F.host_fit(img, wins), 1), 1),
            "exact": bool(st == 0 == hst and got == want)}


def deflate_leg(ctx, torch, F, DF, abi, px, bps, tile, steps, warmup, threads=16):
    import zlib
    from concurrent.futures import ThreadPoolExecutor
    h, w = px.shape
    img = F.Img32(px)
    d = abi.DngDeflateDesc(bps, 3)
    geoms = [(tile, tile, x, y, min(tile, w - x), min(tile, h - y)) for y in range(0, h, tile)
             for x in range(0, w, tile)]
    bound = F.bound_model(tile * tile * bps // 8)
    slot = (bound + 255) // 256 * 256
    jobs = [abi.FpWriteDeflateJob(d, *g, 0, k * slot, bound, abi.Image(None, img.pitch, w, h, 1, 0))
            for k, g in enumerate(geoms)]
    s = torch.cuda.current_stream().cuda_stream
    dimg = torch.from_numpy(img.buf).cuda()
    dout = torch.zeros(len(geoms) * slot + 64, dtype=torch.uint8, device="cuda")
    plan = ctx.fpwrite_deflate_plan(jobs)
    plan.run(dimg.data_ptr(), dout.data_ptr(), s)
    rc, st, cons = plan.results()
    back = dout.cpu().numpy()
    exact = rc == 0 and all(c <= bound for c in cons)
    narrow = F.model_narrow(px, bps)[0]
    tiles_raw = []
    for k, g in enumerate(geoms):
        t = np.zeros((tile, tile), np.uint32)
        t[:g[5], :g[4]] = narrow[g[3]:g[3] + g[5], g[2]:g[2] + g[4]]
        tiles_raw.append(DF.tile_bytes(t, bps, 1))
    for k in range(0, len(geoms), max(1, len(geoms) // 8)):  # a sample against the host core, all of it
        hst, want, hr = F.host_deflate(d, geoms[k], img, guard=0)
        exact = exact and hst == 0 and hr.bytes == cons[k] and np.array_equal(
            back[k * slot:k * slot + cons[k]], want[:cons[k]])
        exact = exact and zlib.decompress(back[k * slot:k * slot + cons[k]].tobytes()) == tiles_raw[k]
    for i in range(warmup):
        plan.run(dimg.data_ptr(), dout.data_ptr(), s)
    plan.results()
    plan.set_timing(True)
    for i in range(steps):
        plan.run(dimg.data_ptr(), dout.data_ptr(), s)
    plan.results()
    table, runs = plan.kernel_table()
    plan.close()
    kernels = {k: round(v, 3) for k, v in table}
    outs = [np.empty(bound, np.uint8) for _ in geoms]
    tl = [F.deflate_tile(g, o.ctypes.data, bound) for g, o in zip(geoms, outs)]
    call = best_of(lambda: ctx.fpwrite_deflate(d, tl, img.view()), 2)
    res = {"bits": bps, "tile": tile, "tiles": len(geoms), "raw_bytes": sum(map(len, tiles_raw)),
           "stream_bytes": int(sum(cons)), "kernels_ms": kernels, "device_ms": round(sum(kernels.values()), 3),
           "host_pointer_call_ms": round(call, 2), "runs": runs, "exact": bool(exact)}
    for level in (1, 6):
        res["zlib%d_1_thread_ms" % level] = round(best_of(
            lambda: [zlib.compress(r, level) for r in tiles_raw], 1), 1)
        with ThreadPoolExecutor(threads) as ex:
            res["zlib%d_%d_threads_ms" % (level, threads)] = round(best_of(
                lambda: list(ex.map(lambda r: zlib.compress(r, level), tiles_raw)), 2), 1)
        res["zlib%d_bytes" % level] = sum(len(zlib.compress(r, level)) for r in tiles_raw)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="a 1024 x 683 image (a quick check)")
    ap.add_argument("--no-deflate", action="store_true", help="skip the deflate legs")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import fpwrite_files as F
    from rawspeed_amd import abi, capi
    ctx = capi.Context(0)
    w, h = (1024, 683) if a.small else (8192, 5464)
    res = {"bench": "fpwrite", "device": torch.cuda.get_device_name(0), "width": w, "height": h,
           "pack": [], "fit": [], "deflate": []}
    import dng_deflate_files as DF
    for bps in F.BPS:
        px = F.exact_samples("bench%d" % bps, bps, h, w)
        res["pack"].append(pack_leg(ctx, torch, F, abi, px, bps, a.steps, a.warmup))
        print("pack %d bits done" % bps, file=sys.stderr, flush=True)
        if bps == 24:
            for tile in (None, 256):
                res["fit"].append(fit_leg(ctx, torch, F, px, tile, a.steps))
        if not a.no_deflate:
            # an image that compresses: a smooth ramp with noise, narrowed exactly
            sm = F.model_widen(DF.random_samples(np.random.default_rng(bps), bps, h, w, "smooth"), bps)
            for tile in (256, 512):
                res["deflate"].append(deflate_leg(ctx, torch, F, DF, abi, sm, bps, tile,
                                                  max(2, a.steps // 5), 1))
                print("deflate %d bits, tiles of %d done" % (bps, tile), file=sys.stderr, flush=True)
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
