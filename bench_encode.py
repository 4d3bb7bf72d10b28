"""Writer benchmark (rsx_encode_pack.hip, rsx_encode_ljpeg.hip; include/rsx.h section 7).

  python bench_encode.py [--steps K] [--warmup W] [--small]

  pack    cfg 2's shape (8192 x 5464, 14-bit MSB) and cfg 1's (4096 x 3072, 12-bit LSB): the
          hipEvent time of encode_pack_kernel from a plan of one image, next to the bare copy probe
          over the same bytes in the same run (rsx_probe_stream_copy: 16-byte loads of the image,
          16-byte stores of the stream), and the unpack kernel of the same shape against its probe.
          Every timed launch takes the next buffers of a ring several times the last-level cache.
          --pmc-leg runs cfg 2's launches alone (scripts/pmc_encode_pack.sh collects counters).
  ljpeg   cfg 3's image (6720 x 4480, 2 components) as one job and the four 4096 x 2732 tiles of
          cfg 4 as one plan, under the Nikon tree and under the tables made from the histogram:
          kernel time per pass, bits per pixel, the host-pointer call, and in the same run
          rsx_synth_ljpeg_encode_scan on one host thread, the host build of the core on 1 and on 16
          threads over the tiles, and the decode of the same stream.
Every device result is compared with the host build's bytes.  One JSON line on stdout; --out FILE
writes it as well."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def best_of(fn, reps):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best


def timed_plan(plan, src, dst, stream, steps, warmup):
    """src, dst: a pointer each, or a list of pointers the runs take in turn"""
    srcs = src if isinstance(src, list) else [src]
    dsts = dst if isinstance(dst, list) else [dst]
    for i in range(warmup):
        plan.run(srcs[i % len(srcs)], dsts[i % len(dsts)], stream)
    plan.results()
    plan.set_timing(True)
    for i in range(steps):
        plan.run(srcs[i % len(srcs)], dsts[i % len(dsts)], stream)
    plan.results()
    table, runs = plan.kernel_table()
    return {k: round(v, 4) for k, v in table}, runs


LAST_LEVEL_CACHE = 256 << 20


def pack_leg(ctx, torch, F, abi, synth, w, h, bps, order, steps, warmup, pmc=False):
    """Timed runs take their buffers from a ring of copies that together are several times the
    last-level cache, so that no run finds its bytes there from the run before; the probes rotate
    over the same ring, one launch a call."""
    px = synth.uniform(w * h, bps, 5).reshape(h, w)
    img = F.Img(px)
    pitch = w * bps // 8
    d = F.pack_desc(0, w, h, pitch, bps, order)
    st, want, written, _ = F.host_pack(d, img, guard=0)
    moved = img.buf.size + written
    ring = max(2, -(-3 * LAST_LEVEL_CACHE // moved))
    s = torch.cuda.current_stream().cuda_stream
    dimgs = [torch.from_numpy(img.buf).cuda() for _ in range(ring)]
    douts = [torch.zeros(written + 64, dtype=torch.uint8, device="cuda") for _ in range(ring)]
    backs = [torch.zeros(img.buf.size + 64, dtype=torch.uint8, device="cuda") for _ in range(ring)]
    ip, op, bp = ([t.data_ptr() for t in ts] for ts in (dimgs, douts, backs))
    plan = ctx.encode_pack_plan([abi.encode_pack_job(d, 0, 0, written, w, h, 1, img.pitch)])
    uplan = ctx.unpack_plan([abi.UnpackJob(d, 0, written, 0, abi.Image(None, img.pitch, w, h, 1, 1))])
    for k in range(ring):
        plan.run(ip[k], op[k], s)
    exact = plan.results()[0] == 0 and all(np.array_equal(t[:written].cpu().numpy(), want) for t in douts)
    if pmc:  # a few launches of both kernels for a counter run; nothing is timed
        for k in range(ring):
            uplan.run(op[k], bp[k], s)
        uplan.results()
        return {"bit_exact": bool(exact), "launches_each": ring}
    ms, runs = timed_plan(plan, ip, op, s, steps, warmup)
    plan.close()
    # the reader of the same shape: the stream in, the image out
    uplan.set_timing(True)
    for i in range(warmup + steps):
        uplan.run(op[i % ring], bp[i % ring], s)
    uplan.results()
    name, ums, n = uplan.kernel_time()
    exact &= all(np.array_equal(t[:img.buf.size].cpu().numpy().view(np.uint16).reshape(h, w), px)
                 for t in backs)
    # the probes write: they go from the images to the `backs` and from the streams to the `backs`
    probe = np.mean([ctx.probe_stream_copy(ip[i % ring], img.buf.size, bp[(i + 1) % ring], written, s, 1)
                     for i in range(warmup + steps)][warmup:])
    uprobe = np.mean([ctx.probe_stream_copy(op[i % ring], written, bp[(i + 1) % ring], img.buf.size, s, 1)
                      for i in range(warmup + steps)][warmup:])
    call_out = np.empty(written, np.uint8)
    call = best_of(lambda: ctx.encode_pack_u16(d, img.view(), call_out.ctypes.data, written), 5)
    k = ms["encode_pack_kernel"]
    return {"width": w, "height": h, "bits": bps, "order": F.ORDER_NAMES[order],
            "bytes_moved": int(moved), "ring_of_buffers": ring, "ring_bytes": int(ring * moved),
            "pack_kernel_ms": k, "pack_gb_s": round(moved / k / 1e6, 1),
            "probe_ms": round(float(probe), 4), "pack_share_of_probe": round(float(probe) / k, 3),
            "unpack_kernel_ms": round(ums, 4), "unpack_gb_s": round(moved / ums / 1e6, 1),
            "unpack_probe_ms": round(float(uprobe), 4),
            "unpack_share_of_probe": round(float(uprobe) / ums, 3),
            "pack_over_unpack": round(k / ums, 2), "host_pointer_call_ms": round(call, 2),
            "runs": runs, "bit_exact": bool(exact)}


def ljpeg_leg(ctx, torch, F, abi, synth, capi, W, H, tiles, n_comp, steps, warmup, host_threads):
    """the image as `tiles` (x, y, w, h in samples of the n_comp-interleaved row) jobs of one plan"""
    px = synth.sensor_image(W, H, 14, 3)
    img = F.Img(px)
    init = [1 << 13] * n_comp
    s = torch.cuda.current_stream().cuda_stream
    dimg = torch.from_numpy(img.buf).cuda()
    res = {"width": W, "height": H, "tiles": len(tiles), "n_comp": n_comp}

    def descs(tables, index):
        return [F.ljpeg_desc(t, img, n_comp, tables, index, init, None) for t in tiles]

    st, hist = ctx.encode_ljpeg_histogram(
        F.ljpeg_desc((0, 0, W, H), img, n_comp, [F.NIKON14], [0] * n_comp, init, None),
        img.view(dimg.data_ptr()))
    # (one table a component for every tile: a tile's first column may hold a category the image's
    # histogram lacks, so the absent ones get a count of 1)
    own = [F.table_of(capi.encode_huff_from_histogram(hist[c], abi.ENCODE_TABLE_ALL_CATEGORIES)[1])
           for c in range(n_comp)]
    for label, tables, index in (("nikon_tree", [F.NIKON14], [0] * n_comp),
                                 ("histogram_tables", own, list(range(n_comp)))):
        ds = descs(tables, index)
        bounds = [capi.encode_ljpeg_bound(d, img.view()) for d in ds]
        offs = np.concatenate([[0], np.cumsum([(b + 255) // 256 * 256 for b in bounds])])
        dout = torch.zeros(int(offs[-1]) + 64, dtype=torch.uint8, device="cuda")
        jobs = [abi.encode_ljpeg_job(d, F.TAIL_JPEG, 0, int(offs[k]), bounds[k], img.dim_x,
                                     img.dim_y, 1, img.pitch) for k, d in enumerate(ds)]
        plan = ctx.encode_ljpeg_plan(jobs)
        plan.run(dimg.data_ptr(), dout.data_ptr(), s)
        rc, sts, cons = plan.results()
        results = [plan.result(k)[1] for k in range(len(jobs))]
        # the host build of the core on 1 and on `host_threads` threads over the tiles
        outs = [np.empty(b, np.uint8) for b in bounds]

        def host_one(k):
            r = abi.EncodeResult()
            v = img.view()
            F.host().rsx_encode_host_ljpeg(C.byref(ds[k]), C.byref(v), F.TAIL_JPEG,
                                           outs[k].ctypes.data, bounds[k], C.byref(r), None)
            return int(r.bytes)
        t0 = time.perf_counter()
        host_bytes = [host_one(k) for k in range(len(ds))]
        host1 = (time.perf_counter() - t0) * 1e3
        with ThreadPoolExecutor(host_threads) as ex:
            t0 = time.perf_counter()
            list(ex.map(host_one, range(len(ds))))
            hostn = (time.perf_counter() - t0) * 1e3
        back = dout.cpu().numpy()
        exact = rc == 0 and cons == host_bytes and all(
            np.array_equal(back[int(offs[k]):int(offs[k]) + host_bytes[k]], outs[k][:host_bytes[k]])
            for k in range(len(ds)))
        ms, runs = timed_plan(plan, dimg.data_ptr(), dout.data_ptr(), s, steps, warmup)
        plan.close()
        leg = {"kernels_ms": ms, "kernels_total_ms": round(sum(ms.values()), 4), "runs": runs,
               "bits_per_pixel": round(sum(int(r.symbol_bits) for r in results) / (W * H), 4),
               "entropy_bytes": int(sum(host_bytes)),
               "host_core_1_thread_ms": round(host1, 1),
               "host_core_%d_threads_over_tiles_ms" % host_threads: round(hostn, 1),
               "bit_exact": bool(exact)}
        if label == "nikon_tree":
            # the test writer on one thread, the host-pointer call, and the decode of the stream
            x, y, w, h = tiles[0]
            t0 = time.perf_counter()
            synth.ljpeg_encode_scan(px[y:y + h, x:x + w], n_comp, init, [F.NIKON14] * n_comp)
            leg["synth_encode_scan_first_tile_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            out = np.empty(bounds[0], np.uint8)
            leg["host_pointer_call_first_tile_ms"] = round(best_of(
                lambda: ctx.encode_ljpeg(ds[0], img.view(), F.TAIL_JPEG, out.ctypes.data, bounds[0]), 3), 2)
            ljobs, dec = [], torch.zeros(img.buf.size, dtype=torch.uint8, device="cuda")
            stream = torch.zeros(int(offs[-1]) + 64, dtype=torch.uint8, device="cuda")
            for k, d in enumerate(ds):
                n = host_bytes[k]
                stream[int(offs[k]):int(offs[k]) + n] = torch.from_numpy(outs[k][:n]).cuda()
                stream[int(offs[k]) + n:int(offs[k]) + n + 2] = torch.tensor([0xFF, 0xD9], dtype=torch.uint8)
                ljobs.append(abi.LJpegJob(d, int(offs[k]), n + 18, 0,
                                          abi.Image(None, img.pitch, img.dim_x, img.dim_y, 1, 1)))
            dplan = ctx.ljpeg_plan(ljobs)
            dplan.run(stream.data_ptr(), dec.data_ptr(), s)
            drc = dplan.results()[0]
            dms, _ = timed_plan(dplan, stream.data_ptr(), dec.data_ptr(), s, steps, warmup)
            dplan.close()
            leg["decode_kernels_total_ms"] = round(sum(dms.values()), 4)
            leg["decode_gives_the_image"] = bool(drc == 0 and np.array_equal(
                dec.cpu().numpy().view(np.uint16).reshape(H, img.pitch // 2)[:, :W], px))
        res[label] = leg
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="small shapes (a quick check of the script)")
    ap.add_argument("--pmc-leg", action="store_true",
                    help="cfg 2's pack and unpack launches alone, untimed (for a counter run)")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import encode_files as F
    from rawspeed_amd import abi, capi, synth
    ctx = capi.Context(0)
    res = {"metric": "encode", "steps": a.steps, "warmup": a.warmup}
    if a.pmc_leg:
        res["pack_cfg2_8192x5464_14bit_msb"] = pack_leg(ctx, torch, F, abi, synth, 8192, 5464, 14,
                                                        abi.ORDER_MSB, a.steps, a.warmup, pmc=True)
    elif a.small:
        res["pack_cfg2"] = pack_leg(ctx, torch, F, abi, synth, 1024, 64, 14, abi.ORDER_MSB, a.steps, a.warmup)
        res["ljpeg_cfg3"] = ljpeg_leg(ctx, torch, F, abi, synth, capi, 512, 64, [(0, 0, 512, 64)], 2,
                                      a.steps, a.warmup, 16)
    else:
        res["pack_cfg2_8192x5464_14bit_msb"] = pack_leg(ctx, torch, F, abi, synth, 8192, 5464, 14,
                                                        abi.ORDER_MSB, a.steps, a.warmup)
        res["pack_cfg1_4096x3072_12bit_lsb"] = pack_leg(ctx, torch, F, abi, synth, 4096, 3072, 12,
                                                        abi.ORDER_LSB, a.steps, a.warmup)
        res["ljpeg_cfg3_6720x4480"] = ljpeg_leg(ctx, torch, F, abi, synth, capi, 6720, 4480,
                                                [(0, 0, 6720, 4480)], 2, a.steps, a.warmup, 16)
        tiles = [(x, y, 4096, 2732) for y in (0, 2732) for x in (0, 4096)]
        res["ljpeg_cfg4_4_tiles_8192x5464"] = ljpeg_leg(ctx, torch, F, abi, synth, capi, 8192, 5464,
                                                        tiles, 2, a.steps, a.warmup, 16)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
