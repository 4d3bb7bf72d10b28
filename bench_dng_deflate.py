"""Deflate DNG benchmark (compression 8, floating point): an 8192 x 5464 image of one component, a
smooth field plus noise, as binary16, binary24 and binary32 with predictor 34894, in tiles of
256 x 256 and 512 x 512, compressed at zlib levels 1 and 6.  Nobody has measured here what real
HDR DNGs look like: the compression ratio is reported next to every time.  Decoded with the input
and output resident in HBM (one plan run per step; both kernels' times from
rsx_plan_kernel_table) and through the host-pointer call; and, in the same run, libz's inflate of
the same tiles through Python's zlib (it releases the GIL) on one thread and on 16 -- the routine
the reference calls, without its delta and widening, so a lower bound on the reference's time.
Every decode is compared with the samples the tiles were written from.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 8192, 5464
PREDICTOR = 34894
THREADS = 16


def make_image(bps, w, h):
    import dng_deflate_files as D
    rng = np.random.default_rng([0xDF1, bps])
    x, y = np.arange(w, dtype=np.float32)[None, :], np.arange(h, dtype=np.float32)[:, None]
    f = 0.18 + 0.15 * np.sin(x / 611.0) * np.cos(y / 433.0) + 0.00002 * x
    f = (f + rng.normal(0, 0.002, (h, w)).astype(np.float32)).astype(np.float32)
    s = D.narrow_from_floats(f, bps)
    return s, D.widen(s, bps)


def make_tiles(samples, bps, tile, level, pool):
    import dng_deflate_files as D
    h, w = samples.shape
    geoms, raws = [], []
    for ty in range(0, h, tile):
        for tx in range(0, w, tile):
            th, tw = min(tile, h - ty), min(tile, w - tx)
            full = np.zeros((tile, tile), np.uint32)
            full[:th, :tw] = samples[ty:ty + th, tx:tx + tw]
            geoms.append((tile, tile, tx, ty, tw, th))
            raws.append(D.tile_bytes(full, bps, D.PREDICTORS[PREDICTOR]))
    datas = list(pool.map(lambda r: zlib.compress(r, level), raws))
    return geoms, datas, sum(len(r) for r in raws)


def device_leg(ctx, torch, bps, geoms, datas, want, steps, warmup):
    from rawspeed_amd import abi
    h, w = want.shape
    pitch = 4 * w
    jobs, off = [], 0
    for g, d in zip(geoms, datas):
        j = abi.DngDeflateJob()
        j.desc = abi.DngDeflateDesc(bps, PREDICTOR)
        j.tile_w, j.tile_h, j.off_x, j.off_y, j.width, j.height = g
        j.in_offset, j.in_bytes, j.img_offset = off, len(d), 0
        j.img = abi.Image(None, pitch, w, h, 1, 0)
        jobs.append(j)
        off += (len(d) + 15) // 16 * 16
    host_in = np.zeros(off + 64, np.uint8)
    for j, d in zip(jobs, datas):
        host_in[j.in_offset:j.in_offset + len(d)] = np.frombuffer(d, np.uint8)
    inp = torch.from_numpy(host_in).cuda()
    out = torch.zeros(pitch * h, dtype=torch.uint8, device="cuda")
    plan = ctx.dng_deflate_plan(jobs)
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
    ms = dict(table)
    exact = rc == 0 and np.array_equal(out.cpu().numpy().view(np.uint32).reshape(h, w), want)
    return ms.get("dfl_inflate_kernel", 0.0), ms.get("dfl_row_kernel", 0.0), wall, runs, bool(exact)


def host_leg(ctx, bps, geoms, datas, want, reps=2):
    from oracle_lib import HostImage
    h, w = want.shape
    best, exact = None, True
    for _ in range(reps):
        out = HostImage(w, h, 1, bpc=4)
        t0 = time.perf_counter()
        rc, _ = ctx.dng_decompress_deflate(bps, PREDICTOR, geoms, datas, out.view())
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
        exact &= rc == 0 and np.array_equal(out.u32()[:, :w], want)
    return best, bool(exact)


def libz_leg(datas, pool, reps=2):
    one = many = None
    for _ in range(reps):
        t0 = time.perf_counter()
        for d in datas:
            zlib.decompress(d)
        dt = (time.perf_counter() - t0) * 1e3
        one = dt if one is None else min(one, dt)
        t0 = time.perf_counter()
        list(pool.map(zlib.decompress, datas))
        dt = (time.perf_counter() - t0) * 1e3
        many = dt if many is None else min(many, dt)
    return one, many


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shrink", type=int, default=1, help="divide the image's sides (a quick look)")
    args = ap.parse_args()
    import torch
    from rawspeed_amd import capi
    ctx = capi.Context(0)
    w, h = W // args.shrink, H // args.shrink
    res = {"metric": "dng_deflate_decode", "image": [w, h], "predictor": PREDICTOR,
           "libz_threads": THREADS}
    exact = True
    with ThreadPoolExecutor(THREADS) as pool:
        for bps in (16, 24, 32):
            samples, want = make_image(bps, w, h)
            for tile in (256, 512):
                for level in (1, 6):
                    geoms, datas, inflated = make_tiles(samples, bps, tile, level, pool)
                    comp = sum(len(d) for d in datas)
                    inf_ms, row_ms, wall, runs, e1 = device_leg(ctx, torch, bps, geoms, datas, want,
                                                                args.steps, args.warmup)
                    host_ms, e2 = host_leg(ctx, bps, geoms, datas, want)
                    z1, z16 = libz_leg(datas, pool)
                    kms = inf_ms + row_ms
                    exact &= e1 and e2
                    res["b%d_t%d_l%d" % (bps, tile, level)] = {
                        "tiles": len(datas), "ratio": round(inflated / comp, 3),
                        "inflate_ms": round(inf_ms, 3), "row_ms": round(row_ms, 3),
                        "kernel_ms": round(kms, 3), "wall_ms_per_step": round(wall, 3),
                        "inflated_gb_s": round(inflated / (kms * 1e-3) / 1e9, 3),
                        "gpix_s": round(w * h / (kms * 1e-3) / 1e9, 3),
                        "host_call_ms": round(host_ms, 2), "libz_1t_ms": round(z1, 1),
                        "libz_%dt_ms" % THREADS: round(z16, 1),
                        "kernel_vs_libz_%dt" % THREADS: round(z16 / kms, 2), "runs": runs,
                        "bit_exact": bool(e1 and e2)}
    res["bit_exact"] = bool(exact)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
