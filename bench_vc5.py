"""VC5Decompressor benchmark: GoPro-sized frames of 4000 x 3000 (the HERO sensor, 12 MPix) decoded
with the tile's bytes and the image resident in HBM -- one frame and --batch frames in one plan,
every kernel's hipEvent time from rsx_plan_kernel_table, the share of the band decode in the total,
and the parse rounds per window the band decode needed --, the wall time of the host-pointer call
(plan creation and both copies included) and, where oracle/_ref is built, the
unmodified reference's whole-file decode of the same frame on 1 and 16 threads in the same run.
A frame is made by the test writer (tests/vc5_files.py) from a forward Haar transform of a smooth
field plus noise, quantised so that the bands have camera-like zero runs.  The device image is
compared bit for bit with the reference's where that is built, else with the host build of the
same core (rawspeed_amd/librsx_vc5_host.so) followed by the numpy model of wavelets and merge.
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 4000, 3000
WHITE = 16383


def make_frame(seed, w=W, h=H):
    """a vc5_files.Tile: per channel a smooth field plus noise, three Haar steps, the details
    divided by the band's quantisation and rounded to values the book can carry"""
    import vc5_files as V
    rng = np.random.default_rng([0xBE7C, seed])
    t = V.Tile(w, h, 0, WHITE)
    t.prescale = [[0, 0, 2]] * 4
    d = t.dims()
    vals = V.book_values()
    near = np.zeros(1200, np.int64)  # |v| -> the nearest value of the book
    near[:] = vals[np.abs(np.arange(1200)[:, None] - vals[None, :]).argmin(1)]
    yy, xx = np.mgrid[0:d[0][1], 0:d[0][0]]
    for c in range(4):
        f = 900 + 500 * np.sin(xx / (180.0 + 40 * c)) * np.cos(yy / (140.0 + 30 * c)) + 0.05 * xx
        plane = f + rng.normal(0, 10.0, f.shape)
        for level in (1, 2, 3):
            wk, hk = d[level]
            p = np.pad(plane, ((0, 2 * hk - plane.shape[0]), (0, 2 * wk - plane.shape[1])), mode="edge")
            a, b, cc, dd = p[0::2, 0::2], p[0::2, 1::2], p[1::2, 0::2], p[1::2, 1::2]
            plane = (a + b + cc + dd) / 4
            for band, detail in ((1, (a - b + cc - dd) / 2), (2, (a + b - cc - dd) / 2), (3, (a - b - cc + dd) / 2)):
                quant = (12, 10, 8)[level - 1]
                q = np.rint(detail / quant).astype(np.int64)
                q = np.sign(q) * near[np.minimum(np.abs(q), 1199)]
                t.set_band(c, level, band, quant=quant, stream=V.encode_values_fast(q))
        t.set_lowpass(c, np.clip(np.rint(plane), 0, 4095).astype(np.int64) if c == 0
                      else np.full(plane.shape, 2048, np.int64), 12)
    return t


def host_core_image(tile, data, bands):
    """the image by the host build of the core (bands) and the numpy model (wavelets, merge)"""
    import vc5_files as V
    from rawspeed_amd import abi, build
    L = C.CDLL(build.build_vc5_host()[0])
    L.rsx_vc5_host_band.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_int32,
                                    C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    rows = V.book()
    codes = (abi.Vc5Code * len(rows))()
    for k, (size, bits, count, value) in enumerate(rows):
        codes[k].bits, codes[k].size, codes[k].count, codes[k].value = bits, size, count, value
    d = tile.dims()
    planes = []
    for c in range(4):
        co = {(3, 0): V.model_lowpass(data[bands[c][0][0]:][:bands[c][0][1]], bands[c][0][3], *d[3])}
        for s in range(1, 10):
            off, n, quant, _ = bands[c][s]
            level = 3 - (s - 1) // 3
            w, h = d[level]
            chunk = np.ascontiguousarray(data[off:off + n])
            out = np.zeros(w * h, np.int16)
            st = L.rsx_vc5_host_band(codes, len(rows), chunk.ctypes.data, chunk.size, quant, w * h,
                                     out.ctypes.data, 256, None, None)
            assert st == 0, (c, s, st)
            co[(level, 1 + (s - 1) % 3)] = out.reshape(h, w)
        for level in (3, 2, 1):
            co[(level - 1, 0)] = V.model_level(co[(level, 0)], co[(level, 1)], co[(level, 2)],
                                               co[(level, 3)], tile.prescale[c][level - 1], level == 1)
        planes.append(co[(0, 0)])
    return V.model_merge(planes, tile.w, tile.h, tile.phase, V.log_table(tile.white))


def device_leg(ctx, torch, tiles, images, steps, warmup, repeats):
    """tiles: the frames decoded by one plan (images: the expected image of each, or None)"""
    import vc5_files as V
    from rawspeed_amd import abi
    jobs, keep, parts, layout = [], [], [], []
    in_off = out_off = 0
    for t in tiles:
        data, bands = t.vc5_block()
        d, kp = V.abi_desc(t, bands)
        keep.append(kp)
        j = abi.Vc5Job()
        j.desc = d
        j.in_offset, j.in_bytes, j.img_offset = in_off, data.size, out_off
        j.img = abi.Image(None, 2 * t.w, t.w, t.h, 1, 1)
        jobs.append(j)
        parts.append(data)
        layout.append(out_off)
        in_off += data.size
        out_off += 2 * t.w * t.h
    inp = torch.from_numpy(np.concatenate(parts)).cuda()
    out = torch.zeros(out_off, dtype=torch.uint8, device="cuda")
    plan = ctx.vc5_plan(jobs)
    s = torch.cuda.current_stream().cuda_stream
    for _ in range(warmup):
        plan.run(inp.data_ptr(), out.data_ptr(), s)
    rc, _, _ = plan.results()
    host = out.cpu().numpy()
    exact = rc == 0
    for off, t, img in zip(layout, tiles, images):
        if img is not None:
            exact &= np.array_equal(host[off:off + 2 * t.w * t.h].view(np.uint16).reshape(t.h, t.w), img)
    st, win, rnd = plan.bands(0)
    tables, walls = [], []
    for _ in range(repeats):
        plan.set_timing(True)
        t0 = time.perf_counter()
        for _ in range(steps):
            plan.run(inp.data_ptr(), out.data_ptr(), s)
        plan.results()
        walls.append((time.perf_counter() - t0) / steps * 1e3)
        table_ms, runs = plan.kernel_table()
        plan.set_timing(False)
        tables.append(table_ms)
    plan.close()
    names = [n for n, _ in tables[0]]
    per = {n: float(np.median([dict(t)[n] for t in tables])) for n in names}
    total = sum(per.values())
    px = sum(t.w * t.h for t in tiles)
    hp = win[:, 1:]
    return {"kernel_ms": {n: round(v, 4) for n, v in per.items()}, "kernel_ms_total": round(total, 4),
            "kernel_ms_total_all": [round(sum(ms for _, ms in t), 4) for t in tables],
            "band_share": round(per["vc5_band_kernel"] / total, 3),
            "wall_ms_per_step": round(float(np.median(walls)), 4),
            "gpix_s": round(px / (total * 1e-3) / 1e9, 3),
            "in_mbytes": round(in_off / 1e6, 2),
            "band_mbytes_s": round(in_off / (per["vc5_band_kernel"] * 1e-3) / 1e6, 1),
            "windows_job0": int(hp.sum()), "rounds_per_window_job0": round(float(rnd[:, 1:].sum()) / max(1, int(hp.sum())), 3),
            "rounds_per_window_max_band_job0": round(float((rnd[:, 1:] / np.maximum(hp, 1)).max()), 3),
            "bit_exact": bool(exact)}


def host_call_leg(ctx, tile, img, calls=4):
    """rsx_vc5_decompress with host pointers, wall clock: the first call makes the plan (scratch,
    the book's table, the descriptors) and every call copies the tile up and the image down --
    none of which the kernel times above hold"""
    import vc5_files as V
    from oracle_lib import HostImage
    data, bands = tile.vc5_block()
    d, keep = V.abi_desc(tile, bands)
    out = HostImage(tile.w, tile.h)
    ms, ok = [], True
    for _ in range(calls):
        t0 = time.perf_counter()
        st = ctx.vc5_decompress(d, data, out.view())
        ms.append((time.perf_counter() - t0) * 1e3)
        ok &= st == 0
    return {"first_ms": round(ms[0], 3), "repeat_ms": round(float(np.median(ms[1:])), 3),
            "bit_exact": bool(ok and np.array_equal(out.pixels(), img))}


def ref_leg(tile, threads, reps=2):
    from oracle_lib import Ref
    if not Ref.available():
        return None, None
    ref = Ref()
    blob, _, _ = tile.dng()
    best, img = None, None
    for _ in range(reps):
        t0 = time.perf_counter()
        st, dec = ref.decode_file(blob, threads=threads)
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
        assert st == 0 and not dec.errors(), ref.last_error()
        img = dec.u16()[:tile.h, :tile.w].copy()
        dec.close()
    return round(best, 2), img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--width", type=int, default=W)
    ap.add_argument("--height", type=int, default=H)
    args = ap.parse_args()
    import torch
    from rawspeed_amd import capi
    ctx = capi.Context(0)
    res = {"metric": "vc5_decode", "frame": [args.width, args.height]}
    frames = [make_frame(k, args.width, args.height) for k in range(2)]
    r1, img = ref_leg(frames[0], 1)
    r16, img16 = ref_leg(frames[0], 16)
    exact = True
    if img is None:
        data, bands = frames[0].vc5_block()
        img = host_core_image(frames[0], data, bands)
        res["checked_against"] = "host core + model"
    else:
        exact &= np.array_equal(img, img16)
        res["checked_against"] = "reference"
    res["one_frame"] = device_leg(ctx, torch, [frames[0]], [img], args.steps, args.warmup, args.repeats)
    batch = [frames[k % 2] for k in range(args.batch)]
    res["batch%d" % args.batch] = device_leg(ctx, torch, batch, [img] + [None] * (args.batch - 1),
                                             max(3, args.steps // 2), args.warmup, args.repeats)
    res["host_call"] = host_call_leg(ctx, frames[0], img)
    exact &= res["one_frame"]["bit_exact"] and res["batch%d" % args.batch]["bit_exact"]
    exact &= res["host_call"]["bit_exact"]
    res["ref_1t_ms"], res["ref_16t_ms"] = r1, r16
    if r1:
        res["speedup_vs_ref_1t"] = round(r1 / res["one_frame"]["kernel_ms_total"], 2)
        res["speedup_vs_ref_16t"] = round(r16 / res["one_frame"]["kernel_ms_total"], 2)
    res["bit_exact"] = bool(exact)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
