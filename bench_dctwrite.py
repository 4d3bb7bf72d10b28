"""Baseline-DCT JPEG tile writer benchmark (include/rsx.h section 7e): an 8192 x 5464 RGB frame
written as JPEG tiles at quality 90.  Not part of bench.py.  One JSON line:

  frames   rgb_256_420, rgb_256_444, rgb_512_420, rgb_512_444 (704 tiles of 256 x 256, 176 tiles of
           512 x 512; edge tiles are whole tiles), each with no restart interval and, as *_restart,
           with an interval of one MCU row
  device   per frame: the image resident in HBM, one plan of all tiles; hipEvent times of the nine
           kernels (rsx_plan_kernel_table, medians over the repeats), the plan's creation, and next
           to them rsx_probe_stream_copy reading the image's bytes and writing the streams' bytes
           in the same run
  host     rsx_dctwrite through host pointers for rgb_256_420 (wall clock, best of 3)
  cpu      libjpeg-turbo through Pillow encoding the same tiles in the same run: one thread, and a
           pool of 16 threads

Every tile's device stream is compared with Pillow's, byte for byte.  Where Pillow does not
import, the streams are compared with the host build's for a sample of the tiles, "source" says
so, and the cpu leg is left out.  --record FILE keeps the line.  Nothing is promised in advance
(profiles/dctwrite/README.md)."""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 8192, 5464
SAMPLING = {0: (1, 1), 2: (2, 2)}
FRAMES = [(name + suffix, tile, sub, (tile // (8 * SAMPLING[sub][0])) if suffix else 0)
          for name, tile, sub in (("rgb_256_420", 256, 2), ("rgb_256_444", 256, 0),
                                  ("rgb_512_420", 512, 2), ("rgb_512_444", 512, 0))
          for suffix in ("", "_restart")]


def picture(w, h):
    rng = np.random.default_rng(3)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    base = 128 + 60 * np.sin(x / 37.0) * np.cos(y / 53.0) + 0.004 * (x - y)
    px = base[..., None] + rng.normal(0, 5, (h, w, 3)).astype(np.float32) + \
        np.stack([20 * np.cos(y / 41.0), 25 * np.sin(x / 29.0), 0 * x], axis=-1)
    return np.clip(px, 0, 255).astype(np.uint8)


def pillow_tiles(img, tile, sub, restart, Image, threads):
    h, w = img.shape[:2]
    where = [(tx, ty) for ty in range(0, h, tile) for tx in range(0, w, tile)]

    def one(at):
        tx, ty = at
        part = img[ty:ty + tile, tx:tx + tile]
        ph, pw = tile - part.shape[0], tile - part.shape[1]
        if ph or pw:  # (a DNG's edge tiles are whole tiles: padded by repeating the edge)
            part = np.pad(part, ((0, ph), (0, pw), (0, 0)), mode="edge")
        kw = {"restart_marker_blocks": restart} if restart else {}
        b = io.BytesIO()
        Image.fromarray(part, "RGB").save(b, "JPEG", quality=90, subsampling=sub, **kw)
        return b.getvalue()
    t0 = time.perf_counter()
    if threads == 1:
        out = [one(at) for at in where]
    else:
        with ThreadPoolExecutor(threads) as ex:
            out = list(ex.map(one, where))
    return (time.perf_counter() - t0) * 1e3, out


def jobs_of(abi, w, h, tile, sub, restart, tables, cap):
    hs, vs = SAMPLING[sub]
    jobs, at = [], 0
    for ty in range(0, h, tile):
        for tx in range(0, w, tile):
            d = abi.dctwrite_desc(tx, ty, tile, tile, 3, hs, vs, tables[0], tables[1], restart)
            jobs.append(abi.dctwrite_job(d, 0, at, cap, w, h, 3, 2 * 3 * w))
            at += cap
    return jobs, at


def device_leg(ctx, torch, abi, dimg, w, h, tile, sub, restart, tables, args):
    s = torch.cuda.current_stream().cuda_stream
    cap = tile * tile * 3  # (a byte a sample: far above what quality 90 writes; the status says so)
    jobs, total = jobs_of(abi, w, h, tile, sub, restart, tables, cap)
    t0 = time.perf_counter()
    plan = ctx.dctwrite_plan(jobs)
    create_ms = (time.perf_counter() - t0) * 1e3
    out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    plan.run(dimg.data_ptr(), out.data_ptr(), s)
    rc, st, cons = plan.results()
    back = out.cpu().numpy()
    streams = [back[k * cap:k * cap + n].tobytes() for k, n in enumerate(cons)]
    per = {}
    for _ in range(args.repeats):
        plan.set_timing(True)
        for _ in range(args.steps):
            plan.run(dimg.data_ptr(), out.data_ptr(), s)
        plan.results()
        table, runs = plan.kernel_table()
        plan.set_timing(False)
        for name, ms in table:
            per.setdefault(name, []).append(ms)
    plan.close()
    kernels = {k: round(float(np.median(v)), 4) for k, v in per.items()}
    all_ms = sum(kernels.values())
    n_bytes = int(sum(cons))
    packed = torch.empty(n_bytes + 64, dtype=torch.uint8, device="cuda")
    probe = [ctx.probe_stream_copy(dimg.data_ptr(), dimg.numel() * 2, packed.data_ptr(), n_bytes, s,
                                   reps=args.steps) for _ in range(args.repeats)]
    res = {"tiles": len(jobs), "stream_bytes": n_bytes, "status": rc, "kernels_ms": kernels,
           "all_kernels_ms": round(all_ms, 4),
           "kernels_ms_all": {k: [round(x, 4) for x in v] for k, v in per.items()},
           "gpix_s": round(w * h / (all_ms * 1e-3) / 1e9, 3) if all_ms else None,
           "plan_create_ms": round(create_ms, 2), "copy_probe_ms": round(float(np.median(probe)), 4)}
    return res, streams


def host_leg(ctx, abi, img16, w, h, tile, sub, tables, want, reps=3):
    hs, vs = SAMPLING[sub]
    cap = tile * tile * 3
    view = abi.Image(img16.ctypes.data, 2 * 3 * w, w, h, 3, 0)
    where = [(tx, ty) for ty in range(0, h, tile) for tx in range(0, w, tile)]
    outs = np.zeros((len(where), cap), np.uint8)
    tiles = [abi.DctWriteTile(abi.dctwrite_desc(tx, ty, tile, tile, 3, hs, vs, tables[0], tables[1]),
                              outs[k].ctypes.data, cap) for k, (tx, ty) in enumerate(where)]
    best, ok = None, True
    for _ in range(reps):
        t0 = time.perf_counter()
        rc, res = ctx.dctwrite(tiles, view)
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
        ok &= rc == 0 and all(outs[k, :int(r.bytes)].tobytes() == want[k] for k, r in enumerate(res))
    return {"dctwrite_host_pointers_ms": round(best, 2), "bit_exact": bool(ok)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--frames", default=",".join(f[0] for f in FRAMES))
    ap.add_argument("--small", action="store_true", help="a 1024 x 600 frame: a rehearsal, not a number")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--record")
    args = ap.parse_args()
    import torch
    from rawspeed_amd import abi, capi
    import dctwrite_files as D
    try:
        from PIL import Image, features
        import PIL
        source = "Pillow %s, libjpeg-turbo %s" % (PIL.__version__,
                                                  features.version("libjpeg_turbo") or "not reported")
    except ImportError:
        Image, source = None, "the host build of the writer's core on a sample of tiles (Pillow does not import)"
    w, h = (1024, 600) if args.small else (W, H)
    ctx = capi.Context(0)
    st, lu, ch = capi.dctwrite_quality_tables(90)
    tables = (lu, ch)
    img = picture(w, h)
    img16 = np.ascontiguousarray(img.astype(np.uint16))
    dimg = torch.from_numpy(img16.reshape(-1)).cuda()
    res = {"metric": "dctwrite", "frame": [w, h], "quality": 90, "source": source, "frames": {}}
    exact = True
    for name, tile, sub, restart in FRAMES:
        if name not in args.frames.split(","):
            continue
        dev, streams = device_leg(ctx, torch, abi, dimg, w, h, tile, sub, restart, tables, args)
        entry = {"tile": tile, "subsampling": sub, "restart_interval": restart, "device": dev}
        if Image is not None:
            t1, want = pillow_tiles(img, tile, sub, restart, Image, 1)
            t16, want16 = pillow_tiles(img, tile, sub, restart, Image, 16)
            assert want == want16
            dev["bit_exact"] = bool(dev["status"] == 0 and streams == want)
            entry["cpu"] = {"pillow_1_thread_ms": round(t1, 1), "pillow_16_threads_ms": round(t16, 1),
                            "gpix_s_1_thread": round(w * h / (t1 * 1e-3) / 1e9, 3),
                            "gpix_s_16_threads": round(w * h / (t16 * 1e-3) / 1e9, 3)}
            entry["device_over_pillow_16_threads"] = round(t16 / dev["all_kernels_ms"], 2)
            entry["device_over_pillow_1_thread"] = round(t1 / dev["all_kernels_ms"], 2)
        else:
            hs, vs = SAMPLING[sub]
            where = [(tx, ty) for ty in range(0, h, tile) for tx in range(0, w, tile)]
            ok = dev["status"] == 0
            for k in range(0, len(where), max(1, len(where) // 8)):
                d = abi.dctwrite_desc(*where[k], tile, tile, 3, hs, vs, lu, ch, restart)
                hst, got, _, _ = D.host_encode(d, D.Img(img, 3))
                ok &= hst == 0 and got.tobytes() == streams[k]
            dev["bit_exact"] = bool(ok)
            want = streams
        exact &= dev["bit_exact"]
        if name == "rgb_256_420" and not args.no_host:
            entry["host"] = host_leg(ctx, abi, img16, w, h, tile, sub, tables, want)
            exact &= entry["host"]["bit_exact"]
        res["frames"][name] = entry
    res["bit_exact"] = bool(exact)
    line = json.dumps(res)
    print(line)
    if args.record:
        with open(args.record, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
