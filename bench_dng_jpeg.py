"""Lossy-JPEG DNG tile benchmark (include/rsx.h section 4e): an 8192 x 5464 frame of baseline JPEG
tiles at quality 90.  Not part of bench.py.  One JSON line:

  frames   rgb_256_444, rgb_256_420, rgb_512_444, rgb_512_420 (cpp 3, tiles of 256 x 256 and
           512 x 512) and grey_256 (cpp 1); rgb_256_420_restart has a restart interval of one MCU
           row (plan creation with the marker scan, and 16 times the segments)
  device   per frame: the tiles resident in HBM, hipEvent times of the two kernels
           (rsx_plan_kernel_table, medians over the repeats), the plan's creation, and next to them
           rsx_probe_stream_copy over the output's bytes in the same run
  host     rsx_dng_decompress_jpeg through host pointers for rgb_256_420 (wall clock, best of 3)
  cpu      libjpeg-turbo through Pillow on the same tiles in the same run: one thread, and a pool
           of 16 threads

Every frame's device output is compared with Pillow's decode of its tiles.  Where Pillow does not
import, the frames are the committed 4:2:0 tile of 256 x 256 (tests/golden/
dng_jpeg_bench_tile.json) repeated, compared with its recorded hash, and "source" says so; the
other frame kinds and the cpu leg are then left out.  --record FILE keeps the line.  Nothing is
promised in advance (profiles/dng_jpeg/README.md)."""
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
FRAMES = [("rgb_256_420", 256, 3, 2, 0), ("rgb_256_444", 256, 3, 0, 0), ("rgb_512_420", 512, 3, 2, 0),
          ("rgb_512_444", 512, 3, 0, 0), ("grey_256", 256, 1, None, 0), ("rgb_256_420_restart", 256, 3, 2, 16)]


def picture(cpp):
    rng = np.random.default_rng(3)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    base = 128 + 60 * np.sin(x / 37.0) * np.cos(y / 53.0) + 0.004 * (x - y)
    if cpp == 1:
        return np.clip(base + rng.normal(0, 5, (H, W)).astype(np.float32), 0, 255).astype(np.uint8)
    px = base[..., None] + rng.normal(0, 5, (H, W, 3)).astype(np.float32) + \
        np.stack([20 * np.cos(y / 41.0), 25 * np.sin(x / 29.0), 0 * x], axis=-1)
    return np.clip(px, 0, 255).astype(np.uint8)


def tiles_of(img, tile, cpp, sub, restart, Image):
    out = []
    for ty in range(0, H, tile):
        for tx in range(0, W, tile):
            # (a DNG's edge tiles are whole tiles: padded by repeating the edge)
            part = img[ty:ty + tile, tx:tx + tile]
            ph, pw = tile - part.shape[0], tile - part.shape[1]
            if ph or pw:
                part = np.pad(part, ((0, ph), (0, pw)) + (((0, 0),) if cpp == 3 else ()), mode="edge")
            kw = {} if cpp == 1 else {"subsampling": sub}
            if restart:
                kw["restart_marker_blocks"] = restart
            b = io.BytesIO()
            Image.fromarray(part, "L" if cpp == 1 else "RGB").save(b, "JPEG", quality=90, **kw)
            out.append((b.getvalue(), tx, ty))
    return out


def pillow_frame(tiles, cpp, Image, threads):
    want = np.zeros((H, W * cpp), np.uint16)

    def one(t):
        s, tx, ty = t
        a = np.asarray(Image.open(io.BytesIO(s)))
        a = a.reshape(a.shape[0], -1)
        h, w = min(H - ty, a.shape[0]), min(W - tx, a.shape[1] // cpp)
        want[ty:ty + h, cpp * tx:cpp * (tx + w)] = a[:h, :cpp * w]
    t0 = time.perf_counter()
    if threads == 1:
        for t in tiles:
            one(t)
    else:
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(one, tiles))
    return (time.perf_counter() - t0) * 1e3, want


def device_leg(ctx, torch, abi, tiles, cpp, args):
    s = torch.cuda.current_stream().cuda_stream
    pitch = 2 * cpp * W
    t0 = time.perf_counter()
    job, keep, packed = abi.dng_jpeg_job([t[0] for t in tiles], [(t[1], t[2]) for t in tiles],
                                         abi.Image(None, pitch, W, H, cpp, 0))
    pack_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    plan = ctx.dng_jpeg_plan([job])
    create_ms = (time.perf_counter() - t0) * 1e3
    inp = torch.from_numpy(packed).cuda()
    out = torch.zeros(pitch * H, dtype=torch.uint8, device="cuda")
    plan.run(inp.data_ptr(), out.data_ptr(), s)
    rc, st, _ = plan.results()
    got = out.cpu().numpy().view(np.uint16).reshape(H, W * cpp)
    per = {}
    for _ in range(args.repeats):
        plan.set_timing(True)
        for _ in range(args.steps):
            plan.run(inp.data_ptr(), out.data_ptr(), s)
        plan.results()
        table, runs = plan.kernel_table()
        plan.set_timing(False)
        for name, ms in table:
            per.setdefault(name, []).append(ms)
    plan.close()
    kernels = {k: round(float(np.median(v)), 4) for k, v in per.items()}
    total = sum(kernels.values())
    other = torch.empty_like(out)
    probe = [ctx.probe_stream_copy(out.data_ptr(), out.numel(), other.data_ptr(), out.numel(), s,
                                   reps=args.steps) for _ in range(args.repeats)]
    res = {"tiles": len(tiles), "stream_bytes": int(sum(len(t[0]) for t in tiles)), "status": rc,
           "kernels_ms": kernels, "all_kernels_ms": round(total, 4),
           "kernels_ms_all": {k: [round(x, 4) for x in v] for k, v in per.items()},
           "gpix_s": round(W * H / (total * 1e-3) / 1e9, 3) if total else None,
           "plan_create_ms": round(create_ms, 2), "pack_ms": round(pack_ms, 2),
           "copy_probe_ms": round(float(np.median(probe)), 4)}
    return res, got


def host_leg(ctx, tiles, cpp, want, reps=3):
    from oracle_lib import HostImage
    best, ok = None, True
    for _ in range(reps):
        img = HostImage(W, H, cpp, is_cfa=False)
        t0 = time.perf_counter()
        rc, st = ctx.dng_decompress_jpeg([t[0] for t in tiles], [(t[1], t[2]) for t in tiles], img.view())
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
        ok &= rc == 0 and np.array_equal(img.pixels(), want)
    return {"dng_decompress_jpeg_host_pointers_ms": round(best, 2), "bit_exact": bool(ok)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--frames", default=",".join(f[0] for f in FRAMES))
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--record")
    args = ap.parse_args()
    import torch
    from rawspeed_amd import abi, capi
    import dng_jpeg_files as J
    try:
        from PIL import Image, features
        source = "Pillow %s, libjpeg-turbo %s" % (Image.__version__,
                                                  features.version("libjpeg_turbo") or "not reported")
    except ImportError:
        Image, source = None, "the committed 4:2:0 tile of 256 x 256 repeated (Pillow does not import)"
    ctx = capi.Context(0)
    res = {"metric": "dng_lossy_jpeg", "frame": [W, H], "quality": 90, "source": source, "frames": {}}
    exact = True
    pictures = {}
    for name, tile, cpp, sub, restart in FRAMES:
        if name not in args.frames.split(","):
            continue
        if Image is None:
            if name != "rgb_256_420":
                continue
            c = J.bench_tile()
            tiles = [(c["stream"], tx, ty) for ty in range(0, H, 256) for tx in range(0, W, 256)]
            st, frame = J.model_decode(c["stream"], 3)
            assert st == J.OK and J.sha(frame) == c["sha256"]
            want = np.tile(frame, (-(-H // 256), W // 256))[:H]
            cpu = None
        else:
            if cpp not in pictures:
                pictures[cpp] = picture(cpp)
            tiles = tiles_of(pictures[cpp], tile, cpp, sub, restart, Image)
            t1, want = pillow_frame(tiles, cpp, Image, 1)
            t16, want16 = pillow_frame(tiles, cpp, Image, 16)
            assert np.array_equal(want, want16)
            cpu = {"pillow_1_thread_ms": round(t1, 1), "pillow_16_threads_ms": round(t16, 1),
                   "gpix_s_1_thread": round(W * H / (t1 * 1e-3) / 1e9, 3),
                   "gpix_s_16_threads": round(W * H / (t16 * 1e-3) / 1e9, 3)}
        dev, got = device_leg(ctx, torch, abi, tiles, cpp, args)
        dev["bit_exact"] = bool(dev["status"] == 0 and np.array_equal(got, want))
        exact &= dev["bit_exact"]
        entry = {"tile": tile, "cpp": cpp, "device": dev}
        if cpu:
            entry["cpu"] = cpu
            entry["device_over_pillow_16_threads"] = round(cpu["pillow_16_threads_ms"] / dev["all_kernels_ms"], 2)
            entry["device_over_pillow_1_thread"] = round(cpu["pillow_1_thread_ms"] / dev["all_kernels_ms"], 2)
        if name == "rgb_256_420" and not args.no_host:
            entry["host"] = host_leg(ctx, tiles, cpp, want)
            exact &= entry["host"]["bit_exact"]
        res["frames"][name] = entry
        del got, want
    res["bit_exact"] = bool(exact)
    line = json.dumps(res)
    print(line)
    if args.record:
        with open(args.record, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
