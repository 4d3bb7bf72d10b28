"""Lossy-DNG chain benchmark (include/rsx.h section 4f): rsx_dng_lossy_decompress against the
sequence of the four stand-alone host-pointer calls it replaces, on the image of
bench_dng_jpeg.py's host leg.  Not part of bench.py.  One JSON line:

  frame     8192 x 5464, cpp 3: the committed 4:2:0 tile of 256 x 256 (tests/golden/
            dng_jpeg_bench_tile.json) 704 times
  stages    a LinearizationTable of 256 entries, black 256 / white 16383 (no skip rule, the SSE2
            variant with dither), an OpcodeList2 of a MapTable and a ScalePerColumn over the image
  chained   rsx_dng_lossy_decompress: one upload of the tiles, one download of the image
  sequence  rsx_dng_decompress_jpeg, rsx_dng_post (the table), rsx_scale_black_white, rsx_dng_post
            (list 2): the tiles up and four images down, three images up
  memory    both through a pageable image and a page-locked one (rsx_host_alloc)

The two alternate in the same run, --reps times each; wall clock, the median and the best.  The
images of the two must be equal.  --record FILE keeps the line.  Nothing is promised in advance
(profiles/dng_lossy/README.md)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, CPP, TILE = 8192, 5464, 3, 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--record")
    args = ap.parse_args()
    from rawspeed_amd import abi, capi
    import dng_jpeg_files as J
    import dng_post_files as P
    c = J.bench_tile()
    streams = [c["stream"]] * ((W // TILE) * -(-H // TILE))
    offsets = [(tx, ty) for ty in range(0, H, TILE) for tx in range(0, W, TILE)]
    rng = np.random.default_rng(0x884C)
    table = np.sort(rng.integers(300, 16384, size=256)).astype(np.uint16)
    list2 = P.opcode_list([
        P.op_table((0, 0, H, W), rng.integers(0, 65536, size=65536), planes=(0, 3)),
        P.op_delta(13, (0, 0, H, W), rng.uniform(0.5, 1.5, size=W).astype(np.float32), planes=(0, 3))])
    crop = (0, 0, W, H)
    stage1 = abi.dng_post_desc(None, table, crop)
    scale = abi.scale_desc(crop, 256, 16383)
    stage2 = abi.dng_post_desc(list2, None, crop)
    lossy, keep = abi.dng_lossy_desc(stage1, list2, scale)
    ctx = capi.Context(0)
    pitch = 2 * CPP * W
    res = {"metric": "dng_lossy_chain", "frame": [W, H], "cpp": CPP, "tiles": len(streams),
           "image_mb": round(pitch * H / 1e6, 1), "reps": args.reps, "memory": {}}
    exact = True

    def chained(view):
        rc, st, r, bad, m = ctx.dng_lossy_decompress(streams, offsets, lossy, view, 0)
        return rc == 0 and r.stages == 7

    def sequence(view):
        ok = ctx.dng_decompress_jpeg(streams, offsets, view)[0] == 0
        ok &= ctx.dng_post(stage1[0], view, 0)[0] == 0
        ok &= ctx.scale_black_white(scale[0], view)[0] == 0
        ok &= ctx.dng_post(stage2[0], view, 0)[0] == 0
        return ok

    for kind in ("pageable", "page_locked"):
        if kind == "pageable":
            bufs = [np.zeros(pitch * H, np.uint8) for _ in range(2)]
        else:
            bufs = [ctx.host_alloc(pitch * H) for _ in range(2)]
        views = [abi.Image(b.ctypes.data, pitch, W, H, CPP, 0) for b in bufs]
        times = {"chained": [], "sequence": []}
        for fn, v in ((chained, views[0]), (sequence, views[1])):  # (warm: staging, page faults)
            exact &= bool(fn(v))
        exact &= bool(np.array_equal(bufs[0], bufs[1]))
        for _ in range(args.reps):
            for name, fn, v in (("chained", chained, views[0]), ("sequence", sequence, views[1])):
                t0 = time.perf_counter()
                ok = fn(v)
                times[name].append((time.perf_counter() - t0) * 1e3)
                exact &= bool(ok)
        exact &= bool(np.array_equal(bufs[0], bufs[1]))
        entry = {}
        for name, t in times.items():
            entry[name + "_ms"] = {"median": round(float(np.median(t)), 2), "best": round(min(t), 2),
                                   "all": [round(x, 2) for x in t]}
        entry["sequence_over_chained"] = round(entry["sequence_ms"]["median"] /
                                               entry["chained_ms"]["median"], 3)
        res["memory"][kind] = entry
        if kind == "page_locked":
            for b in bufs:
                ctx.host_free(b)
        del bufs, views
    res["bit_exact"] = bool(exact)
    line = json.dumps(res)
    print(line)
    if args.record:
        with open(args.record, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
