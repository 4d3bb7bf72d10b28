"""Image hash benchmark (rstest's md5 of per-line md5s and identify's sums, rsx_image_hash.hip).
Images of seeded samples resident in HBM:
  u16_8192x5464, f32_8192x5464, u16_3960x2640x3
                    a plan of one image: the hipEvent times of image_hash_rows_kernel and
                    image_hash_finish_kernel from rsx_plan_kernel_table, each on its own; the rows
                    kernel's time a block (64 bytes of a row: a wavefront's 64 lanes take one each)
                    with one wavefront a SIMD at the most, which is what a single image is; and
                    rsx_image_hash with a device pointer, the call's wall time (it makes its plan,
                    runs it, waits and brings 16 dim_y + 32 bytes back)
  plan64            a plan of 64 copies of the u16 8192 x 5464 image, each at its own address
                    (--plans 1,12,64: one leg a size; RSX_IMAGE_HASH_KERNEL=lds in the environment
                    times the row kernel that stages its blocks through LDS instead)
  host              the yardsticks for the u16 8192 x 5464 image in the same run: its download into
                    page-locked memory, the host build of the core (librsx_image_hash_host.so) on 1
                    and on 16 threads, and hashlib over the rows on one thread
Every device result is compared with the host build's, which tests/test_image_hash_model.py pins to
hashlib, before anything is timed.  Nothing here is a gate.  Prints one JSON line and, with --out,
writes it."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [("u16_8192x5464", 8192, 5464, 1, 2), ("f32_8192x5464", 8192, 5464, 1, 4),
          ("u16_3960x2640x3", 3960, 2640, 3, 2)]


def best_of(fn, reps):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best


def host_truth(F, abi, frame, w, h, cpp, sb, threads):
    view = abi.Image(frame.ctypes.data, w * cpp * sb, w, h, cpp, 0)
    st, r, lines = F.host_hash(view, sb, threads)
    assert st == 0
    return (lines, r.digest(), r.byte_sum, r.sample_sum)


def shape_leg(ctx, torch, F, abi, name, w, h, cpp, sb, steps, warmup):
    rng = np.random.default_rng([21, w, h, cpp, sb])
    row_bytes = w * cpp * sb
    frame = rng.integers(0, 256, row_bytes * h, dtype=np.uint8)
    want = host_truth(F, abi, frame, w, h, cpp, sb, 16)
    dev = torch.from_numpy(frame).cuda()
    out = torch.full((16 * h + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    plan = ctx.image_hash_plan([abi.image_hash_job(0, 0, 16 * h, sb, w, h, cpp, row_bytes)])
    s = torch.cuda.current_stream().cuda_stream
    plan.run(dev.data_ptr(), out.data_ptr(), s)
    exact = plan.results()[0] == 0
    exact &= out.cpu().numpy().tobytes() == want[0] + F.result_bytes(*want[1:])
    for _ in range(warmup):
        plan.run(dev.data_ptr(), out.data_ptr(), s)
    plan.results()
    plan.set_timing(True)
    for _ in range(steps):
        plan.run(dev.data_ptr(), out.data_ptr(), s)
    plan.results()
    table, runs = plan.kernel_table()
    plan.close()
    ms = dict(table)
    view = abi.Image(dev.data_ptr(), row_bytes, w, h, cpp, 0)
    st, r, lines = ctx.image_hash(view, sb)
    exact &= st == 0 and lines == want[0] and F.same(r, want)
    call = best_of(lambda: ctx.image_hash(view, sb), max(steps, 5))
    blocks = row_bytes // 64 + (2 if row_bytes % 64 >= 56 else 1)  # of a row, padding included
    waves = (h + 63) // 64
    rows_ms = ms["image_hash_rows_kernel"]
    return {"width": w, "height": h, "cpp": cpp, "sample_bytes": sb, "bytes": int(frame.size),
            "rows_kernel_ms": round(rows_ms, 4),
            "finish_kernel_ms": round(ms["image_hash_finish_kernel"], 4),
            "wavefronts": waves, "blocks_per_row": blocks,
            "rows_kernel_ns_per_block": round(rows_ms * 1e6 / blocks, 1),
            "finish_blocks": h // 4 + 1,
            "finish_kernel_ns_per_block": round(ms["image_hash_finish_kernel"] * 1e6 / (h // 4 + 1), 1),
            "device_call_ms": round(call, 3), "runs": runs, "bit_exact": bool(exact)}, frame, dev, want


def plan64_leg(ctx, torch, F, abi, dev, want, w, h, steps, warmup, n=64):
    row_bytes, size = 2 * w, 2 * w * h
    stride = (size + 255) // 256 * 256
    images = torch.empty(n * stride, dtype=torch.uint8, device="cuda")
    for k in range(n):
        images[k * stride:k * stride + size].copy_(dev)
    per = 16 * h + 32
    out = torch.full((n * per,), 0xA5, dtype=torch.uint8, device="cuda")
    jobs = [abi.image_hash_job(k * stride, k * per, k * per + 16 * h, 2, w, h, 1, row_bytes)
            for k in range(n)]
    plan = ctx.image_hash_plan(jobs)
    s = torch.cuda.current_stream().cuda_stream
    plan.run(images.data_ptr(), out.data_ptr(), s)
    exact = plan.results()[0] == 0
    one = want[0] + F.result_bytes(*want[1:])
    exact &= out.cpu().numpy().tobytes() == one * n
    for _ in range(warmup):
        plan.run(images.data_ptr(), out.data_ptr(), s)
    plan.results()
    plan.set_timing(True)
    t0 = time.perf_counter()
    for _ in range(steps):
        plan.run(images.data_ptr(), out.data_ptr(), s)
    plan.results()
    wall = (time.perf_counter() - t0) / steps * 1e3
    table, runs = plan.kernel_table()
    plan.close()
    ms = dict(table)
    total = ms["image_hash_rows_kernel"] + ms["image_hash_finish_kernel"]
    return {"frames": n, "bytes": n * size, "rows_kernel_ms": round(ms["image_hash_rows_kernel"], 4),
            "finish_kernel_ms": round(ms["image_hash_finish_kernel"], 4),
            "kernels_ms_per_frame": round(total / n, 4), "wall_ms_per_step": round(wall, 3),
            "gb_s": round(n * size / (total * 1e-3) / 1e9, 1), "runs": runs,
            "bit_exact": bool(exact)}


def host_leg(ctx, torch, F, abi, frame, dev, want, w, h, reps=3):
    pinned = ctx.host_alloc(frame.size)
    dst = torch.from_numpy(pinned)

    def download():
        dst.copy_(dev)
        torch.cuda.synchronize()
    download()
    exact = np.array_equal(pinned, frame)
    down = best_of(download, reps)
    view = abi.Image(pinned.ctypes.data, 2 * w, w, h, 1, 0)
    res = {"download_pinned_ms": round(down, 2)}
    for threads in (1, 16):
        st, r, lines = F.host_hash(view, 2, threads)
        exact &= st == 0 and lines == want[0] and F.same(r, want)
        res["host_build_ms_%d_thread%s" % (threads, "s" if threads > 1 else "")] = round(
            best_of(lambda: F.host_hash(view, 2, threads), reps), 2)
    rows = pinned.reshape(h, 2 * w)

    def with_hashlib():
        return hashlib.md5(b"".join(hashlib.md5(r).digest() for r in rows)).digest()
    exact &= with_hashlib() == want[1]
    res["hashlib_rows_ms_1_thread"] = round(best_of(with_hashlib, 1), 2)
    res["download_and_16_threads_ms"] = round(down + res["host_build_ms_16_threads"], 2)
    res["bit_exact"] = bool(exact)
    del dst
    ctx.host_free(pinned)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--plans", default="64")
    ap.add_argument("--out")
    args = ap.parse_args()
    import image_hash_files as F
    import torch
    from rawspeed_amd import abi, capi
    F.host()
    ctx = capi.Context(0)
    res = {"metric": "image_hash"}
    exact = True
    keep = None
    for name, w, h, cpp, sb in SHAPES:
        leg, frame, dev, want = shape_leg(ctx, torch, F, abi, name, w, h, cpp, sb, args.steps,
                                          args.warmup)
        res[name] = leg
        exact &= leg["bit_exact"]
        if keep is None:
            keep = (frame, dev, want, w, h)
    frame, dev, want, w, h = keep
    res["row_kernel"] = os.environ.get("RSX_IMAGE_HASH_KERNEL") or "direct"
    for n in [int(v) for v in args.plans.split(",")]:
        res["plan%d" % n] = plan64_leg(ctx, torch, F, abi, dev, want, w, h, args.steps,
                                       args.warmup, n=n)
        exact &= res["plan%d" % n]["bit_exact"]
    res["host"] = host_leg(ctx, torch, F, abi, frame, dev, want, w, h)
    exact &= res["host"]["bit_exact"]
    one = res[SHAPES[0][0]]
    res["device_call_beats_download_and_16_threads"] = bool(
        one["device_call_ms"] < res["host"]["download_and_16_threads_ms"])
    res["bit_exact"] = bool(exact)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
