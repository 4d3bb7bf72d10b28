"""DNG opcode list + LinearizationTable benchmark (include/rsx.h section 4d): an 8192 x 5464 uint16
frame, cpp 1.  Not part of bench.py.  One JSON line:

  device       the image resident in HBM, hipEvent time of dng_post_kernel (rsx_plan_kernel_table)
               for three jobs -- the look-up alone (a 4096-entry table), a MapTable alone, and a
               list of four (ScalePerRow, DeltaPerColumn, MapTable, FixBadPixelsConstant) plus the
               look-up -- next to rsx_probe_stream_copy over the same 2 + 2 bytes a pixel in the
               same run: the ceiling of a pass that reads and writes every pixel once
  plan8        eight frames, the list of four plus the look-up, one plan
  host         rsx_dng_decompress_ljpeg_post against rsx_dng_decompress_ljpeg on the same 2 x 2
               LJPEG tiles through host pointers (the plain call splits into bands that overlap
               both directions of the link; the _post call cannot, it needs the whole image), and
               rsx_dng_post alone through host pointers (a round trip over the link)
  reference    where oracle/_ref is built: the unmodified reference's whole-file decode of an
               uncompressed DNG with the same list and table minus the same file without them,
               same process, on one thread and on 16 (the look-up is threaded, the opcodes are
               not)

The device output of every job is compared bit for bit with the host build of the same core
(rawspeed_amd/librsx_dng_post_host.so, pinned against the reference by
tests/test_dng_post_model.py).  Nothing is promised in advance; the comparison points are the copy
probe and the reference."""
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

W, H = 8192, 5464


def make_lists(K):
    rng = np.random.default_rng(0xD46)
    table = np.sort(rng.integers(0, 65536, size=4096)).astype(np.uint16)
    curve = np.clip(np.arange(65536) ** 0.97 * 1.3, 0, 65535).astype(np.uint16)
    full = (0, 0, H, W)
    map_table = K.op_table(full, curve)
    four = [K.op_delta(12, full, rng.uniform(0.9, 1.1, size=H).astype(np.float32)),
            K.op_delta(11, full, rng.uniform(-0.01, 0.01, size=W // 2).astype(np.float32), pitch=(1, 2)),
            map_table, K.op_bad_constant(0)]
    return {"lookup": (None, table), "map_table": (K.opcode_list([map_table]), None),
            "four_plus_lookup": (K.opcode_list(four), table)}


def job_for(abi, opcodes, table, offset=0):
    d, keep = abi.dng_post_desc(opcodes, table, (0, 0, W, H))
    j = abi.DngPostJob()
    j.desc, j.img_offset, j.bad_cap = d, offset, 1 << 20
    j.img = abi.Image(None, 2 * W, W, H, 1, 1)
    return j, keep


def timed(plan, ptr, s, steps, repeats):
    vals = []
    for _ in range(repeats):
        plan.set_timing(True)
        for _ in range(steps):
            plan.run(ptr, ptr, s)
        plan.results()
        table_ms, runs = plan.kernel_table()
        plan.set_timing(False)
        vals.append(sum(ms for name, ms in table_ms if name == "dng_post_kernel"))
    return float(np.median(vals)), [round(v, 4) for v in vals]


def device_leg(ctx, torch, abi, K, img, lists, args):
    from rawspeed_amd import build
    L = C.CDLL(build.build_dng_post_host()[0])
    L.rsx_dng_post_host_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    flat = img.reshape(-1).view(np.uint8)
    dev = torch.from_numpy(flat).cuda()
    other = torch.empty_like(dev)
    s = torch.cuda.current_stream().cuda_stream
    out, wants, exact = {}, {}, True
    for name, (opcodes, table) in lists.items():
        job, keep = job_for(abi, opcodes, table)
        dev.copy_(torch.from_numpy(flat))
        t0 = time.perf_counter()
        plan = ctx.dng_post_plan([job])
        create_ms = (time.perf_counter() - t0) * 1e3
        plan.run(dev.data_ptr(), dev.data_ptr(), s)
        rc, _, _ = plan.results()
        got = dev.cpu().numpy().view(np.uint16).reshape(H, W)
        bst, n_bad, bad = plan.bad_pixels(0, 1 << 20)
        want = img.copy()
        v = abi.Image(want.ctypes.data, 2 * W, W, H, 1, 1)
        r = abi.DngPostResult()
        buf = (C.c_uint32 * (1 << 20))()
        t0 = time.perf_counter()
        st = L.rsx_dng_post_host_apply(C.byref(job.desc), C.byref(v), C.byref(r), buf, 1 << 20)
        host_core_ms = (time.perf_counter() - t0) * 1e3
        ok = rc == 0 and st == 0 and bst == 0 and np.array_equal(got, want) and \
            n_bad == r.n_bad and bad == [int(x) for x in buf[:r.n_bad]]
        exact &= bool(ok)
        wants[name] = want
        dev.copy_(torch.from_numpy(flat))
        med, allv = timed(plan, dev.data_ptr(), s, args.steps, args.repeats)
        plan.close()
        out[name] = {"kernel_ms": round(med, 4), "kernel_ms_all": allv,
                     "gpix_s": round(W * H / (med * 1e-3) / 1e9, 2) if med else None,
                     "plan_create_ms": round(create_ms, 2), "host_core_1t_ms": round(host_core_ms, 1),
                     "pixels_changed_frac": round(float((got != img).mean()), 4),
                     "bad_positions": int(n_bad), "bit_exact": bool(ok)}
    probe = [ctx.probe_stream_copy(dev.data_ptr(), dev.numel(), other.data_ptr(), dev.numel(), s, reps=args.steps)
             for _ in range(args.repeats)]
    pms = float(np.median(probe))
    out["copy_probe_ms"] = round(pms, 4)
    out["copy_probe_ms_all"] = [round(x, 4) for x in probe]
    for name in lists:
        out[name]["frac_of_probe"] = round(pms / out[name]["kernel_ms"], 3) if out[name]["kernel_ms"] else None
    del dev, other
    return out, wants, exact


def plan8_leg(ctx, torch, abi, img, lists, args, frames=8):
    opcodes, table = lists["four_plus_lookup"]
    frame_bytes = 2 * W * H
    jobs, keep = [], []
    for k in range(frames):
        j, kp = job_for(abi, opcodes, table, k * frame_bytes)
        jobs.append(j)
        keep.append(kp)
    dev = torch.from_numpy(np.tile(img.reshape(-1).view(np.uint8), frames)).cuda()
    s = torch.cuda.current_stream().cuda_stream
    plan = ctx.dng_post_plan(jobs)
    med, allv = timed(plan, dev.data_ptr(), s, max(3, args.steps // 4), 3)
    plan.close()
    del dev
    return {"frames": frames, "kernel_ms": round(med, 4), "kernel_ms_all": allv,
            "ms_per_frame": round(med / frames, 4)}


def host_leg(ctx, abi, img_unused, lists, args, reps=3):
    import bench_ljpeg
    import dng_post_files as K
    from oracle_lib import HostImage
    src, jobs, datas, _, _ = bench_ljpeg._dng_tiles(W, H, W // 2, H // 2, seed=5)
    descs = [j.desc for j in jobs]
    opcodes, table = lists["four_plus_lookup"]
    d, keep = abi.dng_post_desc(opcodes, table, (0, 0, W, H))
    out = HostImage(W, H)
    best = {}
    ok = True
    for _ in range(reps):
        t0 = time.perf_counter()
        rc, st, _ = ctx.dng_decompress_ljpeg(descs, datas, out.view())
        dt = (time.perf_counter() - t0) * 1e3
        best["plain"] = min(best.get("plain", dt), dt)
        ok &= rc == 0
    ok &= np.array_equal(out.pixels(), src)
    for _ in range(reps):
        t0 = time.perf_counter()
        rc, st, r, bad = ctx.dng_decompress_ljpeg_post(descs, datas, d, out.view(), 1 << 20)
        dt = (time.perf_counter() - t0) * 1e3
        best["post"] = min(best.get("post", dt), dt)
        ok &= rc == 0
    post_img = out.pixels().copy()
    out.pixels()[:] = src
    for _ in range(reps):
        out.pixels()[:] = src
        t0 = time.perf_counter()
        st, r2, bad2 = ctx.dng_post(d, out.view(), 1 << 20)
        dt = (time.perf_counter() - t0) * 1e3
        best["alone"] = min(best.get("alone", dt), dt)
        ok &= st == 0
    ok &= np.array_equal(out.pixels(), post_img) and bad == bad2
    return {"dng_decompress_ljpeg_ms": round(best["plain"], 2),
            "dng_decompress_ljpeg_post_ms": round(best["post"], 2),
            "post_adds_ms": round(best["post"] - best["plain"], 2),
            "dng_post_host_pointers_ms": round(best["alone"], 2),
            "in_bytes": int(sum(x.size for x in datas))}, bool(ok), src, post_img


def ref_leg(K, img, lists, want, reps=2):
    from oracle_lib import Ref
    if not Ref.available():
        return None
    ref = Ref()
    opcodes, table = lists["four_plus_lookup"]
    blobs = {"without": K.dng_post_file(img), "with": K.dng_post_file(img, 1, opcodes, table)}
    out = {}
    same = None
    for threads in (1, min(16, os.cpu_count() or 1)):
        best = {}
        for name, blob in blobs.items():
            for _ in range(reps):
                t0 = time.perf_counter()
                st, dec = ref.decode_file(blob, threads=threads)
                dt = (time.perf_counter() - t0) * 1e3
                assert st == 0, ref.last_error()
                if name == "with" and same is None:
                    same = bool(np.array_equal(dec.u16()[:H, :W], want))
                dec.close()
                best[name] = min(best.get(name, dt), dt)
        out["threads_%d" % threads] = {"decode_ms": round(best["without"], 1),
                                       "decode_with_list_and_table_ms": round(best["with"], 1),
                                       "list_and_table_ms": round(best["with"] - best["without"], 1)}
    out["same_image_as_device"] = same
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-ref", action="store_true")
    args = ap.parse_args()
    import torch
    import dng_post_files as K
    from rawspeed_amd import abi, capi, synth
    ctx = capi.Context(0)
    img = synth.sensor_image(W, H, 14, seed=5)
    lists = make_lists(K)
    res = {"metric": "dng_post", "frame": [W, H]}
    res["device"], wants, exact = device_leg(ctx, torch, abi, K, img, lists, args)
    res["plan8"] = plan8_leg(ctx, torch, abi, img, lists, args)
    if not args.no_host:
        res["host"], ok, src, post_img = host_leg(ctx, abi, img, lists, args)
        exact &= ok and np.array_equal(src, img) and np.array_equal(post_img, wants["four_plus_lookup"])
    if not args.no_ref:
        res["reference"] = ref_leg(K, img, lists, wants["four_plus_lookup"])
        if res["reference"]:
            exact &= bool(res["reference"]["same_image_as_device"])
    res["bit_exact"] = bool(exact)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
