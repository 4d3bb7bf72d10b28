"""Black/white scaling benchmark (include/rsx.h section 6): an 8192 x 5464 uint16 CFA image (and
the same size in binary32).  Not part of bench.py.  One JSON line:

  device   the image resident in HBM, hipEvent times of the stage's kernels
           (rsx_plan_kernel_table) -- the pass alone and all six launches -- for
             sse2_no_dither / sse2_dither    the SSE2 variant, levels given
             plain_dither / plain_no_dither  the plain variant (host_sse2 = 0), levels given
             f32                             the binary32 pass, levels given
             estimate                        nothing given: the min / max window first (SSE2, dither)
             two_areas                       a horizontal and a vertical black area (SSE2, dither)
           The image is restored in front of every timed run (a device copy outside the events):
           the pass works in place, and a second estimate on a scaled image would skip.
           Next to them rsx_probe_stream_copy over the image's bytes in the same run, out of place
           and IN PLACE (the same pointer read and written): the ceiling of a pass that reads and
           writes every sample once.
  host     rsx_scale_black_white through host pointers (wall clock, best of three) next to the
           two copies over the link alone (torch, pageable memory, same process)

The device output of every case is compared bit for bit with the host build of the same core
(rawspeed_amd/librsx_scale_host.so, pinned against the recorded reference by
tests/test_scale_model.py).  --record FILE keeps the line (profiles/scale/bench_scale.json is one
such run).  Nothing is promised in advance; the comparison point is the look-up stage of
bench_dng_post.py, run in the same session (profiles/scale/README.md)."""
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
SEP, WHITE = (256, 257, 258, 259), 16383

CASES = {
    "sse2_no_dither": dict(black_separate=SEP, white_point=WHITE, dither=False),
    "sse2_dither": dict(black_separate=SEP, white_point=WHITE, dither=True),
    "plain_no_dither": dict(black_separate=SEP, white_point=WHITE, dither=False, host_sse2=False),
    "plain_dither": dict(black_separate=SEP, white_point=WHITE, dither=True, host_sse2=False),
    "f32": dict(black_separate=SEP, white_point=WHITE, is_f32=True),
    "estimate": dict(),
    "two_areas": dict(white_point=WHITE, areas=[(0, 16, False), (8, 32, True)]),
}


def timed(plan, dev, src, torch, s, steps, repeats):
    passes, totals, tables = [], [], None
    for _ in range(repeats):
        plan.set_timing(True)
        for _ in range(steps):
            dev.copy_(src)
            plan.run(dev.data_ptr(), dev.data_ptr(), s)
        plan.results()
        table_ms, runs = plan.kernel_table()
        plan.set_timing(False)
        passes.append(sum(ms for name, ms in table_ms if name == "sc_pass_kernel"))
        totals.append(sum(ms for name, ms in table_ms))
        tables = {name: round(ms, 4) for name, ms in table_ms}
    return float(np.median(passes)), float(np.median(totals)), [round(v, 4) for v in totals], tables


def device_leg(ctx, torch, abi, L, images, args):
    s = torch.cuda.current_stream().cuda_stream
    out, exact = {}, True
    for name, kw in CASES.items():
        f32 = bool(kw.get("is_f32"))
        img = images[f32]
        ss = img.itemsize
        flat = img.reshape(-1).view(np.uint8)
        src = torch.from_numpy(flat).cuda()
        dev = src.clone()
        d, keep = abi.scale_desc((0, 0, W, H), **kw)
        j = abi.ScaleJob()
        j.desc, j.img = d, abi.Image(None, ss * W, W, H, 1, 1)
        t0 = time.perf_counter()
        plan = ctx.scale_plan([j])
        create_ms = (time.perf_counter() - t0) * 1e3
        plan.run(dev.data_ptr(), dev.data_ptr(), s)
        rc, _, _ = plan.results()
        _, r = plan.result(0)
        got = dev.cpu().numpy().view(img.dtype).reshape(H, W)
        want = img.copy()
        hr = abi.ScaleResult()
        t0 = time.perf_counter()
        st = L.rsx_scale_host_black_white(C.byref(d), C.byref(abi.Image(want.ctypes.data, ss * W, W, H, 1, 1)),
                                          C.byref(hr))
        host_core_ms = (time.perf_counter() - t0) * 1e3
        ok = rc == 0 and st == 0 and got.tobytes() == want.tobytes() and bytes(r) == bytes(hr)
        exact &= bool(ok)
        pass_ms, total_ms, allv, table = timed(plan, dev, src, torch, s, args.steps, args.repeats)
        plan.close()
        out[name] = {"pass_ms": round(pass_ms, 4), "all_kernels_ms": round(total_ms, 4),
                     "all_kernels_ms_all": allv, "kernels": table,
                     "gpix_s": round(W * H / (total_ms * 1e-3) / 1e9, 2) if total_ms else None,
                     "variant": r.variant, "levels": list(r.levels()[2]), "white": r.white_point,
                     "plan_create_ms": round(create_ms, 2), "host_core_1t_ms": round(host_core_ms, 1),
                     "bit_exact": bool(ok)}
        if name == "sse2_no_dither":
            other = torch.empty_like(dev)
            n = dev.numel()
            probe = [ctx.probe_stream_copy(dev.data_ptr(), n, other.data_ptr(), n, s, reps=args.steps)
                     for _ in range(args.repeats)]
            inplace = [ctx.probe_stream_copy(dev.data_ptr(), n, dev.data_ptr(), n, s, reps=args.steps)
                       for _ in range(args.repeats)]
            out["copy_probe_ms"] = round(float(np.median(probe)), 4)
            out["copy_probe_ms_all"] = [round(x, 4) for x in probe]
            out["copy_in_place_ms"] = round(float(np.median(inplace)), 4)
            out["copy_in_place_ms_all"] = [round(x, 4) for x in inplace]
            del other
        del dev, src
    for name in CASES:
        scale = 2.0 if CASES[name].get("is_f32") else 1.0  # (twice the bytes)
        out[name]["copy_over_pass"] = round(scale * out["copy_in_place_ms"] / out[name]["pass_ms"], 3)
    return out, exact


def host_leg(ctx, torch, abi, L, img, reps=3):
    kw = CASES["sse2_dither"]
    d, keep = abi.scale_desc((0, 0, W, H), **kw)
    want = img.copy()
    L.rsx_scale_host_black_white(C.byref(d), C.byref(abi.Image(want.ctypes.data, 2 * W, W, H, 1, 1)), None)
    best, ok = None, True
    for _ in range(reps):
        buf = img.copy()
        t0 = time.perf_counter()
        st, r = ctx.scale_black_white(d, abi.Image(buf.ctypes.data, 2 * W, W, H, 1, 1))
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
        ok &= st == 0 and np.array_equal(buf, want)
    up = down = None
    t = torch.from_numpy(img)
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev = t.cuda()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        dev.cpu()
        t2 = time.perf_counter()
        up = (t1 - t0) * 1e3 if up is None else min(up, (t1 - t0) * 1e3)
        down = (t2 - t1) * 1e3 if down is None else min(down, (t2 - t1) * 1e3)
    return {"scale_black_white_host_pointers_ms": round(best, 2), "upload_alone_ms": round(up, 2),
            "download_alone_ms": round(down, 2), "bytes_each_way": int(img.nbytes)}, bool(ok)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--record")
    args = ap.parse_args()
    import torch
    from rawspeed_amd import abi, build, capi, synth
    L = C.CDLL(build.build_scale_host()[0])
    L.rsx_scale_host_black_white.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    ctx = capi.Context(0)
    img = synth.sensor_image(W, H, 14, seed=5)
    images = {False: img, True: img.astype(np.float32)}
    res = {"metric": "scale_black_white", "frame": [W, H]}
    res["device"], exact = device_leg(ctx, torch, abi, L, images, args)
    if not args.no_host:
        res["host"], ok = host_leg(ctx, torch, abi, L, img)
        exact &= ok
    res["bit_exact"] = bool(exact)
    line = json.dumps(res)
    print(line)
    if args.record:
        with open(args.record, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
