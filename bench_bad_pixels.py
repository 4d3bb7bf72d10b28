"""Bad-pixel interpolation benchmark (include/rsx.h section 5): an 8316 x 5640 uint16 CFA image.
Not part of bench.py.  One JSON line:

  device   the image and the positions resident in HBM, hipEvent times of the stage's kernels
           (rsx_plan_kernel_table) for three maps --
             camera    300 positions
             lattice   a phase-detect lattice: every 8th pixel of every 12th row
             block     a 1024 x 1024 block plus 64 border rows, all bad
           -- next to rsx_probe_stream_copy over the image's bytes (read and written once) in the
           same run
  host     the host build of the same core (rawspeed_amd/librsx_bad_pixels_host.so) on 1 thread and
           on 16 with the reference's row split: OUR restatement with the word-wise search, not
           the reference, whose walk is one pixel at a time
  v4       rsx_panasonic_v4_decompress_fixed against rsx_panasonic_v4_decompress (the list handed
           out, nothing fixed) on the same frame through host pointers, alternating in one process

fix_call_device_ptr_ms is one rsx_bad_pixels_fix on the resident image (wall clock, best of three):
the stage plus the per-call plan of a host call.  --record FILE keeps the line
(profiles/bad_pixels/bench_bad_pixels.json is one such run).

The device output of every case is compared bit for bit with the host build (pinned against the
recorded reference by tests/test_bad_pixels_model.py).  Nothing is promised in advance."""
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

W, H = 8316, 5640


def make_positions():
    rng = np.random.default_rng(0xBAD)
    ys, xs = np.meshgrid(np.arange(0, H, 12), np.arange(0, W, 8), indexing="ij")
    by, bx = np.meshgrid(np.arange(2000, 3024), np.arange(3000, 4024), indexing="ij")
    ry, rx = np.meshgrid(np.arange(64), np.arange(W), indexing="ij")
    pos = lambda y, x: (y.reshape(-1).astype(np.uint32) << 16) | x.reshape(-1).astype(np.uint32)  # noqa: E731
    return {"camera": pos(rng.integers(0, H, 300), rng.integers(0, W, 300)),
            "lattice": pos(ys, xs),
            "block": np.concatenate([pos(by, bx), pos(ry, rx)])}


def host_fix(L, abi, img, positions, threads):
    out = img.copy()
    d, keep, _ = abi.bad_pixels_desc(positions, (W, H), want_map=False, map_pitch=0)
    r = abi.BadPixelsResult()
    t0 = time.perf_counter()
    st = L.rsx_bad_pixels_host_fix_threads(C.byref(d), C.byref(abi.Image(out.ctypes.data, 2 * W, W, H, 1, 1)),
                                           C.byref(r), threads)
    return st, out, r, (time.perf_counter() - t0) * 1e3


def device_leg(ctx, torch, abi, L, img, cases, args):
    flat = img.reshape(-1).view(np.uint8)
    dev = torch.from_numpy(flat).cuda()
    other = torch.empty_like(dev)
    s = torch.cuda.current_stream().cuda_stream
    out, exact = {}, True
    for name, positions in cases.items():
        dpos = torch.from_numpy(positions.view(np.uint8).copy()).cuda()
        j = abi.BadPixelsJob()
        j.n_positions, j.img = positions.size, abi.Image(None, 2 * W, W, H, 1, 1)
        dev.copy_(torch.from_numpy(flat))
        t0 = time.perf_counter()
        plan = ctx.bad_pixels_plan([j])
        create_ms = (time.perf_counter() - t0) * 1e3
        plan.run(dpos.data_ptr(), dev.data_ptr(), s)
        rc, _, _ = plan.results()
        _, r = plan.result(0)
        got = dev.cpu().numpy().view(np.uint16).reshape(H, W)
        st1, want, hr, host_1t = host_fix(L, abi, img, positions, 1)
        st16, want16, _, host_16t = host_fix(L, abi, img, positions, 16)
        ok = rc == 0 and st1 == 0 and st16 == 0 and np.array_equal(got, want) and \
            np.array_equal(want16, want) and (r.n_bad, r.n_fixed) == (hr.n_bad, hr.n_fixed)
        exact &= bool(ok)
        vals, tables = [], []
        for _ in range(args.repeats):
            plan.set_timing(True)
            for _ in range(args.steps):
                plan.run(dpos.data_ptr(), dev.data_ptr(), s)
            plan.results()
            table_ms, runs = plan.kernel_table()
            plan.set_timing(False)
            vals.append(sum(ms for _, ms in table_ms))
            tables.append({k: round(ms, 4) for k, ms in table_ms})
        plan.close()
        # one rsx_bad_pixels_fix on the resident image: the stage plus what a host call adds (its
        # one-job plan with both maps made and freed, the positions up, the counts down)
        d, keep, _ = abi.bad_pixels_desc(positions, (W, H), want_map=False, map_pitch=0)
        calls = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st, _ = ctx.bad_pixels_fix(d, abi.Image(dev.data_ptr(), 2 * W, W, H, 1, 1))
            calls.append((time.perf_counter() - t0) * 1e3)
            exact &= st == 0
        med = float(np.median(vals))
        out[name] = {"positions": int(positions.size), "n_bad": int(r.n_bad), "n_fixed": int(r.n_fixed),
                     "stage_ms": round(med, 4), "stage_ms_all": [round(v, 4) for v in vals],
                     "kernels_ms": tables[int(np.argsort(vals)[len(vals) // 2])],
                     "plan_create_ms": round(create_ms, 2),
                     "fix_call_device_ptr_ms": round(min(calls), 3),
                     "fix_call_device_ptr_ms_all": [round(c, 3) for c in calls], "host_core_1t_ms": round(host_1t, 1),
                     "host_core_16t_ms": round(host_16t, 1), "bit_exact": bool(ok)}
        del dpos
    probe = [ctx.probe_stream_copy(dev.data_ptr(), dev.numel(), other.data_ptr(), dev.numel(), s, reps=args.steps)
             for _ in range(args.repeats)]
    pms = float(np.median(probe))
    out["copy_probe_ms"] = round(pms, 4)
    out["copy_probe_ms_all"] = [round(x, 4) for x in probe]
    for name in cases:
        out[name]["stage_over_probe"] = round(out[name]["stage_ms"] / pms, 3)
    del dev, other
    return out, exact


def v4_leg(ctx, abi, L, reps=4):
    import rw2_v4_files as P4
    from oracle_lib import HostImage
    rng = np.random.default_rng(4)
    split = P4.SPLITS[1]
    data = P4.random_stream(rng, split, W, H, "uniform")
    plain, fixed = HostImage(W, H), HostImage(W, H)
    best, ok = {}, True
    cap = 1 << 22
    for _ in range(reps):  # (A, B, A, B ...)
        t0 = time.perf_counter()
        st, n, bad = ctx.panasonic_v4_decompress(split, 1, data, plain.view(), cap)
        dt = (time.perf_counter() - t0) * 1e3
        best["plain"] = min(best.get("plain", dt), dt)
        ok &= st == 0
        t0 = time.perf_counter()
        st, r, m = ctx.panasonic_v4_decompress_fixed(split, 1, data, fixed.view())
        dt = (time.perf_counter() - t0) * 1e3
        best["fixed"] = min(best.get("fixed", dt), dt)
        ok &= st == 0 and r.n_bad == n
    d, keep, map_out = abi.bad_pixels_desc(bad, (W, H))
    want = plain.pixels().copy()
    t0 = time.perf_counter()
    st = L.rsx_bad_pixels_host_fix_threads(C.byref(d), C.byref(abi.Image(want.ctypes.data, 2 * W, W, H, 1, 1)),
                                           None, 16)
    host_ms = (time.perf_counter() - t0) * 1e3
    ok &= st == 0 and np.array_equal(fixed.pixels(), want) and m.tobytes() == map_out.tobytes()
    return {"zero_pixels": int(n), "panasonic_v4_decompress_ms": round(best["plain"], 2),
            "panasonic_v4_decompress_fixed_ms": round(best["fixed"], 2),
            "fixed_adds_ms": round(best["fixed"] - best["plain"], 2),
            "host_core_16t_fix_of_the_list_ms": round(host_ms, 2), "in_bytes": int(data.size)}, bool(ok)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-v4", action="store_true")
    ap.add_argument("--record", metavar="FILE", help="also write the JSON line to FILE")
    args = ap.parse_args()
    import torch
    from rawspeed_amd import abi, build, capi, synth
    L = C.CDLL(build.build_bad_pixels_host()[0])
    L.rsx_bad_pixels_host_fix_threads.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    ctx = capi.Context(0)
    img = synth.sensor_image(W, H, 14, seed=5)
    res = {"metric": "bad_pixels", "frame": [W, H]}
    res["device"], exact = device_leg(ctx, torch, abi, L, img, make_positions(), args)
    if not args.no_v4:
        res["v4"], ok = v4_leg(ctx, abi, L)
        exact &= ok
    res["bit_exact"] = bool(exact)
    line = json.dumps(res)
    if args.record:
        os.makedirs(os.path.dirname(os.path.abspath(args.record)), exist_ok=True)
        with open(args.record, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
