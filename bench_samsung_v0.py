"""SamsungV0Decompressor benchmark (Samsung SRW, compression 32770): frames of 5546 x 3714 (the
largest the reference accepts, with a partial last block), 5536 x 3714 and 4640 x 3084, and a plan
of eight 4640 x 3084 frames, decoded with the input and output resident in HBM (one plan launch
per step; both kernels' hipEvent times from rsx_plan_kernel_table), through the host-pointer call,
and by the unmodified reference (oracle/_ref, whole-file decode, one thread: the reference has no
threaded path for this codec) in the same run where that library is present.  Two encoder
settings: about 1 byte a pixel with about 30 % upward blocks, and the same without upward blocks.
Every decode is compared with the model of tests/srw_v0_files.py.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FRAMES = (("max", (5546, 3714)), ("full_blocks", (5536, 3714)), ("nx", (4640, 3084)))
SETTINGS = (("up30", 0.3), ("left", 0.0))


def make_frame(w, h, p_up):
    import srw_v0_files as S
    rng = np.random.default_rng([0x5B0, w, h, int(100 * p_up)])
    rows = S.tiled_rows(rng, w, h, p_up=p_up, pool=32)
    strip, offs = S.strip_and_offsets(rows)
    st, _, img = S.model_decode(w, h, rows, cache={})
    assert st == 0
    return rows, strip, offs, img


def _job(abi, arr, n, in_off, in_bytes, img_off, pitch, w, h):
    j = abi.SamsungV0Job()
    j.row_offsets, j.n_offsets = arr, n
    j.in_offset, j.in_bytes, j.img_offset = in_off, in_bytes, img_off
    j.img = abi.Image(None, pitch, w, h, 1, 1)
    return j


def device_leg(ctx, torch, strip, offs, img, steps, warmup, frames=1):
    from rawspeed_amd import abi
    h, w = img.shape
    pitch = (2 * w + 15) // 16 * 16
    arr = abi.samsung_v0_offsets(offs)
    in_stride = (len(strip) + 15) // 16 * 16 + 16
    jobs = [_job(abi, arr, len(offs), k * in_stride, len(strip), k * pitch * h, pitch, w, h)
            for k in range(frames)]
    host_in = np.zeros(frames * in_stride, np.uint8)
    for k in range(frames):
        host_in[k * in_stride:k * in_stride + len(strip)] = strip
    inp = torch.from_numpy(host_in).cuda()
    out = torch.zeros(frames * pitch * h, dtype=torch.uint8, device="cuda")
    plan = ctx.samsung_v0_plan(jobs)
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
    kms = sum(ms.values())
    got = out.cpu().numpy().view(np.uint16).reshape(frames, h, pitch // 2)[:, :, :w]
    exact = rc == 0 and all(np.array_equal(got[k], img) for k in range(frames))
    return {"frames": frames, "parse_ms": round(ms.get("sv0_parse_kernel", 0.0), 4),
            "recon_ms": round(ms.get("sv0_recon_kernel", 0.0), 4), "kernel_ms": round(kms, 4),
            "wall_ms_per_step": round(wall, 4),
            "gpix_s": round(frames * w * h / (kms * 1e-3) / 1e9, 3),
            "bytes_per_px": round(len(strip) / (w * h), 3), "runs": runs, "bit_exact": bool(exact)}


def host_leg(ctx, strip, offs, img, reps=3):
    from oracle_lib import HostImage
    h, w = img.shape
    best, exact = None, True
    for _ in range(reps):
        out = HostImage(w, h)
        t0 = time.perf_counter()
        st, _ = ctx.samsung_v0_decompress(strip, offs, out.view(), rows=False)
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
        exact &= st == 0 and np.array_equal(out.pixels(), img)
    return round(best, 3), bool(exact)


def ref_leg(strip, offs, img, reps=2):
    import srw_v0_files as S
    from oracle_lib import Ref
    if not Ref.available():
        return None, None
    ref = Ref()
    h, w = img.shape
    blob = S.srw_v0_file(w, h, strip, offs)
    best, exact = None, True
    for _ in range(reps):
        t0 = time.perf_counter()
        st, dec = ref.decode_file(blob, threads=1)
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
        exact &= st == 0 and np.array_equal(dec.u16()[:h, :w], img)
        dec.close()
    return round(best, 2), bool(exact)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    from rawspeed_amd import capi
    ctx = capi.Context(0)
    res = {"metric": "samsung_v0_decode"}
    exact = True
    for sname, p_up in SETTINGS:
        for fname, (w, h) in FRAMES:
            rows, strip, offs, img = make_frame(w, h, p_up)
            leg = device_leg(ctx, torch, strip, offs, img, args.steps, args.warmup)
            hms, hex_ = host_leg(ctx, strip, offs, img)
            r1, e1 = ref_leg(strip, offs, img)
            leg.update({"host_call_ms": hms, "ref_1t_ms": r1})
            if r1:
                leg["speedup_vs_ref_1t"] = round(r1 / leg["kernel_ms"], 1)
            exact &= leg["bit_exact"] and hex_ and e1 is not False
            res["%s_%s" % (fname, sname)] = leg
            if fname == "nx":
                leg8 = device_leg(ctx, torch, strip, offs, img, args.steps, args.warmup, frames=8)
                exact &= leg8["bit_exact"]
                res["nx_x8_%s" % sname] = leg8
    res["bit_exact"] = bool(exact)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
