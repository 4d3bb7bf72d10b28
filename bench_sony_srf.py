"""Sony SRF benchmark (ArwDecoder::SonyDecrypt + decodeSRF, rsx_sony_srf.hip).  One 3360 x 2460
frame (the DSC-F828's limit in decodeSRF; 16.5 MB of seeded bytes), input and output resident in
HBM:
  plan1, plan8      plans of that many frames, the kernel's hipEvent time from
                    rsx_plan_kernel_table (the jobs of a plan read the same input bytes; their
                    outputs are their own)
  decrypt           rsx_sony_decrypt over the same bytes with device pointers, in place: the call's
                    wall time (it makes its plan, runs it and waits)
  copy_probe        rsx_probe_stream_copy over the frame's bytes in and out, in the same run: the
                    floor of any pass over the bytes
  host_pointers     rsx_sony_srf_decompress through host pointers
  host_build        librsx_sony_srf_host.so on one thread: the reference's loop restated (the ring
                    of SonyDecrypt, then the 16-bit big-endian read); the reference itself cannot
                    be run for this path here
Every leg's output is hashed against the host build's, which tests/test_sony_srf_model.py pins to
the model, before it is timed.  Prints one JSON line and, with --out, writes it."""
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

W, H, KEY = 3360, 2460, 0x1234ABCD


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def host_build(data, reps=3):
    import sony_srf_files as F
    best = {"decode": None, "decrypt": None}
    digest = None
    for _ in range(reps):
        t0 = time.perf_counter()
        st, px = F.host_decode(data, KEY, W, H)
        dt = (time.perf_counter() - t0) * 1e3
        assert st == 0
        digest = sha(px)
        best["decode"] = dt if best["decode"] is None else min(best["decode"], dt)
        dec = data.copy()
        t0 = time.perf_counter()
        F.host_lib().rsx_sony_srf_host_decrypt(dec.ctypes.data, dec.ctypes.data, dec.size // 4, KEY)
        dt = (time.perf_counter() - t0) * 1e3
        best["decrypt"] = dt if best["decrypt"] is None else min(best["decrypt"], dt)
    return {"decode_ms_1_thread": round(best["decode"], 2),
            "decrypt_ms_1_thread": round(best["decrypt"], 2)}, digest, sha(dec)


def plan_leg(ctx, torch, data, n_frames, want, steps, warmup):
    from rawspeed_amd import abi
    jobs = []
    for k in range(n_frames):
        j = abi.SonySrfJob()
        j.in_offset, j.in_bytes, j.img_offset, j.key = 0, len(data), k * 2 * W * H, KEY
        j.img = abi.Image(None, 2 * W, W, H, 1, 1)
        jobs.append(j)
    inp = torch.from_numpy(data).cuda()
    out = torch.zeros(n_frames * 2 * W * H, dtype=torch.uint8, device="cuda")
    plan = ctx.sony_srf_plan(jobs)
    s = torch.cuda.current_stream().cuda_stream
    plan.run(inp.data_ptr(), out.data_ptr(), s)
    exact = plan.results()[0] == 0
    for k in sorted({0, n_frames - 1}):
        exact &= sha(out[k * 2 * W * H:(k + 1) * 2 * W * H].cpu().numpy()) == want
    for _ in range(warmup):
        plan.run(inp.data_ptr(), out.data_ptr(), s)
    plan.results()
    plan.set_timing(True)
    t0 = time.perf_counter()
    for _ in range(steps):
        plan.run(inp.data_ptr(), out.data_ptr(), s)
    plan.results()
    wall = (time.perf_counter() - t0) / steps * 1e3
    table, runs = plan.kernel_table()
    plan.close()
    (kname, ms), = table
    return {"frames": n_frames, "kernel": kname, "kernel_ms": round(ms, 4),
            "kernel_ms_per_frame": round(ms / n_frames, 4), "wall_ms_per_step": round(wall, 3),
            "gb_s": round(n_frames * 4 * W * H / (ms * 1e-3) / 1e9, 1), "runs": runs,
            "bit_exact": bool(exact)}


def decrypt_leg(ctx, torch, data, want_dec, reps=5):
    buf = torch.from_numpy(data).cuda()
    n = len(data) // 4
    st = ctx.sony_decrypt(None, KEY, in_ptr=buf.data_ptr(), out_ptr=buf.data_ptr(), n_words=n)
    torch.cuda.synchronize()
    exact = st == 0 and sha(buf.cpu().numpy()) == want_dec
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        ctx.sony_decrypt(None, KEY, in_ptr=buf.data_ptr(), out_ptr=buf.data_ptr(), n_words=n)
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return {"device_call_ms": round(best, 3), "bit_exact": bool(exact)}


def host_pointer_leg(ctx, data, want, reps=3):
    from oracle_lib import HostImage
    best, exact = None, True
    raw = data.tobytes()
    for _ in range(reps):
        out = HostImage(W, H)
        t0 = time.perf_counter()
        st = ctx.sony_srf_decompress(raw, KEY, out.view())
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
        exact &= st == 0 and sha(out.pixels()) == want
    return {"host_call_ms": round(best, 2), "bit_exact": bool(exact)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--plans", default="1,8")
    ap.add_argument("--out")
    args = ap.parse_args()
    import sony_srf_files as F
    data = F.payload(2 * W * H, seed=11)
    res = {"metric": "sony_srf", "width": W, "height": H, "bytes": int(data.size),
           "chunk_words": F.CHUNK, "chunks": (data.size // 4 + F.CHUNK - 1) // F.CHUNK}
    res["host_build"], want, want_dec = host_build(data)
    import torch
    from rawspeed_amd import capi
    ctx = capi.Context(0)
    exact = True
    for n in [int(v) for v in args.plans.split(",")]:
        leg = plan_leg(ctx, torch, data, n, want, args.steps, args.warmup)
        exact &= leg["bit_exact"]
        res["plan%d" % n] = leg
    inp = torch.from_numpy(data).cuda()
    out = torch.zeros(data.size, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    probe = [ctx.probe_stream_copy(inp.data_ptr(), inp.numel(), out.data_ptr(), out.numel(), s,
                                   reps=max(args.steps, 5)) for _ in range(3)]
    res["copy_probe_ms"] = round(float(np.median(probe)), 4)
    res["decrypt"] = decrypt_leg(ctx, torch, data, want_dec)
    res["host_pointers"] = host_pointer_leg(ctx, data, want)
    exact &= res["decrypt"]["bit_exact"] and res["host_pointers"]["bit_exact"]
    res["bit_exact"] = bool(exact)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
