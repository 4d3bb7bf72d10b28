"""Panasonic RW2 V4 benchmark: an 8316x5640 frame for both values of section_split_offset, decoded
with the input and output resident in HBM (one plan launch per step, the kernel's hipEvent time
from rsx_plan_kernel_table, the image at the RawImage's pitch; --repeats timed rounds of --steps,
the median round and the spread between the rounds), with the zero-pixel list collected (uniform
random bytes: a few zero pixels in EVERY workgroup), without it, on a frame with 896 zero pixels
in all (what a camera's file looks like) and on a frame of half-zero bytes whose list is long.
Yardsticks from the same run: (a) the V6/12 plan, the other layout of 14 pixels a packet, on the
same frame size, (b) the project's
14-bit rsx_unpack_plan on the same pixel count, (c) the unmodified reference (oracle/_ref,
whole-file decode) on --threads host threads -- the new-style file at full size, the old-style
file at 4326x2751, the largest Rw2Decoder takes.  Before it is timed every device output is
compared bit for bit with the model tests/rw2_v4_files.py on its first rows (pinned against the
reference by tests/test_panasonic_v4_model.py) and with the reference where there is one, and
the list with the zero pixels of the whole image.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_panasonic import PEAK_BPS, device_leg, make_frame, out_pitch, summary, timed_rounds, unpack_leg  # noqa: E402

FRAME = (8316, 5640)       # 14 * 594 columns
OLD_STYLE = (4326, 2751)   # Rw2Decoder.cpp:80
MODEL_ROWS = 64            # 38 016 packets: 37 blocks and a part


def v4_leg(ctx, torch, split, flag, w, h, data, steps, warmup, repeats, ref_img=None):
    import rw2_v4_files as V
    from rawspeed_amd import abi
    j = abi.PanasonicV4Job()
    j.desc = abi.PanasonicV4Desc(split, flag)
    j.in_offset, j.in_bytes, j.img_offset = 0, data.size, 0
    j.img = abi.Image(None, out_pitch(w), w, h, 1, 1)
    j.bad_cap = w * h
    inp = torch.from_numpy(data).cuda()
    out = torch.zeros(out_pitch(w) * h, dtype=torch.uint8, device="cuda")
    plan = ctx.panasonic_v4_plan([j])
    s = torch.cuda.current_stream().cuda_stream
    # bit-exactness of what is about to be timed
    plan.run(inp.data_ptr(), out.data_ptr(), s)
    rc, st, cons = plan.results()
    lst, n_bad, bad = plan.bad_pixels(0, w * h)
    got = out.cpu().numpy().view(np.uint16).reshape(h, out_pitch(w) // 2)[:, :w]
    exact = rc == 0 and lst == 0 and cons == [V.consumed(split, w, h)]
    img, _ = V.model_decode(split, w, MODEL_ROWS, data)
    exact &= np.array_equal(got[:MODEL_ROWS], img)
    if ref_img is not None:
        exact &= np.array_equal(got, ref_img)
    exact &= np.array_equal(bad, V.zero_list(got)) if flag else n_bad == 0
    rounds, table = timed_rounds(plan, lambda: plan.run(inp.data_ptr(), out.data_ptr(), s),
                                 steps, warmup, repeats)
    plan.close()
    leg = summary(rounds, w * h, (w * h // 14) * (16 + 28))
    leg.update(kernels=table, bit_exact=bool(exact), n_bad=int(n_bad), w=w, h=h)
    return leg


def few_zeros(rng, split, w, h, packets=64):
    """What a camera's file looks like to the list: no byte has a zero nibble, so no 8-bit field is
    zero and no pixel either, but for `packets` all-zero packets (896 dead pixels)"""
    import rw2_v4_files as V
    n = V.consumed(split, w, h)
    a = (rng.integers(1, 16, size=n, dtype=np.uint8) << 4) | rng.integers(1, 16, size=n, dtype=np.uint8)
    for p in rng.integers(0, w * h // 14, size=packets):
        a[V.packet_offsets(split, int(p))] = 0
    return a


def host_leg(ctx, split, w, h, data, cap, reps=3):
    from oracle_lib import HostImage
    best = None
    for _ in range(reps):
        out = HostImage(w, h)
        t0 = time.perf_counter()
        st, n_bad, bad = ctx.panasonic_v4_decompress(split, 1, data, out.view(), cap)
        dt = (time.perf_counter() - t0) * 1e3
        assert st == 0, st
        best = dt if best is None else min(best, dt)
    return round(best, 3)


def ref_leg(split, w, h, data, threads, reps=2):
    """(best ms, the reference's image); "not measured" without oracle/_ref"""
    import rw2_v4_files as V
    from oracle_lib import Ref
    if not Ref.available():
        return "not measured", None
    ref = Ref()
    blob = V.v4_file(split, w, h, data)
    best, img = None, None
    for _ in range(reps):
        t0 = time.perf_counter()
        st, dec = ref.decode_file(blob, threads=threads)
        dt = (time.perf_counter() - t0) * 1e3
        assert st == 0, ref.last_error()
        best = dt if best is None else min(best, dt)
        img = dec.u16()[:h, :w].copy()
        dec.close()
    return round(best, 2), img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    import torch
    import rw2_v4_files as V
    from rawspeed_amd import capi
    ctx = capi.Context(0)
    res = {"metric": "panasonic_v4_decode", "threads": args.threads, "peak_bps": PEAK_BPS,
           "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats}
    exact = True
    w, h = FRAME
    run = (args.steps, args.warmup, args.repeats)
    for split in V.SPLITS:
        rng = np.random.default_rng([0x9A4, split])
        data = V.random_stream(rng, split, w, h, "uniform")
        name = "split_%x" % split
        ref_ms, ref_img = ref_leg(split, w, h, data, args.threads) if split else ("not measured", None)
        leg = v4_leg(ctx, torch, split, 1, w, h, data, *run, ref_img=ref_img)
        leg["ref_threads_ms"] = ref_ms
        if isinstance(ref_ms, float):
            leg["speedup_kernel_vs_ref_threads"] = round(ref_ms / leg["kernel_ms"], 1)
        leg["host_call_ms"] = host_leg(ctx, split, w, h, data, leg["n_bad"])
        res[name] = leg
        exact &= leg["bit_exact"]
        if split:
            res[name + "_no_list"] = v4_leg(ctx, torch, split, 0, w, h, data, *run, ref_img=ref_img)
            res[name + "_few_zeros"] = v4_leg(ctx, torch, split, 1, w, h, few_zeros(rng, split, w, h), *run)
            exact &= res[name + "_few_zeros"]["bit_exact"]
            half = V.random_stream(rng, split, w, h, "half")
            res[name + "_half_zero"] = v4_leg(ctx, torch, split, 1, w, h, half, *run)
            exact &= res[name + "_no_list"]["bit_exact"] and res[name + "_half_zero"]["bit_exact"]
    # the reference on the largest old-style file
    ow, oh = OLD_STYLE
    rng = np.random.default_rng([0x9A4, 2])
    data = V.random_stream(rng, 0, ow, oh, "uniform")
    ref_ms, ref_img = ref_leg(0, ow, oh, data, args.threads)
    leg = v4_leg(ctx, torch, 0, 1, ow, oh, data, *run, ref_img=ref_img)
    leg["ref_threads_ms"] = ref_ms
    res["split_0_old_style_max"] = leg
    exact &= leg["bit_exact"]
    # yardstick (a): V6/12, 14 pixels a packet; (b): the 14-bit unpack
    v6 = device_leg(ctx, torch, [(6, 12, w, h, make_frame(6, 12, w, h, 1))], *run, check=0)
    res["v6_12"] = v6
    u = unpack_leg(ctx, torch, w, h, *run)
    res["unpack14"] = u
    for name in ("split_0", "split_%x" % V.SPLIT):
        res[name]["vs_v6_12"] = round(res[name]["kernel_ms"] / v6["kernel_ms"], 3)
        res[name]["vs_unpack14"] = round(res[name]["kernel_ms"] / u["kernel_ms"], 3)
    res["bit_exact"] = bool(exact)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
