"""IiqDecoder::CorrectPhaseOneC benchmark (include/rsx.h section 3n): an 11608 x 8708 frame (a 100 MP
back, inside PhaseOneDecompressor's 11976 x 8854) and the list luma flat field + chroma flat field +
quadrant curves.  Not part of bench.py.  One JSON line:

  device       the image resident in HBM: hipEvent times of iiq_ff_rows_kernel, iiq_ff_cols_kernel
               (both plan-creation work, run again by a timed run) and iiq_correct_kernel
               (rsx_plan_kernel_table), next to rsx_probe_stream_copy over the
               same 2 + 2 bytes a pixel in the same run -- the ceiling of a pass that reads and
               writes every pixel once
  cell_sweep   the fused pass at cell widths 8, 32, 128 and 512: what replaying the additions in
               front of a lane's first pixel costs (at most 31 per plane since cells wider than 32
               columns keep a start value every 32; before that, width - 1)
  host         rsx_phase_one_decompress_corrected against rsx_phase_one_decompress alone on the
               same frame through host pointers: what the corrections add before the one download
  defects      the same list with a sensor-defects op (RSX_IIQ_OP_SENSOR_DEFECTS): 16 bad columns
               scattered over the frame in front of and behind the flat fields, and a chain of 8
               adjacent columns (8 dependent launches).  Whole plan runs between two events, no
               per-kernel timing, the variants alternating inside every repeat; `added_us` is the
               median over the repeats of (variant - the same repeat's list without the op).  Next
               to it iiq_bad_columns_kernel's own time from a timed run, and the host build of the
               core on one thread for the op alone.  The front-16 list is compared bit for bit
               with the host build.
  host         ... and, with the op in front, rsx_phase_one_decompress_corrected with and without
               it, alternating
  reference    where oracle/_ref is built: the unmodified reference's whole-file decode with the
               correction block minus the one without, same process, one thread (its loops have
               no threads) -- luma + quadrant only, because its chroma needs a CFA that a decode
               without a camera database does not have

The device output of the main list is compared bit for bit with the host build of the same core
(rawspeed_amd/librsx_iiq_corr_host.so, pinned against the reference by tests/test_iiq_corr_model.py).
The cell sizes of real camera files are not known here: the sweep is the answer to that, and no
ratio is promised."""
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

W, H = 11608, 8708
GRBG = (2, 2, (1, 0, 2, 1))
BLACK, SPLIT_ROW, SPLIT_COL = 1024, H // 2, W // 2


def make_image():
    """a 14-bit ramp with noise: neighbouring pixels index neighbouring curve entries, as a
    photograph's do"""
    rng = np.random.default_rng(0x11C)
    base = (np.arange(W, dtype=np.float32)[None, :] * (9000.0 / W) + np.arange(H, dtype=np.float32)[:, None] * (5000.0 / H))
    img = base + rng.standard_normal((H, W), dtype=np.float32) * 40.0 + 1100.0
    return np.clip(img, 0, 16383).astype(np.uint16)


def make_ops(K, cell_w, cell_h, chroma=True):
    rng = np.random.default_rng([0x410, cell_w, cell_h])
    head = (0, 0, W + cell_w, H + cell_h, cell_w, cell_h)
    ops = [("ff", K.ff_random(rng, head, lo=31000, hi=35000), 0)]
    if chroma:
        ops.append(("ff", K.ff_random(rng, head, planes=2, lo=31000, hi=35000), 1))
    curves = K.quadrant_curves(K.quad_payload(K.QX, rng.integers(9700, 10300, size=(2, 2, 7))))
    ops.append(("quad", curves, SPLIT_ROW, SPLIT_COL, BLACK))
    return ops


def job_for(abi, ops):
    d, keep = abi.iiq_corr(ops, GRBG)
    j = abi.IiqCorrectJob()
    j.corr = d
    j.img_offset = 0
    j.img = abi.Image(None, 2 * W, W, H, 1, 1)
    return j, keep


def timed(plan, ptr, s, steps, repeats):
    out = {}
    for _ in range(repeats):
        plan.set_timing(True)
        for _ in range(steps):
            plan.run(ptr, ptr, s)
        plan.results()
        table_ms, runs = plan.kernel_table()
        plan.set_timing(False)
        for name, ms in table_ms:
            out.setdefault(name, []).append(ms)
    return {k: float(np.median(v)) for k, v in out.items()}, {k: [round(x, 4) for x in v] for k, v in out.items()}


def device_leg(ctx, torch, abi, K, img, args):
    from rawspeed_amd import build
    ops = make_ops(K, args.cell, args.cell)
    job, keep = job_for(abi, ops)
    dev = torch.from_numpy(img.reshape(-1).view(np.uint8)).cuda()
    other = torch.empty_like(dev)
    s = torch.cuda.current_stream().cuda_stream
    t0 = time.perf_counter()
    plan = ctx.iiq_correct_plan([job])
    create_ms = (time.perf_counter() - t0) * 1e3
    plan.run(dev.data_ptr(), dev.data_ptr(), s)
    rc, _, _ = plan.results()
    got = dev.cpu().numpy().view(np.uint16).reshape(H, W)
    # the same list through the host build of the core
    L = C.CDLL(build.build_iiq_corr_host()[0])
    L.rsx_iiq_corr_host_apply.argtypes = [C.c_void_p, C.c_void_p]
    want = img.copy()
    v = abi.Image(want.ctypes.data, 2 * W, W, H, 1, 1)
    t0 = time.perf_counter()
    st = L.rsx_iiq_corr_host_apply(C.byref(job.corr), C.byref(v))
    host_core_ms = (time.perf_counter() - t0) * 1e3
    exact = rc == 0 and st == 0 and np.array_equal(got, want)
    changed = float((got != img).mean())
    dev.copy_(torch.from_numpy(img.reshape(-1).view(np.uint8)))
    med, allv = timed(plan, dev.data_ptr(), s, args.steps, args.repeats)
    probe = [ctx.probe_stream_copy(dev.data_ptr(), dev.numel(), other.data_ptr(), dev.numel(), s, reps=args.steps)
             for _ in range(args.repeats)]
    plan.close()
    pms = float(np.median(probe))
    kb = med.get("iiq_correct_kernel", 0.0)
    return {"cell": [args.cell, args.cell], "ops": "luma+chroma+quadrant",
            "rows_kernel_ms": round(med.get("iiq_ff_rows_kernel", 0.0), 4),
            "cols_kernel_ms": round(med.get("iiq_ff_cols_kernel", 0.0), 4),
            "correct_kernel_ms": round(kb, 4), "kernel_ms_all": allv,
            "copy_probe_ms": round(pms, 4), "copy_probe_ms_all": [round(x, 4) for x in probe],
            "correct_frac_of_probe": round(pms / kb, 3) if kb else None,
            "gpix_s": round(W * H / (kb * 1e-3) / 1e9, 2) if kb else None,
            "plan_create_ms": round(create_ms, 3), "host_core_1t_ms": round(host_core_ms, 1),
            "pixels_changed_frac": round(changed, 4), "bit_exact": bool(exact)}, dev, s, want


def scattered_columns(n=16):
    return [int(c) | 1 for c in np.linspace(100, W - 100, n)]


def defects_leg(ctx, torch, abi, K, D, dev, s, img, args):
    from rawspeed_amd import build
    base = make_ops(K, args.cell, args.cell)
    far = ("defects", D.columns(scattered_columns()))
    chain = ("defects", D.columns(list(range(5001, 5009))))
    variants = {"list": base, "front16": [far] + base, "back16": base + [far], "chain8": [chain] + base}
    plans, keeps = {}, []
    for name, ops in variants.items():
        job, keep = job_for(abi, ops)
        keeps.append(keep)
        plans[name] = (ctx.iiq_correct_plan([job]), job)
    # the front-16 list against the host build of the core, bit for bit
    dev.copy_(torch.from_numpy(img.reshape(-1).view(np.uint8)))
    plans["front16"][0].run(dev.data_ptr(), dev.data_ptr(), s)
    rc, _, _ = plans["front16"][0].results()
    got = dev.cpu().numpy().view(np.uint16).reshape(H, W)
    L = C.CDLL(build.build_iiq_corr_host()[0])
    L.rsx_iiq_corr_host_apply.argtypes = [C.c_void_p, C.c_void_p]
    want = img.copy()
    st = L.rsx_iiq_corr_host_apply(C.byref(plans["front16"][1].corr), C.byref(abi.Image(want.ctypes.data, 2 * W, W, H, 1, 1)))
    exact = rc == 0 and st == 0 and np.array_equal(got, want)
    # the op alone on the host, one thread
    alone, keep = job_for(abi, [far])
    scratch = img.copy()
    host_ms = []
    for _ in range(5):
        t0 = time.perf_counter()
        L.rsx_iiq_corr_host_apply(C.byref(alone.corr), C.byref(abi.Image(scratch.ctypes.data, 2 * W, W, H, 1, 1)))
        host_ms.append((time.perf_counter() - t0) * 1e3)
    # whole runs on a stream of their own (a plan run on the null stream goes to the context's
    # stream, where these events would not see it), the variants alternating inside a repeat
    own = torch.cuda.Stream()
    torch.cuda.synchronize()
    for plan, _ in plans.values():
        for _ in range(3):
            plan.run(dev.data_ptr(), dev.data_ptr(), own.cuda_stream)
    own.synchronize()
    per = {k: [] for k in plans}
    for _ in range(args.repeats):
        for name, (plan, _) in plans.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(own)
            for _ in range(args.steps):
                plan.run(dev.data_ptr(), dev.data_ptr(), own.cuda_stream)
            e1.record(own)
            e1.synchronize()
            per[name].append(e0.elapsed_time(e1) / args.steps * 1e3)
    out = {"columns": {"front16": scattered_columns(), "chain8": [5001, 5008]},
           "run_us": {k: round(float(np.median(v)), 2) for k, v in per.items()},
           "run_us_all": {k: [round(x, 2) for x in v] for k, v in per.items()},
           "added_us": {k: round(float(np.median(np.array(per[k]) - np.array(per["list"]))), 2)
                        for k in per if k != "list"},
           "host_core_1t_op_alone_ms": round(float(np.median(host_ms)), 4),
           "bit_exact": bool(exact)}
    kernel = {}
    for name in ("front16", "chain8"):
        med, _ = timed(plans[name][0], dev.data_ptr(), s, args.steps, 3)
        kernel[name] = round(med.get("iiq_bad_columns_kernel", 0.0) * 1e3, 2)
    out["bad_columns_kernel_us_per_run"] = kernel
    for plan, _ in plans.values():
        plan.close()
    return out, want


def sweep_leg(ctx, abi, K, dev, s, args):
    out = {}
    for cw in (8, 32, 128, 512):
        job, keep = job_for(abi, make_ops(K, cw, 64))
        plan = ctx.iiq_correct_plan([job])
        med, _ = timed(plan, dev.data_ptr(), s, max(5, args.steps // 2), 3)
        plan.close()
        out[str(cw)] = {"correct_kernel_ms": round(med.get("iiq_correct_kernel", 0.0), 4),
                        "rows_kernel_ms": round(med.get("iiq_ff_rows_kernel", 0.0), 4),
                        "cols_kernel_ms": round(med.get("iiq_ff_cols_kernel", 0.0), 4)}
    return out


def host_leg(ctx, abi, K, F, img, want, args, reps=3, D=None, want_defects=None):
    from oracle_lib import HostImage
    rows = F.encode(img, 1)
    raw = np.frombuffer(b"".join(rows), np.uint8)
    strips, off = [], 0
    for r, b in enumerate(rows):
        strips.append((r, off, len(b)))
        off += len(b)
    ops = make_ops(K, args.cell, args.cell)
    d, keep = abi.iiq_corr(ops, GRBG)
    plain = corrected = None
    ok = True
    out = HostImage(W, H)
    for _ in range(reps):
        t0 = time.perf_counter()
        st, _ = ctx.phase_one_decompress(raw, strips, out.view())
        dt = (time.perf_counter() - t0) * 1e3
        plain = dt if plain is None else min(plain, dt)
        ok &= st == 0
    ok &= np.array_equal(out.pixels(), img)
    for _ in range(reps):
        t0 = time.perf_counter()
        st, _ = ctx.phase_one_decompress_corrected(raw, strips, d, out.view())
        dt = (time.perf_counter() - t0) * 1e3
        corrected = dt if corrected is None else min(corrected, dt)
        ok &= st == 0
    ok &= np.array_equal(out.pixels(), want)
    res = {"phase_one_decompress_ms": round(plain, 2), "decompress_corrected_ms": round(corrected, 2),
           "corrections_add_ms": round(corrected - plain, 2), "in_bytes": int(raw.size)}
    if D is not None:
        # the list with 16 scattered bad columns in front, and without, alternating
        d2, keep2 = abi.iiq_corr([("defects", D.columns(scattered_columns()))] + ops, GRBG)
        t = {"without": [], "with": []}
        for _ in range(2 * reps):
            for name, desc, expect in (("without", d, want), ("with", d2, want_defects)):
                t0 = time.perf_counter()
                st, _ = ctx.phase_one_decompress_corrected(raw, strips, desc, out.view())
                t[name].append((time.perf_counter() - t0) * 1e3)
                ok &= st == 0
                if len(t[name]) == 1:
                    ok &= np.array_equal(out.pixels(), expect)
        res["corrected_ms_all"] = {k: [round(x, 2) for x in v] for k, v in t.items()}
        res["corrected_with_defects_ms"] = round(float(np.median(t["with"])), 2)
        res["corrected_without_defects_ms"] = round(float(np.median(t["without"])), 2)
        res["defects_add_ms"] = round(float(np.median(np.array(t["with"]) - np.array(t["without"]))), 3)
    return res, ok


def ref_leg(K, img, args, reps=2):
    from oracle_lib import Ref
    if not Ref.available():
        return None
    ref = Ref()
    rng = np.random.default_rng([0x410, args.cell, args.cell])
    head = (0, 0, W + args.cell, H + args.cell, args.cell, args.cell)
    luma = K.ff_random(rng, head, lo=31000, hi=35000)
    qp = K.quad_payload(K.QX, rng.integers(9700, 10300, size=(2, 2, 7)))
    with_meta = K.iiq_corr_file(img, K.meta_block([(0x410, luma), (0x431, qp)]), BLACK, SPLIT_ROW, SPLIT_COL)
    without = K.iiq_corr_file(img)
    best = {}
    for name, blob in (("without", without), ("with", with_meta)):
        for _ in range(reps):
            t0 = time.perf_counter()
            st, dec = ref.decode_file(blob)
            dt = (time.perf_counter() - t0) * 1e3
            assert st == 0, ref.last_error()
            dec.close()
            best[name] = min(best.get(name, dt), dt)
    return {"ops": "luma+quadrant", "decode_ms": round(best["without"], 1),
            "decode_corrected_ms": round(best["with"], 1),
            "corrections_1t_ms": round(best["with"] - best["without"], 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cell", type=int, default=64)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-ref", action="store_true")
    args = ap.parse_args()
    import torch
    import iiq_corr_files as K
    import iiq_defect_files as D
    import iiq_files as F
    from rawspeed_amd import abi, capi
    ctx = capi.Context(0)
    img = make_image()
    res = {"metric": "iiq_corrections", "frame": [W, H],
           "note": "cell sizes of real camera files are not known here; see cell_sweep"}
    res["device"], dev, s, want = device_leg(ctx, torch, abi, K, img, args)
    res["cell_sweep"] = sweep_leg(ctx, abi, K, dev, s, args)
    res["defects"], want_defects = defects_leg(ctx, torch, abi, K, D, dev, s, img, args)
    exact = res["device"]["bit_exact"] and res["defects"]["bit_exact"]
    del dev
    if not args.no_host:
        res["host"], ok = host_leg(ctx, abi, K, F, img, want, args, D=D, want_defects=want_defects)
        exact &= ok
    if not args.no_ref:
        res["reference"] = ref_leg(K, img, args)
    res["bit_exact"] = bool(exact)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
