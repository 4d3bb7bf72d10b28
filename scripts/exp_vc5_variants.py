"""GPU experiment: the VC-5 band kernel (rsx_vc5.hip) built with other workgroup sizes and segment
lengths (-DRSX_VC5_THREADS, -DRSX_VC5_SEG_BITS; A/B builds loaded through RSX_LIB) on the frames of
bench_vc5.py: one frame and a batch of eight, kernel times, rounds per window, bit-exactness
against the host build of the core.  The numbers of DESIGN.md 4.13 come from this script.

  python scripts/exp_vc5_variants.py --build   cross-compiles the variants (no GPU needed): only
                                               rsx_vc5.hip is compiled again, the other objects
                                               are the core library's
  python scripts/exp_vc5_variants.py           one child process per build, one after the other;
                                               stops at the first child that fails; prints one
                                               JSON line
"""
import argparse
import json
import os
import pickle
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# name -> (lanes of a workgroup = segments of a window, bits of a segment)
BUILT = (1024, 128)  # the library as built
VARIANTS = {"t1024_s128": BUILT, "t512_s128": (512, 128), "t256_s128": (256, 128),
            "t1024_s64": (1024, 64), "t1024_s256": (1024, 256), "t512_s256": (512, 256),
            "t512_s512": (512, 512), "t1024_s512": (1024, 512)}


def lib_path(name):
    from rawspeed_amd import build
    if VARIANTS[name] == BUILT:
        return build.LIB_CORE
    return os.path.join(build.PKG, "variants", "librsx_vc5_%s.so" % name)


def build_variants():
    from rawspeed_amd import build
    build.build_core()
    objdir = os.path.join(build.PKG, "_build", "core")
    os.makedirs(os.path.join(build.PKG, "variants"), exist_ok=True)
    others = [os.path.join(objdir, os.path.splitext(s)[0] + ".o") for s in build.CORE_SOURCES
              if s != "rsx_vc5.hip"]
    for name, (lanes, seg) in VARIANTS.items():
        if (lanes, seg) == BUILT:
            continue
        obj = os.path.join(build.PKG, "_build", "vc5_%s.o" % name)
        build._run([build._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", "-Wall",
                    "-Wno-unused-function", "-I" + build.INCLUDE, "-I" + build.CSRC,
                    "-DRSX_VC5_THREADS=%d" % lanes, "-DRSX_VC5_SEG_BITS=%d" % seg,
                    "-o", obj, os.path.join(build.CSRC, "rsx_vc5.hip")])
        build._link(lib_path(name), others + [obj])
        print("built", lib_path(name))


def child(frames_file, steps, batch):
    import torch
    import bench_vc5 as B
    from rawspeed_amd import capi
    with open(frames_file, "rb") as f:
        frames, img = pickle.load(f)
    ctx = capi.Context(0)
    one = B.device_leg(ctx, torch, [frames[0]], [img], steps, 2, 3)
    many = B.device_leg(ctx, torch, [frames[k % 2] for k in range(batch)], [img] + [None] * (batch - 1),
                        max(3, steps // 2), 2, 3)
    print(json.dumps({"one_frame": one, "batch%d" % batch: many}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--child", nargs=2, metavar=("NAME", "FRAMES"))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--only", nargs="*", default=list(VARIANTS))
    args = ap.parse_args()
    if args.build:
        return build_variants()
    if args.child:
        return child(args.child[1], args.steps, args.batch)
    import bench_vc5 as B
    frames = [B.make_frame(k) for k in range(2)]
    data, bands = frames[0].vc5_block()
    img = B.host_core_image(frames[0], data, bands)
    res = {"metric": "vc5_band_variants", "frame": [B.W, B.H], "variants": {}}
    with tempfile.TemporaryDirectory() as d:
        ff = os.path.join(d, "frames.pkl")
        with open(ff, "wb") as f:
            pickle.dump((frames, img), f)
        for name in args.only:
            if not os.path.exists(lib_path(name)):
                res["variants"][name] = "not built"
                continue
            env = dict(os.environ, RSX_LIB=lib_path(name))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, ff,
                                "--steps", str(args.steps), "--batch", str(args.batch)],
                               env=env, stdout=subprocess.PIPE, text=True, timeout=300)
            if r.returncode != 0:  # nothing more on the device after a child that failed
                res["variants"][name] = "exit %d" % r.returncode
                break
            lanes, seg = VARIANTS[name]
            res["variants"][name] = dict(json.loads(r.stdout.strip().splitlines()[-1]), lanes=lanes,
                                         segment_bits=seg, window_kbit=lanes * seg // 1024)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
