"""In-tree builds of the native libraries (no JIT cache, no site-packages).

  rawspeed_amd/librsx.so        HIP kernels + C-ABI, hipcc --offload-arch=gfx950
  rawspeed_amd/librsx_synth.so  host-side stream writers (gcc)
  rawspeed_amd/librsx_inflate_host.so, rawspeed_amd/rsx_inflate_host_check
                                the inflate core of the deflate DNG kernel as host C++ (g++)
  rawspeed_amd/librsx_vc5_host.so, rawspeed_amd/rsx_vc5_host_check
                                the VC-5 core (rsx_vc5_core.h) as host C++ (g++)
  rawspeed_amd/librsx_iiq_corr_host.so, rawspeed_amd/rsx_iiq_corr_host_check
                                the IIQ correction core (rsx_iiq_corr_core.h) as host C++ (g++)
  rawspeed_amd/librsx_dng_post_host.so, rawspeed_amd/rsx_dng_post_host_check
                                the DNG opcode / look-up core (rsx_dng_post_core.h) as host C++ (g++)
  rawspeed_amd/librsx_bad_pixels_host.so, rawspeed_amd/rsx_bad_pixels_host_check
                                the bad-pixel core (rsx_bad_pixels_core.h) as host C++ (g++)
  rawspeed_amd/librsx_scale_host.so, rawspeed_amd/rsx_scale_host_check
                                the black/white scaling core (rsx_scale_core.h) as host C++ (g++)
  rawspeed_amd/librsx_jpeg_host.so, rawspeed_amd/rsx_jpeg_host_check
                                the lossy-JPEG tile core (rsx_jpeg_core.h) as host C++ (g++)
  rawspeed_amd/librsx_fuji_host.so, rawspeed_amd/rsx_fuji_host_check
                                the compressed-RAF core (rsx_fuji_core.h) as host C++ (g++)
  rawspeed_amd/librsx_olympus_host.so, rawspeed_amd/rsx_olympus_host_check
                                the compressed-ORF core (rsx_olympus_core.h) as host C++ (g++)
  rawspeed_amd/librsx_kodak_host.so, rawspeed_amd/rsx_kodak_host_check
                                the Kodak DCR core (rsx_kodak_core.h) as host C++ (g++)
  rawspeed_amd/librsx_crw_host.so, rawspeed_amd/rsx_crw_host_check
                                the Canon CRW core (rsx_crw_core.h) as host C++ (g++)
  rawspeed_amd/librsx_fuji_rotate_host.so, rawspeed_amd/rsx_fuji_rotate_host_check
                                the SuperCCD rotation core (rsx_fuji_rotate_core.h) as host C++ (g++)
  rawspeed_amd/librsx_sony_srf_host.so, rawspeed_amd/rsx_sony_srf_host_check
                                the Sony SRF core (rsx_sony_srf_core.h) as host C++ (g++)
  rawspeed_amd/librsx_image_hash_host.so, rawspeed_amd/rsx_image_hash_host_check
                                the image hash core (rsx_image_hash_core.h) as host C++ (g++)
  rawspeed_amd/librsx_encode_host.so, rawspeed_amd/rsx_encode_host_check
                                the writers' core (rsx_encode_core.h) as host C++ (g++)
  rawspeed_amd/librsx_fpwrite_host.so, rawspeed_amd/rsx_fpwrite_host_check
                                the F32 writers' core (rsx_fpwrite_core.h, rsx_fp_narrow.h) as host
                                C++ (g++)
  rawspeed_amd/librsx_dctwrite_host.so, rawspeed_amd/rsx_dctwrite_host_check
                                the baseline-JPEG writer's core (rsx_dctwrite_core.h) as host C++ (g++)

hipcc cross-compiles gfx950 without a GPU, so this runs in the build container
as well as on the MI355X box.  A library is rebuilt only when a source is newer.
"""
import os
import shutil
import subprocess

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
INCLUDE = os.path.join(ROOT, "include")

LIB_CORE = os.path.join(PKG, "librsx.so")
LIB_SYNTH = os.path.join(PKG, "librsx_synth.so")
LIB_INFLATE_HOST = os.path.join(PKG, "librsx_inflate_host.so")
BIN_INFLATE_CHECK = os.path.join(PKG, "rsx_inflate_host_check")
LIB_VC5_HOST = os.path.join(PKG, "librsx_vc5_host.so")
BIN_VC5_CHECK = os.path.join(PKG, "rsx_vc5_host_check")
LIB_IIQ_CORR_HOST = os.path.join(PKG, "librsx_iiq_corr_host.so")
BIN_IIQ_CORR_CHECK = os.path.join(PKG, "rsx_iiq_corr_host_check")
LIB_DNG_POST_HOST = os.path.join(PKG, "librsx_dng_post_host.so")
BIN_DNG_POST_CHECK = os.path.join(PKG, "rsx_dng_post_host_check")
LIB_BAD_PIXELS_HOST = os.path.join(PKG, "librsx_bad_pixels_host.so")
BIN_BAD_PIXELS_CHECK = os.path.join(PKG, "rsx_bad_pixels_host_check")
LIB_SCALE_HOST = os.path.join(PKG, "librsx_scale_host.so")
BIN_SCALE_CHECK = os.path.join(PKG, "rsx_scale_host_check")
LIB_JPEG_HOST = os.path.join(PKG, "librsx_jpeg_host.so")
BIN_JPEG_CHECK = os.path.join(PKG, "rsx_jpeg_host_check")
LIB_FUJI_HOST = os.path.join(PKG, "librsx_fuji_host.so")
BIN_FUJI_CHECK = os.path.join(PKG, "rsx_fuji_host_check")
LIB_OLYMPUS_HOST = os.path.join(PKG, "librsx_olympus_host.so")
BIN_OLYMPUS_CHECK = os.path.join(PKG, "rsx_olympus_host_check")
LIB_KODAK_HOST = os.path.join(PKG, "librsx_kodak_host.so")
BIN_KODAK_CHECK = os.path.join(PKG, "rsx_kodak_host_check")
LIB_CRW_HOST = os.path.join(PKG, "librsx_crw_host.so")
BIN_CRW_CHECK = os.path.join(PKG, "rsx_crw_host_check")
LIB_FUJI_ROTATE_HOST = os.path.join(PKG, "librsx_fuji_rotate_host.so")
BIN_FUJI_ROTATE_CHECK = os.path.join(PKG, "rsx_fuji_rotate_host_check")
LIB_SONY_SRF_HOST = os.path.join(PKG, "librsx_sony_srf_host.so")
BIN_SONY_SRF_CHECK = os.path.join(PKG, "rsx_sony_srf_host_check")
LIB_IMAGE_HASH_HOST = os.path.join(PKG, "librsx_image_hash_host.so")
BIN_IMAGE_HASH_CHECK = os.path.join(PKG, "rsx_image_hash_host_check")
LIB_ENCODE_HOST = os.path.join(PKG, "librsx_encode_host.so")
BIN_ENCODE_CHECK = os.path.join(PKG, "rsx_encode_host_check")
LIB_FPWRITE_HOST = os.path.join(PKG, "librsx_fpwrite_host.so")
BIN_FPWRITE_CHECK = os.path.join(PKG, "rsx_fpwrite_host_check")
LIB_DCTWRITE_HOST = os.path.join(PKG, "librsx_dctwrite_host.so")
BIN_DCTWRITE_CHECK = os.path.join(PKG, "rsx_dctwrite_host_check")

CORE_SOURCES = ["rsx_api.hip", "rsx_unpack.hip", "rsx_ljpeg.hip", "rsx_ljpeg_direct.hip",
                "rsx_ljpeg_fast.hip", "rsx_ljpeg_recon.hip", "rsx_sraw.hip", "rsx_samsung_v2.hip",
                "rsx_phase_one.hip", "rsx_sony_arw2.hip", "rsx_panasonic.hip", "rsx_samsung_v0.hip",
                "rsx_panasonic_v4.hip", "rsx_dng_deflate.hip", "rsx_nikon_snef.hip", "rsx_vc5.hip",
                "rsx_iiq_corr.hip", "rsx_iiq_defects.hip", "rsx_dng_post.hip", "rsx_bad_pixels.hip", "rsx_scale.hip",
                "rsx_dng_jpeg.hip", "rsx_fuji.hip", "rsx_olympus.hip", "rsx_kodak.hip",
                "rsx_crw.hip", "rsx_fuji_rotate.hip", "rsx_sony_srf.hip",
                "rsx_image_hash.hip", "rsx_encode_pack.hip", "rsx_encode_ljpeg.hip",
                "rsx_fpwrite_pack.hip", "rsx_fpwrite_deflate.hip", "rsx_dctwrite.hip", "rsx_host.cpp"]
CORE_HEADERS = ["rsx_internal.h", "rsx_plan_host.h", "rsx_device.h", "rsx_stamp.h", "rsx_ljpeg.h", "rsx_ljpeg_dev.h",
                "rsx_ljpeg_bits.h", "rsx_samsung_v2.h", "rsx_phase_one.h",
                "rsx_sony_arw2.h", "rsx_panasonic.h", "rsx_samsung_v0.h",
                "rsx_panasonic_dev.h", "rsx_panasonic_v4.h", "rsx_dng_deflate.h",
                "rsx_inflate_core.h", "rsx_fp_widen.h", "rsx_dither_dev.h", "rsx_nikon_snef.h",
                "rsx_vc5.h", "rsx_vc5_core.h", "rsx_iiq_corr.h", "rsx_iiq_corr_core.h",
                "rsx_dng_post.h", "rsx_dng_post_core.h", "rsx_bad_pixels.h",
                "rsx_bad_pixels_core.h", "rsx_scale.h", "rsx_scale_core.h",
                "rsx_dng_jpeg.h", "rsx_jpeg_core.h", "rsx_fuji.h", "rsx_fuji_core.h",
                "rsx_olympus.h", "rsx_olympus_core.h", "rsx_kodak.h", "rsx_kodak_core.h",
                "rsx_crw.h", "rsx_crw_core.h", "rsx_crw_tables.h", "rsx_fuji_rotate.h",
                "rsx_fuji_rotate_core.h", "rsx_sony_srf.h", "rsx_sony_srf_core.h",
                "rsx_image_hash.h", "rsx_image_hash_core.h", "rsx_encode.h", "rsx_encode_core.h",
                "rsx_fpwrite.h", "rsx_fpwrite_core.h", "rsx_fp_narrow.h",
                "rsx_deflate_core.h", "rsx_dctwrite.h", "rsx_dctwrite_core.h"]


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found")


def _stale(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources if os.path.exists(s))


def _run(cmd):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("build failed: %s\n%s" % (" ".join(cmd), r.stdout))
    return r.stdout


SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
            "-static-libubsan"]


def _links_with_sanitizers():
    """whether g++ has the runtimes of SANITIZE: an empty program links with them"""
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        with open(src, "w") as f:
            f.write("int main() { return 0; }\n")
        r = subprocess.run(["g++", src, "-o", os.path.join(d, "t")] + SANITIZE,
                           stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return r.returncode == 0


def build_synth(force=False):
    src = os.path.join(CSRC, "synth", "rsx_synth.c")
    if force or _stale(LIB_SYNTH, [src, os.path.join(CSRC, "rsx_crw_tables.h")]):
        _run(["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-Wall", "-Wextra",
              "-o", LIB_SYNTH, src])
    return LIB_SYNTH


def _build_host_core(lib, check_bin, src, deps, main_macro, extra_flags, force=False):
    """A kernel's core header as host C++ (csrc/`src`; `deps`: what it includes): the library the
    tests load, and the same source with -D`main_macro` as a program with AddressSanitizer and
    UBSan (an instrumented library cannot be loaded into an uninstrumented Python; the program
    runs its built-in cases and the corpus or case file a test hands it).  Only where an empty
    program does not link with the runtimes is the program built plain: an error of the
    instrumented build is an error."""
    src = os.path.join(CSRC, src)
    deps = [src] + [os.path.join(CSRC, d) for d in deps]
    base = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-I" + CSRC,
            *extra_flags]
    if force or _stale(lib, deps):
        _run(base + ["-O2", "-fPIC", "-shared", "-o", lib, src])
    if force or _stale(check_bin, deps):
        main = base + ["-O1", "-g", "-D" + main_macro, "-o", check_bin, src]
        _run(main + SANITIZE if _links_with_sanitizers() else main)
    return lib, check_bin


# binary32 as the device computes it (no contraction), and the public header
_NO_CONTRACT = ["-ffp-contract=off", "-I" + INCLUDE]
_RSX_H = os.path.join(INCLUDE, "rsx.h")


def build_inflate_host(force=False):
    """rsx_inflate_core.h with a wave of one lane"""
    return _build_host_core(LIB_INFLATE_HOST, BIN_INFLATE_CHECK, "rsx_inflate_host.cpp",
                            ["rsx_inflate_core.h"], "RSX_INFLATE_HOST_MAIN", [], force)


def build_vc5_host(force=False):
    """rsx_vc5_core.h"""
    return _build_host_core(LIB_VC5_HOST, BIN_VC5_CHECK, "rsx_vc5_host.cpp",
                            ["rsx_vc5_core.h"], "RSX_VC5_HOST_MAIN", [], force)


def build_iiq_corr_host(force=False):
    """rsx_iiq_corr_core.h, binary32 without contraction"""
    return _build_host_core(LIB_IIQ_CORR_HOST, BIN_IIQ_CORR_CHECK, "rsx_iiq_corr_host.cpp",
                            ["rsx_iiq_corr_core.h", _RSX_H], "RSX_IIQ_CORR_HOST_MAIN", _NO_CONTRACT,
                            force)


def build_dng_post_host(force=False):
    """rsx_dng_post_core.h, without contraction"""
    return _build_host_core(LIB_DNG_POST_HOST, BIN_DNG_POST_CHECK, "rsx_dng_post_host.cpp",
                            ["rsx_dng_post_core.h", _RSX_H], "RSX_DNG_POST_HOST_MAIN", _NO_CONTRACT,
                            force)


def build_bad_pixels_host(force=False):
    """rsx_bad_pixels_core.h, without contraction; the row bands run on threads"""
    return _build_host_core(LIB_BAD_PIXELS_HOST, BIN_BAD_PIXELS_CHECK, "rsx_bad_pixels_host.cpp",
                            ["rsx_bad_pixels_core.h", _RSX_H], "RSX_BAD_PIXELS_HOST_MAIN",
                            ["-pthread"] + _NO_CONTRACT, force)


def build_scale_host(force=False):
    """rsx_scale_core.h, without contraction"""
    return _build_host_core(LIB_SCALE_HOST, BIN_SCALE_CHECK, "rsx_scale_host.cpp",
                            ["rsx_scale_core.h", "rsx_dither_dev.h", _RSX_H], "RSX_SCALE_HOST_MAIN",
                            _NO_CONTRACT, force)


def build_jpeg_host(force=False):
    """rsx_jpeg_core.h: integers only"""
    return _build_host_core(LIB_JPEG_HOST, BIN_JPEG_CHECK, "rsx_jpeg_host.cpp",
                            ["rsx_jpeg_core.h", _RSX_H], "RSX_JPEG_HOST_MAIN", ["-I" + INCLUDE],
                            force)


def build_fuji_host(force=False):
    """rsx_fuji_core.h: integers only; the strips of a frame run on threads"""
    return _build_host_core(LIB_FUJI_HOST, BIN_FUJI_CHECK, "rsx_fuji_host.cpp",
                            ["rsx_fuji_core.h", _RSX_H], "RSX_FUJI_HOST_MAIN",
                            ["-pthread", "-I" + INCLUDE], force)


def build_olympus_host(force=False):
    """rsx_olympus_core.h: integers only, one thread a frame"""
    return _build_host_core(LIB_OLYMPUS_HOST, BIN_OLYMPUS_CHECK, "rsx_olympus_host.cpp",
                            ["rsx_olympus_core.h", _RSX_H], "RSX_OLYMPUS_HOST_MAIN",
                            ["-I" + INCLUDE], force)


def build_kodak_host(force=False):
    """rsx_kodak_core.h: integers only, one thread a frame"""
    return _build_host_core(LIB_KODAK_HOST, BIN_KODAK_CHECK, "rsx_kodak_host.cpp",
                            ["rsx_kodak_core.h", _RSX_H], "RSX_KODAK_HOST_MAIN",
                            ["-I" + INCLUDE], force)


def build_crw_host(force=False):
    """rsx_crw_core.h: integers only, one thread a frame"""
    return _build_host_core(LIB_CRW_HOST, BIN_CRW_CHECK, "rsx_crw_host.cpp",
                            ["rsx_crw_core.h", "rsx_crw_tables.h", _RSX_H], "RSX_CRW_HOST_MAIN",
                            ["-I" + INCLUDE], force)


def build_fuji_rotate_host(force=False):
    """rsx_fuji_rotate_core.h: integers only, one thread a frame"""
    return _build_host_core(LIB_FUJI_ROTATE_HOST, BIN_FUJI_ROTATE_CHECK,
                            "rsx_fuji_rotate_host.cpp", ["rsx_fuji_rotate_core.h", _RSX_H],
                            "RSX_FUJI_ROTATE_HOST_MAIN", ["-I" + INCLUDE], force)


def build_sony_srf_host(force=False):
    """rsx_sony_srf_core.h: integers only, one thread a buffer"""
    return _build_host_core(LIB_SONY_SRF_HOST, BIN_SONY_SRF_CHECK, "rsx_sony_srf_host.cpp",
                            ["rsx_sony_srf_core.h", _RSX_H], "RSX_SONY_SRF_HOST_MAIN",
                            ["-I" + INCLUDE], force)


def build_image_hash_host(force=False):
    """rsx_image_hash_core.h: integers only; the rows of an image run on threads"""
    return _build_host_core(LIB_IMAGE_HASH_HOST, BIN_IMAGE_HASH_CHECK, "rsx_image_hash_host.cpp",
                            ["rsx_image_hash_core.h", _RSX_H], "RSX_IMAGE_HASH_HOST_MAIN",
                            ["-pthread", "-I" + INCLUDE], force)


def build_encode_host(force=False):
    """rsx_encode_core.h: integers only, one thread a job"""
    return _build_host_core(LIB_ENCODE_HOST, BIN_ENCODE_CHECK, "rsx_encode_host.cpp",
                            ["rsx_encode_core.h", _RSX_H], "RSX_ENCODE_HOST_MAIN",
                            ["-I" + INCLUDE], force)


def build_fpwrite_host(force=False):
    """rsx_fpwrite_core.h and rsx_fp_narrow.h: integers only, one thread a job"""
    return _build_host_core(LIB_FPWRITE_HOST, BIN_FPWRITE_CHECK, "rsx_fpwrite_host.cpp",
                            ["rsx_fpwrite_core.h", "rsx_fp_narrow.h", "rsx_deflate_core.h", _RSX_H],
                            "RSX_FPWRITE_HOST_MAIN", ["-I" + INCLUDE], force)


def build_dctwrite_host(force=False):
    """rsx_dctwrite_core.h: integers only, one thread a tile"""
    return _build_host_core(LIB_DCTWRITE_HOST, BIN_DCTWRITE_CHECK, "rsx_dctwrite_host.cpp",
                            ["rsx_dctwrite_core.h", _RSX_H], "RSX_DCTWRITE_HOST_MAIN",
                            ["-I" + INCLUDE], force)


def _compile_objects(objdir, extra_flags, force=False):
    """One object per source under `objdir`, rebuilt when the source or any header is newer;
    the stale ones in parallel (the sources are independent translation units: one hipcc run
    over all of them took a minute whatever had changed)."""
    from concurrent.futures import ThreadPoolExecutor
    os.makedirs(objdir, exist_ok=True)
    headers = [os.path.join(CSRC, h) for h in CORE_HEADERS] + [os.path.join(INCLUDE, "rsx.h")]
    jobs, objs = [], []
    for name in CORE_SOURCES:
        src = os.path.join(CSRC, name)
        if not os.path.exists(src):
            continue
        obj = os.path.join(objdir, os.path.splitext(name)[0] + ".o")
        objs.append(obj)
        if force or _stale(obj, [src] + headers):
            jobs.append([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c",
                         "-Wall", "-Wno-unused-function", "-I" + INCLUDE, "-I" + CSRC,
                         *extra_flags, "-o", obj, src])
    if jobs:
        with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 1)) as ex:
            list(ex.map(_run, jobs))
    return objs, bool(jobs)


def _link(out, objs):
    _run([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out, *objs])


def build_core(force=False, extra_flags=()):
    srcs = [os.path.join(CSRC, s) for s in CORE_SOURCES]
    srcs = [s for s in srcs if os.path.exists(s)]
    deps = srcs + [os.path.join(CSRC, h) for h in CORE_HEADERS] + \
        [os.path.join(INCLUDE, "rsx.h")]
    if force or _stale(LIB_CORE, deps):
        objs, _ = _compile_objects(os.path.join(PKG, "_build", "core"), extra_flags, force)
        _link(LIB_CORE, objs)
    return LIB_CORE


def build_variant(name, extra_flags):
    """A/B builds: rawspeed_amd/variants/librsx_<name>.so (git-ignored; load with
    RSX_LIB=<path>)."""
    d = os.path.join(PKG, "variants")
    os.makedirs(d, exist_ok=True)
    out = os.path.join(d, "librsx_%s.so" % name)
    import hashlib
    tag = hashlib.sha1(" ".join(extra_flags).encode()).hexdigest()[:8]  # (other flags, other objects)
    objs, _ = _compile_objects(os.path.join(PKG, "_build", "variant_%s_%s" % (name, tag)), extra_flags)
    _link(out, objs)
    return out


def build_all(force=False):
    return (build_core(force), build_synth(force), build_inflate_host(force),
            build_vc5_host(force), build_iiq_corr_host(force), build_dng_post_host(force),
            build_bad_pixels_host(force), build_scale_host(force), build_jpeg_host(force),
            build_fuji_host(force), build_olympus_host(force), build_kodak_host(force),
            build_crw_host(force), build_fuji_rotate_host(force), build_sony_srf_host(force),
            build_image_hash_host(force), build_encode_host(force),
            build_fpwrite_host(force), build_dctwrite_host(force))


if __name__ == "__main__":
    import sys
    print(build_all(force="--force" in sys.argv))
