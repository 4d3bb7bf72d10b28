"""Records tests/golden/kodak_ref.json from the unmodified reference (oracle/_ref, so it runs where
the reference's sources are present and `make -C oracle ref` has been run).

Every case of tests/kodak_files.py goes through the reference's front door as a whole DCR file
(RawParser::getDecoder -> DcrDecoder::decodeRaw -> KodakDecompressor), once with
uncorrectedRawValues and once without (the linearization curve as a dither table).  Per case and
route the file keeps the status and the SHA-256 of the rows without padding.  The reference throws
RawDecoderException for "Value out of bounds" and IOException for a read past the end (which
decodeRaw rethrows with the reader's text); they are recorded as RSX_ERR_VALUE_RANGE and RSX_ERR_IO.

The script refuses to write if the model of tests/kodak_files.py disagrees with the reference on
any case.  With --time it also decodes bench_kodak.py's frame with the reference on one thread (its
loop is single-threaded) and records the best time and the CPU's name, for bench_kodak.py to quote.

  python scripts/record_kodak_ref.py [--time]
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import kodak_files as F  # noqa: E402
from oracle_lib import Ref  # noqa: E402


def ref_status(ref, st):
    if st == F.OK:
        return F.OK
    msg = ref.last_error()
    if isinstance(msg, bytes):
        msg = msg.decode(errors="replace")
    if "Value out of bounds" in msg:
        return F.ERR_VALUE_RANGE
    # RawDecoder::decodeRaw rethrows the decompressor's IOException as a RawDecoderException
    # whose text starts with its own name (decoders/RawDecoder.cpp:337-338)
    if "RawDecoder::decodeRaw()" in msg and ("Buffer overflow" in msg or
                                             "Out of bounds access" in msg):
        return F.ERR_IO
    return st


def through_reference(ref, name, uncorrected):
    """-> (status, sha256 of the rows or None)"""
    c = F.case(name)
    st, img = ref.decode_file(F.case_file(name), uncorrected=uncorrected)
    st = ref_status(ref, st)
    if st != F.OK or img is None:
        return st, None
    px = img.u16()
    assert px.shape == (c["height"], c["width"]), (name, px.shape)
    digest = F.sha_rows(px)
    img.close()
    return st, digest


def compare(ref, name):
    """-> ({route: [status, sha]}, the disagreements with the model)"""
    entry, wrong = {}, []
    for route, uncorrected, mode in (("uncorrected", True, F.NONE), ("corrected", False, F.DITHER)):
        st, digest = through_reference(ref, name, uncorrected)
        mst, mpx = F.expected(name, mode)
        if st != mst or (st == F.OK and digest != F.sha_rows(mpx)):
            wrong.append((name, route, st, mst))
        entry[route] = [st, digest]
    return entry, wrong


def time_reference(ref, reps=5):
    import bench_kodak
    data, img, curve = bench_kodak.make_frame()
    blob = F.dcr_file(bench_kodak.W, bench_kodak.H, np.frombuffer(data, np.uint8), curve)
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        st, out = ref.decode_file(blob, uncorrected=False, threads=1)
        dt = (time.perf_counter() - t0) * 1e3
        assert st == F.OK, (st, ref.last_error())
        want = F.sha_rows(F.apply_table(img.astype(np.int32), F.DITHER, curve))
        assert F.sha_rows(out.u16()) == want, "the reference and the model disagree on the frame"
        out.close()
        best = dt if best is None else min(best, dt)
    cpu = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            cpu = next(l.split(":", 1)[1].strip() for l in f if l.startswith("model name"))
    except (OSError, StopIteration):
        pass
    return {"ms_1_thread": round(best, 1), "cpu": cpu, "what": "decode_file of the whole DCR file "
            "(parse, createData, KodakDecompressor::decompress), best of %d" % reps,
            "stream_sha256": hashlib.sha256(data).hexdigest(), "stream_bytes": len(data)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true")
    args = ap.parse_args()
    if not Ref.available():
        sys.exit("oracle/_ref is not built")
    ref = Ref()
    cases, wrong = {}, []
    for c in F.case_list():
        entry, w = compare(ref, c["name"])
        entry.update(width=c["width"], height=c["height"], bps=c["bps"],
                     in_bytes=len(F.build_case(c["name"])["data"]))
        cases[c["name"]] = entry
        wrong += w
    if wrong:
        for w in wrong:
            print("model and reference disagree: %s %s reference %s model %s" % w)
        sys.exit("nothing written")
    out = {"recorded_from": "the unmodified reference through decode_file, scripts/record_kodak_ref.py",
           "cases": cases}
    if args.time:
        out["reference_timing"] = time_reference(ref)
    elif os.path.exists(F.GOLDEN):
        with open(F.GOLDEN) as f:
            old = json.load(f).get("reference_timing")
        if old:
            out["reference_timing"] = old
    with open(F.GOLDEN, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d cases -> %s" % (len(cases), F.GOLDEN))


if __name__ == "__main__":
    main()
