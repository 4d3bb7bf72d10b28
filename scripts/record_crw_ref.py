"""Records tests/golden/crw_ref.json from the unmodified reference (oracle/_ref, so it runs where
the reference's sources are present and `make -C oracle ref` has been run).

Every case of tests/crw_files.py goes through the reference's front door as a whole CIFF file
(RawParser::getDecoder -> CrwDecoder::decodeRaw -> CrwDecompressor).  The front door has no camera
hints here, so it always decodes with low bits; the route without them rests on the model (see
tests/crw_files.py).  Per case the file keeps the status and the SHA-256 of the rows without
padding.  The reference throws RawDecoderException for "Error decompressing", for a bad Huffman
code and for the constructor's checks, and IOException for the reader's overflow and for an input
below 8 bytes (which decodeRaw rethrows with the reader's text); they are recorded as the statuses
include/rsx.h section 3x gives them.  The validation cases that a file can express (dimensions and
the table number) go the same way.

The script refuses to write if the model of tests/crw_files.py disagrees with the reference on
any case.  With --time it also decodes bench_crw.py's frame with the reference on one thread (its
loop is single-threaded) and records the best time and the CPU's name, for bench_crw.py to quote.

  python scripts/record_crw_ref.py [--time]
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

import crw_files as F  # noqa: E402
from oracle_lib import Ref  # noqa: E402


def ref_status(ref, st):
    if st == F.OK:
        return F.OK
    msg = ref.last_error()
    if isinstance(msg, bytes):
        msg = msg.decode(errors="replace")
    if "Error decompressing" in msg:
        return F.ERR_VALUE_RANGE
    if "bad Huffman code" in msg or "Corrupt Huffman" in msg:
        return F.ERR_BAD_CODE
    if "Buffer overflow read in BitStreamer" in msg:
        return F.ERR_OVERFLOW
    if "Bit stream size is smaller than MaxProcessBytes" in msg:
        return F.ERR_IO
    if ("Unexpected image dimensions" in msg or "Wrong table number" in msg or
            "Unsufficient number of low bit blocks" in msg):
        return F.ERR_INVALID_ARG
    return -abs(st) - 1000  # (nothing the section names: the comparison fails)


def through_reference(ref, blob, shape):
    """-> (status, sha256 of the rows or None)"""
    st, img = ref.decode_file(np.frombuffer(blob, np.uint8))
    st = ref_status(ref, st)
    if st != F.OK or img is None:
        return st, None
    px = img.u16()
    assert px.shape == shape, px.shape
    digest = F.sha_rows(px)
    img.close()
    return st, digest


def time_reference(ref, reps=5):
    import bench_crw
    data, low, want = bench_crw.make_frame()
    blob = F.crw_file(bench_crw.W, bench_crw.H, bench_crw.TABLE, data, low)
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        st, out = ref.decode_file(np.frombuffer(blob, np.uint8), threads=1)
        dt = (time.perf_counter() - t0) * 1e3
        assert st == F.OK, (st, ref.last_error())
        assert F.sha_rows(out.u16()) == F.sha_rows(want), "the reference and the frame disagree"
        out.close()
        best = dt if best is None else min(best, dt)
    cpu = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            cpu = next(l.split(":", 1)[1].strip() for l in f if l.startswith("model name"))
    except (OSError, StopIteration):
        pass
    return {"ms_1_thread": round(best, 1), "cpu": cpu, "what": "decode_file of the whole CIFF file "
            "(parse, createData, CrwDecompressor::decompress), best of %d" % reps,
            "stream_sha256": hashlib.sha256(data).hexdigest(), "stream_bytes": len(data)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true")
    args = ap.parse_args()
    if not Ref.available():
        sys.exit("oracle/_ref is not built")
    ref = Ref()
    cases, validation, wrong = {}, {}, []
    for name in F.case_names():
        c = F.build_case(name)
        st, digest = through_reference(ref, F.case_file(name), (c["height"], c["width"]))
        mst, mpx = F.expected(name, True)
        if st != mst or (st == F.OK and digest != F.sha_rows(mpx)):
            wrong.append((name, st, mst))
        cases[name] = {"lowbits": [st, digest], "width": c["width"], "height": c["height"],
                       "table": c["table"], "in_bytes": len(c["data"]),
                       "zero_low": not any(c["low"])}
    for name, w, h, table, low_short, cpp, pitch, want in F.VALIDATION:
        if cpp != 1 or pitch is not None or w > 65535 or h > 65535:
            continue  # (not something a file says)
        low = bytes(max(0, w * h // 4 - low_short))
        st, _ = through_reference(ref, F.crw_file(w, h, table, bytes(64), low), (h, w))
        # (a file that passes the checks goes on to decode 64 zero bytes: only the checks count)
        st = F.ERR_INVALID_ARG if st == F.ERR_INVALID_ARG else F.OK
        if low_short:
            continue  # (a short chunk fails in CrwDecoder's getStream, not in the constructor)
        if st != want:
            wrong.append((name, st, want))
        validation[name] = st
    if wrong:
        for w in wrong:
            print("model and reference disagree: %s reference %s model %s" % w)
        sys.exit("nothing written")
    out = {"recorded_from": "the unmodified reference through decode_file, scripts/record_crw_ref.py",
           "cases": cases, "validation": validation}
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
