"""The numpy model of DngDecoder's stage behind the tiles (tests/dng_post_files.py: OpcodeList1 and
the LinearizationTable look-up) against the unmodified reference: whole uncompressed DNG files
through RawParser -> DngDecoder -> handleMetadata, so the parse, every check, the table builder and
doLookup are the reference's own.  Where oracle/_ref is not built those tests skip;
tests/golden/dng_post_ref.json holds the SHA-256 of the reference's images, its verdicts (the file
failed / an error was logged) and its final crop for the same cases, and the model is held against
that file everywhere (test_model_matches_recorded_reference never skips).  record_golden() rewrites
the file from the reference (python tests/test_dng_post_model.py); a case enters it only if the
model agreed with the reference when it was recorded.

The reference's shim does not hand out mBadPixelPositions, so the position lists have NO reference
run: they are held against the model only (and the model against the pass-per-opcode restatement in
the sanitizer program).

The host build of rsx_dng_post_core.h (rawspeed_amd/librsx_dng_post_host.so) -- the functions the
kernel runs -- is then held against the model on every case."""
import ctypes as C
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import dng_post_files as K
from oracle_lib import HostImage, Ref
from rawspeed_amd import abi, build


@pytest.fixture(scope="module")
def ref():
    if not Ref.available():
        pytest.skip("oracle/_ref is not built")
    return Ref()


@pytest.fixture(scope="module")
def host():
    lib_path, _ = build.build_dng_post_host()
    L = C.CDLL(lib_path)
    for f in (L.rsx_dng_post_host_apply, L.rsx_dng_post_host_validate):
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    return L


def _reference(ref, case):
    """(decoded, image or None, logged an error, final crop)"""
    img = case[1]
    st, dec = ref.decode_file(K.case_file(case))
    if st != 0:
        return False, None, False, None
    h, ws = img.shape
    assert (dec.cpp, dec.full_w * dec.cpp, dec.full_h) == (case[2], ws, h)
    assert bool(dec.is_f32) == (img.dtype == np.float32)
    px = dec.raw()[:, :ws * img.dtype.itemsize].copy().view(img.dtype)
    return True, px, bool(dec.errors()), (dec.off_x, dec.off_y, dec.w, dec.h_px)


def _agrees(case, got):
    ok, px, logged, crop = got
    st, want, info = K.case_model(case)
    if ok != (st == K.OK):
        return "verdict"
    if not ok:
        return None
    if logged != (info["list_status"] != K.OK):
        return "logged %r, model %r" % (logged, info)
    if crop != info["crop"]:
        return "crop %r, model %r" % (crop, info["crop"])
    if px.tobytes() != want.tobytes():
        return "image"
    return None


def test_model_matches_the_reference(ref):
    for case in K.file_cases():
        assert _agrees(case, _reference(ref, case)) is None, case[0]


def record_golden():
    ref = Ref()
    rec = {"cases": {}}
    for case in K.file_cases():
        got = _reference(ref, case)
        why = _agrees(case, got)
        assert why is None, (case[0], why)
        ok, px, logged, crop = got
        rec["cases"][case[0]] = {"ok": ok, "input": K.sha(case[1]), "image": K.sha(px) if ok else None,
                                 "logged": logged, "crop": list(crop) if ok else None}
    with open(K.GOLDEN, "w") as f:
        json.dump(rec, f, indent=None, sort_keys=True, separators=(",", ":"))
        f.write("\n")


def test_golden_file_is_current(ref):
    rec = K.load_golden()
    assert set(rec["cases"]) == {c[0] for c in K.file_cases()}
    for case in K.file_cases():
        ok, px, logged, crop = _reference(ref, case)
        g = rec["cases"][case[0]]
        assert ok == g["ok"], case[0]
        if ok:
            assert (K.sha(px), logged, list(crop)) == (g["image"], g["logged"], g["crop"]), case[0]


def test_model_matches_recorded_reference():
    rec = K.load_golden()
    cases = K.file_cases()
    assert len(cases) >= 50 and set(rec["cases"]) == {c[0] for c in cases}
    for case in cases:
        g = rec["cases"][case[0]]
        assert g["input"] == K.sha(case[1]), case[0]  # (the seeds give the same bytes)
        st, img, info = K.case_model(case)
        assert g["ok"] == (st == K.OK), case[0]
        if g["ok"]:
            assert K.sha(img) == g["image"], case[0]
            assert g["logged"] == (info["list_status"] != K.OK), case[0]
            assert g["crop"] == list(info["crop"]), case[0]


def test_recorded_verdicts_are_the_expected_classes():
    """which cases fail the file, which are logged, and how much of the list stays applied"""
    rec = K.load_golden()["cases"]
    failed = {n for n, g in rec.items() if not g["ok"]}
    assert failed == {"truncated_list", "truncated_count", "short_opcode", "short_header"}
    logged = {n for n, g in rec.items() if g["ok"] and g["logged"]}
    assert logged == {"offset_beyond_one", "scale_beyond_max", "scale_negative", "rgb_first_plane_3",
                      "rgb_bad_constant", "trim_empty", "bad_roi", "bad_planes", "bad_pitch",
                      "bad_delta_count", "bad_delta_nan", "bad_table_size", "bad_poly_degree",
                      "unknown_opcode", "gainmap_required", "gainmap_optional_payload",
                      "inconsistent_length", "bad_point_outside", "f32_table_refused",
                      # (its ROI fits the image but not the crop the TrimBounds in front of it left)
                      "roi_only_valid_before_trim"}
    by_name = {c[0]: c for c in K.file_cases()}
    applied = {n: K.case_model(by_name[n])[2]["n_applied"] for n in logged}
    # a setup-time refusal keeps what stands in front of it; a parse-time one applies nothing
    assert (applied["offset_beyond_one"], applied["scale_beyond_max"], applied["trim_empty"],
            applied["rgb_bad_constant"], applied["f32_table_refused"]) == (1, 1, 1, 1, 1)
    assert all(applied[n] == 0 for n in logged if n.startswith(("bad_", "unknown", "gainmap", "incons",
                                                                "rgb_first", "roi_only")))
    for n in ("offset_beyond_one", "scale_beyond_max", "f32_table_refused"):
        assert rec[n]["image"] != rec[n]["input"], n  # (the opcode in front of it shows)
    for n in ("bad_planes", "bad_pitch", "bad_delta_count", "gainmap_required"):
        assert rec[n]["image"] == rec[n]["input"], n  # (no table either: untouched)
    assert rec["bad_roi"]["image"] != rec["bad_roi"]["input"]  # (the look-up still runs)


def test_golden_file_tells_the_look_ups_apart():
    """a model that uses the generator and then steps it, one that wraps where doLookup clamps and
    one that looks only rows 0 .. dim.y - 1 of the crop up (startWorker's `cropped` taken at its
    word) each miss recorded images"""
    rec = K.load_golden()["cases"]
    for kw in ({"use_then_step": True}, {"wrap": True}, {"lookup_cropped": True}):
        missed = []
        for case in K.file_cases():
            g = rec[case[0]]
            if g["ok"] and case[4] is not None and K.sha(K.case_model(case, **kw)[1]) != g["image"]:
                missed.append(case[0])
        assert missed, kw
        if "wrap" in kw:
            assert "table_non_monotonic" in missed
        if "lookup_cropped" in kw:
            assert set(missed) >= {"active_area_table", "active_area_list"}


# ---------------------------------------------------------------------------------------
# the host build of the core
# ---------------------------------------------------------------------------------------
def host_apply(L, img, cpp, crop, opcodes, table, pitch=None, bad_cap=1 << 16):
    img = np.asarray(img)
    is_f32 = img.dtype == np.float32
    h, ws = img.shape
    out = HostImage(ws // cpp, h, cpp=cpp, pitch=pitch, bpc=4 if is_f32 else 2)
    rows = out.buf.reshape(h, out.pitch)
    rows[:, :ws * img.itemsize] = img.view(np.uint8).reshape(h, -1)
    before = out.buf.copy()
    d, keep = abi.dng_post_desc(opcodes, table, crop, is_f32)
    v = out.view()
    r = abi.DngPostResult()
    buf = (C.c_uint32 * max(1, bad_cap))()
    st = L.rsx_dng_post_host_apply(C.byref(d), C.byref(v), C.byref(r), buf, bad_cap)
    assert (rows[:, ws * img.itemsize:] == 0xA5).all(), "the pitch padding was written"
    if st not in (K.OK, K.UNSUPPORTED):
        assert np.array_equal(out.buf, before), "a refused list touched the image"
    px = rows[:, :ws * img.itemsize].copy().view(img.dtype)
    return st, px, r, [int(x) for x in buf[:r.n_bad]] if st == K.OK else None


def check_against_model(got, want):
    st, px, r, bad = got
    mst, mimg, info = want
    assert st == mst
    assert px.tobytes() == mimg.tobytes()
    if st == K.OK:
        assert (r.list_status, r.list_reason, r.n_applied) == \
            (info["list_status"], info["reason"], info["n_applied"])
        assert r.crop() == info["crop"]
        assert bad == info["bad"]


def test_host_core_matches_the_model_on_the_reference_cases(host):
    some_bad = 0
    for case in K.file_cases():
        name, img, cpp, opcodes, table, aa = case
        bpc = img.dtype.itemsize
        got = host_apply(host, img, cpp, K.case_crop(case), opcodes, table,
                         pitch=img.shape[1] * bpc + (6 if bpc == 2 else 4))
        try:
            check_against_model(got, K.case_model(case))
        except AssertionError as e:
            raise AssertionError(name) from e
        some_bad += bool(got[3])
    assert some_bad >= 2


def test_position_order_front_insertion_and_capacity(host):
    """FixBadPixelsList goes to the front, in file order; the constant's hits are appended"""
    case = {c[0]: c for c in K.file_cases()}["bad_list"]
    name, img, cpp, opcodes, table, aa = case
    st, _, info = K.case_model(case)
    hits = [(r << 16 | c) for r, c in zip(*np.nonzero(img == 7))]
    assert info["bad"] == [0] + [1 << 16 | 2, 19 << 16 | 69] + \
        [y << 16 | x for y in (2, 3) for x in (3, 4, 5)] + hits
    n = len(info["bad"])
    got = host_apply(host, img, cpp, K.case_crop(case), opcodes, table, bad_cap=n)
    assert got[0] == K.OK and got[3] == info["bad"]
    st, px, r, _ = host_apply(host, img, cpp, K.case_crop(case), opcodes, table, bad_cap=n - 1)
    assert st == K.UNSUPPORTED and r.n_bad == n and np.array_equal(px, img)


def _case_blob(case, pitch):
    """the sanitizer program's case file (rsx_dng_post_host.cpp: read_case)"""
    name, img, cpp, opcodes, table, aa = case
    st, want, info = K.case_model(case)
    h, ws = img.shape
    bpc = img.dtype.itemsize

    def rows(a):
        b = np.full((h, pitch), 0xA5, np.uint8)
        b[:, :ws * bpc] = a.view(np.uint8).reshape(h, -1)
        return b.tobytes()
    table = [] if table is None else [int(v) for v in table]
    opcodes = b"" if opcodes is None else bytes(opcodes)
    crop = K.case_crop(case)
    head = struct.pack("<19i", ws // cpp, h, cpp, int(bpc == 4), pitch, *crop, len(table), len(opcodes),
                       len(info["bad"]), st, info["list_status"], info["n_applied"], *info["crop"])
    return head + struct.pack("<%dH" % len(table), *table) + opcodes + rows(img) + rows(want) + \
        struct.pack("<%dI" % len(info["bad"]), *info["bad"])


def test_sanitizer_program_passes(tmp_path):
    """the stand-alone program (AddressSanitizer and UBSan where g++ has their runtimes): its own
    lists against a pass per opcode and 200 damaged lists, then every reference case as a file"""
    _, prog = build.build_dng_post_host()
    r = subprocess.run([prog], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "200 damaged" in r.stdout
    paths = []
    for case in K.file_cases():
        p = os.path.join(tmp_path, case[0] + ".case")
        with open(p, "wb") as f:
            f.write(_case_blob(case, case[1].shape[1] * case[1].dtype.itemsize + 4))
        paths.append(p)
    r = subprocess.run([prog] + paths, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d case files" % len(paths) in r.stdout


if __name__ == "__main__":
    record_golden()
