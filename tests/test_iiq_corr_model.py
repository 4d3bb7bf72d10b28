"""The numpy models of IiqDecoder::CorrectPhaseOneC's pixel passes (tests/iiq_corr_files.py) against
the unmodified reference: whole IIQ "L" files with a correction block through RawParser ->
IiqDecoder -> CorrectPhaseOneC, so the parse, the spline and both loops are the reference's own.
Where oracle/_ref is not built those tests skip; tests/golden/iiq_corr_ref.json holds the SHA-256
of the reference's images and its verdicts for the same cases, and the model is held against that
file everywhere (test_model_matches_recorded_reference never skips).  record_golden() rewrites the
file from the reference (python tests/test_iiq_corr_model.py).

The host build of rsx_iiq_corr_core.h (rawspeed_amd/librsx_iiq_corr_host.so) -- the functions the
kernels run -- is then held against the model on every case.  The chroma cases have NO reference
run: a whole-file decode without a camera database has no CFA, and the reference throws "No CFA
size set"; their only yardstick is the model that the luma cases pin."""
import ctypes as C
import json
import subprocess

import numpy as np
import pytest

import iiq_corr_files as K
from oracle_lib import HostImage, Ref
from rawspeed_amd import abi, build


@pytest.fixture(scope="module")
def ref():
    if not Ref.available():
        pytest.skip("oracle/_ref is not built")
    return Ref()


@pytest.fixture(scope="module")
def host():
    lib_path, _ = build.build_iiq_corr_host()
    L = C.CDLL(lib_path)
    L.rsx_iiq_corr_host_apply.argtypes = [C.c_void_p, C.c_void_p]
    return L


def _model(case):
    name, img, entries, black, split_row, split_col = case
    return K.apply(img, K.case_ops(entries, black, split_row, split_col))


def _reference(ref, case):
    st, dec = ref.decode_file(K.case_file(case))
    if st != 0:
        return False, None
    h, w = case[1].shape
    assert (dec.cpp, dec.full_w, dec.full_h) == (1, w, h)
    return True, dec.u16()[:h, :w].copy()


def test_the_spline_is_the_references(ref):
    blob, payload, perms = K.curve_pin_file()
    st, dec = ref.decode_file(blob)
    assert st == 0, ref.last_error()
    got = K.curves_from_image(dec.u16()[:512, :512], perms)
    assert np.array_equal(got, K.quadrant_curves(payload))


def test_model_matches_the_reference(ref):
    for case in K.file_cases():
        ok, img = _reference(ref, case)
        st, want = _model(case)
        assert ok == (st == K.OK), case[0]
        if ok:
            assert np.array_equal(img, want), case[0]


def test_an_uncorrected_file_decodes_to_its_image(ref):
    case = K.file_cases()[0]
    st, dec = ref.decode_file(K.iiq_corr_file(case[1]))
    assert st == 0 and np.array_equal(dec.u16()[:40, :64], case[1])


def record_golden():
    ref = Ref()
    blob, payload, perms = K.curve_pin_file()
    st, dec = ref.decode_file(blob)
    curves = K.curves_from_image(dec.u16()[:512, :512], perms)
    assert st == 0 and np.array_equal(curves, K.quadrant_curves(payload))
    rec = {"curves": K.sha(curves), "cases": {}}
    for case in K.file_cases():
        ok, img = _reference(ref, case)
        st, want = _model(case)
        # a case goes into the file only as one the model agreed with the reference on
        assert ok == (st == K.OK) and (not ok or np.array_equal(img, want)), case[0]
        rec["cases"][case[0]] = {"ok": ok, "input": K.sha(case[1]), "image": K.sha(img) if ok else None}
    with open(K.GOLDEN, "w") as f:
        json.dump(rec, f, indent=None, sort_keys=True, separators=(",", ":"))
        f.write("\n")


def test_golden_file_is_current(ref):
    rec = K.load_golden()
    assert set(rec["cases"]) == {c[0] for c in K.file_cases()}
    for case in K.file_cases():
        ok, img = _reference(ref, case)
        assert ok == rec["cases"][case[0]]["ok"], case[0]
        if ok:
            assert K.sha(img) == rec["cases"][case[0]]["image"], case[0]


def test_model_matches_recorded_reference():
    rec = K.load_golden()
    _, payload, _ = K.curve_pin_file()
    assert K.sha(K.quadrant_curves(payload)) == rec["curves"]
    cases = K.file_cases()
    assert len(cases) >= 16 and set(rec["cases"]) == {c[0] for c in cases}
    for case in cases:
        g = rec["cases"][case[0]]
        assert g["input"] == K.sha(case[1]), case[0]  # (the seeds give the same bytes)
        st, img = _model(case)
        assert g["ok"] == (st == K.OK), case[0]
        if g["ok"]:
            assert K.sha(img) == g["image"], case[0]


def test_golden_file_tells_repeated_addition_from_a_product():
    """a model that computes the running sums as a + k * step misses the recorded images"""
    rec = K.load_golden()
    missed = []
    for case in K.file_cases():
        name, img, entries, black, split_row, split_col = case
        if not rec["cases"][name]["ok"] or not any(t == 0x410 for t, _ in entries):
            continue
        st, out = K.apply(img, K.case_ops(entries, black, split_row, split_col), sums=False)
        if K.sha(out) != rec["cases"][name]["image"]:
            missed.append(name)
    assert len(missed) >= 3, missed


# ---------------------------------------------------------------------------------------
# the host build of the core
# ---------------------------------------------------------------------------------------
def host_apply(L, img, ops, cfa=None, pitch=None):
    h, w = img.shape
    out = HostImage(w, h, pitch=pitch)
    out.pixels()[:] = img
    before = out.buf.copy()
    d, keep = abi.iiq_corr(ops, cfa)
    v = out.view()
    st = L.rsx_iiq_corr_host_apply(C.byref(d), C.byref(v))
    pad = out.buf.reshape(h, out.pitch)[:, 2 * w:]
    assert (pad == 0xA5).all(), "the pitch padding was written"
    if st != K.OK:
        assert np.array_equal(out.buf, before), "a refused list touched the image"
    return st, out.pixels().copy()


def test_host_core_matches_the_model_on_the_reference_cases(host):
    for case in K.file_cases():
        name, img, entries, black, split_row, split_col = case
        ops = K.case_ops(entries, black, split_row, split_col)
        st, want = _model(case)
        got_st, got = host_apply(host, img, ops, pitch=2 * 64 + 6)
        assert got_st == st, name
        assert np.array_equal(got, want), name


CFAS = {"rggb": (2, 2, (0, 1, 1, 2)), "grbg": (2, 2, (1, 0, 2, 1)),
        "2x4": (2, 4, (0, 1, 1, 2, 2, 1, 1, 0))}
HEADS = [(3, 2, 56, 30, 7, 5), (0, 0, 64, 40, 8, 8), (5, 3, 130, 121, 13, 11), (0, 0, 40, 20, 1, 1),
         (0, 0, 400, 40, 200, 4), (0, 0, 8, 40, 8, 4), (0, 0, 64, 8, 8, 8), (2, 1, 60, 300, 6, 100),
         (1, 0, 140, 40, 70, 8), (0, 0, 99, 40, 33, 8), (3, 1, 128, 64, 64, 32)]


def test_host_core_matches_the_model_on_luma_geometries(host):
    rng = np.random.default_rng(0xC3)
    for w, h in ((64, 40), (72, 38)):
        img = rng.integers(0, 65536, size=(h, w)).astype(np.uint16)
        for head in HEADS:
            ops = [("ff", K.ff_random(rng, head), 0)]
            st, want = K.apply(img, ops)
            got_st, got = host_apply(host, img, ops)
            assert (got_st, st) == (K.OK, K.OK)
            assert np.array_equal(got, want), (w, h, head)


@pytest.mark.parametrize("cfa", sorted(CFAS))
def test_host_core_matches_the_model_on_chroma(host, cfa):
    rng = np.random.default_rng([0xC4, len(cfa)])
    for w, h in ((64, 40), (72, 38)):
        img = rng.integers(0, 65536, size=(h, w)).astype(np.uint16)
        for head in HEADS:
            ops = [("ff", K.ff_random(rng, head, planes=2), 1)]
            st, want = K.apply(img, ops, CFAS[cfa])
            got_st, got = host_apply(host, img, ops, CFAS[cfa])
            assert (got_st, st) == (K.OK, K.OK)
            assert np.array_equal(got, want), (cfa, w, h, head)


def test_an_untransposed_cfa_lookup_differs_on_grbg():
    """cfa[(col mod w) + (row mod h) w] instead of the reference's transposed lookup corrects other
    pixels of a GRBG image: the chroma cases can tell the two apart"""
    rng = np.random.default_rng(5)
    img = rng.integers(1000, 60000, size=(40, 64)).astype(np.uint16)
    p = K.ff_random(rng, (0, 0, 64, 40, 8, 8), planes=2, lo=40000, hi=50000)
    w, h, c = CFAS["grbg"]
    swapped = (h, w, [c[x + y * w] for x in range(w) for y in range(h)])
    a = K.flat_field(img, p, True, (w, h, c))[1]
    b = K.flat_field(img, p, True, swapped)[1]
    assert (a != b).sum() > 500


def test_sanitizer_program_passes():
    """the validation and clipped-area cases through the stand-alone program (AddressSanitizer and
    UBSan where g++ has their runtimes)"""
    _, prog = build.build_iiq_corr_host()
    r = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


if __name__ == "__main__":
    record_golden()
