"""Samsung SRW compression 32770: the model of the device decode (tests/srw_v0_files.py) against
the unmodified reference's whole-file decode (RawParser -> SrwDecoder -> SamsungV0Decompressor).
No GPU needed.  The reference comparisons need oracle/_ref; tests/golden/samsung_v0_ref.json
holds SHA-256 of the reference's images for a fixed list of small files (and the reference's
ok / fail for damaged ones), so that a checkout without the reference still pins the model
(test_model_matches_recorded_reference_hashes never skips).  record_golden() rewrites that file
from the reference:  python tests/test_samsung_v0_model.py"""
import hashlib
import json
import os

import numpy as np
import pytest

import srw_v0_files as S
from oracle_lib import Ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "samsung_v0_ref.json")
needs_ref = pytest.mark.skipif(not Ref.available(), reason="oracle/_ref not built")


@pytest.fixture(scope="module")
def ref():
    return Ref()


def _check(ref, w, h, rows):
    """every valid file must decode: status 0, and the model's image"""
    st, dec = ref.decode_file(S.rows_file(w, h, rows))
    assert st == 0, (w, h, st, ref.last_error())
    mst, _, img = S.model_decode(w, h, rows)
    assert mst == S.OK
    got = dec.u16()[:h, :w]
    assert (dec.full_w, dec.full_h) == (w, h)
    assert np.array_equal(got, img), (w, h, np.argwhere(got != img)[:5])


# ---- planted rows: what the reference says about each -----------------------------------------
def _header(w, up, ops, vals=()):
    w.put(up, 1)
    for op in ops:
        w.put(op, 2)
    for v in vals:
        w.put(v, 4)


def planted(kind, width=48):
    """(width, height, rows, failing row, model status, the reference's message); row 0 and 1 are
    plain rows, the planted one is row 2 unless the kind is about the first rows"""
    rng = np.random.default_rng([0x51, len(kind)])
    plain = [S.encode_row(rng, width, y, p_up=0.0) for y in range(3)]
    w = S.BitWriter()
    if kind == "len_below_0":  # len 4 -> op 3 to 0 -> op 2
        _header(w, 0, [3, 0, 0, 0], [0])
        for _ in range(12):
            w.put(0, 4)
        _header(w, 0, [2, 0, 0, 0])
        bad, st, msg = 2, S.VALUE_RANGE, "Bit length less than 0."
    elif kind == "len_above_16":  # 15 -> 16 decodes, -> 17 throws
        _header(w, 0, [3, 0, 0, 0], [15])
        for _ in range(4):
            w.put(0x7FFF, 15)
        for _ in range(12):
            w.put(0, 4)
        _header(w, 0, [1, 0, 0, 0])
        for _ in range(4):
            w.put(0xFFFF, 16)
        for _ in range(12):
            w.put(0, 4)
        _header(w, 0, [1, 0, 0, 0])
        bad, st, msg = 2, S.VALUE_RANGE, "Bit Length more than 16."
    elif kind == "up_in_row_1":
        _header(w, 1, [0, 0, 0, 0])
        bad, st, msg = 1, S.INVALID_ARG, "Upward prediction for the first two rows"
    elif kind == "up_in_last_block":
        for _ in range(2):
            _header(w, 0, [0, 0, 0, 0])
            for _ in range(16):
                w.put(0, 4)
        _header(w, 1, [0, 0, 0, 0])
        bad, st, msg = 2, S.INVALID_ARG, "Upward prediction for the last block of pixels"
    elif kind == "up_in_only_block":
        width = 16
        plain = [S.encode_row(rng, width, y, p_up=0.0) for y in range(3)]
        _header(w, 1, [0, 0, 0, 0])
        bad, st, msg = 2, S.INVALID_ARG, "Upward prediction for the last block of pixels"
    elif kind == "two_byte_row":
        rows = plain[:2] + [b"\x00\x00"]
        return width, 3, rows, 2, S.IO, "Bit stream size is smaller than MaxProcessBytes"
    else:
        raise ValueError(kind)
    data = w.bytes() + bytes(160)  # (enough bytes behind the planted header: no over-read first)
    rows = list(plain)
    rows[bad] = data
    return width, 3, rows, bad, st, msg


PLANTED = ["len_below_0", "len_above_16", "up_in_row_1", "up_in_last_block", "up_in_only_block",
           "two_byte_row"]


def truncated_cases():
    """frames whose last row is cut at every size: (w, h, rows)"""
    out = []
    for k, (w, h) in enumerate([(50, 4), (121, 3), (200, 2)]):
        rng = np.random.default_rng([0x7C, k])
        rows = S.random_rows(rng, w, h)
        out += [(w, h, rows[:-1] + [rows[-1][:n]]) for n in range(1, len(rows[-1]) + 1)]
    return out


# ---- the recorded hashes --------------------------------------------------------------------
GOLDEN_SHAPES = [(16, 1), (17, 2), (31, 3), (48, 5), (50, 8), (95, 7), (129, 12), (200, 23), (333, 9),
                 (64, 16)]


def golden_cases():
    """(name, w, h, rows): seeded small files; odd widths and heights, partial last blocks, lengths
    0 and 16 planted in every second one"""
    out = []
    for k, (w, h) in enumerate(GOLDEN_SHAPES):
        rng = np.random.default_rng([0x5A0, k])
        rows = S.random_rows(rng, w, h, p_up=0.35, plant=bool(k & 1))
        out.append(("v0_%dx%d" % (w, h), w, h, rows))
    return out


def _sha(img):
    return hashlib.sha256(np.ascontiguousarray(img, dtype="<u2").tobytes()).hexdigest()


def _sha_rows(rows):
    m = hashlib.sha256()
    for r in rows:
        m.update(len(r).to_bytes(4, "little") + bytes(r))
    return m.hexdigest()


def large_case():
    """the largest frame the reference accepts, with a partial last block (GPU tests)"""
    rng = np.random.default_rng(0x1A46E)
    return S.MAX_W, S.MAX_H, S.tiled_rows(rng, S.MAX_W, S.MAX_H, p_up=0.3)


def record_golden():
    ref = Ref()
    rec = {"images": {}, "planted": {}, "truncated": []}
    for name, w, h, rows in golden_cases():
        st, dec = ref.decode_file(S.rows_file(w, h, rows))
        assert st == 0, (name, ref.last_error())
        rec["images"][name] = {"input_sha256": _sha_rows(rows), "image_sha256": _sha(dec.u16()[:h, :w])}
    w, h, rows = large_case()
    st, dec = ref.decode_file(S.rows_file(w, h, rows))
    assert st == 0, ref.last_error()
    rec["large"] = {"input_sha256": _sha_rows(rows), "image_sha256": _sha(dec.u16()[:h, :w])}
    for kind in PLANTED:
        w, h, rows, _, _, msg = planted(kind)
        st, _ = ref.decode_file(S.rows_file(w, h, rows))
        assert st != 0 and msg in ref.last_error(), (kind, st, ref.last_error())
        rec["planted"][kind] = {"input_sha256": _sha_rows(rows), "ok": False}
    for w, h, rows in truncated_cases():
        st, _ = ref.decode_file(S.rows_file(w, h, rows))
        rec["truncated"].append(st == 0)
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


def test_model_matches_recorded_reference_hashes():
    """Fails when one model line is broken on purpose; tried: the row above for odd pixels taken
    one row up instead of two, 127 for the 128 at column 0, and the swap left out."""
    with open(GOLDEN) as f:
        rec = json.load(f)
    cases = golden_cases()
    assert sorted(rec["images"]) == sorted(c[0] for c in cases) and len(cases) >= 8
    for name, w, h, rows in cases:
        # (the generator still makes the bytes the hashes were recorded for)
        assert _sha_rows(rows) == rec["images"][name]["input_sha256"], name
        st, _, img = S.model_decode(w, h, rows)
        assert st == S.OK and _sha(img) == rec["images"][name]["image_sha256"], name
    # the reference's ok / fail for the planted rows and for a row cut at every size
    for kind in PLANTED:
        w, h, rows, bad, want, _ = planted(kind)
        assert _sha_rows(rows) == rec["planted"][kind]["input_sha256"], kind
        st, rs, img = S.model_decode(w, h, rows)
        assert (st, img) == (want, None) and rs[bad] == want and not any(rs[:bad]), (kind, st, rs)
    cut = truncated_cases()
    assert len(cut) == len(rec["truncated"])
    assert [S.model_decode(w, h, rows)[0] == S.OK for w, h, rows in cut] == rec["truncated"]
    assert True in rec["truncated"] and False in rec["truncated"]


def test_random_files_are_not_easy():
    """what the random files of the tests below (and of the GPU tests) reach"""
    st = S.new_stats()
    shapes = []
    for seed in range(60):
        w, h, rows = random_case(seed, st)
        shapes.append((w, h))
    assert st["up"] >= 0.2 * st["eligible"] > 0
    assert all(n >= 0.1 * 4 * st["headers"] for n in st["ops"]), st["ops"]
    assert {0, 16} <= st["lens"]
    assert any(w & 1 for w, _ in shapes) and any(h & 1 for _, h in shapes)
    assert any(w % 16 for w, _ in shapes)


def random_case(seed, stats=None):
    rng = np.random.default_rng([0x5E, seed])
    w, h = int(rng.integers(16, 200)), int(rng.integers(1, 24))
    return w, h, S.random_rows(rng, w, h, p_up=0.3, stats=stats, plant=seed % 5 == 0)


def test_overread_rule_is_the_model_s():
    """the closed form over a row's requests says what the model's request-by-request check says"""
    n = 0
    for w, h, rows in truncated_cases():
        req = []
        st, _, _ = S.parse_row(rows[-1], h - 1, w, req)
        if st in (S.OK, S.INPUT_OVERFLOW):
            # (on an over-read the list ends with the request that threw)
            assert S.overreads(req, len(rows[-1])) == (st == S.INPUT_OVERFLOW)
            n += 1
    assert n > 100


# ---- against the reference ------------------------------------------------------------------
@pytest.mark.ref
@needs_ref
def test_recorded_hashes_are_the_reference_s(ref):
    with open(GOLDEN) as f:
        rec = json.load(f)
    for name, w, h, rows in golden_cases():
        st, dec = ref.decode_file(S.rows_file(w, h, rows))
        assert st == 0 and _sha(dec.u16()[:h, :w]) == rec["images"][name]["image_sha256"], name


@pytest.mark.ref
@needs_ref
def test_model_matches_reference_on_random_files(ref):
    for seed in range(60):
        w, h, rows = random_case(seed)
        _check(ref, w, h, rows)


@pytest.mark.ref
@needs_ref
@pytest.mark.parametrize("h", [1, 2, 3, 5])
def test_every_width(ref, h):
    rng = np.random.default_rng([0xE7, h])
    for w in range(16, 401):
        _check(ref, w, h, S.random_rows(rng, w, h, p_up=0.4))


@pytest.mark.ref
@needs_ref
@pytest.mark.parametrize("w", [5536, 5546])
def test_widest_rows(ref, w):
    rng = np.random.default_rng(w)
    _check(ref, w, 4, S.random_rows(rng, w, 4, p_up=0.3))


def _long_run_frames():
    """the planned frames of tests/long_runs.py one block into pass 1 and at the widest row"""
    import long_runs as L
    return [c for c in L.v0_frames() if c[1] in (3088, 5546)]


@pytest.mark.ref
@needs_ref
@pytest.mark.parametrize("w", [3088, 5546])
def test_model_matches_reference_on_long_runs_without_upward_blocks(ref, w):
    """Frames whose upward blocks are planned (none; one in row 2 or 3 at a wave or pass edge;
    every eligible one; two 200 blocks apart): the root of a run lies up to 347 blocks to the
    left, where the random files above never have it more than 27.  The hash recorded in
    tests/golden/long_runs_ref.json is the reference's."""
    import long_runs as L
    rec = L.golden()["samsung_v0"]
    for case in _long_run_frames():
        name, cw, h, _ = case
        if cw != w:
            continue
        rows = L.v0_build(case)
        _check(ref, w, h, rows)
        st, dec = ref.decode_file(S.rows_file(w, h, rows))
        assert (L.sha_rows(rows)[:16], L.sha(dec.u16()[:h, :w])) == (rec[name]["input"], rec[name]["image"])


@pytest.mark.parametrize("width", [3088, 5546])
def test_model_matches_recorded_hashes_of_long_runs_without_upward_blocks(width):
    """the same without the reference: the model against what was recorded from it (never skips)"""
    import long_runs as L
    rec = L.golden()["samsung_v0"]
    assert sorted(rec) == sorted(c[0] for c in L.v0_frames())
    for case in _long_run_frames():
        name, w, h, _ = case
        if w != width:
            continue
        rows = L.v0_build(case)
        assert L.sha_rows(rows)[:16] == rec[name]["input"], name
        st, _, img = S.model_decode(w, h, rows)
        assert st == S.OK and L.sha(img) == rec[name]["image"], name


@pytest.mark.ref
@needs_ref
def test_truncated_rows_at_every_size(ref):
    n_ok = 0
    for w, h, rows in truncated_cases():
        st, dec = ref.decode_file(S.rows_file(w, h, rows))
        mst, _, img = S.model_decode(w, h, rows)
        assert (st == 0) == (mst == S.OK), (len(rows[-1]), st, mst, ref.last_error())
        if st == 0:
            n_ok += 1
            assert np.array_equal(dec.u16()[:h, :w], img)
        else:
            assert mst in (S.INPUT_OVERFLOW, S.IO)
            assert ("Buffer overflow read in BitStreamer" in ref.last_error()) == (mst == S.INPUT_OVERFLOW)
    assert n_ok > 0


@pytest.mark.ref
@needs_ref
@pytest.mark.parametrize("kind", PLANTED)
def test_planted_rows(ref, kind):
    w, h, rows, bad, want, msg = planted(kind)
    st, _ = ref.decode_file(S.rows_file(w, h, rows))
    assert st == 1 and msg in ref.last_error(), (st, ref.last_error())
    mst, rs, img = S.model_decode(w, h, rows)
    assert (mst, img) == (want, None) and rs[bad] == want


@pytest.mark.ref
@needs_ref
def test_length_16_decodes(ref):
    """len = 16 itself is fine: the planted row up to its second block"""
    rng = np.random.default_rng(16)
    w = S.BitWriter()
    _header(w, 0, [3, 3, 3, 3], [15, 15, 15, 15])
    for v in rng.integers(0, 1 << 15, size=16):
        w.put(v, 15)
    _header(w, 0, [1, 1, 1, 1])
    for v in rng.integers(0, 1 << 16, size=16):
        w.put(v, 16)
    _check(ref, 32, 1, [w.bytes()])


@pytest.mark.ref
@needs_ref
def test_container_rejections(ref):
    rng = np.random.default_rng(0xC0)
    w, h = 40, 5
    rows = S.random_rows(rng, w, h)
    strip, offs = S.strip_and_offsets(rows)
    n = len(strip)

    def err(width, offsets, data=strip):
        st, _ = ref.decode_file(S.srw_v0_file(width, h, data, offsets))
        assert st == 1
        return ref.last_error()

    seq = "Line offsets are out of sequence or slice is empty."
    assert seq in err(w, offs[:2] + [offs[2], offs[2]] + offs[4:])       # equal offsets
    assert seq in err(w, offs[:-1] + [n])                                # the last = the strip size
    assert "Out of bounds access in ByteStream" in err(w, [n + 1] + offs[1:])  # skipBytes
    # a later offset past the strip while the pair is still increasing: getStream of that pair,
    # before the next pair's sequence check (which would fail too)
    msg = err(w, offs[:3] + [n + 4, n + 2])
    assert seq not in msg and "getSubView" in msg and "Buffer overflow" in msg  # (an IOException)
    # ... and the sequence check of an earlier pair comes before a later pair's bounds
    assert seq in err(w, [offs[0], offs[2], offs[1], n + 4, n + 8])
    assert "Unexpected image dimensions" in err(15, offs)


if __name__ == "__main__":
    record_golden()
