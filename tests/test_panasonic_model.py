"""Panasonic RW2 V5 / V6 / V7: the model of the device decode (tests/rw2_files.py) against the
unmodified reference's whole-file decode (RawParser -> Rw2Decoder -> PanasonicV5Decompressor /
PanasonicV6Decompressor / PanasonicV7Decompressor).  No GPU needed.  The reference comparisons
need oracle/_ref; tests/golden/panasonic_ref.json holds SHA-256 of the reference's images for a
fixed list of small files, so that a checkout without the reference still pins the model
(test_model_matches_recorded_reference_hashes never skips).  record_golden() rewrites that file
from the reference:  python tests/test_panasonic_model.py"""
import hashlib
import json
import os

import numpy as np
import pytest

import rw2_files as P
from oracle_lib import Ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "panasonic_ref.json")
needs_ref = pytest.mark.skipif(not Ref.available(), reason="oracle/_ref not built")


@pytest.fixture(scope="module")
def ref():
    return Ref()


def _check(ref, version, bps, w, h, data, gap=0, stats=None):
    """every valid file must decode: status 0, and the model's image"""
    st, dec = ref.decode_file(P.rw2_file(w, h, version, bps, data, gap))
    assert st == 0, (version, bps, w, h, st, ref.last_error())
    img = P.model_decode(version, bps, w, h, data, stats)
    got = dec.u16()[:h, :w]
    assert (dec.full_w, dec.full_h) == (w, h)
    assert np.array_equal(got, img), (version, bps, w, h, np.argwhere(got != img)[:5])


# ---- the recorded hashes --------------------------------------------------------------------
def golden_cases():
    """(name, version, bps, w, h, data): seeded, at least two per layout; V5 with a partial
    and with a second block, V6 with zeroed bytes"""
    out = []
    for k, (version, bps) in enumerate(P.LAYOUTS):
        n = P.PIXELS[(version, bps)]
        for t, (packets_w, h, zero_half) in enumerate([(3, 5, False), (41, 7, True), (130, 9, False)]):
            rng = np.random.default_rng([0x2A7, k, t])
            w = n * packets_w
            data = P.random_stream(rng, version, bps, w, h, zero_half)
            out.append(("v%d_%d_%dx%d%s" % (version, bps, w, h, "_z" if zero_half else ""),
                        version, bps, w, h, data))
    return out


def _sha(img):
    return hashlib.sha256(np.ascontiguousarray(img, dtype="<u2").tobytes()).hexdigest()


def record_golden():
    ref = Ref()
    rec = {}
    for name, version, bps, w, h, data in golden_cases():
        st, dec = ref.decode_file(P.rw2_file(w, h, version, bps, data))
        assert st == 0, (name, ref.last_error())
        rec[name] = {"input_sha256": hashlib.sha256(data.tobytes()).hexdigest(),
                     "image_sha256": _sha(dec.u16()[:h, :w])}
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


def test_model_matches_recorded_reference_hashes():
    with open(GOLDEN) as f:
        rec = json.load(f)
    cases = golden_cases()
    assert sorted(rec) == sorted(c[0] for c in cases) and len(cases) >= 2 * len(P.LAYOUTS)
    for name, version, bps, w, h, data in cases:
        # (the generator still makes the bytes the hashes were recorded for)
        assert hashlib.sha256(data.tobytes()).hexdigest() == rec[name]["input_sha256"], name
        assert _sha(P.model_decode(version, bps, w, h, data)) == rec[name]["image_sha256"], name


@pytest.mark.ref
@needs_ref
def test_recorded_hashes_are_the_reference_s(ref):
    with open(GOLDEN) as f:
        rec = json.load(f)
    for name, version, bps, w, h, data in golden_cases():
        st, dec = ref.decode_file(P.rw2_file(w, h, version, bps, data))
        assert st == 0 and _sha(dec.u16()[:h, :w]) == rec[name]["image_sha256"], name


# ---- against the reference ------------------------------------------------------------------
@pytest.mark.ref
@needs_ref
@pytest.mark.parametrize("version,bps", P.LAYOUTS)
def test_model_matches_reference_on_random_files(ref, version, bps):
    n = P.PIXELS[(version, bps)]
    stats = {}
    for seed in range(60):
        rng = np.random.default_rng([0x52, version, bps, seed])
        w = n * int(rng.choice([1, 2, 3, int(rng.integers(1, 200))]))
        h = int(rng.integers(1, 40))
        zero_half = version == 6 and seed % 2 == 1
        data = P.random_stream(rng, version, bps, w, h, zero_half)
        _check(ref, version, bps, w, h, data, gap=seed % 3, stats=stats)
    if version == 6:
        # both kinds of bytes reached the branches they are there for; the `else` of the last
        # test was never reached with e >= 15
        assert stats["first_zero"] > 0.01 * stats["pixels"]
        assert stats["below_15"] > 0.05 * stats["pixels"]
        assert stats["else_large"] == 0


@pytest.mark.ref
@needs_ref
@pytest.mark.parametrize("version,bps", [(7, 14), (5, 12), (6, 14), (6, 12)])  # n = 9, 10, 11, 14
def test_every_width_at_height_two(ref, version, bps):
    n = P.PIXELS[(version, bps)]
    rng = np.random.default_rng([version, bps])
    for w in range(n, 9600 + n, n):
        _check(ref, version, bps, w, 2, P.random_stream(rng, version, bps, w, 2, bool(w & 1)))


@pytest.mark.ref
@needs_ref
@pytest.mark.parametrize("bps", [12, 14])
@pytest.mark.parametrize("packets", [1, 1023, 1024, 1025, 2048, 2049])
def test_v5_block_boundaries(ref, bps, packets):
    """the partial last block, exact multiples of a block, and one packet more"""
    n = P.PIXELS[(5, bps)]
    rng = np.random.default_rng([5, bps, packets])
    for w, h in {(n * packets, 1), (n, packets)} | ({(n * (packets // 2), 2)} if packets % 2 == 0 else set()):
        if w > 65535 or h > 65535:
            continue
        data = P.random_stream(rng, 5, bps, w, h)
        assert data.size == -(-packets // 1024) * 0x4000
        _check(ref, 5, bps, w, h, data)


def test_v5_writer_places_packets_where_the_model_reads_them():
    """stream_from_packets (the inverse rotation) against the model's reading; packet 512 of a
    block wraps around the block's end"""
    rng = np.random.default_rng(55)
    for bps in (12, 14):
        n = P.PIXELS[(5, bps)]
        packets = 1024 + 600
        vals = rng.integers(0, 1 << bps, size=(packets, n))
        data = P.stream_from_packets(5, [np.frombuffer(P.pack_plain(v, bps), np.uint8) for v in vals])
        assert data.size == 2 * P.BLOCK
        assert np.array_equal(P.model_decode(5, bps, n * packets, 1, data).reshape(packets, n), vals)
        blk = data[P.BLOCK:]
        p512 = np.frombuffer(P.pack_plain(vals[1024 + 512], bps), np.uint8)
        assert np.array_equal(blk[-8:], p512[:8]) and np.array_equal(blk[:8], p512[8:])


def _v6_planted(bps):
    """pixelbuffer entries of the planted packets"""
    fb, triples = (10, 3) if bps == 14 else (8, 4)
    first, field = (1 << bps) - 1, (1 << fb) - 1
    out = [[0, 0] + [0, 0, 0, 0] * triples,                           # all zero
           [first, first] + [3, field, field, field] * triples]       # all ones
    for s in range(4):                                                  # every scale, every triple
        for t in range(triples):
            e = [1000, 77] + [1, 5, 9, 200] * triples
            e[2 + 4 * t] = s
            out.append(e)
        out.append([first, 300] + [s, field, 1, field] * triples)
    out.append([0, 0] + [2, 7, 0, 100] * triples)                      # first pixel 0, then fields
    out.append([0, 500] + [0, 0, 0, 3] + [1, field, 0, 9] * (triples - 1))
    out.append([20, 14] + [0, 0, 15, 14] * triples)                    # around e = 15
    out.append([first, first] + [0, field, field, field] * triples)   # climbs, scale 1
    out.append([first, first] + [2, field, field, field] * triples)   # climbs, scale 4
    return out


@pytest.mark.ref
@needs_ref
@pytest.mark.parametrize("bps", [12, 14])
def test_planted_v6_packets(ref, bps):
    n = P.PIXELS[(6, bps)]
    planted = _v6_planted(bps)
    data = P.stream_from_packets(6, [np.frombuffer(P.pack_v6(e, bps), np.uint8) for e in planted])
    w, h = n, len(planted)
    img = P.model_decode(6, bps, w, h, data)
    assert (img[0] == 0).all()
    if bps == 12:
        assert img.max() > 4095  # a 12-bit packet climbs past 4095: nothing clamps it
    _check(ref, 6, bps, w, h, data)
    # the same packets side by side in one row
    _check(ref, 6, bps, w * h, 1, data)


@pytest.mark.ref
@needs_ref
@pytest.mark.parametrize("version,bps", P.LAYOUTS)
def test_input_size_and_width_rejections(ref, version, bps):
    n = P.PIXELS[(version, bps)]
    rng = np.random.default_rng([9, version, bps])
    w, h = 3 * n, 4
    data = P.random_stream(rng, version, bps, w, h)
    _check(ref, version, bps, w, h, data, gap=0)
    _check(ref, version, bps, w, h, data, gap=13)  # trailing bytes are ignored
    st, _ = ref.decode_file(P.rw2_file(w, h, version, bps, data[:-1]))
    assert st == P.INVALID_ARG and "Insufficient count of input blocks" in ref.last_error()
    st, _ = ref.decode_file(P.rw2_file(w + 1, h, version, bps, np.concatenate([data, data])))
    assert st == P.INVALID_ARG and "Unexpected image dimensions" in ref.last_error()


if __name__ == "__main__":
    record_golden()
