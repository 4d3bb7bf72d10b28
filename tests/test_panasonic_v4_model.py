"""Panasonic RW2 V4: the model of the device decode (tests/rw2_v4_files.py) against the unmodified
reference's whole-file decode (RawParser -> Rw2Decoder -> PanasonicV4Decompressor), through both
kinds of file: old-style (STRIPOFFSETS, section_split_offset 0) and PANASONIC_RAWFORMAT 4 (0x1FF8).
No GPU needed.  The reference's shim does not hand out mBadPixelPositions; pred == 0 exactly where
the stored pixel is 0 (pred stays in 0 .. 16287), so the model's list is held against the zero
pixels of the reference's image.  The reference comparisons need oracle/_ref;
tests/golden/panasonic_v4_ref.json holds SHA-256 of the reference's images for a fixed list of
small files, so that a checkout without the reference still pins the model
(test_model_matches_recorded_reference_hashes never skips).  record_golden() rewrites that file
from the reference:  python tests/test_panasonic_v4_model.py"""
import hashlib
import json
import os

import numpy as np
import pytest

import rw2_v4_files as V
from oracle_lib import Ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "panasonic_v4_ref.json")
needs_ref = pytest.mark.skipif(not Ref.available(), reason="oracle/_ref not built")


@pytest.fixture(scope="module")
def ref():
    return Ref()


def _check(ref, split, w, h, data, gap=0, stats=None):
    """every valid file must decode: status 0, the model's image, and the model's list = the
    zero pixels of the reference's image"""
    st, dec = ref.decode_file(V.v4_file(split, w, h, data, gap))
    assert st == 0, (split, w, h, st, ref.last_error())
    img, zeros = V.model_decode(split, w, h, data, stats)
    got = dec.u16()[:h, :w]
    assert (dec.full_w, dec.full_h) == (w, h)
    assert np.array_equal(got, img), (split, w, h, np.argwhere(got != img)[:5])
    rows_cols = np.argwhere(got == 0)
    assert np.array_equal(zeros, (rows_cols[:, 0] << 16 | rows_cols[:, 1]).astype(np.uint32)), (split, w, h)


# ---- the recorded hashes --------------------------------------------------------------------
def golden_cases():
    """(name, split, w, h, data): seeded; per split one block, a partial block (split 0) resp.
    a padded one, and more than two blocks with packet 512's wrap, every generator"""
    out = []
    for s, split in enumerate(V.SPLITS):
        for t, (packets_w, h, kind) in enumerate([(3, 5, "uniform"), (41, 7, "half"), (128, 8, "sparse"),
                                                  (130, 9, "uniform"), (293, 7, "sparse")]):
            rng = np.random.default_rng([0x4A7, s, t])
            w = V.N * packets_w
            data = V.random_stream(rng, split, w, h, kind)
            out.append(("split%x_%dx%d_%s" % (split, w, h, kind), split, w, h, data))
    return out


def _sha(img):
    return hashlib.sha256(np.ascontiguousarray(img, dtype="<u2").tobytes()).hexdigest()


def record_golden():
    ref = Ref()
    rec = {}
    for name, split, w, h, data in golden_cases():
        st, dec = ref.decode_file(V.v4_file(split, w, h, data))
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
    assert sorted(rec) == sorted(c[0] for c in cases) and len(cases) >= 3 * len(V.SPLITS)
    packets = {split: sorted(c[2] * c[3] // V.N for c in cases if c[1] == split) for split in V.SPLITS}
    for split in V.SPLITS:  # below one block, exactly one, a partial second, more than two
        assert packets[split][0] < 1024 and 1024 in packets[split] and packets[split][-1] > 2048
        assert any(1024 < p < 2048 for p in packets[split])
    stats = {}
    for name, split, w, h, data in cases:
        # (the generator still makes the bytes the hashes were recorded for)
        assert hashlib.sha256(data.tobytes()).hexdigest() == rec[name]["input_sha256"], name
        img, zeros = V.model_decode(split, w, h, data, stats)
        assert _sha(img) == rec[name]["image_sha256"], name
        assert np.array_equal(zeros, V.zero_list(img)), name
    assert all(stats[k] > 0 for k in V.STATS), stats


@pytest.mark.ref
@needs_ref
def test_recorded_hashes_are_the_reference_s(ref):
    with open(GOLDEN) as f:
        rec = json.load(f)
    for name, split, w, h, data in golden_cases():
        st, dec = ref.decode_file(V.v4_file(split, w, h, data))
        assert st == 0 and _sha(dec.u16()[:h, :w]) == rec[name]["image_sha256"], name


# ---- the writers ----------------------------------------------------------------------------
def test_packet_writer_places_the_fields_where_the_model_reads_them():
    """all-zero fields: 14 zero pixels; only the late 4-bit fields: the pixels 12 and 13; a
    first non-zero field takes its 4-bit field at once; scale 3 means a shift of 4"""
    W = lambda pk: np.concatenate([pk.view("<u4").astype(np.uint64), [np.uint64(0)]])[None, :]  # noqa: E731
    assert (V.decode_packets(W(V.pack_v4([0] * 14))) == 0).all()
    assert V.decode_packets(W(V.pack_v4([0] * 14, g=(5, 9))))[0].tolist() == [0] * 12 + [5, 9]
    got = V.decode_packets(W(V.pack_v4([3, 0, 0, 7] + [0] * 10, g=(2, 12))))[0].tolist()
    assert got == [50, 0, 50, 124] + [50, 124] * 5
    # pred = 0x30, then scale 3: 0x30 - 0x800 < 0 -> & 15 = 0, + (1 << 4)
    got = V.decode_packets(W(V.pack_v4([3, 3, 1, 0] + [0] * 10, (3, 0, 0, 0), (0, 0))))[0].tolist()
    assert got[:3] == [48, 48, 16]


def test_stream_builder_and_packet_offsets_agree():
    rng = np.random.default_rng(44)
    packets = rng.integers(0, 256, size=(1024 + 600, 16), dtype=np.uint8)
    for split in V.SPLITS:
        data = V.stream_from_packets(split, packets)
        assert data.size == (len(packets) * 16 if split == 0 else 2 * V.BLOCK)
        for p in (0, 1, 511, 512, 513, 1023, 1024, 1536, 1623):
            assert np.array_equal(data[V.packet_offsets(split, p)], packets[p]), (split, p)
    blk = V.stream_from_packets(V.SPLIT, packets)[V.BLOCK:]  # packet 512 of a block wraps
    assert np.array_equal(blk[-8:], packets[1536][:8]) and np.array_equal(blk[:8], packets[1536][8:])


# ---- against the reference ------------------------------------------------------------------
@pytest.mark.ref
@needs_ref
@pytest.mark.parametrize("split", V.SPLITS)
def test_model_matches_reference_on_random_files(ref, split):
    stats = {}
    for seed in range(60):
        rng = np.random.default_rng([0x54, split, seed])
        w = V.N * int(rng.choice([1, 2, 3, int(rng.integers(1, 200))]))
        h = int(rng.integers(1, 40))
        data = V.random_stream(rng, split, w, h, V.KINDS[seed % 3])
        _check(ref, split, w, h, data, gap=seed % 3 if split else 0, stats=stats)
    # every branch of processPixelPacket was reached, the rare ones often enough to matter
    assert all(stats[k] > 0 for k in V.STATS), stats
    assert stats["late4"] > 0.001 * stats["pixels"] and stats["lead_zero"] > 0.01 * stats["pixels"]
    assert stats["max_pred"] <= 16287


@pytest.mark.ref
@needs_ref
@pytest.mark.parametrize("split", V.SPLITS)
def test_every_width_at_height_two(ref, split):
    """14 .. 4326, the widest an old-style file may be (Rw2Decoder.cpp:80); new-style up to 9996"""
    rng = np.random.default_rng([2, split])
    for w in range(V.N, (4326 if split == 0 else 9996) + V.N, V.N):
        _check(ref, split, w, 2, V.random_stream(rng, split, w, 2, V.KINDS[(w // V.N) % 3]))


@pytest.mark.ref
@needs_ref
@pytest.mark.parametrize("split", V.SPLITS)
@pytest.mark.parametrize("packets", [1, 1023, 1024, 1025, 2048, 2049])
def test_block_boundaries(ref, split, packets):
    """the partial last block (split 0) resp. the padded one, exact multiples of a block, and one
    packet more"""
    rng = np.random.default_rng([4, split, packets])
    shapes = {(V.N, packets)} | ({(V.N * (packets // 8), 8)} if packets % 8 == 0 else set()) | \
        ({(V.N * packets, 1)} if V.N * packets <= 4330 or split else set())
    for w, h in sorted(shapes):
        if h > 2751 and split == 0:
            continue
        data = V.random_stream(rng, split, w, h, "sparse" if packets & 1 else "uniform")
        assert data.size == (16 * packets if split == 0 else -(-packets // 1024) * 0x4000)
        _check(ref, split, w, h, data)


@pytest.mark.ref
@needs_ref
@pytest.mark.parametrize("split", V.SPLITS)
def test_planted_packets(ref, split):
    planted = V.planted_packets()
    data = V.stream_from_packets(split, planted)
    w, h = V.N, len(planted)
    img, zeros = V.model_decode(split, w, h, data)
    assert (img[0] == 0).all() and img[1].tolist() == [0] * 12 + [5, 9]
    assert len(zeros) >= 14 + 12
    _check(ref, split, w, h, data)
    _check(ref, split, w * h, 1, data)  # the same packets side by side in one row


if __name__ == "__main__":
    record_golden()
