"""The Python model of tests/dng_deflate_files.py against tests/golden/dng_deflate_ref.json, which
was recorded from the reference's own DeflateDecompressor::decode; the tile writer against the
model; the corpora the other tests use."""
import hashlib
import json
import os

import numpy as np
import pytest

import dng_deflate_files as D

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dng_deflate_ref.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_model_gives_what_the_reference_gave(golden):
    seen = set()
    for t in golden["tiles"]:
        data, geom = bytes.fromhex(t["input_hex"]), tuple(t["geom"])
        v, bits, used = D.model_decode(data, t["bps"], t["predictor"], t["cpp"], geom)
        want = np.frombuffer(bytes.fromhex(t["output_hex"]), "<u4").reshape(geom[5], geom[4])
        assert v == D.OK and used == len(data)
        assert np.array_equal(bits, want), (t["bps"], t["predictor"], t["cpp"])
        seen.add((t["bps"], t["predictor"]))
        seen.add(("cpp", t["cpp"]))
        if geom[4] < geom[0] and geom[5] < geom[1] and geom[2] and geom[3]:
            seen.add("edge")
    assert seen >= {(b, p) for b in D.BPS for p in D.PREDICTORS} | {("cpp", 1), ("cpp", 3), "edge"}
    assert "provenance" in golden


def test_the_large_tile(golden):
    g = golden["large"]
    s = D.random_samples(np.random.default_rng(g["seed"]), g["bps"], 512, 512, "mixed")
    data = D.write_tile(s, g["bps"], g["predictor"], g["cpp"])
    assert hashlib.sha256(data).hexdigest() == g["input_sha256"]
    v, bits, _ = D.model_decode(data, g["bps"], g["predictor"], g["cpp"], tuple(g["geom"]))
    assert v == D.OK
    assert hashlib.sha256(bits.astype("<u4").tobytes()).hexdigest() == g["output_sha256"]
    assert np.array_equal(bits, D.widen(s, g["bps"]))


@pytest.mark.parametrize("bps", D.BPS)
@pytest.mark.parametrize("predictor", sorted(D.PREDICTORS))
@pytest.mark.parametrize("cpp", (1, 3))
def test_the_writer_round_trips_through_the_model(bps, predictor, cpp):
    rng = np.random.default_rng([1, bps, predictor, cpp])
    for tw, th in ((1, 1), (3, 2), (21, 5), (65, 2)):
        s = D.random_samples(rng, bps, th, tw * cpp, "bits")
        data = D.write_tile(s, bps, predictor, cpp)
        geom = (tw * cpp, th, 0, 0, tw * cpp, th)
        v, bits, used = D.model_decode(data, bps, predictor, cpp, geom)
        assert v == D.OK and used == len(data) and np.array_equal(bits, D.widen(s, bps))
        crop = (tw * cpp, th, 4, 2, max(1, tw * cpp - 1), max(1, th - 1))
        v, bits, _ = D.model_decode(data, bps, predictor, cpp, crop)
        assert np.array_equal(bits, D.widen(s, bps)[:crop[5], :crop[4]])


def test_the_verdicts_of_the_model():
    data = D.compress(bytes(range(48)))
    assert D.inflate_verdict(data, 48)[0] == D.OK
    assert D.inflate_verdict(data + b"xx", 48)[::2] == (D.OK, len(data))
    assert D.inflate_verdict(data, 49)[0] == D.SHORT
    assert D.inflate_verdict(data, 47)[0] == D.FAIL
    assert D.inflate_verdict(data[:-1], 48)[0] == D.FAIL
    assert D.inflate_verdict(b"", 48)[0] == D.FAIL


def test_hand_assembled_streams_are_what_they_were_made_for():
    names = set()
    for name, data, n, made_for in D.hand_streams():
        assert D.inflate_verdict(data, n)[0] == made_for, name
        assert n >= 2 and (n % 2 == 0 or n % 3 == 0), name  # (a tile of some sample width has that size)
        names.add(name)
    assert len(names) == len(D.hand_streams())


def test_the_mutation_corpus_has_both_verdicts():
    m = D.mutants()
    verdicts = [D.inflate_verdict(d, (b // 8) * g[0] * g[1])[0] for b, _, _, g, d in m]
    assert len(m) >= 300 and verdicts.count(D.OK) >= 30 and verdicts.count(D.FAIL) >= 100
    assert all((b // 8) * g[0] * g[1] <= 4096 for b, _, _, g, _ in m)
