"""The model of ArwDecoder::SonyDecrypt / decodeSRF (tests/sony_srf_files.py, transcribed from
decoders/ArwDecoder.cpp:524-560 and :99-115) against its own restatements, the identities the
device relies on, and the host build of the core header (librsx_sony_srf_host.so).  The reference
cannot be run for this path here: the model and the host build are the yardstick of the device
tests."""
import numpy as np
import pytest

import sony_srf_files as F


def test_the_pad_of_key_zero_by_hand():
    # key 0: pad[0] = 1, pad[1] = 48828126, pad[2], pad[3] follow the recurrence, then the swap
    p = F.pad_from_key(0)
    k = [1]
    for _ in range(3):
        k.append((k[-1] * 48828125 + 1) & F.M32)
    k[3] = ((k[3] << 1) & F.M32) | ((k[0] ^ k[2]) >> 31)
    assert p[0] == 0x01000000 and p[1] == int.from_bytes(k[1].to_bytes(4, "little"), "big")
    assert p[3] == int.from_bytes(k[3].to_bytes(4, "little"), "big")
    assert len(p) == 128


@pytest.mark.parametrize("key", F.KEYS)
def test_flat_recurrence_equals_the_ring(key):
    ring = F.stream_ring(key, 1000)
    w = F.flat(key, 127 + 1000)
    assert w[127:] == ring
    assert F.stream(key, 1000).tolist() == ring
    for n in (1, 62, 63, 64, 126, 127, 128, 129):
        assert F.stream(key, n).tolist() == ring[:n]


@pytest.mark.parametrize("key", F.KEYS)
def test_doubling_identity(key):
    w = F.flat(key, 127 * 32 + 500)
    for k in range(1, 6):
        a, b = 127 << k, 63 << k
        for n in range(a, len(w)):
            assert w[n] == w[n - a] ^ w[n - b], (k, n)


@pytest.mark.parametrize("key", F.KEYS)
def test_decrypting_twice_is_the_identity(key):
    data = F.payload(4 * 777, seed=key & 0xFF)
    once = F.decrypt(data, key)
    assert not np.array_equal(once, data)
    assert np.array_equal(F.decrypt(once, key), data)


def test_decrypt_reads_the_input_as_little_endian_words():
    data = bytes(range(8))
    s = F.stream_ring(5, 2)
    want = (int.from_bytes(data[:4], "little") ^ s[0]).to_bytes(4, "little") + \
           (int.from_bytes(data[4:], "little") ^ s[1]).to_bytes(4, "little")
    assert F.decrypt(data, 5).tobytes() == want


def test_decode_srf_reads_big_endian_pairs():
    key, w, h = 9, 3, 2
    data = F.payload(2 * w * h)
    dec = F.decrypt(data, key)
    pix = F.decode_srf(data, key, w, h)
    for q in range(w * h):
        assert pix[q // w, q % w] == (int(dec[2 * q]) << 8) | int(dec[2 * q + 1])


@pytest.mark.parametrize("key", F.KEYS)
@pytest.mark.parametrize("n_words", F.N_WORDS + F.N_WORDS_CHUNK)
def test_host_library_equals_the_model(key, n_words):
    data = F.payload(4 * n_words, seed=n_words)
    want = F.decrypt(data, key)
    assert np.array_equal(F.host_decrypt(data, key), want)
    assert np.array_equal(F.host_decrypt(data, key, chunked=True), want)
    assert np.array_equal(F.host_decrypt(data, key, in_place=True), want)
    assert np.array_equal(F.host_decrypt(data, key, chunked=True, in_place=True), want)


def test_host_ring_equals_the_literal_ring():
    for key in F.KEYS:
        ring = np.array(F.stream_ring(key, 300), np.uint32)
        got = F.host_decrypt(bytes(1200), key).view("<u4")
        assert np.array_equal(got, ring)


@pytest.mark.parametrize("key", F.KEYS)
def test_host_jump_equals_the_flat_stream(key):
    w = np.array(F.flat(key, 127 + 3 * F.CHUNK + 200), np.uint32)
    for n in (0, 1, 2, 63, 64, 126, 127, 128, 254, F.CHUNK, F.CHUNK + 1, 2 * F.CHUNK, 3 * F.CHUNK + 73):
        assert np.array_equal(F.host_jump(key, n), w[n:n + 127]), n


def test_host_jump_far_out_agrees_with_the_chunked_walk():
    # word 4132800 is where a 3360 x 2460 frame ends; the jump there against the ring's walk
    key, n = 0x9E3779B9, 3360 * 2460 // 2
    tail = F.host_decrypt(bytes(4 * (n + 127)), key).view("<u4")[n - 127:]  # w[n .. n + 254)
    assert np.array_equal(F.host_jump(key, n), tail[:127])


@pytest.mark.parametrize("w,h", F.IMAGES)
def test_host_decode_equals_the_model(w, h):
    data = F.payload(2 * w * h + 6, seed=w)
    for pitch in (2 * w, (2 * w + 15) // 16 * 16 + 16):
        st, pix = F.host_decode(data, 0x9E3779B9, w, h, pitch)
        assert st == F.OK
        assert np.array_equal(pix, F.decode_srf(data, 0x9E3779B9, w, h))
