"""The inflate core of the deflate DNG kernel (rawspeed_amd/csrc/rsx_inflate_core.h) as host C++:
librsx_inflate_host.so over the valid, hand-assembled and mutation corpora of
tests/dng_deflate_files.py against libz's verdict, bytes and stream length; and the same corpora
through rsx_inflate_host_check, the sanitizer build, where every stream lies in an allocation of
exactly its size.  The GPU tests run the same corpora."""
import ctypes as C
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import dng_deflate_files as D
from rawspeed_amd import build


def _corpus():
    out = [(data, n) for _, data, n in D.inflate_shapes()]
    out += [(data, n) for _, data, n, _ in D.hand_streams()]
    out += [(d, (b // 8) * g[0] * g[1]) for b, _, _, g, d in D.mutants()]
    out += [(d, (b // 8) * g[0] * g[1]) for _, b, _, _, g, d in D.small_valid_tiles()]
    return out


@pytest.fixture(scope="module")
def corpus():
    c = _corpus()
    return c, [D.inflate_verdict(d, n) for d, n in c]


@pytest.fixture(scope="module")
def built():
    return build.build_inflate_host()


def test_the_library_agrees_with_libz(corpus, built):
    L = C.CDLL(built[0])
    L.rsx_inflate_host.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    assert L.rsx_inflate_host_shared_bytes() <= 40 * 1024
    cases, verdicts = corpus
    seen = set()
    for (data, n), (v, raw, used) in zip(cases, verdicts):
        src = np.frombuffer(bytes(data), np.uint8).copy() if data else np.zeros(1, np.uint8)
        out = np.full(n + 16, 0xA5, np.uint8)
        produced, consumed = C.c_uint32(0), C.c_uint32(0)
        got = L.rsx_inflate_host(src.ctypes.data, len(data), out.ctypes.data, n, C.byref(produced),
                                 C.byref(consumed))
        assert got == v, (len(data), n, got, v)
        assert (out[n:] == 0xA5).all()
        if v != D.FAIL:
            assert consumed.value == used and produced.value == len(raw)
        if v == D.OK:
            assert out[:n].tobytes() == raw
        seen.add(v)
    assert seen == {D.OK, D.SHORT, D.FAIL}


def test_the_sanitizer_build_agrees_with_libz(corpus, built):
    cases, verdicts = corpus
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "corpus.bin")
        with open(path, "wb") as f:
            for data, n in cases:
                f.write(struct.pack("<II", len(data), n))
                f.write(bytes(data))
        r = subprocess.run([built[1], path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    lines = r.stdout.split()
    assert len(lines) == 4 * len(cases)
    for k, (v, raw, used) in enumerate(verdicts):
        got, produced, consumed, h = (int(x) for x in lines[4 * k:4 * k + 4])
        assert got == v, k
        if v != D.FAIL:
            assert (produced, consumed) == (len(raw), used), k
        if v == D.OK:
            want = 2166136261
            for b in raw[:4096]:
                want = ((want ^ b) * 16777619) & 0xFFFFFFFF
            if len(raw) <= 4096:
                assert h == want, k
