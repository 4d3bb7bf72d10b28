"""rsx_vc5_core.h as host C++ (rawspeed_amd/librsx_vc5_host.so): the code look-up, the segment
walks in the band kernel's window scheme, and one wavelet level, against the numpy model
(tests/vc5_files.py) -- and the same corpora through a stand-alone program built with
AddressSanitizer and UBSan where g++ has their runtimes, every chunk in an allocation of exactly
its size.  Nothing here is loaded into Python under a sanitizer.  No GPU needed."""
import ctypes as C
import functools
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import vc5_files as V
from rawspeed_amd import abi, build


@pytest.fixture(scope="module")
def host():
    lib_path, _ = build.build_vc5_host()
    L = C.CDLL(lib_path)
    L.rsx_vc5_host_band.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_int32,
                                    C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.rsx_vc5_host_level.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.c_void_p]
    return L


def _codes(rows):
    arr = (abi.Vc5Code * len(rows))()
    for k, (size, bits, count, value) in enumerate(rows):
        arr[k].bits, arr[k].size, arr[k].count, arr[k].value = bits, size, count, value
    return arr


def _band(L, rows, data, quant, n, lanes):
    data = np.ascontiguousarray(data, np.uint8)
    out = np.full(n, 0x5A5A, np.int16)
    win, rnd = C.c_uint32(0), C.c_uint32(0)
    arr = _codes(rows)
    st = L.rsx_vc5_host_band(arr, len(rows), data.ctypes.data, data.size, quant, n,
                             out.ctypes.data, lanes, C.byref(win), C.byref(rnd))
    return st, out, win.value, rnd.value


def band_corpus():
    """[(name, rows, stream, quant, n)]: valid and damaged streams of one band"""
    out = []
    rng = np.random.default_rng(0xC0DE)
    rows = V.book()
    by_value, by_run, marker = V._rows_by_key()
    for k, (w, h, density, vmax) in enumerate(((17, 9, 0.0, 5), (33, 21, 0.05, 40), (40, 31, 0.6, 1023),
                                               (64, 50, 1.0, 8), (5, 3, 0.3, 20))):
        vals = V.random_band(rng, w, h, density, vmax)
        for quant in (1, -3, 32):
            out.append(("valid%d_q%d" % (k, quant), rows, V.encode_values(vals), quant, w * h))
        syms = V.symbols_of(vals)
        half = len(syms) // 2
        n = w * h
        out.append(("early%d" % k, rows, V.encode_symbols(syms[:half] + [(marker, False)] + syms[half:]), 2, n))
        out.append(("missing%d" % k, rows, V.encode_symbols(syms, marker=False, pad_to=1), 2, n))
        out.append(("past%d" % k, rows, V.encode_symbols(syms + [(by_run[12], False)]), 2, n - 3))
        out.append(("garbage%d" % k, rows, V.encode_symbols(syms, tail=V.Bits().put(0x2AAAAAAAAAA, 44)), 2, n))
        whole = V.encode_symbols(syms, pad_to=1)
        for cut in range(1, 9):  # truncated at every byte of its last symbols
            if len(whole) - cut >= 4:
                out.append(("cut%d_%d" % (k, cut), rows, whole[:len(whole) - cut], 2, n))
    holed, (bits, size) = V.book_with_hole()
    vals = V.random_band(rng, 20, 20, 0.3, 10)
    with V.use_book(holed):
        tail = V.Bits().put(bits, size).put(0, 30)
        out.append(("hole", holed, V.encode_symbols(V.symbols_of(vals.ravel()[:200]), marker=False, tail=tail), 1, 400))
        out.append(("hole_unused", holed, V.encode_values(vals), 1, 400))
    # value * quant at the edges of int16_t: 1023 * 32 = 32736, 993 * 33 = 32769, -(1024) * 32 = -32768
    for value, quant, neg in ((1023, 32, False), (1023, 32, True), (993, 33, False), (993, 33, True),
                              (1023, -32, False)):
        s = [(by_value[value], neg)] + V.symbols_of(np.zeros(29))
        out.append(("edge_%d_%d_%d" % (value, quant, neg), rows, V.encode_symbols(s), quant, 30))
    return out


def _model(rows, stream, quant, n):
    with V.use_book(rows):
        return V.model_band(stream, quant, n)


def test_band_decode_matches_the_model_at_every_window_size(host):
    for name, rows, stream, quant, n in band_corpus():
        want_st, want = _model(rows, stream, quant, n)
        for lanes in (1, 2, 3, 256):
            st, got, win, rnd = _band(host, rows, stream, quant, n, lanes)
            assert st == want_st, (name, lanes, st, want_st)
            if st == V.OK:
                assert np.array_equal(got, want), (name, lanes)
            assert win >= 1 and rnd >= win


def test_rounds_are_what_the_model_counts(host):
    rng = np.random.default_rng(5)
    vals = V.random_band(rng, 96, 64, 0.5, 1023)
    stream = V.encode_values(vals)
    for lanes in (4, 16, 256):
        st, _, win, rnd = _band(host, V.book(), stream, 1, vals.size, lanes)
        model = V.rounds_needed(stream, 1, vals.size, lanes)
        assert st == V.OK and (win, rnd) == (len(model), sum(model)), (lanes, win, rnd, model)


EDGE_LANES = (2, 3, 256, 1024)
EDGE_D = (-27, -1, 0, 1, 26)


@functools.lru_cache(maxsize=None)
def edge_corpus():
    """[(name, stream, quant, n, lanes, k, d, last)]: dense bands whose end marker starts d bits
    from the end of window k of `lanes` segments -- the marker sound, with its sign bit set, and a
    zero run in its place -- the chunk ending with the marker's last byte or padded to four.
    last: the bits of the last coefficient's symbol, or None; d = 26 comes with one of 27 bits,
    which starts in window k, and with one of 3, which starts in the window behind it."""
    out = []
    rng = np.random.default_rng(0xED6E)
    _, by_run, marker = V._rows_by_key()
    dense = V.symbols_of(V.random_band(rng, 1, 2 * V.WIN_BITS // 3, 1.0, 200))
    for lanes in EDGE_LANES:
        for k in (1, 2):
            for d, last in [(d, None) for d in EDGE_D[:-1]] + [(26, 27), (26, 3)]:
                target = k * lanes * V.SEG_BITS + d
                syms, n = V.symbols_ending_at(dense, target, last=last)
                for kind, end in (("sound", (marker, False)), ("sign", (marker, True)), ("run", (by_run[12], False))):
                    for pad in ((1, 4) if lanes < 256 else (1,) if k == 1 else (4,)):
                        stream = V.encode_symbols(syms + [end], marker=False, pad_to=pad)
                        name = "%s_%d_%d_%+d_%s_%d" % (kind, lanes, k, d, last, pad)
                        out.append((name, stream, -3, n, lanes, k, d, last))
    return out


def test_the_band_end_helper_lands_on_any_bit_and_count(host):
    rng = np.random.default_rng(7)
    dense = V.symbols_of(V.random_band(rng, 1, 600, 1.0, 200))
    for target, n, last in ((3, None, None), (97, None, None), (1000, None, 27), (1001, 700, None),
                            (1002, 2000, 3), (4099, 9000, 27)):
        syms, count = V.symbols_ending_at(dense, target, n=n, last=last)
        assert sum(V.symbol_bits(s)[0] for s in syms) == target
        assert count == sum(V.symbol_bits(s)[1] for s in syms) and (n is None or count == n)
        assert last is None or V.symbol_bits(syms[-1]) == (last, 1)
        stream = V.encode_symbols(syms, pad_to=1)
        assert 8 * stream.size == -(-(target + 27) // 8) * 8
        st, got, _, _ = _band(host, V.book(), stream, 2, count, 3)
        want_st, want = V.model_band(stream, 2, count)
        assert st == want_st == V.OK and np.array_equal(got, want)
    with pytest.raises(ValueError):
        V.symbols_ending_at(dense, 5)         # (no value symbol has 1, 2 or 5 bits)


def test_band_end_at_a_window_edge(host):
    """verdict and coefficients as the model's, windows and rounds as rounds_needed counts them:
    the band ends in the window whose lane reaches the last coefficient, and its marker is read
    from behind that window when it starts there"""
    for name, stream, quant, n, lanes, k, d, last in edge_corpus():
        want_st, want = V.model_band(stream, quant, n)
        assert want_st == (V.OK if name.startswith("sound") else V.MARKER), name
        st, got, win, rnd = _band(host, V.book(), stream, quant, n, lanes)
        assert st == want_st, (name, st, want_st)
        if st == V.OK:
            assert np.array_equal(got, want), name
        model = V.rounds_needed(stream, quant, n, lanes)
        assert (win, rnd) == (len(model), sum(model)), (name, win, rnd, model)
        assert win == (k + 1 if last == 3 else k), (name, win)


def test_rounds_needed_without_the_coefficient_count_walks_too_far(host):
    """what the count is for: a band that ends with a window's last segment (its marker starts at
    the edge or a bit behind it) ends in that window, as the core does; the walk that knows the
    stream alone goes on into the next one"""
    differ = 0
    for name, stream, quant, n, lanes, k, d, last in edge_corpus():
        if not name.startswith("sound") or lanes < 256:
            continue
        new = V.rounds_needed(stream, quant, n, lanes)
        old = V.rounds_needed_by_stream_alone(stream, quant, lanes)
        st, _, win, rnd = _band(host, V.book(), stream, quant, n, lanes)
        assert (win, rnd) == (len(new), sum(new))
        if d in (0, 1) or last == 27:
            assert len(old) == len(new) + 1 == k + 1 and (win, rnd) != (len(old), sum(old)), name
            differ += 1
        else:
            assert old == new, name
    assert differ == 12


def test_code_books_the_table_builder_refuses(host):
    rows = V.book()
    ok = lambda r: _band(host, r, V.encode_values(np.zeros(4)), 1, 4, 4)[0]  # noqa: E731
    assert ok(rows) == V.OK
    assert ok(rows[:1] + rows[:1]) == -1                        # the same word twice
    assert ok([(1, 0, 1, 0), (2, 1, 1, 1)]) == -1               # 0 is a prefix of 01
    assert ok([(0, 0, 1, 0)]) == -1 and ok([(27, 0, 1, 0)]) == -1
    assert ok([(2, 4, 1, 0)]) == -1                             # bits that do not fit the size
    assert ok([(2, 1, 512, 0)]) == -1 and ok([(2, 1, 1, 1024)]) == -1 and ok([(2, 1, 1, -1024)]) == -1
    assert ok(rows + [(26, 0, 1, 0)]) == -1                     # 265 words


def level_corpus():
    rng = np.random.default_rng(0x1E7E1)
    out = []
    for w, h, extra in ((3, 3, 0), (5, 3, 1), (3, 9, 0), (17, 17, 1), (64, 5, 0), (65, 4, 1)):
        for shift, clamp, lo, hi in ((0, 0, -32768, 32768), (2, 1, -2000, 20000), (2, 0, -32768, 32768)):
            pitch0 = w + extra
            b0 = rng.integers(lo, hi, (h + extra, pitch0)).astype(np.int16)
            b = [rng.integers(lo // 4, hi // 4, (h, w)).astype(np.int16) for _ in range(3)]
            out.append((w, h, pitch0, shift, clamp, b0, b))
    return out


def test_one_level_matches_the_model(host):
    for w, h, pitch0, shift, clamp, b0, b in level_corpus():
        got = np.zeros((2 * h, 2 * w), np.int16)
        host.rsx_vc5_host_level(b0.ctypes.data, pitch0, b[0].ctypes.data, b[1].ctypes.data,
                                b[2].ctypes.data, w, h, shift, clamp, got.ctypes.data)
        want = V.model_level(b0, b[0], b[1], b[2], 2 if shift else 0, bool(clamp))
        assert np.array_equal(got, want), (w, h, shift, clamp)


def _fnv(a):
    h = 2166136261
    for b in np.ascontiguousarray(a).tobytes():
        h = ((h ^ b) * 16777619) & 0xFFFFFFFF
    return h


def _sanitizers_link():
    """can g++ link a program against the static ASan and UBSan runtimes?"""
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        with open(src, "w") as f:
            f.write("int main() { return 0; }\n")
        r = subprocess.run(["g++", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                            "-o", os.path.join(d, "t"), src], capture_output=True)
        return r.returncode == 0


def test_the_check_program_is_instrumented_where_the_runtimes_exist():
    """build_vc5_host falls back to a plain program without the sanitizer runtimes; the run below
    must not pass for a plain program where an instrumented one could have been built"""
    _, prog = build.build_vc5_host()
    with open(prog, "rb") as f:
        instrumented = b"__asan_init" in f.read()
    print("rsx_vc5_host_check:", "ASan + UBSan" if instrumented else "plain (no sanitizer runtimes)")
    assert instrumented == _sanitizers_link()


def test_corpora_through_the_sanitizer_program(host):
    """the same streams and levels through rsx_vc5_host_check (ASan + UBSan where available):
    it must end cleanly and report what the library reported -- verdict, windows, rounds and the
    hash of the output"""
    _, prog = build.build_vc5_host()
    rows = V.book()
    holed, _ = V.book_with_hole()
    for book_rows, pick in ((rows, lambda r: r is rows), (holed, lambda r: r is not rows)):
        want = []
        with tempfile.NamedTemporaryFile(suffix=".bin") as f:
            f.write(struct.pack("<I", len(book_rows)))
            for size, bits, count, value in book_rows:
                f.write(struct.pack("<IIIi", bits, size, count, value))
            for name, r, stream, quant, n in band_corpus():
                if not pick(r):
                    continue
                for lanes in (1, 3, 256):
                    f.write(struct.pack("<IIiII", 1, len(stream), quant, n, lanes))
                    f.write(bytes(stream))
                    st, got, win, rnd = _band(host, r, stream, quant, n, lanes)
                    want.append("band %d %d %d %d" % (st, win, rnd, _fnv(got) if st == 0 else 0))
            if book_rows is rows:
                for name, stream, quant, n, lanes, _, _, _ in edge_corpus():
                    f.write(struct.pack("<IIiII", 1, len(stream), quant, n, lanes))
                    f.write(bytes(stream))
                    st, got, win, rnd = _band(host, rows, stream, quant, n, lanes)
                    want.append("band %d %d %d %d" % (st, win, rnd, _fnv(got) if st == 0 else 0))
                for w, h, pitch0, shift, clamp, b0, b in level_corpus():
                    f.write(struct.pack("<IIIIii", 2, w, h, pitch0, shift, clamp))
                    f.write(b0[:h].tobytes() + b[0].tobytes() + b[1].tobytes() + b[2].tobytes())
                    got = np.zeros((2 * h, 2 * w), np.int16)
                    host.rsx_vc5_host_level(b0.ctypes.data, pitch0, b[0].ctypes.data, b[1].ctypes.data,
                                            b[2].ctypes.data, w, h, shift, clamp, got.ctypes.data)
                    want.append("level %d" % _fnv(got))
            f.flush()
            r = subprocess.run([prog, f.name], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.splitlines() == want
