"""VC5Decompressor on the device (rsx_vc5_*, rawspeed_amd/csrc/rsx_vc5.hip) through the C-ABI --
the host-pointer call and plans of several jobs -- against the model tests/vc5_files.py (which
tests/test_vc5_model.py pins against the reference's whole-file decode) and against
tests/golden/vc5_ref.json, the reference's recorded images and verdicts."""
import copy
import functools

import numpy as np
import pytest
import torch

import vc5_files as V
from oracle_lib import HostImage
from rawspeed_amd import abi

pytestmark = pytest.mark.gpu

OK = abi.RSX_OK


@pytest.fixture(scope="module")
def gpu():
    import gpu_util
    return gpu_util.ctx()


@pytest.fixture(scope="module")
def golden():
    rec = V.load_golden()
    return {int(k): np.array(v, np.uint16) for k, v in rec["tables"].items()}, rec


def _host(gpu, tile, table=None, gap=0, pitch=None, codes="book", container=False):
    data, bands = tile.vc5_block() if container else tile.layout(gap)
    d, keep = V.abi_desc(tile, bands, table, codes)
    out = HostImage(tile.w, tile.h, pitch=pitch)
    st = gpu.vc5_decompress(d, data, out.view())
    return st, out, data, bands


def _padding_kept(out):
    return (out.buf.reshape(out.dim_y, out.pitch)[:, 2 * out.dim_x:] == 0xA5).all()


def _plan(gpu, tiles, tables=None, codes=None, gaps=None, pads=None, times=1, pitches=None,
          models=None, info=None):
    """tiles in one plan: odd input offsets, padded pitches, gaps between images.
    [(rc, statuses, image bytes, per-job (band status, windows, rounds))] per run, the expected
    (offset, pitch, tile, model status, model image, model band statuses).
    pitches: the pitch of every job; an image whose pitch is a multiple of 16 then starts on 16
    bytes.  models: model_decode's answer per job, where the caller has it.  info: a dict that
    gets in_offsets and bands, where every job's input and its chunks lie."""
    jobs, keep, parts, expect = [], [], [np.full(3, 0x5A, np.uint8)], []
    in_off, img_off = 3, 0
    if info is not None:
        info["in_offsets"], info["bands"] = [], []
    for k, t in enumerate(tiles):
        data, bands = t.layout(gap=(gaps or [0, 1, 5])[k % 3])
        table = None if tables is None else tables[k]
        rows = "book" if codes is None or codes[k] is None else codes[k]
        d, kp = V.abi_desc(t, bands, table, rows)
        keep.append(kp)
        pitch = 2 * t.w + (pads or [0, 2, 16, 6])[k % 4] if pitches is None else pitches[k]
        if pitches is not None and pitch % 16 == 0:
            img_off = -(-img_off // 16) * 16
        if info is not None:
            info["in_offsets"].append(in_off)
            info["bands"].append(bands)
        j = abi.Vc5Job()
        j.desc = d
        j.in_offset, j.in_bytes, j.img_offset = in_off, data.size, img_off
        j.img = abi.Image(None, pitch, t.w, t.h, 1, 1)
        jobs.append(j)
        parts += [data, np.full(1 + k % 3, 0x5A, np.uint8)]
        if models is not None:
            st, img, bst = models[k]
        elif rows == "book":
            st, img, bst = V.model_decode(t, data, bands, table)
        else:
            with V.use_book(rows):
                st, img, bst = V.model_decode(t, data, bands, table)
        expect.append((img_off, pitch, t, st, img, bst))
        in_off += data.size + 1 + k % 3
        img_off += pitch * t.h + [0, 2, 16][k % 3]
    din = torch.from_numpy(np.concatenate(parts)).cuda()
    plan = gpu.vc5_plan(jobs)
    outs = []
    for _ in range(times):
        out = torch.full((img_off,), 0xA5, dtype=torch.uint8, device="cuda")
        plan.run(din.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        rc, st, cons = plan.results()
        outs.append((rc, st, out.cpu().numpy(), [plan.bands(k) for k in range(len(jobs))]))
    plan.close()
    return outs, expect


def _check_plan(outs, expect):
    covered = np.zeros(outs[0][2].size, bool)
    for off, pitch, t, st, img, bst in expect:
        if st == OK:
            for r in range(t.h):
                covered[off + r * pitch:off + r * pitch + 2 * t.w] = True
    for rc, sts, host, bands in outs:
        assert sts == [e[3] for e in expect]
        assert (rc == OK) == all(s == OK for s in sts)
        assert (host[~covered] == 0xA5).all()  # padding, gaps, and every image of a failed job
        for k, (off, pitch, t, st, img, bst) in enumerate(expect):
            assert np.array_equal(bands[k][0], bst), k
            if st == OK:
                px = np.stack([host[off + r * pitch:off + r * pitch + 2 * t.w].view(np.uint16)
                               for r in range(t.h)])
                assert np.array_equal(px, img), (k, t.w, t.h)
    assert all(np.array_equal(outs[0][2], o[2]) for o in outs)  # a second run repeats the first


# ---------------------------------------------------------------------------- geometry, merge
@pytest.mark.parametrize("w,h", [(34, 34), (36, 34), (48, 40), (34, 52), (130, 66)])
def test_host_call_matches_the_model(gpu, w, h):
    """34 x 34: every level odd (17 / 9 / 5 / 3).  Both phases, three white levels, prescale 0
    and 2 per level and differing per channel, pitches on and off the 16-byte grid."""
    for k in range(4):
        t = V.make_tile(w * 7 + k, w, h, phase=k % 2, white=V.WHITES[k % 3],
                        prescale=V.PRESCALES[k], precision=(16, 12, 8, 10)[k],
                        low=((0, 65536), (0, 4096), (0, 256), (0, 1024))[k])
        st, out, data, bands = _host(gpu, t, gap=k, pitch=2 * w + (0, 6, 16, 2)[k], container=k == 3)
        mst, want, _ = V.model_decode(t, data, bands)
        assert st == OK == mst
        assert np.array_equal(out.pixels(), want), (w, h, k)
        assert _padding_kept(out)


def test_recorded_reference_images(gpu, golden):
    """the reference's own answers (SHA-256), with the log tables the reference agreed with;
    every row of the book with both signs is among them"""
    tables, rec = golden
    for name, tile in V.golden_cases():
        st, out, _, _ = _host(gpu, tile, tables[tile.white], container=True)
        assert st == OK and V.sha(out.pixels()) == rec["cases"][name]["image"], name
        assert _padding_kept(out)


def test_recorded_reference_failures(gpu, golden):
    tables, rec = golden
    for name, tile, expect in V.failing_cases():
        st, out, data, bands = _host(gpu, tile, tables[tile.white], container=True)
        want = rec["failing"][name]["image"]
        assert (st == OK) == (want is not None), name
        if want is None:
            assert (out.buf == 0xA5).all(), name
            assert st == V.model_decode(tile, data, bands)[0], name
        else:
            assert V.sha(out.pixels()) == want, name


def test_value_edges_of_wavelet_and_merge(gpu):
    """16-bit low-pass values above 32767 wrap; level-1 results below 0 and above 16383 are
    clamped; merge values below 0 and above 4095 take the table's ends"""
    t = V.make_tile(77, 48, 40, prescale=V.PRESCALES[1], low=(0, 65536), vmax=1023, density=0.5,
                    quant=lambda c, l, b: 32 if (c + l + b) % 2 else -31)
    data, bands = t.layout()
    planes = []
    mst, want, _ = V.model_decode(t, data, bands, planes_out=planes)
    low = V.model_lowpass(t.chunks[0][0], 16, *t.dims()[3])
    assert (low < 0).any()                                     # above 32767 as written
    assert all((p == 0).any() and (p == 16383).any() for p in planes)
    gs, gd = planes[0].astype(int), planes[3].astype(int) - 2048
    assert (gs + gd > 4095).any() and (gs - gd < 0).any()
    table = np.arange(4096, dtype=np.uint16) * 16 + 7           # the ends are told apart
    st, out, data, bands = _host(gpu, t, table)
    assert st == OK and np.array_equal(out.pixels(), V.model_decode(t, data, bands, table)[1])
    assert (out.pixels() == 7).any() and (out.pixels() == 4095 * 16 + 7).any()


def test_dequantisation_edges(gpu):
    """value * quant of exactly 32767 / -32768 passes, one more fails; negative quant"""
    by_value, by_run, marker = V._rows_by_key()
    w, h = 48, 40
    n = V.dims(w, h)[1][0] * V.dims(w, h)[1][1]
    cases = []
    # the book's values: 1 * 32767, -1 * -32768 -> 32768 fails, 1 * -32768, 2 * 16384 fails,
    # 1023 * 32 = 32736, 993 * 33 = 32769 fails, -993 * 33 fails, 4 * -8192 = -32768, -4 * -8192 fails
    for value, neg, quant, ok in ((1, False, 32767, True), (1, True, -32768, False), (1, False, -32768, True),
                                  (2, False, 16384, False), (2, True, 16384, True), (1023, False, 32, True),
                                  (993, False, 33, False), (993, True, 33, False), (4, False, -8192, True),
                                  (4, True, -8192, False)):
        t = V.make_tile(5, w, h)
        syms = V.symbols_of(np.zeros(n - 1)) + [(by_value[value], neg)]
        t.set_band(1, 1, 2, quant=quant, stream=V.encode_symbols(syms))
        cases.append((t, ok))
    outs, expect = _plan(gpu, [t for t, _ in cases])
    assert [e[3] == OK for e in expect] == [ok for _, ok in cases]
    assert {e[3] for e in expect} == {OK, V.RANGE}
    _check_plan(outs, expect)


# ---------------------------------------------------------------------------- band streams
def _window_tile(extra_segments=5):
    """A level-1 band whose stream is one window and a few segments long.  The size follows from
    the window: a dense coefficient takes 8 bits or more, so WIN_BITS / 8 of them are enough; the
    dense part is cut where the stream has the wanted length, zero runs follow."""
    w1 = 3 * V.WIN_BITS // 4096
    h1 = -(-V.WIN_BITS // 8 // w1)
    w, h = 4 * w1, 4 * h1
    t = V.make_tile(9, w, h, density=0.02)
    assert t.dims()[1] == (w1, h1)
    rng = np.random.default_rng(99)
    dense = V.random_band(rng, w1, h1, 1.0, 200).ravel()
    lo, hi = 0, dense.size
    while hi - lo > 1:  # the longest dense prefix whose stream stays within the target
        mid = (lo + hi) // 2
        v = np.concatenate((dense[:mid], np.zeros(dense.size - mid, np.int64)))
        bits = 8 * V.encode_values(v, pad_to=1).size
        lo, hi = (mid, hi) if bits <= V.WIN_BITS + extra_segments * V.SEG_BITS else (lo, mid)
    v = np.concatenate((dense[:lo], np.zeros(dense.size - lo, np.int64)))
    stream = V.encode_values(v)
    assert V.WIN_BITS + 2 * V.SEG_BITS < 8 * stream.size <= V.WIN_BITS + (extra_segments + 1) * V.SEG_BITS
    t.set_band(2, 1, 3, quant=-5, stream=stream)
    return t


def _never_meeting_stream(n):
    """n coefficients 4, 2, -2, 2, -2, ..: behind a 7-bit symbol the stream is 1110 1111 repeated,
    and every segment starts one bit into that period, from where a parse reads other symbols
    for ever and never lands on a true symbol boundary"""
    by_value, _, _ = V._rows_by_key()
    syms = [(by_value[4], False)] + [(by_value[2], k % 2 == 1) for k in range(n - 1)]
    return V.encode_symbols(syms)


def test_band_streams(gpu):
    """an all-zero band, runs that cross rows, segments and windows, a dense band of random rows
    of the book, a stream one window and a few segments long (384 x 684 at 128-Kbit windows), a stream whose guessed
    parses never meet the true one, a band that ends mid-segment with garbage behind the marker"""
    tiles = []
    t = V.make_tile(31, 130, 66, density=0.9, vmax=1023,
                    quant=lambda c, l, b: (1, -1, 3, -2)[(c + l + b) % 4])   # dense, any row
    w1, h1 = t.dims()[1]
    t.set_band(0, 1, 1, np.zeros((h1, w1), np.int64), 9)                      # all zero
    sparse = np.zeros(w1 * h1, np.int64)
    sparse[[0, 321, 322, w1 * h1 - 1]] = [3, -1023, 7, -1]                     # runs across rows
    t.set_band(1, 1, 2, sparse.reshape(h1, w1), -7)
    vals = V.random_band(np.random.default_rng(4), w1, h1, 0.4)
    tail = V.Bits().put(0x155555555555555, 57).put(0x3FFFFFF, 26)            # garbage behind the marker
    t.set_band(3, 1, 3, quant=2, stream=V.encode_symbols(V.symbols_of(vals), tail=tail))
    tiles.append(t)
    tiles.append(_window_tile())
    t = V.make_tile(32, 512, 384, density=0.02)
    w1, h1 = t.dims()[1]
    stream = _never_meeting_stream(w1 * h1)
    rounds = V.rounds_needed(stream, 3, w1 * h1)
    assert len(rounds) == 1 and rounds[0] > 100        # (checked, not assumed: about one a segment)
    t.set_band(1, 1, 1, quant=3, stream=stream)
    tiles.append(t)
    outs, expect = _plan(gpu, tiles, times=2)
    assert all(e[3] == OK for e in expect)
    _check_plan(outs, expect)
    st, win, rnd = outs[0][3][1]                        # the window tile: two windows
    assert win[2, V.subband(1, 3)] == 2
    st, win, rnd = outs[0][3][2]
    assert (win[1, 7], rnd[1, 7]) == (1, rounds[0])
    for k, t in enumerate(tiles):                       # rounds as the model counts them
        st, win, rnd = outs[0][3][k]
        for c in range(4):
            for s in range(1, 10):
                wk, hk = t.dims()[3 - (s - 1) // 3]
                r = V.rounds_needed(t.chunks[c][s], t.quant[c][s], wk * hk)
                assert (win[c, s], rnd[c, s]) == (len(r), sum(r)), (k, c, s)


# ---------------------------------------------------------------------------- past the first tile
EDGE_TABLE = np.arange(4096, dtype=np.uint16) * 16 + 7   # tells the clamped ends apart


def _variant(t, **kw):
    """the tile with other attributes; its chunk and quant lists are its own"""
    v = copy.copy(t)
    v.chunks, v.quant = [list(c) for c in t.chunks], [list(q) for q in t.quant]
    for k, x in kw.items():
        setattr(v, k, x)
    return v


def _tiles(n, per):
    return (n + per - 1) // per


@pytest.mark.parametrize("w,tx,last", [(514, 2, 1), (518, 2, 3), (1026, 3, 1), (1030, 3, 3)])
def test_merge_workgroups_behind_the_first_of_a_row(gpu, w, tx, last):
    """w / 2 = 257, 259, 513, 515 cells a row: a second and a third merge workgroup across, whose
    last lane holds 1 or 3 cells (its other cells read clamped columns and are not written), and
    33 cell rows, a second workgroup down.  Both phases, the three white levels' tables and one
    that tells the clamped ends apart; pitches on the 16-byte grid (16-byte stores in the full
    lanes) and 2, 6 and 16 bytes off it; a plan and the host-pointer call."""
    h = 66
    w2, h2 = w // 2, h // 2
    assert _tiles(w2, V.MERGE_CELLS) == tx >= 2 and w2 % V.MERGE_LANE_CELLS == last
    assert (w2 - 1) // V.MERGE_LANE_CELLS % 64 == 0           # the ragged lane is lane 0 of its tile
    assert _tiles(h2, V.MERGE_ROWS) == 2 and _tiles(V.dims(w, h)[1][0], V.LEVEL_X) >= 3
    base = V.make_tile(w, w, h, prescale=V.PRESCALES[1], low=(0, 65536), vmax=1023, density=0.5,
                       quant=lambda c, l, b: 32 if (c + l + b) % 2 else -31)
    data, bands = base.layout()
    planes = []
    st, _, bst = V.model_decode(base, data, bands, planes_out=planes)
    assert st == OK
    grid = (2 * w + 15) // 16 * 16
    tiles, tables, pitches, models = [], [], [], []
    for k, off in enumerate((0, 2, 6, 16, 0, 6)):
        t = _variant(base, phase=k % 2 if k < 4 else 1 - k % 2, white=V.WHITES[(0, 1, 2, 1, 0, 2)[k]])
        table = EDGE_TABLE if k in (1, 2, 4) else V.log_table(t.white)
        tiles.append(t), tables.append(table), pitches.append(grid + off)
        models.append((OK, V.model_merge(planes, w, h, t.phase, table), bst))
    assert {(t.phase, p % 16 == 0) for t, p in zip(tiles, pitches)} == {(0, True), (0, False), (1, True), (1, False)}
    assert {t.white for t, x in zip(tiles, tables) if x is not EDGE_TABLE} == set(V.WHITES)
    outs, expect = _plan(gpu, tiles, tables=tables, pitches=pitches, models=models, times=2)
    assert all((off | pitch) % 16 == 0 for off, pitch, *_ in expect if pitch % 16 == 0)
    _check_plan(outs, expect)
    edge = models[1][1][:, 2 * V.MERGE_CELLS * (tx - 1):]     # the last workgroup's columns
    assert edge.shape[1] == 2 * (w2 - V.MERGE_CELLS * (tx - 1)) and (edge == 7).any() and (edge == 4095 * 16 + 7).any()
    for k in (1, 3, 5):
        st, out, _, _ = _host(gpu, tiles[k], tables[k], pitch=pitches[k])
        assert st == OK and np.array_equal(out.pixels(), models[k][1]), (w, k)
        assert _padding_kept(out)


@pytest.mark.parametrize("w,h,precision", [(V.MAX_DIM, V.MIN_DIM, 13), (V.MIN_DIM, V.MAX_DIM, 14)])
def test_largest_side_against_the_smallest(gpu, w, h, precision):
    """65534 x 34 and 34 x 65534: 128 merge workgroups a row or 1024 rows of them, 256 level-1
    workgroups across or 4096 down, and a low-pass band of 4096 x 3 fields, three trips of the
    low-pass kernel's loop"""
    t = V.make_tile(w // 7, w, h, phase=int(w > h), density=0.02, precision=precision, low=(0, 1 << precision))
    d = t.dims()
    assert max(_tiles(w // 2, V.MERGE_CELLS), _tiles(h // 2, V.MERGE_ROWS)) == (128 if w > h else 1024)
    assert max(_tiles(d[1][0], V.LEVEL_X), _tiles(d[1][1], V.LEVEL_Y)) == (256 if w > h else 4096)
    assert d[3][0] * d[3][1] == 3 * V.LP_STRIDE and min(d[3]) == 3
    outs, expect = _plan(gpu, [t], times=2)
    assert expect[0][3] == OK
    _check_plan(outs, expect)


def test_lowpass_band_past_one_stride_and_every_precision(gpu):
    """A band of 129 x 34 = 4386 fields (the loop's second trip) and three of 32 x 24 = 768, whose
    chunks end with their last field for every precision; precisions 8 .. 16, one per channel;
    full-range fields, the last one all ones, a foreign 0xEE behind every chunk; chunks at every
    address residue mod 4."""
    rng = np.random.default_rng(0x10A5)
    tiles = [V.make_tile(40, 2050, 530, density=0.02)]
    tiles += [V.make_tile(41 + k, 512, 384, phase=k % 2, density=0.02) for k in range(3)]
    precisions = [(9, 11, 13, 15), (8, 9, 10, 11), (12, 13, 14, 15), (16, 14, 10, 12)]
    for t, pp in zip(tiles, precisions):
        w3, h3 = t.dims()[3]
        for c, p in enumerate(pp):
            v = rng.integers(0, 1 << p, (h3, w3))
            v[-1, -1] = (1 << p) - 1
            t.set_lowpass(c, v, p)
            if t.w == 512:
                assert 8 * t.chunks[c][0].size == w3 * h3 * p  # no padding behind the last field
    w3, h3 = tiles[0].dims()[3]
    assert V.LP_STRIDE < w3 * h3 < 2 * V.LP_STRIDE
    assert {p for pp in precisions[1:] for p in pp} == set(range(8, 17))
    info = {}
    outs, expect = _plan(gpu, tiles, gaps=[1, 1, 1], times=2, info=info)
    where = {(o + b[c][0][0]) % 4 for o, b in zip(info["in_offsets"], info["bands"]) for c in range(4)}
    assert where == {0, 1, 2, 3}
    assert all(e[3] == OK for e in expect)
    _check_plan(outs, expect)


# ---------------------------------------------------------------------------- the window's edge
EDGE_BAND = (2, 1, 3)          # (channel, level, band) of the stream under test, as in _window_tile
EDGE_QUANT = -5
PLACES = ((1, -27, None), (1, -1, None), (1, 0, None), (1, 1, None), (1, 26, 27), (1, 26, 3),
          (2, 0, None), (2, 26, 27), (2, 26, 3))   # (window edge k, marker's distance d, last symbol's bits)


@functools.lru_cache(maxsize=None)
def _edge_base(windows):
    """(a sparse tile whose level-1 bands can hold `windows` windows of dense symbols, such symbols)"""
    w1 = 3 * V.WIN_BITS // 4096
    h1 = windows * -(-V.WIN_BITS // 8 // w1)
    t = V.make_tile(9, 4 * w1, 4 * h1, density=0.02)
    assert t.dims()[1] == (w1, h1)
    rng = np.random.default_rng([99, windows])
    return t, V.symbols_of(V.random_band(rng, w1, h1, 1.0, 200))


@functools.lru_cache(maxsize=None)
def _edge_symbols(k, d, last):
    """symbols of a whole band of _edge_base(k) whose end marker starts d bits behind window k"""
    t, dense = _edge_base(k)
    w1, h1 = t.dims()[1]
    syms, n = V.symbols_ending_at(dense, k * V.WIN_BITS + d, n=w1 * h1, last=last)
    if last is not None:   # 27 bits: the symbol starts in front of the edge; 3: behind it
        assert (k * V.WIN_BITS + d - last < k * V.WIN_BITS) == (last == 27)
    return syms


def _edge_tile(k, stream):
    t = _variant(_edge_base(k)[0])
    t.set_band(*EDGE_BAND, quant=EDGE_QUANT, stream=stream)
    return t


def _edge_counters(outs, tiles):
    """[(windows, rounds)] of the band under test as the device counted, and as the model counts"""
    c, s = EDGE_BAND[0], V.subband(*EDGE_BAND[1:])
    got, want = [], []
    for k, t in enumerate(tiles):
        w1, h1 = t.dims()[1]
        r = V.rounds_needed(t.chunks[c][s], EDGE_QUANT, w1 * h1)
        want.append((len(r), sum(r)))
        got.append((int(outs[0][3][k][1][c, s]), int(outs[0][3][k][2][c, s])))
    return got, want


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("end", ["sound", "sign", "run"])
def test_band_end_at_a_window_edge(gpu, end, k):
    """The end marker starts d = -27 .. 26 bits from the end of the first window, or of the
    second: it lies in the window, across its edge, or in the four words loaded behind it, which
    lane 1023 reads when it holds the band's last coefficient.  The band ends in that lane's
    window; only a coefficient symbol that starts behind the edge (d = 26 behind a 3-bit symbol)
    brings the next window in, the third for k = 2.  Chunks that end with the marker's last byte
    and chunks padded to four, behind them foreign bytes.  sound: OK, the model's pixels; sign /
    run: the marker with its sign bit set or a zero run in its place fail the band, which shows
    that the bits behind the window are read; the image stays untouched.  Windows and rounds are
    those of the model in every case."""
    _, by_run, marker = V._rows_by_key()
    last_symbol = {"sound": (marker, False), "sign": (marker, True), "run": (by_run[12], False)}[end]
    tiles, windows, behind = [], [], []
    for kk, d, last in PLACES:
        if kk != k:
            continue
        syms = _edge_symbols(k, d, last)
        assert sum(V.symbol_bits(s)[0] for s in syms) == k * V.WIN_BITS + d
        for pad in (1, 4):
            stream = V.encode_symbols(syms + [last_symbol], marker=False, pad_to=pad)
            behind.append(8 * stream.size - k * V.WIN_BITS)
            tiles.append(_edge_tile(k, stream))
            windows.append(k + 1 if last == 3 else k)
    if end != "run":   # the chunks end with the window, or in the words loaded behind it
        assert min(behind) == (0 if k == 1 else 32) and 32 < max(behind) <= 32 * V.WIN_EXTRA_WORDS
    outs, expect = _plan(gpu, tiles, times=2)
    assert [e[3] for e in expect] == [OK if end == "sound" else V.MARKER] * len(tiles)
    assert all((e[5] != OK).sum() == (end != "sound") for e in expect)
    _check_plan(outs, expect)
    got, want = _edge_counters(outs, tiles)
    assert got == want
    assert [w for w, _ in got] == windows and (k == 1 or 3 in windows)


def test_chunk_that_ends_at_the_window_edge_without_a_marker(gpu):
    """Chunks of WIN_BITS / 8 bytes and 4, 8, 12 and 16 less: the reader's limit lies 64 bits
    behind the chunk, at WIN_BITS + 64 .. WIN_BITS - 64, and the band wants 10 or 100 coefficients
    more than its symbols give.  The zeros behind the chunk are coefficients: 10 of them end the
    band without a marker, 100 run into the limit -- in lane 1023, behind it, or in lane 0 of a
    second window that holds no byte of the chunk."""
    t0, dense = _edge_base(1)
    w1, h1 = t0.dims()[1]
    tiles, limits = [], []
    for less in (0, 4, 8, 12, 16):
        nbytes = V.WIN_BITS // 8 - less
        limits.append(V.start_limit(nbytes) - V.WIN_BITS)
        for short in (10, 100):
            syms, _ = V.symbols_ending_at(dense, 8 * nbytes, n=w1 * h1 - short)
            stream = V.encode_symbols(syms, marker=False, pad_to=1)
            assert stream.size == nbytes
            tiles.append(_edge_tile(1, stream))
    assert limits == [64, 32, 0, -32, -64]
    outs, expect = _plan(gpu, tiles, times=2)
    assert [e[3] for e in expect] == [V.MARKER, V.OVERREAD] * 5
    _check_plan(outs, expect)
    got, want = _edge_counters(outs, tiles)
    assert got == want and {w for w, _ in got} == {1, 2}


def test_longest_symbol_across_the_window_edge(gpu):
    """A coefficient symbol of 27 bits (the book's one value word of 26) that starts at the
    window's last bit: lane 0 of the second window enters 26 bits in, the largest carry there is,
    and dense coefficients follow."""
    t0, dense = _edge_base(1)
    w1, h1 = t0.dims()[1]
    rest = dense[-300:]
    assert all(V.symbol_bits(s)[1] == 1 for s in rest)
    syms, _ = V.symbols_ending_at(dense, V.WIN_BITS + 26, n=w1 * h1 - len(rest), last=27)
    stream = V.encode_symbols(syms + rest)
    carries = []
    rounds = V.rounds_needed(stream, EDGE_QUANT, w1 * h1, carries=carries)
    assert len(rounds) == 2 and carries == [0, 26] and carries[1] >= 20
    tiles = [_edge_tile(1, stream)]
    outs, expect = _plan(gpu, tiles, times=2)
    assert expect[0][3] == OK
    _check_plan(outs, expect)
    got, want = _edge_counters(outs, tiles)
    assert got == want == [(2, sum(rounds))]


# ---------------------------------------------------------------------------- failures
def _damage(kind, c, level, band, w=48, h=40, seed=60, hole=None):
    """a tile whose band (c, level, band) fails in the given way ("code": inside a use_book block
    of a book with a hole, `hole` the (bits, size) that begin no word there)"""
    by_value, by_run, marker = V._rows_by_key()
    t = V.make_tile(seed, w, h)
    wk, hk = t.dims()[level]
    n = wk * hk
    vals = V.random_band(np.random.default_rng([seed, c, level]), wk, hk, 0.3)
    syms = V.symbols_of(vals)
    half = len(syms) // 2
    if kind == "early":
        stream = V.encode_symbols(syms[:half] + [(marker, False)] + syms[half:])
    elif kind == "missing":
        stream = V.encode_symbols(syms, marker=False, tail=V.Bits().put(0, 64))
    elif kind == "past":
        stream = V.encode_symbols(V.symbols_of(vals.ravel()[:n - 5]) + [(by_run[12], False)])
    elif kind == "code":
        stream = V.encode_symbols(syms[:half], marker=False, tail=V.Bits().put(*hole).put(0, 64))
    else:
        whole = V.encode_symbols(syms, pad_to=1)
        stream = whole[:max(4, len(whole) - int(kind))]
    t.set_band(c, level, band, quant=3, stream=stream)
    return t


BANDS = ((0, 3, 1), (1, 2, 2), (3, 1, 3))  # the first, a middle and the last band


@pytest.mark.parametrize("kind", ["early", "missing", "past"])
def test_failures_in_the_first_a_middle_and_the_last_band(gpu, kind):
    tiles = [_damage(kind, *b) for b in BANDS]
    # two at once, of the same kind and of two kinds: the first one gives the status
    tiles += [_two_damaged(kind, kind), _two_damaged("past" if kind != "past" else "early", kind)]
    tiles.append(V.make_tile(61, 48, 40))          # and a sound one beside them
    outs, expect = _plan(gpu, tiles, times=2)
    assert [e[3] for e in expect] == [V.MARKER] * 5 + [OK]
    assert [(e[5] != OK).sum() for e in expect] == [1, 1, 1, 2, 2, 0]
    _check_plan(outs, expect)
    # the host-pointer call: the status, and the caller's image untouched, canary included
    st, out, _, _ = _host(gpu, tiles[1], pitch=2 * 48 + 16)
    assert st == V.MARKER and (out.buf == 0xA5).all()


def _two_damaged(first, last, **kw):
    """a tile whose first band fails as `first` and whose last band fails as `last`"""
    t, other = _damage(last, *BANDS[2], **kw), _damage(first, *BANDS[0], **kw)
    s = V.subband(*BANDS[0][1:])
    t.chunks[BANDS[0][0]][s], t.quant[BANDS[0][0]][s] = other.chunks[BANDS[0][0]][s], other.quant[BANDS[0][0]][s]
    return t


def test_invalid_code_with_a_book_that_has_a_hole(gpu):
    """a book with a hole: 25 bits that begin no word, alone in each band, in two bands at once,
    and beside a band that fails in another way (the first failing band gives the status); jobs
    with the whole book and sound jobs with the holed one run in the same plan"""
    rows, hole = V.book_with_hole()
    with V.use_book(rows):
        tiles = [_damage("code", *b, hole=hole) for b in BANDS]
        tiles += [_two_damaged("code", "code", hole=hole), _two_damaged("code", "early", hole=hole),
                  _two_damaged("past", "code", hole=hole), V.make_tile(41, 48, 40)]
    tiles.append(V.make_tile(41, 48, 40))
    outs, expect = _plan(gpu, tiles, codes=[rows] * 7 + [None], times=2)
    assert [e[3] for e in expect] == [V.CODE] * 5 + [V.MARKER, OK, OK]
    assert [(e[5] != OK).sum() for e in expect] == [1, 1, 1, 2, 2, 2, 0, 0]
    assert (expect[3][5] == V.CODE).sum() == 2
    _check_plan(outs, expect)
    # the host-pointer call: the status, and the caller's image untouched, canary included
    for k in (0, 2, 3):
        st, out, _, _ = _host(gpu, tiles[k], pitch=2 * 48 + 16, codes=rows)
        assert st == V.CODE and (out.buf == 0xA5).all()


def test_chunk_truncated_at_every_byte_of_its_last_symbols(gpu):
    """the bytes that are gone read as zeros -- coefficients of 0, never the end marker -- and a
    chunk cut far in front of its end runs into the reader's limit; then two truncated bands at
    once, cut near their ends and far in front of them"""
    kw = dict(w=130, h=66)
    tiles = [_damage(str(cut), *BANDS[cut % 3], **kw) for cut in range(1, 13)]
    tiles += [_damage(str(cut), 2, 1, 1, **kw) for cut in (40, 120)]
    tiles += [_two_damaged("9", "5", **kw), _two_damaged("3", "11", **kw), _two_damaged("40", "120", **kw)]
    outs, expect = _plan(gpu, tiles)
    assert {e[3] for e in expect} == {V.MARKER, V.OVERREAD}
    assert [(e[5] != OK).sum() for e in expect] == [1] * 14 + [2] * 3
    _check_plan(outs, expect)
    st, out, _, _ = _host(gpu, tiles[-1], pitch=2 * 130 + 16)
    assert st == expect[-1][3] and (out.buf == 0xA5).all()


def test_plan_of_jobs_of_different_sizes_and_a_rejected_one(gpu):
    tiles = [V.make_tile(70 + k, w, h, phase=k % 2, white=V.WHITES[k % 3], prescale=V.PRESCALES[k % 4])
             for k, (w, h) in enumerate(((34, 34), (130, 66), (36, 34), (48, 40), (66, 130)))]
    outs, expect = _plan(gpu, tiles, times=2)
    _check_plan(outs, expect)
    # a job the validation refuses gets its status; the others decode
    data, bands = tiles[0].layout()
    d, keep = V.abi_desc(tiles[0], bands)
    jobs = []
    for k in range(2):
        j = abi.Vc5Job()
        j.desc = d
        j.in_offset, j.in_bytes, j.img_offset = 0, data.size - k, k * 34 * 68
        j.img = abi.Image(None, 68, 34, 34, 1, 1)
        jobs.append(j)
    plan = gpu.vc5_plan(jobs)
    out = torch.full((2 * 34 * 68,), 0xA5, dtype=torch.uint8, device="cuda")
    plan.run(torch.from_numpy(data).cuda().data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    rc, st, cons = plan.results()
    plan.close()
    assert st == [OK, abi.RSX_ERR_IO] and rc == abi.RSX_ERR_IO
    host = out.cpu().numpy()
    assert np.array_equal(host[:34 * 68].view(np.uint16).reshape(34, 34), V.model_decode(tiles[0], data, bands)[1])
    assert (host[34 * 68:] == 0xA5).all()


def test_host_call_rejections_leave_the_image_alone(gpu):
    t = V.make_tile(1, 32, 48)
    st, out, _, _ = _host(gpu, t)
    assert st == abi.RSX_ERR_UNSUPPORTED and (out.buf == 0xA5).all()
    t = V.make_tile(1, 48, 40)
    data, bands = t.layout()
    d, keep = V.abi_desc(t, bands)
    out = HostImage(48, 40)
    assert gpu.vc5_decompress(d, data[:-1], out.view()) == abi.RSX_ERR_IO and (out.buf == 0xA5).all()


def test_kernel_table_names_the_vc5_kernels(gpu):
    t = V.make_tile(3, 130, 66)
    data, bands = t.layout()
    d, keep = V.abi_desc(t, bands)
    j = abi.Vc5Job()
    j.desc = d
    j.in_offset, j.in_bytes, j.img_offset = 0, data.size, 0
    j.img = abi.Image(None, 260, 130, 66, 1, 1)
    plan = gpu.vc5_plan([j])
    plan.set_timing(True)
    din = torch.from_numpy(data).cuda()
    out = torch.zeros(260 * 66, dtype=torch.uint8, device="cuda")
    for _ in range(3):
        plan.run(din.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    rc, st, _ = plan.results()
    table, runs = plan.kernel_table()
    plan.close()
    assert rc == OK and runs == 3
    assert [n for n, _ in table] == ["vc5_lowpass_kernel", "vc5_band_kernel", "vc5_level_kernel(3)",
                                     "vc5_level_kernel(2)", "vc5_level_kernel(1)", "vc5_merge_kernel"]
