"""Nikon's cousins on the device: PentaxDecompressor (isIntN(value, 16), PentaxDecompressor.cpp:
155-177) and SamsungV1Decompressor (isIntN(value, 12), SamsungV1Decompressor.cpp:123-137) take the
single-pass kernel's nikon-type route (lj_fast_kernel<2, 0, ., false, true>).  Its sums are mod 2^16:
a value with bit 15 set -- a valid Pentax pixel from 32768 on, or a negative sum -- or, for SamsungV1,
one outside 12 bits hands the stream to the legacy route (rsx_ljpeg_recon.hip), which checks the
range and stores the value's low 16 bits.

  value edges     ONE excursion planted in a smooth frame of a few hundred workgroups, at the start
                  of rows 0 and 1, at col 0 / 1 of a later row, mid-row in a late workgroup and at
                  the last pixel; the host call and a plan on each route against the oracle, the
                  oracle against the int64 model (tests/nikon_cases.prefix_model)
  random plans    2-5 frames of unrelated sizes at any input offset, OK frames next to truncated,
                  out-of-range and invalid ones; Hasselblad and Sony ARW1 plans the same way
  bench shapes    the frames bench_ljpeg.py times, whole and truncated in the last workgroup
"""
import os

import numpy as np
import pytest

from rawspeed_amd import abi, synth

import golden_cases as G
import nikon_cases as N
from oracle_lib import HostImage

pytestmark = pytest.mark.gpu

ROUTES = ((), ("RSX_NO_FAST_NK",), ("RSX_NO_FAST_NK", "RSX_NO_FAST_DIFFS"))
# RSX_FUZZ_BASE=<k> moves the random-plan cases to other seeds (soak runs)
BASE = int(os.environ.get("RSX_FUZZ_BASE", "0"))
WG_BYTES = 255 * 64  # stream bytes a workgroup of the single-pass kernel owns (LJ_R)
EDGE_H, EDGE_W = 1280, 2400  # (a multiple of 32: SamsungV1)


@pytest.fixture(scope="module")
def gpu():
    import gpu_util
    return gpu_util.ctx()


def _decode(oracle, gpu, fam, desc, data, img):
    """(oracle status, device status) of one frame, host call."""
    want = HostImage(img.dim_x, img.dim_y)
    if N.PREFIX_FAMILY[fam][1] == 16:
        return oracle.pentax(desc, data, want), gpu.pentax_decompress(desc, data, img.view()), want
    return oracle.samsung_v1(desc, data, want), gpu.samsung_v1_decompress(desc, data, img.view()), want


def _desc(fam):
    code = N.PREFIX_FAMILY[fam][0]
    return N.pentax_desc(code) if N.PREFIX_FAMILY[fam][1] == 16 else abi.SamsungV1Desc.make(code)


def _plan_of(gpu, fam):
    return gpu.pentax_plan if N.PREFIX_FAMILY[fam][1] == 16 else gpu.samsung_v1_plan


def _job(fam, desc, in_off, in_bytes, out_off, w, h, pitch):
    import gpu_util
    j = abi.PentaxJob() if N.PREFIX_FAMILY[fam][1] == 16 else abi.SamsungV1Job()
    j.desc = desc
    j.in_offset, j.in_bytes, j.img_offset = in_off, in_bytes, out_off
    j.img = gpu_util.image_job_view(w, h, 1, pitch)
    return j


class _EdgeStream:
    """A smooth frame's stream, kept as bits: an image that differs from it in a band of rows is
    the same stream with that band's symbols spliced in (a few hundred workgroups, encoded once)."""

    def __init__(self, fam):
        self.code, self.bits, _, maxv = N.PREFIX_FAMILY[fam]
        rng = np.random.default_rng([72, self.bits, maxv])
        self.base = N.smooth15(rng, EDGE_H, EDGE_W, maxv=maxv, sigma=30.0).astype(np.int64)
        self.diff = N.prefix_diffs(self.base, [0, 0, 0, 0])
        val, ln = N.prefix_symbols(self.diff, self.code)
        self.row_bit = np.concatenate([[0], np.cumsum(ln.reshape(EDGE_H, EDGE_W).sum(1))])
        self.stream_bits = N.symbol_bits(val, ln)

    def stream(self, img):
        """(stream, differences) of `img`: the rows that differ from the base and the two below
        them (whose first pair is predicted from them) re-encoded."""
        rows = np.flatnonzero((img != self.base).any(1))
        y0, y1 = int(rows[0]), min(EDGE_H, int(rows[-1]) + 3)
        ys = max(0, y0 - 2)
        band = N.prefix_diffs(img[ys:y1], [0, 0, 0, 0])[y0 - ys:]  # (rows ys, ys + 1: unchanged)
        diff = self.diff.copy()
        diff[y0:y1] = band
        mid = N.symbol_bits(*N.prefix_symbols(band, self.code))
        bits = np.concatenate([self.stream_bits[:self.row_bit[y0]], mid,
                               self.stream_bits[self.row_bit[y1]:], np.zeros(8, np.uint8)])
        return np.concatenate([np.packbits(bits), np.zeros(16, np.uint8)]), diff


@pytest.fixture(scope="module")
def edge_stream():
    made = {}

    def get(fam):
        if fam not in made:
            made[fam] = _EdgeStream(fam)
        return made[fam]
    return get


def _edge_cases():
    out = []
    for fam, (_, bits, _, _) in N.PREFIX_FAMILY.items():
        out += [(fam, v, p) for v, p in N.edge_cases(fam)]
        if bits == 16:
            out += [(fam, 40000, "plateau"), (fam, 65528, "plateau")]  # (+ 7: up to 65535)
    return out


@pytest.mark.parametrize("fam,value,place", _edge_cases(), ids=lambda x: str(x))
def test_prefix_family_value_edges(gpu, oracle, edge_stream, fam, value, place):
    import gpu_util
    E = edge_stream(fam)
    img, at = N.edge_image(fam, E.base, value, place)
    data, diff = E.stream(img)
    assert data.size >= 150 * WG_BYTES
    model, fail = N.prefix_model(diff, E.bits)
    valid = 0 <= value < (1 << E.bits)
    assert fail == (None if valid else at), (fail, at)
    desc = _desc(fam)
    got = HostImage(EDGE_W, EDGE_H)
    so, sg, want = _decode(oracle, gpu, fam, desc, data, got)
    assert so == (0 if valid else abi.RSX_ERR_VALUE_RANGE), so
    assert sg == so, (sg, so)
    if valid:
        assert np.array_equal(want.pixels(), model)
        assert np.array_equal(got.buf, want.buf)
    n = want.buf.size
    job = _job(fam, desc, 0, data.size, 0, EDGE_W, EDGE_H, want.pitch)
    in_host = np.concatenate([data, np.zeros(64, np.uint8)])
    # a value the mod-2^16 sums cannot vouch for: bit 15 set (Pentax), outside 12 bits (SamsungV1)
    inside = bool(img.min() >= 0 and img.max() < min(1 << E.bits, 1 << 15))
    for route in ROUTES:
        status, a, b, names, _ = gpu_util.run_plan(_plan_of(gpu, fam), [job], in_host, n, route)
        assert status == [so], (route, status, so)
        if so == 0:
            assert np.array_equal(a[:n], want.buf) and np.array_equal(b[:n], want.buf), route
        assert (a[n:] == 0xA5).all() and (b[n:] == 0xA5).all(), route
        legacy = bool([x for x in names if "legacy" in x])
        if route == ():
            assert any("nikon-type" in x for x in names), names
            if valid:
                assert legacy == (not inside), (inside, names)
        elif route == ("RSX_NO_FAST_NK",):
            assert any("differences" in x for x in names) and not any("nikon-type" in x for x in names), names
        else:
            assert not any("lj_fast_kernel" in x for x in names), names


# ---- random batched plans ---------------------------------------------------------------

def _kinds(rng, seed):
    """Every fourth seed: OK frames next to each way of failing; the others: 2-5 OK frames."""
    if seed % 4 == 0:
        kinds = ["ok", "trunc", "range", "invalid"] + ["ok"] * int(rng.integers(0, 2))
        return [kinds[i] for i in rng.permutation(len(kinds))]
    return ["ok"] * int(rng.integers(2, 6))


def _prefix_frame(rng, fam, kind):
    """(w, h, stream) of a frame of `kind`."""
    code, bits, _, maxv = N.PREFIX_FAMILY[fam]
    if bits == 16:
        w = 2 * int(rng.integers(1, 1600)) if rng.random() < 0.8 else 2 * int(rng.integers(1, 9))
        h = 1 if rng.random() < 0.15 else int(rng.integers(1, 120))
    else:  # (whole multiples of 32 wide, an even number of rows: no single-row frames)
        w, h = 32 * int(rng.integers(1, 60)), 2 * int(rng.integers(1, 60))
    if kind == "invalid":  # (an odd width, or one that is not a multiple of 32)
        return w + (1 if bits == 16 else 16), h, rng.integers(0, 256, size=256, dtype=np.uint8)
    sigma = float(rng.choice([2.0, 12.0, 60.0]))
    src = N.smooth15(rng, h, w, maxv=maxv, sigma=sigma).astype(np.int64)
    try:
        N.prefix_symbols(N.prefix_diffs(src, [0, 0, 0, 0]), code)
    except ValueError:  # (a difference the code has no length for: a flatter image)
        src = N.smooth15(rng, h, w, maxv=maxv // 2, sigma=2.0).astype(np.int64)
    if kind == "range":  # late: in the last row
        bad = -1 if bits == 16 or rng.random() < 0.5 else 1 << bits
        src = N.plant(src, h - 1, int(rng.integers(0, w)), bad)
    data = N.encode_ints(src, [0, 0, 0, 0], code)
    if kind == "trunc":
        data = data[:int(rng.integers(data.size // 8, data.size // 2 + 1))]
    return w, h, data


def _check_plan(frames, status, outs, names):
    """frames: [(offset, HostImage of the oracle's, oracle status)]; every status the oracle's,
    an OK frame's bytes (its row padding included) the oracle's, and nothing outside the frames'
    rectangles touched."""
    assert status == [so for _, _, so in frames], (status, [so for _, _, so in frames], names)
    for got in outs:
        keep = np.ones(got.size, bool)
        for off, want, so in frames:
            rows = off + want.pitch * np.arange(want.dim_y)[:, None]
            keep[(rows + np.arange(want.dim_x * want.cpp * 2)[None, :]).ravel()] = False
            if so == 0:
                assert np.array_equal(got[off:off + want.buf.size], want.buf), (off, names)
        assert (got[keep] == 0xA5).all(), names


def _assemble(rng, pieces):
    """pieces: [(data, HostImage)] -> (input buffer, [(in_offset, out_offset)], output bytes): streams
    at any byte offset, outputs on the 16-byte grid with gaps."""
    in_off = out_off = 0
    where = []
    for data, want in pieces:
        where.append((in_off, out_off))
        in_off += data.size + int(rng.integers(0, 40))
        out_off += want.buf.size + 16 * int(rng.integers(0, 3))
    in_host = np.zeros(in_off + 64, np.uint8)
    for (data, _), (i, _) in zip(pieces, where):
        in_host[i:i + data.size] = data
    return in_host, where, out_off


@pytest.mark.parametrize("fam", ["pentax_legacy", "pentax_modern", "samsung_v1"])
@pytest.mark.parametrize("seed", range(8))
def test_prefix_family_plans_of_random_frames(gpu, oracle, fam, seed):
    import gpu_util
    rng = np.random.default_rng([73, BASE, seed, N.PREFIX_FAMILY[fam][1], N.PREFIX_FAMILY[fam][2]])
    desc = _desc(fam)
    pieces, sts = [], []
    for kind in _kinds(rng, seed):
        w, h, data = _prefix_frame(rng, fam, kind)
        want = HostImage(w, h)
        so = oracle.pentax(desc, data, want) if N.PREFIX_FAMILY[fam][1] == 16 else \
            oracle.samsung_v1(desc, data, want)
        assert (so == 0) == (kind == "ok"), (kind, so)
        pieces.append((data, want))
        sts.append(so)
    in_host, where, out_bytes = _assemble(rng, pieces)
    jobs = [_job(fam, desc, i, data.size, o, want.dim_x, want.dim_y, want.pitch)
            for (data, want), (i, o) in zip(pieces, where)]
    status, a, b, names, _ = gpu_util.run_plan(_plan_of(gpu, fam), jobs, in_host, out_bytes)
    _check_plan([(o, want, so) for (_, want), (_, o), so in zip(pieces, where, sts)], status, (a, b), names)


@pytest.mark.parametrize("seed", range(8))
def test_hasselblad_plans_of_random_frames(gpu, oracle, seed):
    import gpu_util
    rng = np.random.default_rng([74, BASE, seed])
    kinds = [k for k in _kinds(rng, seed) if k != "range"][:4]  # (no range check: values mod 2^16)
    kinds += ["ok"] * (2 - len(kinds))
    pieces, descs, sts = [], [], []
    for kind in kinds:
        c = G.HASSELBLAD_CASES[int(rng.integers(0, len(G.HASSELBLAD_CASES)))]
        d, data, (w, h, _), _ = G.build_hasselblad(c, seed=818 + int(rng.integers(0, 1000)))
        if kind == "trunc":
            data = data[:int(rng.integers(data.size // 8, data.size // 2 + 1))]
        want = HostImage(w + (1 if kind == "invalid" else 0), h)
        so = oracle.hasselblad(d, data, want)
        assert (so[0] == 0) == (kind == "ok"), (kind, so)
        pieces.append((data, want))
        descs.append(d)
        sts.append(so)
    in_host, where, out_bytes = _assemble(rng, pieces)
    jobs = []
    for (data, want), (i, o), d in zip(pieces, where, descs):
        j = abi.HasselbladJob()
        j.desc = d
        j.in_offset, j.in_bytes, j.img_offset = i, data.size, o
        j.img = gpu_util.image_job_view(want.dim_x, want.dim_y, 1, want.pitch)
        jobs.append(j)
    status, a, b, names, consumed = gpu_util.run_plan(gpu.hasselblad_plan, jobs, in_host, out_bytes)
    _check_plan([(o, want, so[0]) for (_, want), (_, o), so in zip(pieces, where, sts)], status, (a, b), names)
    for k, so in enumerate(sts):
        if so[0] == 0:
            assert consumed[0][k] == consumed[1][k] == so[1], (k, consumed, so)


@pytest.mark.parametrize("seed", range(8))
def test_sony_arw1_plans_of_random_frames(gpu, oracle, seed):
    import gpu_util
    rng = np.random.default_rng([75, BASE, seed])
    kinds = _kinds(rng, seed)[:4]
    ok_cases = [c for c in G.SONY_ARW1_CASES if not (c.get("poison") or c.get("symbols"))]
    bad_cases = [c for c in G.SONY_ARW1_CASES if c.get("poison") or c.get("symbols")]
    pieces, sts = [], []
    for kind in kinds:
        cs = bad_cases if kind == "range" else ok_cases
        c = cs[int(rng.integers(0, len(cs)))]
        data, (w, h, _), _ = G.build_sony_arw1(c, seed=919 + int(rng.integers(0, 1000)))
        if kind == "trunc":
            data = data[:int(rng.integers(data.size // 8, data.size // 2 + 1))]
        want = HostImage(w, h + (1 if kind == "invalid" else 0))
        so = oracle.sony_arw1(data, want)
        assert (so == 0) == (kind == "ok"), (kind, c["name"], so)
        pieces.append((data, want))
        sts.append(so)
    in_host, where, out_bytes = _assemble(rng, pieces)
    jobs = []
    for (data, want), (i, o) in zip(pieces, where):
        j = abi.SonyArw1Job()
        j.in_offset, j.in_bytes, j.img_offset = i, data.size, o
        j.img = gpu_util.image_job_view(want.dim_x, want.dim_y, 1, want.pitch)
        jobs.append(j)
    status, a, b, names, _ = gpu_util.run_plan(gpu.sony_arw1_plan, jobs, in_host, out_bytes)
    _check_plan([(o, want, so) for (_, want), (_, o), so in zip(pieces, where, sts)], status, (a, b), names)


# ---- the shapes bench_ljpeg.py times ------------------------------------------------------

@pytest.fixture(scope="module")
def bench_frames():
    """run_pentax / run_samsung_v1's frames, built once: {fam: (w, h, stream, stream bytes)}."""
    W, H = 7392, 4950
    src = N.smooth15(np.random.default_rng(41), H, W, maxv=16383, sigma=9.0)
    p, _ = N.pentax_encode(src, N.PENTAX_MODERN)
    W1, H1 = 5472, 3648
    src1 = N.smooth15(np.random.default_rng(43), H1, W1, maxv=4095, sigma=6.0)
    s, _ = synth.prefix_encode(src1, [0, 0, 0, 0], synth.SAMSUNG_V1_TAB)
    pad = lambda d: np.concatenate([d, np.zeros(16 + (-len(d)) % 16, np.uint8)])  # noqa: E731
    return {"pentax_modern": (W, H, pad(p), p.size), "samsung_v1": (W1, H1, pad(s), s.size)}


@pytest.mark.parametrize("fam", ["pentax_modern", "samsung_v1"])
def test_prefix_family_bench_shapes(gpu, oracle, bench_frames, fam):
    import gpu_util
    w, h, data, n_real = bench_frames[fam]
    desc = _desc(fam)
    got = HostImage(w, h)
    so, sg, want = _decode(oracle, gpu, fam, desc, data, got)
    assert so == sg == 0
    assert np.array_equal(got.buf, want.buf)
    # a 2-frame plan: the second stream at an offset off the 16-byte grid
    n = want.buf.size
    off = data.size + 3
    in_host = np.zeros(off + data.size + 64, np.uint8)
    in_host[:data.size] = in_host[off:off + data.size] = data
    jobs = [_job(fam, desc, 0, data.size, 0, w, h, want.pitch),
            _job(fam, desc, off, data.size, n, w, h, want.pitch)]
    status, a, b, names, _ = gpu_util.run_plan(_plan_of(gpu, fam), jobs, in_host, 2 * n)
    assert status == [0, 0], (status, names)
    for out in (a, b):
        assert np.array_equal(out[:n], want.buf) and np.array_equal(out[n:2 * n], want.buf)
    assert any("nikon-type" in x for x in names) and not [x for x in names if "legacy" in x], names


@pytest.mark.parametrize("fam", ["pentax_modern", "samsung_v1"])
def test_prefix_family_bench_shapes_truncated(gpu, oracle, bench_frames, fam):
    """Cuts in the last workgroup's bytes, and one at a third: the status is the oracle's at every
    cut (and so are the pixels where both decode)."""
    w, h, data, n_real = bench_frames[fam]
    desc = _desc(fam)
    seen = set()
    for cut in list(range(n_real - 24, n_real)) + [n_real // 3]:
        got = HostImage(w, h)
        so, sg, want = _decode(oracle, gpu, fam, desc, data[:cut], got)
        assert sg == so, (cut, sg, so)
        if so == 0:
            assert np.array_equal(got.buf, want.buf), cut
        seen.add(so)
    assert len(seen - {0}) >= 1, seen
