"""Device plans at the edges of their layout: more than 65535 Huffman tables in one plan, and
jobs whose input or output lies past 2^31 and 2^32 bytes of the plan's buffers.

  tables      The single-pass LJPEG kernel keeps 16 bits of a stream's table base in a
              workgroup's table word (lf_table_word, rsx_ljpeg_dev.h).  A plan of tiny filler
              jobs that all use table A brings the plan's table count to just below 65535, then
              probes of every single-pass route follow at table bases around 65535 -- each probe
              with tables of its own that decode A's bit patterns differently.  An LJPEG plan
              (one table, two alternating, a table per component over 3 and 4 components, three
              components with one table, restart intervals) and a Pentax plan (the Nikon-type
              route, and again under RSX_NO_FAST_NK: the differences route).
  offsets     For every plan type, one small job placed at offset 0, straddling 2^31,
              straddling 2^32 and wholly above 2^32 -- of the input and, separately, of the
              output -- and one job whose own rows cross 4 GiB (a pitch of 1 MiB + 16, 4100
              rows).  Every copy against the oracle (Phase One / ARW2 / Olympus: the source
              image / the numpy model / the host build) in status, consumed bytes and pixels; every byte of the output buffer
              a job does not own is still 0xA5.

The two 6.6 GB buffers are allocated once for the module, and a plan is given a base 2 GiB into
each: a job address truncated to 32 bits, or sign-extended from 32 bits, still lands inside the
allocation and shows as a mismatch, not as a memory fault.  Peak device memory about 13.2 GB
(the two buffers; the table plans, about 1 GB, are made and freed before them); the module runs
in about 10 s on one MI355X."""
import numpy as np
import pytest
import torch

import arw2_files as A
import cases as C
import golden_cases as G
import iiq_files as I
import nikon_cases as N
import olympus_files as O
import samsung_v2_cases as V2
from oracle_lib import HostImage
from rawspeed_amd import abi, synth

pytestmark = pytest.mark.gpu

G31, G32 = 1 << 31, 1 << 32
BASE = G31                              # the plan's buffers start this far into the allocations
EXTENT = G32 + (1 << 27)                # bytes behind BASE: the tall image (4.3 GB) and the copies above 2^32
ABOVE = G32 + (64 << 20) + 48           # "wholly above 2^32" (its 32-bit image: 64 MiB, nobody's)
SLOTS = 1 << 29                         # where a copy's other side goes (well away from every image of a wrap)
TALL_PITCH = (1 << 20) + 16
TALL_ROWS = 4100
SHORT_ROWS, SHORT_PITCH = 3072, 1400016  # (SamsungV1 and Sony ARW1 allow fewer rows: a wider pitch)
PAT = int.from_bytes(b"\xa5" * 8, "little", signed=True)


@pytest.fixture(scope="module")
def gpu():
    import gpu_util
    return gpu_util.ctx()


def _al(x):
    return x // 16 * 16


def _view(w, pitch):
    import gpu_util
    return gpu_util.image_job_view(w.dim_x, w.dim_y, w.cpp, pitch, is_cfa=w.is_cfa)


# ---- A. more than 65535 tables ---------------------------------------------------------------

def _lut(tree, bits=11):
    """(code length, value) of every `bits`-bit pattern a canonical table decodes (0: none)"""
    counts, values = tree
    lut = np.zeros(1 << bits, np.int32)
    code = k = 0
    for ln in range(1, 17):
        for _ in range(counts[ln - 1]):
            if ln <= bits:
                lo = code << (bits - ln)
                lut[lo:lo + (1 << (bits - ln))] = (ln << 8) | (int(values[k]) + 1)
            code += 1
            k += 1
        code <<= 1
    return lut


def _unlike(tree, a):
    """the share of bit patterns `tree` decodes differently from table `a`"""
    return float(np.mean(_lut(tree) != _lut(a)))


def _run_table_plan(make_plan, jobs, in_host, out_bytes, route=()):
    import gpu_util
    status, a, b, names, consumed = gpu_util.run_plan(make_plan, jobs, in_host, out_bytes, route)
    assert (a[out_bytes:] == 0xA5).all() and (b[out_bytes:] == 0xA5).all()
    return status, (a, b), names, consumed


def _check_table_plan(fill, probes, status, outs, consumed, names):
    """fill: (n, status, consumed, image bytes); probes: dicts with kind, base, so (status,
    consumed), want, out_off.  A consumed count of None (Pentax: the oracle has none) is checked
    against the run's first filler / the other run."""
    n, fst, fcons, fbuf = fill
    bad = []
    assert consumed[0] == consumed[1]
    for out, cons in zip(outs, consumed):
        sz = fbuf.size
        assert status[:n] == [fst] * n
        assert cons[:n] == [cons[0] if fcons is None else fcons] * n
        rows_ok = (out[:n * sz].reshape(n, sz) == fbuf).all(axis=1)
        assert rows_ok.all(), "filler jobs %s wrong" % np.flatnonzero(~rows_ok)[:8]
        for k, p in enumerate(probes):
            st, c = status[n + k], cons[n + k]
            px = np.array_equal(out[p["out_off"]:p["out_off"] + p["want"].buf.size], p["want"].buf)
            want_c = c if p["so"][1] is None else p["so"][1]
            if (st, c) != (p["so"][0], want_c) or not px:
                bad.append((p["kind"], p["base"], "status %d (want %d)" % (st, p["so"][0]),
                            "consumed %d (want %d)" % (c, want_c), "pixels ok" if px else "pixels wrong"))
    assert not bad, "probes that failed: %s\nkernels: %s" % (bad, names)


LJ_PROBES = ("1c", "2c2t", "4c4t", "fast3", "fast3", "fast3", "3c3t", "1c", "2c2t", "fast3",
             "4c4t", "dri", "3c3t")
LJ_SHAPE = {"1c": ((1, 1), [0]), "2c2t": ((2, 1), [0, 1]), "3c3t": ((3, 1), [0, 1, 2]),
            "4c4t": ((4, 1), [0, 1, 2, 3]), "fast3": ((3, 1), [0, 0, 0]), "dri": ((2, 1), [0, 0])}
LJ_FIRST_BASE = 65527  # (fast3 probes at 65534, 65535, 65536, 65543)


def test_ljpeg_plan_past_65535_tables(gpu, oracle):
    """Filler streams (table A) up to table 65527, then a probe of every single-pass LJPEG route
    at table bases 65527 .. 65550: status, consumed bytes and pixels of every job."""
    rng = np.random.default_rng(0x7AB1)
    tab_a = C.NIKON
    fd, fdata, _, _ = C.make_ljpeg_case(rng, img_w=8, img_h=2, cpp=1, tile=(0, 0, 8, 2), mcu=(1, 1))
    fwant = HostImage(8, 2)
    fso = oracle.ljpeg(fd, fdata, fwant)
    assert fso[0] == 0
    n_fill = LJ_FIRST_BASE
    W, H = 192, 32
    probes, in_parts = [], [fdata, np.zeros(_al(fdata.size + 64) - fdata.size, np.uint8)]
    in_off, out_off, base = _al(fdata.size + 64), n_fill * fwant.buf.size, n_fill
    for kind in LJ_PROBES:
        mcu, idx = LJ_SHAPE[kind]
        tabs = tuple(C.random_huffman_table(rng) for _ in range(max(idx) + 1))
        for t in tabs:
            assert _unlike(t, tab_a) > 0.5, "a probe table too close to the fillers' table"
        d, data, _, _ = C.make_ljpeg_case(rng, img_w=W, img_h=H, cpp=1, tile=(0, 0, W, H), mcu=mcu,
                                          tables=tabs, table_index=idx,
                                          rows_per_ri=8 if kind == "dri" else 0)
        want = HostImage(W, H)
        so = oracle.ljpeg(d, data, want)
        assert so[0] == 0, (kind, so)
        # (a job with restart intervals runs as a child plan: its tables are not this plan's)
        probes.append(dict(kind=kind, base=None if kind == "dri" else base, d=d, data=data,
                           want=want, so=so, in_off=in_off, out_off=out_off))
        base += 0 if kind == "dri" else len(tabs)
        pad = _al(data.size + 64) - data.size
        in_parts += [data, np.zeros(pad, np.uint8)]
        in_off += data.size + pad
        out_off += want.buf.size
    assert [p["base"] for p in probes if p["kind"] == "fast3"] == [65534, 65535, 65536, 65543]
    jobs = []
    for i in range(n_fill):
        j = abi.LJpegJob()
        j.desc = fd
        j.in_offset, j.in_bytes, j.img_offset = 0, fdata.size, i * fwant.buf.size
        j.img = _view(fwant, fwant.pitch)
        jobs.append(j)
    for p in probes:
        j = abi.LJpegJob()
        j.desc = p["d"]
        j.in_offset, j.in_bytes, j.img_offset = p["in_off"], p["data"].size, p["out_off"]
        j.img = _view(p["want"], p["want"].pitch)
        jobs.append(j)
    status, outs, names, consumed = _run_table_plan(gpu.ljpeg_plan, jobs, np.concatenate(in_parts),
                                                    out_off)
    print("ljpeg table plan kernels:", names)
    _check_table_plan((n_fill, fso[0], fso[1], fwant.buf), probes, status, outs, consumed, names)


PX_FIRST_BASE = 65532


@pytest.mark.parametrize("route", [(), ("RSX_NO_FAST_NK",)], ids=["nikon_type", "no_fast_nk"])
def test_pentax_plan_past_65535_tables(gpu, oracle, route):
    """Pentax fillers (the legacy tree) up to table 65532, then nine Pentax probes with trees of
    their own at table bases 65532 .. 65540."""
    rng = np.random.default_rng(0x7AB2)
    tree_a = synth.PENTAX_TREE
    src = N.smooth15(rng, 2, 8, maxv=4095, sigma=6.0)
    fdata = np.concatenate([N.pentax_encode(src, tree_a)[0], np.zeros(8, np.uint8)])
    fd = N.pentax_desc(tree_a)
    fwant = HostImage(8, 2)
    fst = oracle.pentax(fd, fdata, fwant)
    assert fst == 0
    n_fill = PX_FIRST_BASE
    W, H = 128, 16
    probes, in_parts = [], [fdata, np.zeros(_al(fdata.size + 64) - fdata.size, np.uint8)]
    in_off, out_off = _al(fdata.size + 64), n_fill * fwant.buf.size
    for k in range(9):
        tree = C.random_huffman_table(rng, n_cat=13)
        assert _unlike(tree, tree_a) > 0.5, "a probe tree too close to the fillers' tree"
        img = N.smooth15(rng, H, W, maxv=4095, sigma=6.0)
        data = np.concatenate([N.pentax_encode(img, tree)[0], np.zeros(8, np.uint8)])
        d = N.pentax_desc(tree)
        want = HostImage(W, H)
        so = oracle.pentax(d, data, want)
        assert so == 0 and np.array_equal(want.pixels(), img)
        probes.append(dict(kind="pentax", base=n_fill + k, d=d, data=data, want=want, so=(so, None),
                           in_off=in_off, out_off=out_off))
        pad = _al(data.size + 64) - data.size
        in_parts += [data, np.zeros(pad, np.uint8)]
        in_off += data.size + pad
        out_off += want.buf.size
    jobs = []
    for i in range(n_fill):
        j = abi.PentaxJob()
        j.desc = fd
        j.in_offset, j.in_bytes, j.img_offset = 0, fdata.size, i * fwant.buf.size
        j.img = _view(fwant, fwant.pitch)
        jobs.append(j)
    for p in probes:
        j = abi.PentaxJob()
        j.desc = p["d"]
        j.in_offset, j.in_bytes, j.img_offset = p["in_off"], p["data"].size, p["out_off"]
        j.img = _view(p["want"], p["want"].pitch)
        jobs.append(j)
    status, outs, names, consumed = _run_table_plan(gpu.pentax_plan, jobs, np.concatenate(in_parts),
                                                    out_off, route)
    print("pentax table plan kernels (%s):" % (route,), names)
    _check_table_plan((n_fill, fst, None, fwant.buf), probes, status, outs, consumed, names)


# ---- B. jobs past 2^31 and 2^32 --------------------------------------------------------------

class Case:
    """One small job of a plan type: its input block and what the oracle (or the source image)
    says it decodes to, in a compact 0xA5-filled image."""

    def __init__(self, plan, cls, desc, data, want, status, consumed=None, bpc=2, in_bytes=None,
                 extra=None, in_view=None):
        self.plan, self.cls, self.desc = plan, cls, desc
        self.data = np.array(data, np.uint8).reshape(-1)
        self.want, self.status, self.consumed = want, status, consumed
        self.row_bytes = want.dim_x * want.cpp * bpc
        self.in_bytes = self.data.size if in_bytes is None else in_bytes
        self.extra = extra or {}
        self.in_view = in_view  # (sRaw interpolation: the input is an image)

    def job(self, in_off, img_off, pitch):
        j = self.cls()
        if self.desc is not None:
            j.desc = self.desc
        for k, v in self.extra.items():
            setattr(j, k, v)
        j.in_offset, j.img_offset = in_off, img_off
        if self.in_view is None:
            j.in_bytes = self.in_bytes
        else:
            j.in_ = self.in_view
        j.img = _view(self.want, pitch)
        return j

    def rows(self):
        w = self.want
        return w.buf.reshape(w.dim_y, w.pitch)[:, :self.row_bytes]


def _unpack(oracle, tall):
    rng = np.random.default_rng([0xB01, tall])
    w, h, oy, bps = (64, TALL_ROWS - 2000, 2000, 14) if tall else (200, 12, 1, 12)
    pitch = w * bps // 8 + 3
    data = rng.integers(0, 256, size=h * pitch, dtype=np.uint8)
    d = abi.UnpackDesc(0, oy, w, h, pitch, bps, abi.ORDER_MSB)
    want = HostImage(w, h + oy)
    return Case("unpack_plan", abi.UnpackJob, d, data, want, oracle.unpack(d, data, want))


def _unpack_f32(oracle, tall):
    rng = np.random.default_rng([0xB02, tall])
    w, h, oy, cpp = (16, TALL_ROWS - 2000, 2000, 1) if tall else (40, 6, 1, 2)
    pitch = w * cpp * 3 + 1
    data = rng.integers(0, 256, size=h * pitch, dtype=np.uint8)
    d = abi.UnpackDesc(1, oy, w, h, pitch, 24, 0)
    want = HostImage(w + 2, h + oy, cpp, bpc=4)
    return Case("unpack_f32_plan", abi.UnpackJob, d, data, want, oracle.unpack_f32(d, data, want),
                bpc=4)


def _unpack_variant(oracle, tall):
    rng = np.random.default_rng([0xB03, tall])
    w, h = 40, TALL_ROWS if tall else 5
    data = rng.integers(0, 256, size=G.variant_bpl(1, w) * h, dtype=np.uint8)
    d = abi.UnpackVariantDesc(1, 1, w, h)
    want = HostImage(w, h)
    return Case("unpack_variant_plan", abi.UnpackVariantJob, d, data, want,
                oracle.unpack_variant(d, data, want))


def _ljpeg(n):
    def make(oracle, tall):
        rng = np.random.default_rng([0xB04, n, tall])
        W, H = 96, TALL_ROWS if tall else 16
        tile = (0, 2000, W, H - 2000) if tall else (0, 0, W, H)
        d, data, _, _ = C.make_ljpeg_case(rng, img_w=W, img_h=H, cpp=1, tile=tile, mcu=(n, 1))
        want = HostImage(W, H)
        st, cons = oracle.ljpeg(d, data, want)
        return Case("ljpeg_plan", abi.LJpegJob, d, data, want, st, cons)
    return make


def _cr2(oracle, tall):
    rng = np.random.default_rng([0xB05, tall])
    H = TALL_ROWS if tall else 16
    d, data, _, _ = C.make_cr2_case(rng, 96, H, 2, (2, 48, 48))
    want = HostImage(96, H)
    st, cons = oracle.cr2(d, data, want)
    return Case("cr2_plan", abi.Cr2Job, d, data, want, st, cons)


def _cr2_sraw(oracle, tall):
    rng = np.random.default_rng([0xB06, tall])
    H = TALL_ROWS if tall else 12
    d, data, img, _ = C.make_cr2_sraw_case(rng, 1, (2, 8, 8), H)
    want = HostImage(img.shape[1], H, 1, is_cfa=False)
    st, cons = oracle.cr2(d, data, want)
    return Case("cr2_plan", abi.Cr2Job, d, data, want, st, cons)


def _sraw(oracle, tall):
    import gpu_util
    rng = np.random.default_rng([0xB07, tall])
    groups, rows = 16, TALL_ROWS if tall else 9
    w = groups * 4
    src = HostImage(w, rows, 1, is_cfa=False)
    g = src.pixels().reshape(rows, groups, 4)
    g[:, :, :2] = rng.integers(200, 15000, size=(rows, groups, 2))
    g[:, :, 2:] = rng.integers(16384 - 3000, 16384 + 3000, size=(rows, groups, 2))
    d = abi.SrawDesc.make(1, 1, [int(x) for x in rng.integers(800, 2600, size=3)], 123)
    want = HostImage(2 * groups, rows, 3, is_cfa=False)
    st = oracle.sraw(d, src, want)
    return Case("sraw_plan", abi.SrawJob, d, src.buf, want, st,
                in_view=gpu_util.image_job_view(w, rows, 1, src.pitch, is_cfa=False))


def _nikon(split):
    def make(oracle, tall):
        h = TALL_ROWS if tall else 16
        if split:
            c = dict(name="lossy12_split", v0=68, v1=32, bits=12, w=40, h=h, split=h // 2,
                     kind="symbols", unc=0)
        else:
            c = dict(name="lossless14_dither", v0=70, v1=0, bits=14, w=64, h=h, kind="image", unc=0)
        _, d, data, (w, h, _), _ = G.build_nikon(c, seed=0xB08 + tall)
        want = HostImage(w, h)
        return Case("nikon_plan", abi.NikonJob, d, data, want, oracle.nikon(d, data, want))
    return make


def _pentax(oracle, tall):
    c = dict(name="legacy_small", tree="legacy", w=64, h=TALL_ROWS if tall else 20, maxv=4095)
    _, d, data, (w, h, _), _ = G.build_pentax(c, seed=0xB09 + tall)
    want = HostImage(w, h)
    return Case("pentax_plan", abi.PentaxJob, d, data, want, oracle.pentax(d, data, want))


def _samsung_v1(oracle, tall):
    d, data, (w, h, _), _ = G.build_samsung_v1(dict(name="small", w=64, h=SHORT_ROWS if tall else 20),
                                               seed=0xB0A + tall)
    want = HostImage(w, h)
    return Case("samsung_v1_plan", abi.SamsungV1Job, d, data, want, oracle.samsung_v1(d, data, want))


def _samsung_v2(oracle, tall):
    rng = np.random.default_rng([0xB0B, tall])
    w, h, bits = 64, TALL_ROWS if tall else 20, 14
    x, y = np.arange(w)[None, :], np.arange(h)[:, None]
    target = np.clip(4000 + 9 * x + (2 if tall else 20) * y + rng.normal(0, 40, (h, w)), 0,
                     (1 << bits) - 1)
    data, _ = V2.encode(rng, target.astype(np.int64), bits, 0)
    want = HostImage(w, h)
    st = oracle.samsung_v2(bits, data, want)
    d, _ = abi.SamsungV2Desc.from_header(data[:16])
    payload = data[16:]
    return Case("samsung_v2_plan", abi.SamsungV2Job, d, payload, want, st)


def _hasselblad(oracle, tall):
    c = dict(name="small", w=64, h=TALL_ROWS if tall else 20)
    d, data, (w, h, _), _ = G.build_hasselblad(c, seed=0xB0C + tall)
    want = HostImage(w, h)
    st, cons = oracle.hasselblad(d, data, want)
    return Case("hasselblad_plan", abi.HasselbladJob, d, data, want, st, cons)


def _sony_arw1(oracle, tall):
    c = dict(name="small", w=37, h=SHORT_ROWS if tall else 20, sigma=5.0)
    data, (w, h, _), _ = G.build_sony_arw1(c, seed=0xB0D + tall)
    want = HostImage(w, h)
    return Case("sony_arw1_plan", abi.SonyArw1Job, None, data, want, oracle.sony_arw1(data, want))


def _phase_one(oracle, tall):
    w, h = 66, TALL_ROWS if tall else 6
    rng = np.random.default_rng([0xB0E, tall])
    img = I.sample_image(rng, w, h)
    blob = I.iiq_file(I.encode(img, 3), w, rng, gap_max=5)
    raw, strips, _, _ = I.iiq_strips(blob)
    arr = abi.phase_one_strips(strips)
    want = HostImage(w, h)
    want.pixels()[:] = img
    return Case("phase_one_plan", abi.PhaseOneJob, None, np.frombuffer(raw, np.uint8), want, 0,
                extra=dict(strips=arr, n_strips=len(strips)))


def _sony_arw2(oracle, tall):
    w, h = 64, TALL_ROWS if tall else 6
    rng = np.random.default_rng([0xB0F, tall])
    data = A.random_stream(rng, w, h)
    table = A.table_dither(A.decode_curve(A.REALISTIC_CURVE))
    d, arr = abi.sony_arw2_desc(A.DITHER, table)
    mst, img, _ = A.model_decode(data, w, h, A.DITHER, table)
    want = HostImage(w, h)
    want.pixels()[:] = img
    c = Case("sony_arw2_plan", abi.SonyArw2Job, d, data, want, mst, w * h)
    c.keep = arr
    return c


def _olympus(oracle, tall):
    # (130 wide: three batches of the walk a row, two tiles of the reconstruction; the tall image
    # has 33 bands; the expected image is the host build's)
    w, h = 130, TALL_ROWS if tall else 6
    data = synth.olympus_encode(O.content("noise12", w, h, 0xB10 + tall))
    st, px = O.host_decode(data, w, h)
    want = HostImage(w, h)
    want.pixels()[:] = px
    return Case("olympus_plan", abi.OlympusJob, None, np.frombuffer(data, np.uint8), want, st)


KINDS = {
    "unpack_u16": _unpack, "unpack_f32": _unpack_f32, "unpack_variant": _unpack_variant,
    "ljpeg_1c": _ljpeg(1), "ljpeg_2c": _ljpeg(2), "ljpeg_3c": _ljpeg(3), "ljpeg_4c": _ljpeg(4),
    "cr2": _cr2, "cr2_sraw": _cr2_sraw, "sraw_interpolate": _sraw,
    "nikon_split": _nikon(True), "nikon_curve": _nikon(False), "pentax": _pentax,
    "samsung_v1": _samsung_v1, "samsung_v2": _samsung_v2, "hasselblad": _hasselblad,
    "sony_arw1": _sony_arw1, "phase_one": _phase_one, "sony_arw2": _sony_arw2,
    "olympus": _olympus,
}


@pytest.fixture(scope="module")
def bufs():
    """(input, output): BASE + EXTENT bytes each, allocated once"""
    inp = torch.empty(BASE + EXTENT, dtype=torch.uint8, device="cuda")
    out = torch.empty(BASE + EXTENT, dtype=torch.uint8, device="cuda")
    yield inp, out
    del inp, out
    torch.cuda.empty_cache()


def _rect(buf, off, h, row_bytes, pitch):
    assert 0 <= off and off + (h - 1) * pitch + row_bytes <= EXTENT
    return torch.as_strided(buf, (h, row_bytes), (pitch, 1), BASE + off)


def _first_dirty(out):
    """offset (from BASE) of the first 8-byte word of the output allocation that is not 0xA5"""
    words = out.view(torch.int64)
    step = 1 << 27
    for s in range(0, words.numel(), step):
        bad = words[s:s + step] != PAT
        if bool(bad.any()):
            return (int(torch.nonzero(bad)[0, 0]) + s) * 8 - BASE
    return None


def _places_in(n):
    return [0, _al(G31 - n // 2), _al(G32 - n // 2), ABOVE]


def _places_out(h, row_bytes, pitch):
    # (the boundary falls in the middle of a row of pixels)
    mid = (h // 2) * pitch + row_bytes // 2
    return [0, _al(G31 - mid), _al(G32 - mid), ABOVE]


def _run_placed(gpu, bufs, case, placed, pitch):
    """placed: [(input offset, image offset)] of copies of `case`; returns per copy (status,
    consumed, image rows), with the output buffer checked for bytes no copy owns"""
    inp, out = bufs
    inp.fill_(0x5A)
    out.fill_(0xA5)
    src = torch.from_numpy(case.data).cuda()
    for io, _ in placed:
        assert io % 16 == 0 and io + case.data.size <= EXTENT
        inp[BASE + io:BASE + io + case.data.size].copy_(src)
    h, rb = case.want.dim_y, case.row_bytes
    jobs = [case.job(io, oo, pitch) for io, oo in placed]
    plan = getattr(gpu, case.plan)(jobs)
    res = []
    try:
        for run in range(2):
            if run:
                out.fill_(0xA5)
            plan.run(inp.data_ptr() + BASE, out.data_ptr() + BASE)
            rc, status, consumed = plan.results()
            rows = [_rect(out, oo, h, rb, pitch).contiguous().cpu().numpy() for _, oo in placed]
            for _, oo in placed:
                _rect(out, oo, h, rb, pitch).fill_(0xA5)
            dirty = _first_dirty(out)
            assert dirty is None, "run %d wrote at offset %#x, outside every job's image" % (run, dirty)
            res.append(list(zip(status, consumed, rows)))
    finally:
        plan.close()
    return res


def _check_copies(case, res, what):
    want = case.rows()
    for run, copies in enumerate(res):
        st0, c0, px0 = copies[0]
        assert st0 == case.status == 0
        if case.consumed is not None:
            assert c0 == case.consumed, (run, c0, case.consumed)
        assert np.array_equal(px0, want), "run %d: the offset-0 copy differs from the oracle" % run
        for k, (st, c, px) in enumerate(copies):
            assert (st, c) == (st0, c0), (run, what[k], st, c, st0, c0)
            assert np.array_equal(px, px0), "run %d: %s differs from the offset-0 copy" % (run, what[k])


@pytest.mark.parametrize("kind", list(KINDS))
def test_copies_past_2g_and_4g(gpu, oracle, bufs, kind):
    """The same job at input offsets 0, across 2^31, across 2^32 and above 2^32 (image in a slot
    of its own), and at those image offsets (input in a slot): every copy the same."""
    case = KINDS[kind](oracle, False)
    assert case.status == 0
    pitch = (case.row_bytes + 16 + 15) // 16 * 16  # (padding behind every row: nobody's)
    h = case.want.dim_y
    span_in, span_out = _al(case.data.size + 4096 + 15), _al(h * pitch + 4096 + 15)
    ins, outs = _places_in(case.data.size), _places_out(h, case.row_bytes, pitch)
    placed = [(io, SLOTS + k * span_out) for k, io in enumerate(ins)]
    placed += [(SLOTS + k * span_in, oo) for k, oo in enumerate(outs)]
    what = ["input at %#x" % io for io in ins] + ["image at %#x" % oo for oo in outs]
    _check_copies(case, _run_placed(gpu, bufs, case, placed, pitch), what)


@pytest.mark.parametrize("kind", list(KINDS))
def test_image_whose_rows_cross_4g(gpu, oracle, bufs, kind):
    """One job, pitch 1 MiB + 16, 4100 rows (3072 rows of 1.34 MB where the decoder allows no
    more): its last rows lie past 2^32 of the output.  Against the oracle and against the same
    image at a compact pitch."""
    case = KINDS[kind](oracle, True)
    h = case.want.dim_y
    pitch = TALL_PITCH if h >= TALL_ROWS else SHORT_PITCH
    assert case.status == 0 and (h - 1) * pitch > G32
    compact = (case.row_bytes + 15) // 16 * 16
    res = _run_placed(gpu, bufs, case, [(SLOTS, 0)], pitch)
    small = _run_placed(gpu, bufs, case, [(SLOTS, 0)], compact)
    want = case.rows()
    for run, copies in enumerate(res):
        st, c, px = copies[0]
        assert st == 0 == small[run][0][0]
        assert c == small[run][0][1]
        if case.consumed is not None:
            assert c == case.consumed
        bad = np.flatnonzero((px != want).any(axis=1))
        assert bad.size == 0, "run %d: rows %s differ from the oracle" % (run, bad[:10])
        assert np.array_equal(small[run][0][2], want)
