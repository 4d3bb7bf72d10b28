"""Device plans at the edges of their layout: more than 65535 Huffman tables in one plan, jobs
whose input or output lies past 2^31 and 2^32 bytes of the plan's buffers, and plans of exactly
65535 jobs, the largest grid axis.

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
              rows; where a decoder allows fewer rows, a pitch that puts the last row past
              2^32).  Every copy against the oracle in status, consumed bytes and pixels; every
              byte of the output buffer a job does not own is still 0xA5.  The oracle is the
              CPU oracle for the plan types it knows, and otherwise
                the source image            Phase One
                the numpy / Python model    ARW2, Panasonic V5 / V6 / V4 (with V4's list of zero
                  of tests/*_files.py       pixels), Samsung V0, sNEF, VC5, deflate and lossy-JPEG
                                            tiles, Kodak, CRW, the IIQ corrections, the DNG
                                            opcode stage, black / white scaling, bad pixels
                the decoder's host build    Olympus, Fuji (and the pixels its writer reached)
              A job's offsets that follow its input (CRW's low bits, the lossy-JPEG tiles'
              table) are set anew for every placement; the offsets inside a descriptor (Fuji's
              strips, VC5's bands, Samsung V0's rows) count from the job's input and stay.  The
              stages that work in place get their source image written into every rectangle
              before a run; those that read no input have the four image placements alone.
  jobs        Kodak, CRW, scale, DNG post, bad pixels and IIQ corrections put the job on a grid
              axis.  A plan of exactly 65535 of the smallest job runs, every image against the
              oracle and every gap still 0xA5; 65536 valid jobs are refused when the plan is
              made; a job Kodak or CRW refuse takes no row of the grid, so 65535 valid jobs and
              one refused one are a plan.  A lossy-JPEG job of 65536 tiles is refused.

The two 6.6 GB buffers are allocated once for the module, and a plan is given a base 2 GiB into
each: a job address truncated to 32 bits, or sign-extended from 32 bits, still lands inside the
allocation and shows as a mismatch, not as a memory fault.  Peak device memory about 13.2 GB
(the two buffers; the table plans, about 1 GB, are made and freed before them; the 65535-job
plans work on buffers of 10 MB at the most); the module runs in about 12 s on one MI355X."""
import ctypes
import random

import numpy as np
import pytest
import torch

import arw2_files as A
import bad_pixels_files as BP
import cases as C
import crw_files as CW
import dng_deflate_files as DD
import dng_jpeg_files as DJ
import dng_post_files as DP
import fuji_files as FJ
import golden_cases as G
import iiq_corr_files as IC
import iiq_files as I
import kodak_files as KD
import nikon_cases as N
import olympus_files as O
import rw2_files as P
import rw2_v4_files as P4
import samsung_v2_cases as V2
import scale_files as SC
import snef_files as SN
import srw_v0_files as S0
import vc5_files as VC
from oracle_lib import HostImage
from rawspeed_amd import abi, capi, synth

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
    says it decodes to, in a compact 0xA5-filled image.

      in_mid    the byte of the input block that goes on the 2^31 / 2^32 line (default: its middle)
      place     place(job, input offset): sets the job's fields that follow the block's placement
                (an offset of a second blob, a table of offsets); their arrays stay with the job
      source    (rows, row bytes) uint8: a plan that works in place gets this image written into
                its rectangle of the output buffer before every run
      no_input  the job reads nothing from the input buffer: it has no input placements
      per_job   per_job(plan, k) -> what job k reports beyond status and consumed bytes, as a
                tuple that compares with ==; per_job_want: what the oracle says it is
      tall_pitch  the pitch at which this image's rows cross 4 GiB, where its height is its own"""

    def __init__(self, plan, cls, desc, data, want, status, consumed=None, bpc=2, in_bytes=None,
                 extra=None, in_view=None, in_mid=None, place=None, source=None, no_input=False,
                 per_job=None, per_job_want=None, tall_pitch=None):
        self.plan, self.cls, self.desc = plan, cls, desc
        self.data = np.array(data, np.uint8).reshape(-1)
        self.want, self.status, self.consumed = want, status, consumed
        self.row_bytes = want.dim_x * want.cpp * bpc
        self.in_bytes = self.data.size if in_bytes is None else in_bytes
        self.extra = extra or {}
        self.in_view = in_view  # (sRaw interpolation: the input is an image)
        self.in_mid = self.data.size // 2 if in_mid is None else in_mid
        self.place, self.no_input = place, no_input
        self.source = None if source is None else np.ascontiguousarray(source, np.uint8)
        assert self.source is None or self.source.shape == (want.dim_y, self.row_bytes)
        self.per_job, self.per_job_want = per_job, per_job_want
        self.tall_pitch = tall_pitch

    def job(self, in_off, img_off, pitch):
        j = self.cls()
        fields = {f[0] for f in self.cls._fields_}
        if self.desc is not None:
            j.desc = self.desc
        for k, v in self.extra.items():
            assert k in fields, k
            setattr(j, k, v)
        j.img_offset = img_off
        if "in_offset" in fields:
            j.in_offset = in_off
        if self.in_view is not None:
            j.in_ = self.in_view
        elif "in_bytes" in fields:
            j.in_bytes = self.in_bytes
        if self.place is not None:
            self.place(j, in_off)
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


def _panasonic(version, bps, small, tall_w, zero_half=False):
    # (V5/12, 700 x 17: 1190 packets -- packet 512 wraps around its block's end, and a second,
    # partial block; the expected image is the numpy model's)
    def make(oracle, tall):
        w, h = (tall_w, TALL_ROWS) if tall else small
        rng = np.random.default_rng([0xB11, version, bps, tall])
        data = P.random_stream(rng, version, bps, w, h, zero_half)
        want = HostImage(w, h)
        want.pixels()[:] = P.model_decode(version, bps, w, h, data)
        return Case("panasonic_plan", abi.PanasonicJob, abi.PanasonicDesc(version, bps), data, want,
                    0, P.consumed(version, bps, w, h))
    return make


def _panasonic_v4(oracle, tall):
    # (split 0x1FF8, zero_is_bad; half the bytes zero, so there are zero pixels to list; the list
    # of every copy must be the model's)
    w, h = (28, TALL_ROWS) if tall else (980, 17)
    rng = np.random.default_rng([0xB12, tall])
    data = P4.random_stream(rng, P4.SPLIT, w, h, "half")
    img, zeros = P4.model_decode(P4.SPLIT, w, h, data)
    zeros = np.asarray(zeros, np.uint32)
    cap = int(zeros.size)
    assert cap > 0
    want = HostImage(w, h)
    want.pixels()[:] = img

    def report(plan, k):
        st, n, bad = plan.bad_pixels(k, cap)
        return st, n, None if bad is None else bad.tobytes()
    return Case("panasonic_v4_plan", abi.PanasonicV4Job, abi.PanasonicV4Desc(P4.SPLIT, 1), data,
                want, 0, P4.consumed(P4.SPLIT, w, h), extra=dict(bad_cap=cap), per_job=report,
                per_job_want=(0, cap, zeros.tobytes()))


def _samsung_v0(oracle, tall):
    # (two blocks a row: the first may point upwards; the row offsets count from the job's input
    # and are one array for every copy; the tall frame draws its rows from a pool, so the model
    # parses each once)
    w, h = (32, S0.MAX_H) if tall else (40, 7)
    rng = np.random.default_rng([0xB13, tall])
    rows = S0.tiled_rows(rng, w, h, p_up=0.4) if tall else S0.random_rows(rng, w, h, p_up=0.4)
    st, _, img = S0.model_decode(w, h, rows, cache={})
    assert st == S0.OK
    strip, offs = S0.strip_and_offsets(rows)
    want = HostImage(w, h)
    want.pixels()[:] = img
    return Case("samsung_v0_plan", abi.SamsungV0Job, None, strip, want, st,
                extra=dict(row_offsets=abi.samsung_v0_offsets(offs), n_offsets=len(offs)))


def _nikon_snef(oracle, tall):
    # (three components, 6 dim_x bytes a row; a dithering table with large deltas: every sample
    # depends on the seed the kernel reads from the first three bytes of its input row)
    w, h = (8, SN.MAX_H) if tall else (10, 5)
    rng = np.random.default_rng([0xB14, tall])
    data = rng.integers(0, 256, 3 * w * h, dtype=np.uint8)
    table, wb = SN.arbitrary_table(rng), (512, 682)
    d, keep = abi.nikon_snef_desc(wb[0], wb[1], table)
    want = HostImage(w, h, cpp=3, is_cfa=False)
    want.pixels()[:] = SN.model_decode(data, w, h, wb[0], wb[1], table)
    c = Case("nikon_snef_plan", abi.NikonSnefJob, d, data, want, 0, 3 * w * h)
    c.keep = keep
    return c


def _vc5(oracle, tall):
    # (34: the smallest side, every level odd; the band offsets count from the job's input)
    w, h = 34, TALL_ROWS if tall else 34
    t = VC.make_tile(0xB15 + tall, w, h, prescale=VC.PRESCALES[2], density=0.05 if tall else 0.2)
    data, bands = t.layout(1)
    d, keep = VC.abi_desc(t, bands)
    st, img, _ = VC.model_decode(t, data, bands)
    assert st == VC.OK
    want = HostImage(w, h)
    want.pixels()[:] = img
    c = Case("vc5_plan", abi.Vc5Job, d, data, want, st)
    c.keep = keep
    return c


def _dng_deflate(oracle, tall):
    # (a 32 x 16 tile of 24-bit floats, horizontal predictor of two bytes; small: inside a
    # 64 x 40 image; tall: the last 16 rows of a 16-sample-wide image, which cuts it to 16 samples)
    bps, predictor = 24, 34894
    dim_x, dim_y, off_x, off_y = (16, TALL_ROWS, 0, TALL_ROWS - 16) if tall else (64, 40, 24, 17)
    geom = (32, 16, off_x, off_y, min(32, dim_x - off_x), 16)
    rng = np.random.default_rng([0xB16, tall])
    data = DD.write_tile(DD.random_samples(rng, bps, 16, 32), bps, predictor, 1)
    v, bits, used = DD.model_decode(data, bps, predictor, 1, geom)
    want = HostImage(dim_x, dim_y, is_cfa=False, bpc=4)
    DD.paste(want.u32(), geom, bits)
    tile_w, tile_h, _, _, width, height = geom
    return Case("dng_deflate_plan", abi.DngDeflateJob, abi.DngDeflateDesc(bps, predictor),
                np.frombuffer(data, np.uint8), want, DD.STATUS[v], used, bpc=4,
                extra=dict(tile_w=tile_w, tile_h=tile_h, off_x=off_x, off_y=off_y, width=width,
                           height=height))


def _dng_jpeg(oracle, tall):
    # (two tiles of the 8 x 8 grey fixture, the smallest of a whole block; the job's table of
    # input offsets is made anew for every placement, and the second stream starts on the line)
    c = DJ.case("grey_8x8")
    st, frame = DJ.model_decode(c["stream"], 1)
    assert st == DJ.OK and DJ.sha(frame) == c["sha256"]
    dim_x, dim_y, offs = (16, TALL_ROWS, [(0, 0), (8, TALL_ROWS - 8)]) if tall else (21, 13, [(1, 2), (12, 5)])
    want = HostImage(dim_x, dim_y, is_cfa=False)
    for ox, oy in offs:
        DJ.paste(want.pixels(), frame, ox, oy, 1)
    tiles, keep = abi.dng_jpeg_tiles([c["stream"]] * 2, offs)
    second = _al(len(c["stream"]) + 15)
    data = np.full(second + len(c["stream"]), 0x5A, np.uint8)
    for at in (0, second):
        data[at:at + len(c["stream"])] = np.frombuffer(c["stream"], np.uint8)

    def place(j, in_off):
        j.in_offsets = (ctypes.c_uint64 * 2)(in_off, in_off + second)
    case = Case("dng_jpeg_plan", abi.DngJpegJob, None, data, want, st, in_mid=second, place=place,
                extra=dict(n_tiles=2, tiles=tiles))
    case.keep = keep
    return case


def _fuji(oracle, tall):
    # (768 columns: one strip, the narrowest frame; the strip offsets count from the job's input
    # (rsx_fuji.hip: in_offset + strip_offset); the expected image is the host build's, held
    # against the pixels the writer reached.  A strip is one workgroup's serial work: 4104 rows took
    # 6.5 s on an MI355X, so the tall frame has 516 rows at a pitch of 8.6 MB, which puts its last
    # 15 rows -- two and a half lines -- past 2^32)
    w, h = FJ.BLOCK, 516 if tall else 12
    hd = FJ.header(16, 14, w, h)
    target = FJ.content("steps" if tall else "noisy", 14, w, h, 0xB18 + tall)
    strip, reached = synth.fuji_encode_strip(16, 14, h // 6, target, None)[:2]
    data = FJ.container(hd, [strip])
    st, ss, px = FJ.host_decode(data)
    assert (st, ss) == (FJ.OK, [FJ.OK]) and np.array_equal(px, reached)
    pst, _, strips = FJ.parse(data)
    assert pst == FJ.OK
    want = HostImage(w, h)
    want.pixels()[:] = px
    return Case("fuji_plan", abi.FujiJob, abi.fuji_desc(hd, strips), np.frombuffer(data, np.uint8),
                want, st, tall_pitch=_al(EXTENT // h))


def _kodak(oracle, tall):
    # (260 columns: a full segment and a tail of four a row; the dither table's entries)
    w, h, bps = (12, KD.MAX_Y, 12) if tall else (260, 4, 12)
    rng = random.Random("plan limits: kodak %d" % tall)
    data = b"".join(KD.encode_segment(lens, fields, rng)
                    for lens, fields in KD._gen_noise(w, h, bps, rng))
    st, values, _ = KD.decode(data, w, h, bps)
    assert st == KD.OK
    curve = KD.curve("camera", bps)
    d, keep = abi.kodak_desc(bps, KD.DITHER, KD.dither_table(curve))
    want = HostImage(w, h)
    want.pixels()[:] = KD.apply_table(values, KD.DITHER, curve)
    c = Case("kodak_plan", abi.KodakJob, d, np.frombuffer(data, np.uint8), want, st)
    c.keep = keep
    return c


def _crw(oracle, tall):
    # (the scan and the low bits are two blobs of one input block; low_offset follows the block)
    c = CW.build_case("geom_64x3048_mostly_eob" if tall else "geom_68x16")
    st, px = CW.expected(c["name"], True)
    assert st == CW.OK
    scan, low = np.frombuffer(c["data"], np.uint8), np.frombuffer(c["low"], np.uint8)
    at = _al(scan.size + 16 + 15)
    data = np.full(at + low.size, 0x5A, np.uint8)
    data[:scan.size], data[at:] = scan, low
    want = HostImage(c["width"], c["height"])
    want.pixels()[:] = px

    def place(j, in_off):
        j.low_offset = in_off + at
    return Case("crw_plan", abi.CrwJob, abi.crw_desc(c["table"], True), data, want, st,
                in_bytes=scan.size, in_mid=at, place=place, extra=dict(low_bytes=low.size))


def _stage_shape(tall):
    return (64, TALL_ROWS) if tall else (68, 12)


def _u16_rows(img):
    return np.ascontiguousarray(img, np.uint16).view(np.uint8).reshape(img.shape[0], -1)


def _iiq_correct(oracle, tall):
    # (the quadrant curves: every row is written, and the split row is the model's)
    w, h = _stage_shape(tall)
    rng = np.random.default_rng([0xB1B, tall])
    img = rng.integers(0, 65536, size=(h, w)).astype(np.uint16)
    ops = [("quad", IC.random_curves(rng), h // 2 + 1, 29, 1000)]
    st, px = IC.apply(img, ops)
    d, keep = abi.iiq_corr(ops)
    want = HostImage(w, h)
    want.pixels()[:] = px
    c = Case("iiq_correct_plan", abi.IiqCorrectJob, None, (), want, st, source=_u16_rows(img),
             no_input=True, extra=dict(corr=d))
    c.keep = keep
    return c


def _dng_post(oracle, tall):
    # (DeltaPerRow over the whole image -- a delta of its own for every row -- then the
    # linearization table)
    w, h = _stage_shape(tall)
    rng = np.random.default_rng([0xB1C, tall])
    img = rng.integers(0, 65536, size=(h, w)).astype(np.uint16)
    opcodes = DP.opcode_list([DP.op_delta(10, (0, 0, h, w), rng.uniform(-1, 1, size=h).astype(np.float32))])
    table = np.sort(rng.integers(0, 65536, size=700)).astype(np.uint16)
    st, px, info = DP.apply(img, 1, (0, 0, w, h), opcodes, table)
    assert info["n_applied"] == 1 and not info["bad"]
    d, keep = abi.dng_post_desc(opcodes, table, (0, 0, w, h))
    want = HostImage(w, h)
    want.pixels()[:] = px
    c = Case("dng_post_plan", abi.DngPostJob, d, (), want, st, source=_u16_rows(img),
             no_input=True, extra=dict(bad_cap=16))
    c.keep = keep
    return c


def _scale(oracle, tall):
    # (a black and a white level over the whole image, dithered: a generator seeded per row)
    w, h = _stage_shape(tall)
    sc = SC.Case("limits", SC._u16([0xB1D, tall], w, h, lo=100, hi=5000), black=64, white=4095)
    st, px, _ = SC.apply(sc)
    d, keep = abi.scale_desc(sc.crop, sc.black, sc.white, sc.sep, sc.areas, sc.dither, sc.sse2)
    want = HostImage(w, h)
    want.pixels()[:] = px
    c = Case("scale_plan", abi.ScaleJob, d, (), want, st, source=_u16_rows(sc.img), no_input=True)
    c.keep = keep
    return c


def _bad_pixels(oracle, tall):
    # (positions in the first row, in the two rows around the 4 GiB line of the tall pitch, and in
    # the last row; the positions are the job's input)
    w, h = _stage_shape(tall)
    line = G32 // TALL_PITCH if tall else h // 2
    img = BP._image(0xB1E + tall, w, h, False)
    positions = [BP.pos(x, y) for y in (0, line, line + 1, h - 1) for x in (0, 5, 6, 33, w - 1)]
    positions += [BP.pos(x, y) for y in (line - 1, line + 2) for x in (6, 40)]
    px, _, n_bad, _ = BP.model_fix(img, True, positions)
    assert n_bad == len(positions) and (px != img).sum() > len(positions) // 2
    want = HostImage(w, h)
    want.pixels()[:] = px
    return Case("bad_pixels_plan", abi.BadPixelsJob, None, np.asarray(positions, np.uint32).view(np.uint8),
                want, 0, source=_u16_rows(img), extra=dict(n_positions=len(positions)))


KINDS = {
    "unpack_u16": _unpack, "unpack_f32": _unpack_f32, "unpack_variant": _unpack_variant,
    "ljpeg_1c": _ljpeg(1), "ljpeg_2c": _ljpeg(2), "ljpeg_3c": _ljpeg(3), "ljpeg_4c": _ljpeg(4),
    "cr2": _cr2, "cr2_sraw": _cr2_sraw, "sraw_interpolate": _sraw,
    "nikon_split": _nikon(True), "nikon_curve": _nikon(False), "pentax": _pentax,
    "samsung_v1": _samsung_v1, "samsung_v2": _samsung_v2, "hasselblad": _hasselblad,
    "sony_arw1": _sony_arw1, "phase_one": _phase_one, "sony_arw2": _sony_arw2,
    "olympus": _olympus,
    "panasonic_v5_12": _panasonic(5, 12, (700, 17), 20),
    "panasonic_v6_14": _panasonic(6, 14, (77, 9), 22, zero_half=True),
    "panasonic_v4": _panasonic_v4, "samsung_v0": _samsung_v0, "nikon_snef": _nikon_snef,
    "vc5": _vc5, "dng_deflate": _dng_deflate, "dng_jpeg": _dng_jpeg, "fuji": _fuji,
    "kodak": _kodak, "crw": _crw, "iiq_correct": _iiq_correct, "dng_post": _dng_post,
    "scale": _scale, "bad_pixels": _bad_pixels,
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


def _places_in(mid):
    # (the boundary falls on byte `mid` of the input block, 15 bytes behind it at the most)
    return [0, _al(G31 - mid), _al(G32 - mid), ABOVE]


def _places_out(h, row_bytes, pitch):
    # (the boundary falls in the middle of a row of pixels)
    mid = (h // 2) * pitch + row_bytes // 2
    return [0, _al(G31 - mid), _al(G32 - mid), ABOVE]


def _run_placed(gpu, bufs, case, placed, pitch):
    """placed: [(input offset, image offset)] of copies of `case`; returns per copy (status,
    consumed, image rows, what case.per_job reports), with the output buffer checked for bytes no
    copy owns"""
    inp, out = bufs
    inp.fill_(0x5A)
    out.fill_(0xA5)
    if case.data.size:
        src = torch.from_numpy(case.data).cuda()
        for io, _ in placed:
            assert io % 16 == 0 and io + case.data.size <= EXTENT
            inp[BASE + io:BASE + io + case.data.size].copy_(src)
    h, rb = case.want.dim_y, case.row_bytes
    source = None if case.source is None else torch.from_numpy(case.source).cuda()
    jobs = [case.job(io, oo, pitch) for io, oo in placed]
    plan = getattr(gpu, case.plan)(jobs)
    res = []
    try:
        for run in range(2):
            if run:
                out.fill_(0xA5)
            if source is not None:
                for _, oo in placed:
                    _rect(out, oo, h, rb, pitch).copy_(source)
            plan.run(inp.data_ptr() + BASE, out.data_ptr() + BASE)
            rc, status, consumed = plan.results()
            more = [case.per_job(plan, k) if case.per_job else None for k in range(len(placed))]
            rows = [_rect(out, oo, h, rb, pitch).contiguous().cpu().numpy() for _, oo in placed]
            for _, oo in placed:
                _rect(out, oo, h, rb, pitch).fill_(0xA5)
            dirty = _first_dirty(out)
            assert dirty is None, "run %d wrote at offset %#x, outside every job's image" % (run, dirty)
            res.append(list(zip(status, consumed, rows, more)))
    finally:
        plan.close()
    return res


def _check_copies(case, res, what):
    want = case.rows()
    for run, copies in enumerate(res):
        st0, c0, px0, more0 = copies[0]
        assert st0 == case.status == 0
        if case.consumed is not None:
            assert c0 == case.consumed, (run, c0, case.consumed)
        assert np.array_equal(px0, want), "run %d: the offset-0 copy differs from the oracle" % run
        assert more0 == case.per_job_want, "run %d: the offset-0 copy's report differs from the oracle" % run
        for k, (st, c, px, more) in enumerate(copies):
            assert (st, c) == (st0, c0), (run, what[k], st, c, st0, c0)
            assert np.array_equal(px, px0), "run %d: %s differs from the offset-0 copy" % (run, what[k])
            assert more == more0, "run %d: the report of %s differs from the offset-0 copy's" % (run, what[k])


def _tall_pitch(h):
    """1 MiB + 16 for 4100 rows and more, 1400016 for 3072; for any other height the smallest
    multiple of 16 above 2^32 / (h - 1), plus 16: the last row starts past 2^32 and the image
    ends inside the buffer"""
    if h >= TALL_ROWS:
        return TALL_PITCH
    if h == SHORT_ROWS:
        return SHORT_PITCH
    pitch = (G32 // (h - 1) // 16 + 1) * 16 + 16
    assert (h - 1) * pitch > G32 and h * pitch <= EXTENT
    return pitch


@pytest.mark.parametrize("kind", list(KINDS))
def test_copies_past_2g_and_4g(gpu, oracle, bufs, kind):
    """The same job at input offsets 0, across 2^31, across 2^32 and above 2^32 (image in a slot
    of its own), and at those image offsets (input in a slot): every copy the same.  A plan that
    reads no input has the four image placements alone."""
    case = KINDS[kind](oracle, False)
    assert case.status == 0
    pitch = (case.row_bytes + 16 + 15) // 16 * 16  # (padding behind every row: nobody's)
    h = case.want.dim_y
    span_in, span_out = _al(case.data.size + 4096 + 15), _al(h * pitch + 4096 + 15)
    ins, outs = _places_in(case.in_mid), _places_out(h, case.row_bytes, pitch)
    if case.no_input:
        ins = []
    placed = [(io, SLOTS + k * span_out) for k, io in enumerate(ins)]
    placed += [(SLOTS + k * span_in, oo) for k, oo in enumerate(outs)]
    what = ["input at %#x" % io for io in ins] + ["image at %#x" % oo for oo in outs]
    _check_copies(case, _run_placed(gpu, bufs, case, placed, pitch), what)


@pytest.mark.parametrize("kind", list(KINDS))
def test_image_whose_rows_cross_4g(gpu, oracle, bufs, kind):
    """One job, pitch 1 MiB + 16, 4100 rows (3072 rows of 1.34 MB where the decoder allows no
    more; any other height: _tall_pitch, or the case's own pitch): its last rows lie past 2^32 of
    the output.  Against the oracle and against the same image at a compact pitch."""
    case = KINDS[kind](oracle, True)
    h = case.want.dim_y
    pitch = case.tall_pitch or _tall_pitch(h)
    assert case.status == 0 and (h - 1) * pitch > G32 and h * pitch <= EXTENT
    compact = (case.row_bytes + 15) // 16 * 16
    res = _run_placed(gpu, bufs, case, [(SLOTS, 0)], pitch)
    small = _run_placed(gpu, bufs, case, [(SLOTS, 0)], compact)
    want = case.rows()
    for run, copies in enumerate(res):
        st, c, px, more = copies[0]
        assert st == 0 == small[run][0][0]
        assert c == small[run][0][1]
        if case.consumed is not None:
            assert c == case.consumed
        bad = np.flatnonzero((px != want).any(axis=1))
        assert bad.size == 0, "run %d: rows %s differ from the oracle" % (run, bad[:10])
        assert np.array_equal(small[run][0][2], want)
        assert more == case.per_job_want == small[run][0][3]


# ---- C. 65535 jobs: the largest grid axis ----------------------------------------------------

MAX_JOBS = 65535


class Edge:
    """The smallest job of a plan type that puts the job index on a grid axis, and what a plan of n
    of them looks like: the template job copied n times, its input and image offsets stepping
    through compact buffers.

      job        the template (offsets of copy 0; the image's pitch is its row)
      data       the input block of one job (empty: the plan reads no input)
      in_fields  the job's fields that step with the input block
      source     (rows, row bytes) uint8 written into every image before the run (in place), or None
      want       (rows, row bytes) uint8: what the oracle says every image holds afterwards"""
    GAP = 16  # bytes between two images: nobody's

    def __init__(self, plan, job, data, want, source=None, in_fields=("in_offset",), keep=None):
        self.plan, self.job, self.keep = plan, job, keep
        self.data = np.array(data, np.uint8).reshape(-1)
        self.want = np.ascontiguousarray(want, np.uint8)
        self.source = None if source is None else np.ascontiguousarray(source, np.uint8)
        self.in_fields = in_fields if self.data.size else ()
        self.in_stride = _al(self.data.size + 15) + 16
        h, rb = self.want.shape
        assert job.img.pitch_bytes == rb and (job.img.dim_y, job.img.dim_x * job.img.cpp * 2) == (h, rb)
        self.out_stride = h * rb + self.GAP

    def jobs(self, n, odd_image=None):
        """a ctypes array of n jobs; job `odd_image` (if any) gets an odd img_offset"""
        cls = type(self.job)
        raw = np.tile(np.frombuffer(bytes(self.job), np.uint8), n).reshape(n, ctypes.sizeof(cls))
        k = np.arange(n, dtype=np.uint64)
        steps = [(f, self.in_stride) for f in self.in_fields] + [("img_offset", self.out_stride)]
        for name, stride in steps:
            field = getattr(cls, name)
            assert field.size == 8
            vals = np.uint64(getattr(self.job, name)) + k * np.uint64(stride)
            if name == "img_offset" and odd_image is not None:
                vals[odd_image] += np.uint64(1)
            raw[:, field.offset:field.offset + 8] = vals.view(np.uint8).reshape(n, 8)
        return (cls * n).from_buffer(raw)

    def buffers(self, n):
        """(device input, device output as the run finds it, host output as it must leave it)"""
        inp = np.full((n, self.in_stride), 0x5A, np.uint8)
        inp[:, :self.data.size] = self.data
        h, rb = self.want.shape
        before = np.full((n, self.out_stride), 0xA5, np.uint8)
        after = before.copy()
        if self.source is not None:
            before[:, :h * rb] = self.source.reshape(-1)
        after[:, :h * rb] = self.want.reshape(-1)
        return (torch.from_numpy(inp.reshape(-1)).cuda(), torch.from_numpy(before.reshape(-1)).cuda(),
                after)


def _edge_image(w, h, pitch):
    import gpu_util
    return gpu_util.image_job_view(w, h, 1, pitch)


def _edge_kodak():
    # (4 x 1 of zeros: one segment of four, its 16 leading bits and no difference bits)
    seg = KD.encode_segment([0] * 4, [0] * 4, random.Random("plan limits: kodak edge"))
    st, values, _ = KD.decode(seg, 4, 1, 12)
    assert st == KD.OK and KD.validate(4, 1, 12, len(seg)) == KD.OK
    j = abi.KodakJob()
    j.desc, _ = abi.kodak_desc(12, KD.NONE)
    j.in_bytes, j.img = len(seg), _edge_image(4, 1, 8)
    return Edge("kodak_plan", j, np.frombuffer(seg, np.uint8), _u16_rows(values.astype(np.uint16)))


def _edge_crw():
    c = CW.build_case("geom_8x8")
    st, px = CW.expected("geom_8x8", True)
    assert st == CW.OK
    scan, low = np.frombuffer(c["data"], np.uint8), np.frombuffer(c["low"], np.uint8)
    at = _al(scan.size + 15)
    data = np.full(at + low.size, 0x5A, np.uint8)
    data[:scan.size], data[at:] = scan, low
    j = abi.CrwJob()
    j.desc = abi.crw_desc(c["table"], True)
    j.in_bytes, j.low_offset, j.low_bytes = scan.size, at, low.size
    j.img = _edge_image(8, 8, 16)
    return Edge("crw_plan", j, data, _u16_rows(px), in_fields=("in_offset", "low_offset"))


STAGE_W, STAGE_H = 16, 2


def _edge_scale():
    sc = SC.Case("edge", SC._u16(0xC01, STAGE_W, STAGE_H, lo=100, hi=5000), black=64, white=4095)
    st, px, _ = SC.apply(sc)
    assert st == SC.OK and (px != sc.img).any()
    j = abi.ScaleJob()
    j.desc, keep = abi.scale_desc(sc.crop, sc.black, sc.white, sc.sep, sc.areas, sc.dither, sc.sse2)
    j.img = _edge_image(STAGE_W, STAGE_H, 2 * STAGE_W)
    return Edge("scale_plan", j, (), _u16_rows(px), _u16_rows(sc.img), keep=keep)


def _edge_dng_post():
    # (one DeltaPerRow and no linearization table: the plan keeps a 256 KiB look-up per job with
    # a table, 17 GB for 65535 of them)
    rng = np.random.default_rng(0xC02)
    img = rng.integers(0, 65536, size=(STAGE_H, STAGE_W)).astype(np.uint16)
    opcodes = DP.opcode_list([DP.op_delta(10, (0, 0, STAGE_H, STAGE_W), [0.25, -0.125])])
    st, px, info = DP.apply(img, 1, (0, 0, STAGE_W, STAGE_H), opcodes, None)
    assert st == DP.OK and info["n_applied"] == 1 and (px != img).sum() > STAGE_W
    j = abi.DngPostJob()
    j.desc, keep = abi.dng_post_desc(opcodes, None, (0, 0, STAGE_W, STAGE_H))
    j.bad_cap, j.img = 16, _edge_image(STAGE_W, STAGE_H, 2 * STAGE_W)
    return Edge("dng_post_plan", j, (), _u16_rows(px), _u16_rows(img), keep=keep)


def _edge_bad_pixels():
    # (32 columns, not 16: fixBadPixels walks the columns below (dim_x + 15) / 32 * 32, which is
    # none of a 16-column image)
    w = 32
    img = BP._image(0xC03, w, STAGE_H, False)
    positions = [BP.pos(5, 0), BP.pos(26, 1)]
    px, _, n_bad, n_fixed = BP.model_fix(img, True, positions)
    assert (n_bad, n_fixed) == (2, 2) and (px != img).sum() == 2
    j = abi.BadPixelsJob()
    j.n_positions, j.img = 2, _edge_image(w, STAGE_H, 2 * w)
    return Edge("bad_pixels_plan", j, np.asarray(positions, np.uint32).view(np.uint8), _u16_rows(px),
                _u16_rows(img))


def _edge_iiq_correct():
    # (a luma flat field of 4 x 2 cells over the whole image)
    rng = np.random.default_rng(0xC04)
    img = rng.integers(0, 65536, size=(STAGE_H, STAGE_W)).astype(np.uint16)
    ops = [("ff", IC.ff_random(rng, (0, 0, STAGE_W, STAGE_H, 4, 1)), 0)]
    st, px = IC.apply(img, ops)
    assert st == IC.OK and (px != img).sum() > 8
    j = abi.IiqCorrectJob()
    j.corr, keep = abi.iiq_corr(ops)
    j.img = _edge_image(STAGE_W, STAGE_H, 2 * STAGE_W)
    return Edge("iiq_correct_plan", j, (), _u16_rows(px), _u16_rows(img), keep=keep)


EDGES = {"kodak": _edge_kodak, "crw": _edge_crw, "scale": _edge_scale, "dng_post": _edge_dng_post,
         "bad_pixels": _edge_bad_pixels, "iiq_correct": _edge_iiq_correct}


def _run_edge(gpu, edge, jobs, slots):
    """the plan of `jobs` run once over buffers of `slots` jobs -> (statuses, output bytes, the
    output as it must be where every slot's job ran)"""
    inp, out, after = edge.buffers(slots)
    plan = getattr(gpu, edge.plan)(jobs)
    try:
        plan.run(inp.data_ptr(), out.data_ptr())
        rc, status, _ = plan.results()
    finally:
        plan.close()
    return rc, status, out.cpu().numpy().reshape(after.shape), after


@pytest.mark.parametrize("kind", list(EDGES))
def test_plan_of_65535_jobs(gpu, kind):
    """Exactly 65535 jobs, the largest grid axis: every status 0, every image the oracle's, every
    byte between two images still 0xA5."""
    edge = EDGES[kind]()
    rc, status, got, want = _run_edge(gpu, edge, edge.jobs(MAX_JOBS), MAX_JOBS)
    assert rc == 0 and status == [0] * MAX_JOBS
    wrong = np.flatnonzero((got != want).any(axis=1))
    assert wrong.size == 0, "jobs %s wrote something else than the oracle's image" % wrong[:10]


@pytest.mark.parametrize("kind", list(EDGES))
def test_plan_of_65536_jobs_is_refused(gpu, kind):
    """One valid job more than a grid axis takes: no plan."""
    edge = EDGES[kind]()
    with pytest.raises(capi.RsxError) as e:
        getattr(gpu, edge.plan)(edge.jobs(MAX_JOBS + 1))
    assert e.value.status == abi.RSX_ERR_UNSUPPORTED


@pytest.mark.parametrize("kind", ["kodak", "crw"])
def test_a_refused_job_takes_no_row_of_the_grid(gpu, kind):
    """65535 valid jobs and, among them, one with an odd img_offset: the plan is made, the odd job
    reports RSX_ERR_INVALID_ARG and writes nothing, every other job is the oracle's."""
    edge = EDGES[kind]()
    odd = 40001
    rc, status, got, want = _run_edge(gpu, edge, edge.jobs(MAX_JOBS + 1, odd_image=odd), MAX_JOBS + 1)
    assert status[odd] == abi.RSX_ERR_INVALID_ARG == rc
    assert status[:odd] + status[odd + 1:] == [0] * MAX_JOBS
    want[odd] = 0xA5
    wrong = np.flatnonzero((got != want).any(axis=1))
    assert wrong.size == 0, "jobs %s wrote something else than expected" % wrong[:10]


def test_dng_jpeg_job_of_65536_tiles_is_refused(gpu):
    """65536 tiles of 8 x 8 that fill a 2048 x 2048 image: one tile more than the finish kernel's
    grid takes.  (The same job with its first four tiles is a plan.)"""
    import gpu_util
    c = DJ.case("grey_8x8")
    n = MAX_JOBS + 1
    tiles, keep = abi.dng_jpeg_tiles([c["stream"]] * n, [(8 * (k % 256), 8 * (k // 256)) for k in range(n)])
    j = abi.DngJpegJob()
    j.tiles, j.in_offsets = tiles, (ctypes.c_uint64 * n)()  # (every tile reads the one stream)
    j.img = gpu_util.image_job_view(2048, 2048, 1, 4096, is_cfa=False)
    j.n_tiles = 4
    gpu.dng_jpeg_plan([j]).close()
    j.n_tiles = n
    with pytest.raises(capi.RsxError) as e:
        gpu.dng_jpeg_plan([j])
    assert e.value.status == abi.RSX_ERR_UNSUPPORTED
