"""SamsungV2Decompressor on the device (rsx_samsung_v2_*, rawspeed_amd/csrc/rsx_samsung_v2.hip)
through the C-ABI against the oracle's restatement -- which tests/test_oracle_samsung_v2.py
pins against the reference build: streams of the writer in samsung_v2_cases.py (every block
mode, scale changes, all eight optimisation-flag combinations, both bit depths), damaged
ones (same status), batches, and a frame at the constructor's size limit; then, in plans of
many jobs, the value classes, frame geometries, row lengths, output layouts and verdicts of
samsung_v2_cases.py (second half of the file)."""
import collections
import threading

import numpy as np
import pytest
import torch

from rawspeed_amd import abi

import samsung_v2_cases as V2
from oracle_lib import HostImage
from test_oracle_samsung_v2 import _target

pytestmark = pytest.mark.gpu

INVALID_ARG = 1


@pytest.fixture(scope="module")
def gpu():
    import gpu_util
    return gpu_util.ctx()


def open_stream(data, bits, w, h):
    """What SamsungV2Decompressor's constructor does with the strip (cpp:87-141): status of
    its checks, the descriptor, the member `data`."""
    if data.size < 16:
        return 2, None, None  # bs.check(headerSize)
    d, flags = abi.SamsungV2Desc.from_header(data[:16])
    if d.bit_depth != bits:
        return INVALID_ARG, None, None
    if flags > 7:
        return INVALID_ARG, None, None
    return 0, d, data[16:]


def decode(gpu, data, bits, w, h):
    img = HostImage(w, h)
    st, d, payload = open_stream(np.asarray(data, np.uint8), bits, w, h)
    if st:
        return st, img
    return gpu.samsung_v2_decompress(d, payload, img.view()), img


@pytest.mark.parametrize("optflags", range(8))
@pytest.mark.parametrize("bits", [12, 14])
def test_writer_streams(gpu, oracle, optflags, bits):
    rng = np.random.default_rng([190, optflags, bits])
    for trial in range(3):
        h, w = int(rng.integers(2, 70)), 16 * int(rng.integers(1, 30))
        data, want = V2.encode(rng, _target(rng, h, w, bits), bits, optflags)
        host = HostImage(w, h)
        assert oracle.samsung_v2(bits, data, host) == 0
        st, img = decode(gpu, data, bits, w, h)
        assert st == 0
        assert np.array_equal(img.pixels(), host.pixels()), (trial, h, w)
        assert np.array_equal(img.pixels(), want)


@pytest.mark.parametrize("seed", range(60))
def test_damaged_streams_same_verdict(gpu, oracle, seed):
    rng = np.random.default_rng([191, seed])
    bits = int(rng.choice([12, 14]))
    h, w = int(rng.integers(2, 40)), 16 * int(rng.integers(1, 12))
    data, _ = V2.encode(rng, _target(rng, h, w, bits), bits, int(rng.integers(0, 8)))
    data = data.copy()
    kind = seed % 4
    if kind == 0:
        for _ in range(int(rng.integers(1, 6))):
            data[int(rng.integers(16, data.size))] ^= 1 << int(rng.integers(0, 8))
    elif kind == 1:
        data = data[:int(rng.integers(16, data.size))]
    elif kind == 2:
        data[int(rng.integers(0, 16))] ^= 1 << int(rng.integers(0, 8))
    else:
        data[16:] = rng.integers(0, 256, size=data.size - 16, dtype=np.uint8)
    host = HostImage(w, h)
    s_or = oracle.samsung_v2(bits, data, host)
    st, img = decode(gpu, data, bits, w, h)
    assert st == s_or, (st, s_or)
    if s_or == 0:
        assert np.array_equal(img.pixels(), host.pixels())


def test_validate_is_the_constructor(gpu):
    from rawspeed_amd import capi
    import ctypes as C
    L = capi.lib()
    img = HostImage(64, 8)
    d = abi.SamsungV2Desc()
    d.bit_depth, d.width, d.height, d.optflags, d.init_val = 12, 64, 8, 0, 5
    v = img.view()
    assert L.rsx_samsung_v2_validate(C.byref(d), C.byref(v)) == 0
    for field, bad in (("bit_depth", 13), ("width", 48), ("width", 6512), ("height", 4337),
                       ("height", 9), ("optflags", 8), ("width", 0)):
        e = abi.SamsungV2Desc.from_buffer_copy(d)
        setattr(e, field, bad)
        assert L.rsx_samsung_v2_validate(C.byref(e), C.byref(v)) == INVALID_ARG, (field, bad)


def _job(d, off, n, w, h, img_off):
    j = abi.SamsungV2Job()
    j.desc = d
    j.in_offset, j.in_bytes, j.img_offset = off, n, img_off
    j.img.pitch_bytes, j.img.dim_x, j.img.dim_y, j.img.cpp, j.img.is_cfa = w * 2, w, h, 1, 1
    return j


def test_batch_of_frames_in_one_plan(gpu, oracle):
    """Several frames of different sizes, one of them damaged, one launch sequence."""
    rng = np.random.default_rng(192)
    frames, jobs, parts, off, img_off = [], [], [], 0, 0
    for k in range(5):
        bits = (12, 14)[k & 1]
        h, w = int(rng.integers(20, 120)), 16 * int(rng.integers(4, 40))
        data, want = V2.encode(rng, _target(rng, h, w, bits), bits, int(rng.integers(0, 8)))
        if k == 3:
            data = data[:data.size // 2]
        host = HostImage(w, h)
        s_or = oracle.samsung_v2(bits, data, host)
        st, d, payload = open_stream(data, bits, w, h)
        assert st == 0
        pad = (-payload.size) % 16
        parts.append(np.concatenate([payload, np.zeros(pad, np.uint8)]))
        jobs.append(_job(d, off, payload.size, w, h, img_off))
        frames.append((w, h, img_off, s_or, host.pixels().copy()))
        off += payload.size + pad
        img_off += w * h * 2
    plan = gpu.samsung_v2_plan(jobs)
    inp = torch.from_numpy(np.concatenate(parts)).cuda()
    out = torch.zeros(img_off, dtype=torch.uint8, device="cuda")
    for run in range(2):
        out.zero_()
        plan.run(inp.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        rc, st, _ = plan.results()
        got = out.cpu().numpy()
        for k, (w, h, io, s_or, px) in enumerate(frames):
            assert st[k] == s_or, (k, st, s_or)
            if s_or == 0:
                assert np.array_equal(got[io:io + w * h * 2].view(np.uint16).reshape(h, w), px), k
        assert (rc == 0) == all(f[3] == 0 for f in frames)


@pytest.mark.parametrize("w,h", [(6496, 100), (1024, 700)])
def test_frames_at_the_size_limits(gpu, oracle, w, h):
    """The widest row the constructor accepts (406 blocks: the anti-diagonals of the
    reconstruction are longest), and a tall frame (the row-start table over many hops)."""
    rng = np.random.default_rng([193, w])
    bits = 14
    data, want = V2.encode(rng, _target(rng, h, w, bits), bits, 0)
    host = HostImage(w, h)
    assert oracle.samsung_v2(bits, data, host) == 0
    st, img = decode(gpu, data, bits, w, h)
    assert st == 0
    assert np.array_equal(img.pixels(), host.pixels())


# ---------------------------------------------------------------------------------------------
# Value, geometry, layout and verdict edges, each in a plan of many jobs.  Every expectation is
# the oracle's (which tests/test_samsung_v2_model.py pins against the reference build and the
# Python model on these same streams); the whole output buffer is compared, so a store outside
# a good job's pixels -- row padding, the gaps between jobs, the rectangle of a failed job --
# fails the test as well.
# ---------------------------------------------------------------------------------------------
OK, IO, INPUT_OVERFLOW = 0, 2, 5
SENTINEL = 0xA5

_TRUTH = {}


def truth(oracle, key, bits, w, h, data):
    """(status, pixels) of the oracle for a stream, computed once per key"""
    if key not in _TRUTH:
        host = HostImage(w, h)
        st = oracle.samsung_v2(bits, np.asarray(data, np.uint8), host)
        px = host.pixels().copy()
        px.flags.writeable = False
        _TRUTH[key] = (st, px)
    return _TRUTH[key]


class Layout:
    """The jobs of one rsx_samsung_v2_plan_create plan in one input and one output buffer.
    Input: every payload at a multiple of 16, followed by at least 16 bytes of 0xFF (a kernel
    that read past in_bytes would see ones where the reference pads with zeros).  Output:
    every job's rectangle where the test puts it; everything else keeps the sentinel."""

    Entry = collections.namedtuple("Entry", "name w h img_off pitch status px")

    def __init__(self):
        self.jobs, self.parts, self.entries = [], [], []
        self.in_end = self.out_end = 0

    def add(self, name, data, bits, w, h, status, px, pitch=None, shift=0, gap=0, reject=None):
        """data: the whole stream (header included); status / px: what the oracle says;
        pitch: bytes per output row (2 w); shift + gap: bytes between the end of the job before
        and this one's first pixel; reject: None, or a function that damages the job so that
        the host refuses it (the expected status is then INVALID_ARG)"""
        data = np.asarray(data, np.uint8)
        st, d, payload = open_stream(data, bits, w, h)
        if st:  # the constructor's own checks (the container's, here): no device involved
            assert st == status, (name, st, status)
            d, payload = abi.SamsungV2Desc(), data[:0]
            d.bit_depth, d.width, d.height = 0, w, h  # (a job the host rejects)
        pitch = pitch or 2 * w
        img_off = self.out_end + gap + shift
        j = _job(d, self.in_end, payload.size, w, h, img_off)
        j.img.pitch_bytes = pitch
        if reject:
            reject(j)
            status = INVALID_ARG
        self.jobs.append(j)
        pad = (-payload.size) % 16 + 16
        self.parts.append(payload)
        self.parts.append(np.full(pad, 0xFF, np.uint8))
        self.in_end += payload.size + pad
        self.entries.append(self.Entry(name, w, h, img_off, pitch, status, px))
        self.out_end = img_off + pitch * h
        return j

    def run(self, gpu, runs=2):
        """run the plan `runs` times into sentinel-filled buffers and check each"""
        plan = gpu.samsung_v2_plan(self.jobs)
        inp = torch.from_numpy(np.concatenate(self.parts + [np.full(64, 0xFF, np.uint8)])).cuda()
        n = self.out_end + 64
        want = np.full(n, SENTINEL, np.uint8)
        for e in self.entries:
            if e.status == OK:
                b = np.ascontiguousarray(e.px).view(np.uint8).reshape(e.h, 2 * e.w)
                for r in range(e.h):
                    lo = e.img_off + r * e.pitch
                    want[lo:lo + 2 * e.w] = b[r]
        for run in range(runs):
            out = torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda")
            plan.run(inp.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
            rc, st, _ = plan.results()
            self.check(out.cpu().numpy(), st, want, run)
            assert (rc == 0) == all(e.status == OK for e in self.entries)
        plan.close()
        return collections.Counter(e.status for e in self.entries)

    def check(self, got, st, want, run):
        bad = [(e.name, s, e.status) for e, s in zip(self.entries, st) if s != e.status]
        assert not bad, "run %d: (job, status, the oracle's) %s" % (run, bad[:8])
        rest = got != want
        if not rest.any():
            return
        for e in self.entries:
            if e.status != OK:
                continue
            for r in range(e.h):
                lo = e.img_off + r * e.pitch
                assert not rest[lo:lo + 2 * e.w].any(), "run %d, %s: row %d differs at pixel %d" % (
                    run, e.name, r, int(np.argmax(rest[lo:lo + 2 * e.w])) // 2)
                rest[lo:lo + 2 * e.w] = False
        k = int(np.argmax(rest))
        raise AssertionError("run %d: byte %d outside every good job's pixels was written: 0x%02x"
                             % (run, k, int(got[k])))


VALUE_WIDTHS = ((256, 40), (16, 40), (64, 40), (80, 40))


@pytest.mark.parametrize("cls", V2.CLASSES)
def test_value_class(gpu, oracle, cls):
    """one plan per class: every depth x flag set at 256 x 40, and 16 (one block: no scale
    field after block 0), 64 and 80 (the scale field of every fourth block, and one block
    behind it) wide at two flag sets"""
    lay = Layout()
    for w, h in VALUE_WIDTHS:
        for bits in (12, 14):
            for optflags in (range(8) if w == 256 else (0, 3)):
                c = V2.value_case(cls, bits, optflags, w, h)
                key = ("value", cls, bits, optflags, w, h)
                st, px = truth(oracle, key, bits, w, h, c.data)
                assert st == OK
                lay.add("%s_%d_f%d_%dx%d" % (cls, bits, optflags, w, h), c.data, bits, w, h, st, px)
    lay.run(gpu, runs=1)


def test_negative_scale_by_hand(gpu, oracle):
    data, _ = V2.negative_scale_rows()
    st, px = truth(oracle, "negative_by_hand", 12, 32, 4, data)
    assert st == OK and (px[:, :16] == 95).all() and (px[:, 16:] == 93).all()
    lay = Layout()
    lay.add("negative_by_hand", data, 12, 32, 4, st, px)
    lay.run(gpu, runs=1)


SEAM_HEIGHTS = (1, 2, 3, 4, 33, 34, 35, 36, 65, 66, 67)


def test_geometry(gpu, oracle):
    """6496 x 272: 203 blocks on a diagonal while the ring's 256 rows wrap; 16 and 48 x 4336:
    the height limit, 136 hops of the row-start table; 6496 x 3; and every height around the
    seams of the row-start machinery (rows 0 and 1, row 2, every 32nd row behind it) one and
    three blocks wide.  The frames are short ones of the writer with their rows repeated."""
    lay = Layout()
    frames = [(14, 6496, 272), (12, 16, 4336), (14, 48, 4336), (14, 6496, 3)]
    frames += [((12, 14)[k & 1], w, h) for w in (16, 48) for k, h in enumerate(SEAM_HEIGHTS)]
    for bits, w, h in frames:
        data = V2.tall_frame(bits, w, h)
        st, px = truth(oracle, ("tall", bits, w, h), bits, w, h, data)
        assert st == OK
        lay.add("%dx%d_%d" % (w, h, bits), data, bits, w, h, st, px)
    lay.run(gpu, runs=1)


def _residue_frames():
    """16-wide frames whose rows take 15, 16, 17 and 32 bytes (getStreamPosition() behind the
    one block of 28 bits + sixteen differences: 116, 124, 132 and 252 bits), cut behind the
    last row's last byte ("cut+0"), one byte further ("cut+1") and one byte short ("short");
    and cut behind the last row but one of a frame that claims one row more ("missing"):
    (name, bits, w, h, stream)"""
    out = []
    for nbytes, lens in ((15, (5, 5, 6, 6)), (16, (6, 6, 6, 6)), (17, (6, 6, 7, 7)),
                         (32, (14, 14, 14, 14))):
        for h in (1, 2, 3, 4, 35):
            rows = [V2.RowAsm(r, 14, 0).block(lens=lens, diffs=[(3 * i + r) % 5 - 2 for i in range(16)])
                    for r in range(h)]
            used = {r.bytes_used() for r in rows}
            assert used == {nbytes}, (used, nbytes)
            end = 16 + 16 * ((nbytes + 15) // 16) * (h - 1) + nbytes
            data = V2.assemble(14, 16, h, rows, 0, 9000)
            for tag, n in (("cut+0", end), ("cut+1", end + 1), ("short", end - 1)):
                out.append(("row%dB_h%d_%s" % (nbytes, h, tag), 14, 16, h, data[:n].copy()))
            more = V2.assemble(14, 16, h + 1, rows, 0, 9000)
            out.append(("row%dB_h%d_missing" % (nbytes, h), 14, 16, h + 1, more[:end].copy()))
    return out


def test_row_length_residues(gpu, oracle):
    """rows that end one byte before, at and one byte behind a 16-byte boundary; the last row
    ending exactly at in_bytes, one byte before the end of the data, and one byte past it
    (RSX_ERR_IO, :337); and a row that would start at the boundary past the data (:331-332)"""
    lay = Layout()
    residues, verdicts = set(), collections.Counter()
    for name, bits, w, h, data in _residue_frames():
        st, px = truth(oracle, ("residue", name), bits, w, h, data)
        lay.add(name, data, bits, w, h, st, px)
        residues.add((data.size - 16) % 16)
        verdicts[(name.rsplit("_", 1)[1], st)] += 1
    assert {0, 1, 15} <= residues, residues
    # a frame cut right behind its last row is whole; one byte short, it is not
    assert verdicts[("cut+0", OK)] == 20 and verdicts[("cut+1", OK)] == 20, verdicts
    assert verdicts[("short", IO)] == 20 and verdicts[("missing", IO)] == 20, verdicts
    lay.run(gpu)


def _layout_plan(oracle, kinds):
    """nine frames of three sizes; kind "odd": img_offset % 8 == 2 and a pitch of 2 w + 2 (rows
    start at every residue of 2 mod 8: the 16-bit stores); kind "padded": img_offset % 8 == 0
    and a pitch of 2 w + 24.  The fourth frame is cut short: its rectangle stays untouched."""
    lay = Layout()
    for k in range(9):
        bits, (w, h) = (12, 14)[k & 1], ((64, 9), (16, 35), (272, 6))[k % 3]
        c = V2.value_case(("extremes", "sensor", "max_len")[k % 3], bits, k % 8, w, h)
        data = c.data[:c.data.size // 2] if k == 3 else c.data
        st, px = truth(oracle, ("layout", k), bits, w, h, data)
        assert (st == OK) == (k != 3)
        kind = kinds[k % len(kinds)]
        if kind == "odd":
            j = lay.add("odd%d" % k, data, bits, w, h, st, px, pitch=2 * w + 2,
                        shift=(2 - lay.out_end) % 8, gap=8 * k)
            assert j.img_offset % 8 == 2 and j.img.pitch_bytes % 8 == 2
        else:
            j = lay.add("padded%d" % k, data, bits, w, h, st, px, pitch=2 * w + 24,
                        shift=(-lay.out_end) % 8, gap=8 * k)
            assert j.img_offset % 8 == 0 and j.img.pitch_bytes % 8 == 0
    return lay


@pytest.mark.parametrize("kinds", [("odd",), ("padded",), ("odd", "padded")],
                         ids=["16bit_stores", "64bit_stores", "mixed"])
def test_output_layouts(gpu, oracle, kinds):
    """a plan with any job whose rows do not start at multiples of 8 bytes runs
    sv2_recon_kernel<false> (four 16-bit stores a lane) for all its jobs, the others
    sv2_recon_kernel<true>: same pixels, and not a byte outside them"""
    _layout_plan(oracle, kinds).run(gpu)


def _rejections():
    def width(j):
        j.desc.width = 48 if j.desc.width != 48 else 32

    def flags(j):
        j.desc.optflags = 8

    def in_offset(j):
        j.in_offset += 4

    def pitch(j):
        j.img.pitch_bytes -= 2

    def img_offset(j):
        j.img_offset += 1

    return (width, flags, in_offset, pitch, img_offset)


def test_many_jobs(gpu, oracle):
    """140 jobs of one to four blocks a row (sv2_chain_kernel: one lane per job, three
    workgroups of 64): every seventh is refused by the host, every fifth is damaged and fails
    on the device, the others decode; run twice"""
    lay = Layout()
    rej = _rejections()
    for k in range(140):
        bits, w, h = (12, 14)[k & 1], 16 * (1 + k % 4), 2 + k % 5
        c = V2.value_case(V2.CLASSES[k % 4], bits, k % 8, w, h)
        data = c.data
        if k % 5 == 2:
            data = data.copy()
            if k % 10 == 2:
                data = data[:16 + (data.size - 32) // 2]
            else:
                data[16:] = np.random.default_rng([194, k]).integers(0, 256, data.size - 16)
        st, px = truth(oracle, ("many", k), bits, w, h, data)
        lay.add("job%d" % k, data, bits, w, h, st, px, gap=2 * (k % 3),
                reject=rej[(k // 7) % len(rej)] if k % 7 == 3 else None)
    counts = collections.Counter(e.status for e in lay.entries)
    assert counts[OK] >= 90 and counts[INVALID_ARG] >= 20 and len(counts) >= 3, counts
    assert lay.entries[64].status == OK and lay.entries[128].status == OK  # (lane 0 of a workgroup)
    lay.run(gpu)


def test_truncation_sweep(gpu, oracle):
    """one 48 x 6 stream cut at every length from the bare header to all of it: the status is
    the oracle's job by job -- the by-position parse's `limit` against the reference's bit
    pump at every way a stream can end"""
    bits, w, h, data = V2.sweep_stream("truncate")
    lay = Layout()
    for n in range(16, data.size + 1):
        st, px = truth(oracle, ("truncate", n), bits, w, h, data[:n].copy())
        lay.add("cut%d" % n, data[:n], bits, w, h, st, px)
    counts = lay.run(gpu, runs=1)
    print("truncation sweep, jobs per status:", dict(counts))
    assert all(counts[s] > 0 for s in (OK, INVALID_ARG, IO, INPUT_OVERFLOW)), counts


def test_bit_flip_sweep(gpu, oracle):
    """every single-bit flip of one 16 x 4 stream, the header's bits included"""
    bits, w, h, data = V2.sweep_stream("flip")
    assert data.size <= 150
    lay = Layout()
    for k in range(8 * data.size):
        d = data.copy()
        d[k >> 3] ^= 1 << (k & 7)
        st, px = truth(oracle, ("flip", k), bits, w, h, d)
        lay.add("flip%d" % k, d, bits, w, h, st, px)
    counts = lay.run(gpu, runs=1)
    print("bit-flip sweep, jobs per status:", dict(counts))
    assert counts[OK] > 0 and counts[INVALID_ARG] > 0, counts


def test_directed_verdicts(gpu, oracle):
    """every motion forced at either end of rows 0..3, and the difference-length checks, next
    to their valid neighbours (tests/test_samsung_v2_model.py: the reference says the same)"""
    lay = Layout()
    for d in V2.motion_cases() + V2.length_cases():
        st, px = truth(oracle, ("directed", d.name), d.bits, d.w, d.h, d.data)
        lay.add(d.name, d.data, d.bits, d.w, d.h, st, px)
    counts = collections.Counter(e.status for e in lay.entries)
    assert counts[OK] >= 30 and counts[INVALID_ARG] >= 40 and len(counts) == 2, counts
    lay.run(gpu, runs=1)


@pytest.mark.parametrize("in_bytes", [(1 << 29) - 16, 1 << 29], ids=["control", "2^29"])
def test_half_a_gigabyte_behind_the_frame(gpu, oracle, in_bytes):
    """A good 64 x 4 frame followed by zeros up to in_bytes: the reference decodes it (a row's
    BitStreamer sees all that is left of the strip, and never gets there).  The bound on a
    row's bit offsets, 32 * ((size + 8) / 4 + 1), was computed in 32 bits and wrapped to 96 for
    size = 2^29: the first row longer than 96 bits failed with RSX_ERR_INPUT_OVERFLOW.  It is
    saturated now (sv2_bit_limit in rsx_samsung_v2.hip; a row's offsets stay under 2^20).
    The input lives on the device only: allocated as zeros, the frame copied in."""
    bits, w, h = 14, 64, 4
    c = V2.value_case("sensor", bits, 0, w, h)
    data = np.zeros(16 + in_bytes, np.uint8)
    data[:c.data.size] = c.data
    host = HostImage(w, h)
    st = oracle.samsung_v2(bits, data, host)
    assert st == OK
    _, d, _ = open_stream(c.data, bits, w, h)
    inp = torch.zeros(in_bytes + 64, dtype=torch.uint8, device="cuda")
    inp[:c.data.size - 16] = torch.from_numpy(c.data[16:].copy()).cuda()
    out = torch.full((2 * w * h + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    plan = gpu.samsung_v2_plan([_job(d, 0, in_bytes, w, h, 0)])
    plan.run(inp.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    rc, status, _ = plan.results()
    plan.close()
    assert status == [st], (status, st)
    got = out.cpu().numpy()
    assert np.array_equal(got[:2 * w * h].view(np.uint16).reshape(h, w), host.pixels())
    assert (got[2 * w * h:] == SENTINEL).all()


def test_two_threads_share_a_context(gpu, oracle):
    """two threads, six host-pointer calls each on one context, on different frames"""
    work = []
    for t in range(2):
        items = []
        for k in range(6):
            cls, bits, optflags = V2.CLASSES[(2 * k + t) % 6], (12, 14)[(k + t) & 1], (k + 4 * t) % 8
            w, h = (256, 40) if t == 0 else (80, 40)
            c = V2.value_case(cls, bits, optflags if w == 256 else (0, 3)[k & 1], w, h)
            st, px = truth(oracle, ("value", c.cls, c.bits, c.optflags, w, h), bits, w, h, c.data)
            items.append((c, px))
        work.append(items)
    failures, barrier = [], threading.Barrier(2)

    def worker(items):
        try:
            barrier.wait()
            for c, px in items:
                st, img = decode(gpu, c.data, c.bits, c.w, c.h)
                assert st == OK
                assert np.array_equal(img.pixels(), px), (c.cls, c.bits, c.optflags)
        except BaseException as e:  # (an assertion in a thread would otherwise go unseen)
            failures.append(e)
            barrier.abort()

    ts = [threading.Thread(target=worker, args=(w,)) for w in work]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not failures, failures
