"""The unpack step: a timed launch is the same single packet as an untimed one -- the kernels
stamp their own begin and end into slots the plan owns (rsx_stamp.h), no hipEventRecord goes on
the queue.  Every kernel that takes the stamps, at the smallest shapes at which its paths can
go wrong: every case runs with timing off and on into 0xA5-filled buffers and compares the
WHOLE buffer -- padding and the bytes between the images included -- with the oracle's answer
and the runs with each other.  The timing checks are deterministic: counts, names, and sums
that cannot exceed the host's wall clock; no speed is asserted."""
import time

import numpy as np
import pytest
import torch

from rawspeed_amd import abi

import golden_cases as G
from oracle_lib import HostImage, dither_lut8

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import gpu_util
    return gpu_util.ctx()


class Layout:
    """Jobs laid out in one input and one output buffer; `want` is the expected output buffer
    (0xA5 wherever no job writes)."""

    def __init__(self, in_base=0, in_fill=0):
        self.jobs, self.chunks, self.images = [], [], []
        self.in_off, self.out_off, self.in_fill = in_base, 0, in_fill

    def add(self, job, data, want, in_gap=0):
        job.in_offset, job.img_offset = self.in_off, self.out_off
        if hasattr(job, "in_bytes"):
            job.in_bytes = data.size
        self.jobs.append(job)
        self.chunks.append((self.in_off, data))
        self.images.append((self.out_off, want.buf))
        self.in_off += data.size + in_gap
        self.out_off += want.buf.size  # (pitch * rows: a multiple of 16)

    def in_host(self):
        a = np.full(self.in_off + 64, self.in_fill, np.uint8)
        for off, data in self.chunks:
            a[off:off + data.size] = data
        return a

    def want(self):
        a = np.full(self.out_off + 32, 0xA5, np.uint8)
        for off, buf in self.images:
            a[off:off + buf.size] = buf
        return a


def u16_job(oracle, rng, w, h, bps, order, pitch=None, expect=0):
    import gpu_util
    pitch = pitch or (w * bps + 7) // 8
    data = rng.integers(0, 256, size=h * pitch, dtype=np.uint8)
    d = abi.UnpackDesc(0, 0, w, h, pitch, bps, order)
    want = HostImage(w, h, 1)
    assert oracle.unpack(d, data, want) == expect
    j = abi.UnpackJob()
    j.desc = d
    j.img = gpu_util.image_job_view(w, h, 1, want.pitch)
    return j, data, want


def equal_jobs(oracle, lay, seed, heights=(5, 5, 5)):
    rng = np.random.default_rng(seed)
    for h in heights:
        lay.add(*u16_job(oracle, rng, 40, h, 14, abi.ORDER_MSB))
    return lay


def run_off_on(plan, lay, stream=None, out_shift=0, n_launches=1, name="unpack_kernel"):
    """timing off, then on: both outputs equal the expected buffer (and so each other); the
    timed run reports its launches"""
    import gpu_util
    d_in = gpu_util.to_dev(lay.in_host())
    want = lay.want()
    outs = []
    for timing in (False, True):
        plan.set_timing(timing)
        d_out = torch.full((want.size + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        plan.run(d_in.data_ptr(), d_out.data_ptr() + out_shift, stream)
        rc, status, _ = plan.results()
        assert rc == 0 and not any(status)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        assert np.array_equal(got[out_shift:out_shift + want.size], want), "timing=%s" % timing
        assert (got[:out_shift] == 0xA5).all() and (got[out_shift + want.size:] == 0xA5).all()
        outs.append(got)
    assert np.array_equal(outs[0], outs[1])
    kt = plan.kernel_time()
    assert kt is not None and kt[0] == name and kt[2] == n_launches and kt[1] > 0, kt
    assert plan.kernel_time() is None  # nothing timed since
    plan.set_timing(False)
    return outs[0]


_STREAM = []


def cuda_stream():
    """a caller's stream: one of torch's own, not the null stream (whose handle, 0, means
    "the context's stream" to rsx_plan_run); the callers synchronise after filling buffers"""
    if not _STREAM:
        _STREAM.append(torch.cuda.Stream())
    return _STREAM[0].cuda_stream


# ---- outputs: every mapping and staging path, timing off and on ---------------------------

def test_three_equal_jobs(gpu, oracle):
    """case 1: three equal jobs in one launch"""
    lay = equal_jobs(oracle, Layout(), 1)
    run_off_on(gpu.unpack_plan(lay.jobs), lay, cuda_stream())


def test_unequal_jobs_take_the_search(gpu, oracle):
    """case 2: one job of another height (unequal block ranges under the job search)"""
    lay = equal_jobs(oracle, Layout(), 2, heights=(5, 3, 5))
    run_off_on(gpu.unpack_plan(lay.jobs), lay, cuda_stream())


def test_several_launches_in_one_plan(gpu, oracle):
    """case 3: cases 1 and 2 and an LSB job -- the six MSB jobs in one launch, the LSB job in
    another, each with slots of its own; then three equal MSB jobs next to an LSB one"""
    lay = equal_jobs(oracle, equal_jobs(oracle, Layout(), 3), 4, heights=(5, 3, 5))
    lay.add(*u16_job(oracle, np.random.default_rng(5), 40, 5, 14, abi.ORDER_LSB))
    run_off_on(gpu.unpack_plan(lay.jobs), lay, cuda_stream(), n_launches=2)
    lay = equal_jobs(oracle, Layout(), 6)
    lay.add(*u16_job(oracle, np.random.default_rng(7), 48, 2, 12, abi.ORDER_LSB))
    run_off_on(gpu.unpack_plan(lay.jobs), lay, cuda_stream(), n_launches=2)


def test_two_segments_second_off_the_16_byte_grid(gpu, oracle):
    """case 4: 8200 x 3, 12-bit LSB: 1025 groups = segments of 513 + 512; the second starts
    at byte 513 * 12 = 6156 of the row = 16 * 384 + 12, a lead of 12"""
    lay = Layout()
    lay.add(*u16_job(oracle, np.random.default_rng(8), 8200, 3, 12, abi.ORDER_LSB))
    run_off_on(gpu.unpack_plan(lay.jobs), lay, cuda_stream())


def test_unaligned_rows_and_zero_fill(gpu, oracle):
    """case 5: 100 x 4, 14-bit, pitch 175: odd row starts, and the 20-byte window of the last
    row's last lane runs past the end of the strip: bytes there read as zero, whatever follows
    in the buffer (0xFF here)"""
    lay = Layout(in_fill=0xFF)
    lay.add(*u16_job(oracle, np.random.default_rng(9), 100, 4, 14, abi.ORDER_MSB, pitch=175))
    run_off_on(gpu.unpack_plan(lay.jobs), lay, cuda_stream())


def test_input_base_not_16_byte_aligned(gpu, oracle):
    """case 6: case 1 with in_offset = 1"""
    lay = equal_jobs(oracle, Layout(in_base=1), 11)
    assert lay.jobs[0].in_offset == 1
    run_off_on(gpu.unpack_plan(lay.jobs), lay, cuda_stream())


def test_output_base_off_by_two_then_aligned(gpu, oracle):
    """case 7: the output base 2 bytes off the grid (per-sample stores), then the same plan
    on an aligned base (the alignment flags are uploaded again), then off again"""
    lay = equal_jobs(oracle, Layout(), 12)
    plan = gpu.unpack_plan(lay.jobs)
    a = run_off_on(plan, lay, cuda_stream(), out_shift=2)
    b = run_off_on(plan, lay, cuda_stream(), out_shift=0)
    c = run_off_on(plan, lay, cuda_stream(), out_shift=2)
    assert np.array_equal(a, c) and np.array_equal(a[2:], b[:-2])


@pytest.mark.parametrize("bps", [8, 16])
def test_whole_byte_samples_direct_path(gpu, oracle, bps):
    """case 8: bps 8 and 16 load their groups straight from memory (no LDS image): every
    order, equal jobs, a partial last group, two segments"""
    for order in range(4):
        rng = np.random.default_rng([13, bps, order])
        lay = Layout()
        for _ in range(2):
            lay.add(*u16_job(oracle, rng, 44, 3, bps, order), in_gap=3)
        run_off_on(gpu.unpack_plan(lay.jobs), lay, cuda_stream())
    lay = Layout()
    lay.add(*u16_job(oracle, np.random.default_rng([14, bps]), 8200, 2, bps, abi.ORDER_MSB))
    run_off_on(gpu.unpack_plan(lay.jobs), lay, cuda_stream())


@pytest.mark.parametrize("w", [33, 36])
@pytest.mark.parametrize("order", range(4))
def test_all_bit_orders_bps_10(gpu, oracle, order, w):
    """case 9: every bit order at bps 10, three rows.  33 samples are 330 bits, not whole
    bytes: the reference refuses such a row (UncompressedDecompressor.cpp:145-149), and so do
    the oracle and the plan, which writes nothing.  36 is the nearest width it accepts that
    still ends in a partial group (4 samples) on odd-length rows (45 bytes)."""
    import gpu_util
    rng = np.random.default_rng([15, order, w])
    if w == 36:
        lay = Layout()
        lay.add(*u16_job(oracle, rng, w, 3, 10, order))
        run_off_on(gpu.unpack_plan(lay.jobs), lay, cuda_stream())
        return
    lay = Layout()
    lay.add(*u16_job(oracle, rng, w, 3, 10, order, expect=abi.RSX_ERR_INVALID_ARG))
    plan = gpu.unpack_plan(lay.jobs)
    d_in = gpu_util.to_dev(lay.in_host())
    for timing in (False, True):
        plan.set_timing(timing)
        d_out = torch.full((lay.want().size,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        plan.run(d_in.data_ptr(), d_out.data_ptr(), cuda_stream())
        rc, status, _ = plan.results()
        assert rc == abi.RSX_ERR_INVALID_ARG and status == [abi.RSX_ERR_INVALID_ARG]
        assert np.array_equal(d_out.cpu().numpy(), lay.want())  # (the oracle wrote nothing either)
    assert plan.kernel_time() is None  # no launch, nothing timed


def variant_job(oracle, rng, variant, big, w, h, lut=None):
    import gpu_util
    d = abi.UnpackVariantDesc(variant, big, w, h)
    if lut is not None:
        d.set_lut(lut)
    bpl = w if variant == abi.UNPACK_8BIT_LOOKUP else G.variant_bpl(variant, w)
    data = rng.integers(0, 256, size=bpl * h, dtype=np.uint8)
    want = HostImage(w, h, 1)
    assert oracle.unpack_variant(d, data, want) == 0
    j = abi.UnpackVariantJob()
    j.desc = d
    j.img = gpu_util.image_job_view(w, h, 1, want.pitch)
    return j, data, want


@pytest.mark.parametrize("big", [0, 1])
def test_control_kernel(gpu, oracle, big):
    """case 10a: decode12BitRawWithControl, both endiannesses: two equal jobs, then unequal
    ones; 2570 pixels are 257 units = two segments"""
    rng = np.random.default_rng([16, big])
    for heights in ((3, 3), (3, 2)):
        lay = Layout()
        for h in heights:
            lay.add(*variant_job(oracle, rng, abi.UNPACK_12BIT_WITH_CONTROL, big, 2570, h), in_gap=5)
        run_off_on(gpu.unpack_variant_plan(lay.jobs), lay, cuda_stream(),
                   name="unpack_control_kernel")


def test_lut8_variant(gpu, oracle):
    """case 10c: decode8BitRaw<false>: two equal jobs with tables of their own (the tables
    sit behind the job array), then unequal ones"""
    rng = np.random.default_rng(17)
    for heights in ((3, 3), (3, 4)):
        lay = Layout()
        for h in heights:
            curve = np.sort(rng.integers(0, 65536, size=256)).astype(np.uint16)
            lay.add(*variant_job(oracle, rng, abi.UNPACK_8BIT_LOOKUP, 0, 44, h,
                                 lut=dither_lut8(curve)), in_gap=1)
        run_off_on(gpu.unpack_variant_plan(lay.jobs), lay, cuda_stream())


@pytest.mark.parametrize("bps,order", [(16, 0), (16, 1), (24, 0), (24, 1), (32, 0)])
def test_fp_kernel(gpu, oracle, bps, order):
    """case 10b: F32 images of 16, 24 and 32 bits: equal jobs and unequal ones; 1030 samples
    are 258 groups of 4 = two segments, the last group partial (lanes past the row leave the
    kernel early: the exit stamp is taken on that way out too)"""
    import gpu_util
    rng = np.random.default_rng([18, bps, order])
    for heights in ((2, 2), (2, 3)):
        lay = Layout()
        for h in heights:
            w = 1030
            pitch = w * bps // 8 + 3
            data = rng.integers(0, 256, size=h * pitch, dtype=np.uint8)
            d = abi.UnpackDesc(0, 0, w, h, pitch, bps, order)
            want = HostImage(w, h, 1, bpc=4)
            assert oracle.unpack_f32(d, data, want) == 0
            j = abi.UnpackJob()
            j.desc = d
            j.img = gpu_util.image_job_view(w, h, 1, want.pitch)
            lay.add(j, data, want, in_gap=2)
        run_off_on(gpu.unpack_f32_plan(lay.jobs), lay, cuda_stream())


def sraw_job(oracle, name):
    import gpu_util
    c = next(c for c in G.SRAW_CASES if c["name"] == name)
    d, px, (iw, ih), (ow, oh) = G.build_sraw(c)
    src = HostImage(iw, ih, 1, is_cfa=False)
    src.pixels()[:] = px
    want = HostImage(ow, oh, 3, is_cfa=False)
    assert oracle.sraw(d, src, want) == 0
    j = abi.SrawJob()
    j.desc = d
    j.in_ = gpu_util.image_job_view(iw, ih, 1, src.pitch, is_cfa=False)
    j.img = gpu_util.image_job_view(ow, oh, 3, want.pitch, is_cfa=False)
    return j, src.buf, want


@pytest.mark.parametrize("names", [("422_v2",), ("422_v1", "420_v2_two_groups")],
                         ids=["smallest", "two_versions"])
def test_sraw_plan(gpu, oracle, names):
    """case 11: the smallest sRaw plan of the golden cases (2 groups x 3 rows); and a plan of
    two versions, which is two kernels folding into the slots of one launch"""
    lay = Layout()
    for n in names:
        lay.add(*sraw_job(oracle, n))
    run_off_on(gpu.sraw_plan(lay.jobs), lay, cuda_stream(), name="sraw_kernel")


# ---- timing behaviour ---------------------------------------------------------------------

def timed_runs(plan, d_in, d_out, n, stream):
    """n runs; (kernel_time() answer, host seconds from before the first enqueue to after the
    stream has drained)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        plan.run(d_in.data_ptr(), d_out.data_ptr(), stream)
    torch.cuda.synchronize()
    return plan.kernel_time(), time.perf_counter() - t0


@pytest.mark.parametrize("own_stream", [False, True], ids=["caller_stream", "stream_none"])
def test_timed_runs_count_and_bound(gpu, oracle, own_stream):
    """n timed runs report n launches of the right kernel; every average is positive, and
    n x average <= host wall clock around them (sequential kernels on one stream cannot sum to
    more: garbage timestamps fail this without a tolerance).  Past the 64 sets of slots a
    plan has, launches go untimed.  On a caller's stream and on the context's own (stream=None)."""
    import gpu_util
    lay = equal_jobs(oracle, Layout(), 20)
    plan = gpu.unpack_plan(lay.jobs)
    d_in = gpu_util.to_dev(lay.in_host())
    want = lay.want()
    d_out = torch.full((want.size,), 0xA5, dtype=torch.uint8, device="cuda")
    stream = None if own_stream else cuda_stream()
    plan.set_timing(True)
    for n in (1, 5, 70):
        kt, wall = timed_runs(plan, d_in, d_out, n, stream)
        assert kt is not None, n
        name, avg_ms, launches = kt
        assert name == "unpack_kernel" and launches == min(n, 64)
        assert 0 < avg_ms and launches * avg_ms * 1e-3 <= wall, (n, avg_ms, wall)
        assert plan.kernel_time() is None  # read out: nothing timed until the next run
    assert plan.results()[0] == 0
    assert np.array_equal(d_out.cpu().numpy(), want)


def test_timing_toggled_off_on_off(gpu, oracle):
    """the same outputs whichever way the launches go out; untimed runs leave nothing to
    read, and set_timing() drops what was timed before it"""
    import gpu_util
    lay = equal_jobs(oracle, Layout(), 21, heights=(5, 3, 5))
    lay.add(*u16_job(oracle, np.random.default_rng(22), 40, 5, 14, abi.ORDER_LSB))
    plan = gpu.unpack_plan(lay.jobs)
    d_in = gpu_util.to_dev(lay.in_host())
    want = lay.want()
    for timing in (False, True, False):
        plan.set_timing(timing)
        d_out = torch.full((want.size,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        plan.run(d_in.data_ptr(), d_out.data_ptr(), cuda_stream())
        assert plan.results()[0] == 0
        assert np.array_equal(d_out.cpu().numpy(), want), timing
    assert plan.kernel_time() is None
    plan.set_timing(True)
    assert plan.kernel_time() is None
    plan.run(d_in.data_ptr(), d_out.data_ptr(), cuda_stream())
    plan.set_timing(True)
    assert plan.kernel_time() is None


def test_two_plans_timed_alternately(gpu, oracle):
    """two plans on one stream, runs interleaved: each counts its own launches only, and the
    two sums together stay within the wall clock"""
    import gpu_util
    lay_a = equal_jobs(oracle, Layout(), 23)
    lay_b = Layout()
    lay_b.add(*u16_job(oracle, np.random.default_rng(24), 8200, 3, 12, abi.ORDER_LSB))
    plans, bufs = [], []
    for lay in (lay_a, lay_b):
        plans.append(gpu.unpack_plan(lay.jobs))
        bufs.append((gpu_util.to_dev(lay.in_host()),
                     torch.full((lay.want().size,), 0xA5, dtype=torch.uint8, device="cuda")))
        plans[-1].set_timing(True)
    s = cuda_stream()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(7):
        for p, (d_in, d_out) in list(zip(plans, bufs))[:2 if k < 4 else 1]:
            p.run(d_in.data_ptr(), d_out.data_ptr(), s)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    kt_a, kt_b = plans[0].kernel_time(), plans[1].kernel_time()
    assert kt_a[2] == 7 and kt_b[2] == 4
    assert kt_a[1] > 0 and kt_b[1] > 0
    assert (kt_a[1] * kt_a[2] + kt_b[1] * kt_b[2]) * 1e-3 <= wall
    for lay, (_, d_out) in zip((lay_a, lay_b), bufs):
        assert np.array_equal(d_out.cpu().numpy(), lay.want())
