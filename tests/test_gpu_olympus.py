"""OlympusDecompressor on the device (rsx_olympus_*, rawspeed_amd/csrc/rsx_olympus.hip) through the
C-ABI: every case of tests/olympus_files.py through rsx_olympus_decompress with device pointers
and with host pointers, and through a plan; pixels against the host build bit for bit, hashes
against the reference's recorded ones (tests/golden/olympus_ref.json), statuses identical.  The
walk writes differences into the image, so every image buffer starts as 0xA5A5 and the bytes of a
row past 2 dim_x, in front of img_offset and behind the last row must stay as they were.  Behind
every stream lie 16 bytes of 0xFF: what a walk reads behind its stream is zero, not memory."""
import numpy as np
import pytest
import torch

import olympus_files as F
from oracle_lib import HostImage
from rawspeed_amd import abi, capi

pytestmark = pytest.mark.gpu

CASES = F.case_list()
NAMES = [c["name"] for c in CASES]
GEOMETRY = [c["name"] for c in CASES if c["name"].startswith("g_")]
DENSE = [c["name"] for c in CASES if c["name"].startswith("d_")]
TRUNCATED = [c["name"] for c in CASES if c["name"].startswith("t_")]
LEAD, TAIL = 6, 10  # canary bytes around a device image
BEHIND = b"\xff" * 16  # what lies behind a stream


@pytest.fixture(scope="module")
def gpu():
    import gpu_util
    return gpu_util.ctx()


@pytest.fixture(scope="module")
def golden():
    return F.golden()


def _pitch(name, w):
    # off and on the 16-byte grid, never below 2 w
    return 2 * max(w, 0) + (0, 2, 14, 16)[len(name) % 4]


def _rows(host, off, pitch, w, h):
    return np.stack([host[off + r * pitch:off + r * pitch + 2 * w].view(np.uint16)
                     for r in range(h)])


def _check_canaries(host, rects):
    """host: the whole output buffer; rects: (offset, pitch, w, h) of the images in it"""
    covered = np.zeros(host.size, bool)
    for off, pitch, w, h in rects:
        for r in range(h):
            covered[off + r * pitch:off + r * pitch + 2 * w] = True
    assert (host[~covered] == 0xA5).all(), "bytes outside the images' rows were written"


def _device_call(gpu, data, w, h, pitch, lead_in=0):
    """-> (status, the output buffer on the host); the image lies LEAD bytes into the buffer"""
    inp = torch.from_numpy(np.frombuffer(bytes(lead_in) + data + BEHIND, np.uint8).copy()).cuda()
    out = torch.full((LEAD + pitch * max(h, 1) + TAIL,), 0xA5, dtype=torch.uint8, device="cuda")
    view = abi.Image(out.data_ptr() + LEAD, pitch, w, h, 1, 1)
    st = gpu.olympus_decompress(None, view, in_ptr=inp.data_ptr() + lead_in, in_bytes=len(data))
    torch.cuda.synchronize()
    return st, out.cpu().numpy()


@pytest.mark.parametrize("name", NAMES)
def test_case_device_and_host_pointers(gpu, golden, name):
    c = F.case(name)
    w, h = c["width"], c["height"]
    data = F.build_case(name)["data"]
    rc, px = F.host_expected(name)
    g = golden[name]
    assert g["ok"] == (rc == F.OK)
    assert capi.olympus_validate(len(data), abi.Image(None, 2 * max(w, 0), w, h, 1, 1)) == \
        F.validate(len(data), w, h)
    # device pointers, the stream at an odd address
    pitch = _pitch(name, w)
    st, host = _device_call(gpu, data, w, h, pitch, lead_in=1 + len(name) % 4)
    assert st == rc
    if rc == F.OK:
        got = _rows(host, LEAD, pitch, w, h)
        assert np.array_equal(got, px), np.argwhere(got != px)[:5]
        assert F.sha_rows(got) == g["sha256"]
        _check_canaries(host, [(LEAD, pitch, w, h)])
    elif F.validate(len(data), w, h) != F.OK:
        assert (host == 0xA5).all(), "a refused call wrote"
    else:
        # (the image behind a reader failure is unspecified; everything around it is not)
        _check_canaries(host, [(LEAD, pitch, w, h)])
    # host pointers: a failing call leaves the caller's image as it was
    if w > 0 and h > 0:
        out = HostImage(w, h, pitch=pitch)
        st = gpu.olympus_decompress(data, out.view())
        assert st == rc
        if rc == F.OK:
            assert np.array_equal(out.pixels(), px)
            assert (out.buf.reshape(h, pitch)[:, 2 * w:] == 0xA5).all()
        else:
            assert (out.buf == 0xA5).all(), "a failed decode wrote into the caller's image"


def _plan_of(gpu, names, every_alignment=False):
    """-> (plan, input tensor, output size, [(name, img_offset, pitch, w, h)]); the streams lie at
    staggered odd offsets of one input buffer (every_alignment: back to back behind gaps of 0xFF,
    job k at an offset that is k + k // 4 mod 4, so that
    every length mod 4 meets several alignments), the images at even ones of one output buffer"""
    jobs, parts, where = [], [], []
    in_off, img_off = 0, 4
    for k, name in enumerate(names):
        c = F.case(name)
        w, h = c["width"], c["height"]
        data = F.build_case(name)["data"]
        if every_alignment:
            gap = 1 + (k + k // 4 - in_off - 1) % 4
        else:
            gap = 1 + 2 * (k % 4)
            gap += (in_off + gap + 1) % 2  # (an odd in_offset)
        parts += [np.full(gap, 0xFF if every_alignment else 0x5A, np.uint8),
                  np.frombuffer(data, np.uint8)]
        in_off += gap
        pitch = _pitch(name, w) + 2 * (k % 3)
        j = abi.OlympusJob()
        assert in_off % 4 == (k + k // 4) % 4 if every_alignment else in_off % 2 == 1
        assert img_off % 2 == 0
        j.in_offset, j.in_bytes, j.img_offset = in_off, len(data), img_off
        j.img = abi.Image(None, pitch, w, h, 1, 1)
        jobs.append(j)
        where.append((name, img_off, pitch, w, h))
        in_off += len(data)
        img_off += pitch * max(h, 0) + 6 + 2 * (k % 2)
    inp = torch.from_numpy(np.concatenate(parts + [np.frombuffer(BEHIND, np.uint8)])).cuda()
    return gpu.olympus_plan(jobs), inp, img_off, where


def _run(plan, inp, out_bytes):
    out = torch.full((out_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
    plan.run(inp.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    rc, st, _ = plan.results()
    return rc, st, out.cpu().numpy()


@pytest.mark.parametrize("name", NAMES)
def test_case_through_a_plan(gpu, golden, name):
    rc, px = F.host_expected(name)
    plan, inp, n, where = _plan_of(gpu, [name])
    got_rc, st, host = _run(plan, inp, n)
    assert (got_rc, st) == (rc, [rc])
    _, off, pitch, w, h = where[0]
    if F.validate(len(F.build_case(name)["data"]), w, h) == F.OK:
        assert plan.job_status(0) == (abi.RSX_OK, rc)
        _check_canaries(host, [(off, pitch, w, h)])
    else:
        assert (host == 0xA5).all()
    if rc == F.OK:
        got = _rows(host, off, pitch, w, h)
        assert np.array_equal(got, px)
        assert F.sha_rows(got) == golden[name]["sha256"]
    plan.close()


def test_plan_of_all_geometries_at_odd_offsets(gpu, golden):
    plan, inp, n, where = _plan_of(gpu, GEOMETRY)
    rc, st, host = _run(plan, inp, n)
    assert rc == 0 and st == [0] * len(GEOMETRY)
    for name, off, pitch, w, h in where:
        got = _rows(host, off, pitch, w, h)
        assert np.array_equal(got, F.host_expected(name)[1]), name
        assert F.sha_rows(got) == golden[name]["sha256"]
    _check_canaries(host, [x[1:] for x in where])
    plan.close()


def test_plan_of_the_truncated_streams_at_every_alignment(gpu, golden):
    """the streams cut short, back to back with 0xFF between them, their first bytes at all four
    alignments: what a walk reads behind its stream's end is zero, not the gap or the next stream"""
    plan, inp, n, where = _plan_of(gpu, TRUNCATED, every_alignment=True)
    want = [F.host_expected(name)[0] for name in TRUNCATED]
    by_residue = {(len(F.build_case(name)["data"]) - F.SKIP) % 4 for name, st in zip(TRUNCATED, want)
                  if st == F.OK}
    assert by_residue == {0, 1, 2, 3} and set(want) == {F.OK, F.ERR_INPUT_OVERFLOW}
    rc, st, host = _run(plan, inp, n)
    assert st == want
    assert rc == F.ERR_INPUT_OVERFLOW
    for (name, off, pitch, w, h), status in zip(where, want):
        if status == F.OK:
            got = _rows(host, off, pitch, w, h)
            assert np.array_equal(got, F.host_expected(name)[1]), name
            assert F.sha_rows(got) == golden[name]["sha256"]
    _check_canaries(host, [x[1:] for x in where])
    plan.close()


def test_plan_of_the_dense_rows_run_twice(gpu, golden):
    """every window word in use and non-zero, four walks side by side, twice into one buffer"""
    plan, inp, n, where = _plan_of(gpu, DENSE)
    out = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
    hosts = []
    for _ in range(2):
        plan.run(inp.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        rc, st, _ = plan.results()
        assert rc == 0 and st == [0] * len(DENSE)
        hosts.append(out.cpu().numpy())
    assert np.array_equal(hosts[0], hosts[1])
    for name, off, pitch, w, h in where:
        got = _rows(hosts[1], off, pitch, w, h)
        assert np.array_equal(got, F.host_expected(name)[1]), name
        assert F.sha_rows(got) == golden[name]["sha256"]
    _check_canaries(hosts[1], [x[1:] for x in where])
    plan.close()


def test_plan_where_jobs_1_and_3_fail(gpu):
    names = ["g_130x6_noise12", "r_cut_2", "c_130x6_checker", "r_2x2_10_bytes", "g_4x130_noise12"]
    want = [F.host_expected(n)[0] for n in names]
    assert want == [F.OK, F.ERR_INPUT_OVERFLOW, F.OK, F.ERR_IO, F.OK]
    plan, inp, n, where = _plan_of(gpu, names)
    rc, st, host = _run(plan, inp, n)
    assert st == want
    assert rc == F.ERR_INPUT_OVERFLOW, "the status of the lowest-numbered failing job"
    assert [plan.job_status(k) for k in range(5)] == [(abi.RSX_OK, s) for s in want]
    for k in (0, 2, 4):
        name, off, pitch, w, h = where[k]
        assert np.array_equal(_rows(host, off, pitch, w, h), F.host_expected(name)[1]), name
    _check_canaries(host, [x[1:] for x in where])
    _, off, pitch, w, h = where[3]
    assert (_rows(host, off, pitch, w, h) == 0xA5A5).all(), "a job the host refused was written"
    plan.close()


def test_job_status_before_a_run_and_on_other_plans(gpu):
    plan, inp, n, where = _plan_of(gpu, ["g_4x4_noise12", "x_3x2"])
    assert plan.job_status(0)[0] == abi.RSX_ERR_INVALID_ARG
    assert plan.job_status(1) == (abi.RSX_OK, F.ERR_INVALID_ARG)  # (refused when the plan was made)
    assert plan.job_status(2)[0] == abi.RSX_ERR_INVALID_ARG
    rc, st, _ = _run(plan, inp, n)
    assert st == [F.OK, F.ERR_INVALID_ARG] and rc == F.ERR_INVALID_ARG
    assert plan.job_status(0) == (abi.RSX_OK, F.OK)
    plan.close()


def test_a_plan_run_twice_gives_the_same_bytes(gpu):
    """the reconstruction is in place: a second run starts from freshly parsed differences"""
    names = ["g_258x4_noise12", "g_4x258_noise12", "c_130x6_noise16"]
    plan, inp, n, where = _plan_of(gpu, names)
    out = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
    hosts = []
    for _ in range(2):
        plan.run(inp.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert plan.results()[0] == 0
        hosts.append(out.cpu().numpy())
    assert np.array_equal(hosts[0], hosts[1])
    for name, off, pitch, w, h in where:
        assert np.array_equal(_rows(hosts[1], off, pitch, w, h), F.host_expected(name)[1]), name
    plan.close()


def test_plan_timing_names_the_kernels(gpu):
    plan, inp, n, where = _plan_of(gpu, ["g_6x6_noise12"])
    plan.set_timing(True)
    out = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
    plan.run(inp.data_ptr(), out.data_ptr())
    assert plan.results()[0] == 0
    names = [k for k, _ in plan.kernel_table()[0]]
    plan.close()
    assert names == ["olympus_parse_kernel", "olympus_recon_kernel"]


def test_refusals_of_the_call(gpu):
    data = F.build_case("g_4x4_noise12")["data"]
    out = HostImage(4, 4)
    inp = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    # host and device pointers mixed
    st = gpu.olympus_decompress(None, out.view(), in_ptr=inp.data_ptr(), in_bytes=len(data))
    assert st == abi.RSX_ERR_INVALID_ARG
    # a pitch below 2 dim_x, and an odd one
    for pitch in (6, 9):
        v = out.view()
        v.pitch_bytes = pitch
        assert gpu.olympus_decompress(data, v) == abi.RSX_ERR_INVALID_ARG
    assert capi.olympus_validate(len(data), abi.Image(None, 6, 4, 4, 1, 1)) == abi.RSX_ERR_INVALID_ARG
    assert (out.buf == 0xA5).all()
    # an odd image offset in a plan
    j = abi.OlympusJob()
    j.in_offset, j.in_bytes, j.img_offset = 0, len(data), 1
    j.img = abi.Image(None, 8, 4, 4, 1, 1)
    plan = gpu.olympus_plan([j])
    assert plan.results()[1] == [abi.RSX_ERR_INVALID_ARG]
    plan.close()
