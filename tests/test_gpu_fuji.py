"""FujiDecompressor on the device (rsx_fuji_*, rawspeed_amd/csrc/rsx_fuji.hip) through the C-ABI:
every case of tests/fuji_files.py through rsx_fuji_decompress with host pointers and with device
pointers, pixels and per-strip statuses against the model (which tests/test_fuji_model.py pins
against the reference's recorded answers, tests/golden/fuji_ref.json) and the hashes of that file;
padded pitches; a plan of several frames of mixed geometry, types and verdicts in one launch; the
strips that end early with 0xFF instead of nothing behind them; a plan of more strips than are
resident at once."""
import numpy as np
import pytest
import torch

import fuji_files as F
from oracle_lib import HostImage
from rawspeed_amd import abi, capi

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in F.case_list()]


@pytest.fixture(scope="module")
def gpu():
    import gpu_util
    return gpu_util.ctx()


@pytest.fixture(scope="module")
def golden():
    return F.golden()


def _desc(data):
    st, d = capi.fuji_parse(data)
    assert st == abi.RSX_OK
    return d


def _check_padding(out):
    pad = out.buf.reshape(out.dim_y, out.pitch)[:, 2 * out.dim_x:]
    assert (pad == 0xA5).all(), "the pitch padding was written"


def _device_call(gpu, data, w, h, pitch, lead=0, behind=b""):
    """-> (status, strip statuses, (h, w) pixels); `lead` bytes in front of the container, and
    `behind` it bytes that are in the tensor and not in the call's in_bytes"""
    d = _desc(data)
    for s in range(d.n_strips):
        d.strip_offset[s] += lead
    inp = torch.from_numpy(np.frombuffer(bytes(lead) + data + behind, np.uint8).copy()).cuda()
    out = torch.full((pitch * h,), 0xA5, dtype=torch.uint8, device="cuda")
    view = abi.Image(out.data_ptr(), pitch, w, h, 1, 1)
    st, ss = gpu.fuji_decompress(d, None, view, in_ptr=inp.data_ptr(), in_bytes=lead + len(data))
    host = out.cpu().numpy().reshape(h, pitch)
    assert (host[:, 2 * w:] == 0xA5).all(), "the pitch padding was written"
    return st, ss, np.ascontiguousarray(host[:, :2 * w]).view(np.uint16)


@pytest.mark.parametrize("name", NAMES)
def test_case_host_and_device_pointers(gpu, golden, name):
    b = F.build_case(name)
    c = b["case"]
    w, h = c["width"], c["height"]
    rc, sts, px = F.expected(name)
    assert golden[name]["ok"] == (rc == F.OK)
    # host pointers: a failing frame leaves the caller's image untouched
    out = HostImage(w, h)
    st, ss = gpu.fuji_decompress(_desc(b["data"]), b["data"], out.view())
    assert (st, ss) == (rc, sts)
    if rc == F.OK:
        assert np.array_equal(out.pixels(), px), np.argwhere(out.pixels() != px)[:5]
        assert F.sha_rows(out.pixels()) == golden[name]["sha256"]
        _check_padding(out)
    else:
        assert (out.buf == 0xA5).all(), "a failed decode wrote into the caller's image"
    # device pointers: the strips that decode are written, a failing one up to its last whole line
    st, ss, got = _device_call(gpu, b["data"], w, h, (2 * w + 15) // 16 * 16, lead=name.count("1") % 4)
    assert (st, ss) == (rc, sts)
    F.check_pixels(name, got, 0xA5A5)
    if rc == F.OK:
        assert F.sha_rows(got) == golden[name]["sha256"]


@pytest.mark.parametrize("name", [next(n for n in NAMES if n.startswith(p))
                                  for p in ("x14_792x12_", "b16_1560x12_", "x16_1512x6_",
                                            "b14_1512x6_")])
@pytest.mark.parametrize("extra", [2, 16, 22])
def test_padded_pitch(gpu, name, extra):
    """pitches off and on the 16-byte grid: the narrow and the wide stores"""
    assert name in NAMES
    b = F.build_case(name)
    c = b["case"]
    w, h = c["width"], c["height"]
    rc, sts, px = F.expected(name)
    pitch = 2 * w + extra
    out = HostImage(w, h, pitch=pitch)
    st, ss = gpu.fuji_decompress(_desc(b["data"]), b["data"], out.view())
    assert (st, ss) == (F.OK, [0] * len(sts))
    assert np.array_equal(out.pixels(), px)
    _check_padding(out)
    st, ss, got = _device_call(gpu, b["data"], w, h, pitch)
    assert st == F.OK and np.array_equal(got, px)


def test_plan_of_mixed_jobs(gpu):
    """frames of both types, both depths, different geometries and verdicts in one launch: the
    good jobs intact beside the failed ones, and nothing written outside the jobs' rectangles"""
    picks = ["x14_768x6_noisy", "b16_768x6_checker", "x16_multi", "b14_plant_escape",
             "x16_768x6_saturated", "reject", "b14_768x6_steps"]
    jobs, parts, expect = [], [], []
    in_off, img_off = 5, 0
    for k, name in enumerate(picks):
        real = "b16_768x6_flat" if name == "reject" else name
        b = F.build_case(real)
        c = b["case"]
        w, h = c["width"], c["height"]
        pitch = (2 * w + 15) // 16 * 16 + 2 * k
        j = abi.FujiJob()
        j.desc = _desc(b["data"])
        if name == "reject":
            j.desc.raw_bits = 12
        j.in_offset, j.in_bytes, j.img_offset = in_off, len(b["data"]), img_off
        j.img = abi.Image(None, pitch, w, h, 1, 1)
        jobs.append(j)
        parts += [np.frombuffer(b["data"], np.uint8), np.full(3 + k, 0x5A, np.uint8)]
        expect.append((name, real, img_off, pitch, w, h))
        in_off += len(b["data"]) + 3 + k
        img_off += pitch * h + 6
    inp = torch.from_numpy(np.concatenate([np.full(5, 0x5A, np.uint8)] + parts)).cuda()
    out = torch.full((img_off,), 0xA5, dtype=torch.uint8, device="cuda")
    plan = gpu.fuji_plan(jobs)
    for _ in range(2):  # (a plan runs again)
        out.fill_(0xA5)
        plan.run(inp.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        rc, st, _ = plan.results()
        assert rc != 0
        host = out.cpu().numpy()
        covered = np.zeros(host.size, bool)
        for k, (name, real, off, pitch, w, h) in enumerate(expect):
            if name == "reject":
                assert st[k] == abi.RSX_ERR_UNSUPPORTED
                assert plan.strip_status(k, 1)[0] == abi.RSX_ERR_INVALID_ARG
                continue
            want, sts, px = F.expected(real)
            assert st[k] == want
            assert plan.strip_status(k, len(sts)) == (abi.RSX_OK, sts)
            got = np.stack([host[off + r * pitch:off + r * pitch + 2 * w].view(np.uint16)
                            for r in range(h)])
            F.check_pixels(real, got, 0xA5A5)
            for r in range(h):
                covered[off + r * pitch:off + r * pitch + 2 * w] = True
        assert (host[~covered] == 0xA5).all(), "bytes outside the jobs' rectangles were written"
    plan.close()


def test_plan_returns_the_last_failing_jobs_status(gpu):
    """Three one-strip 768 x 6 jobs: the host refuses job 0 (its strip ends behind its in_bytes),
    job 1 decodes, the strip of job 2 fails on the device with another status.  Every job gets its
    own status and results() returns job 2's, the last failing job's; the strip statuses of a
    refused job are not to be had, those of job 2 name the strip."""
    names = ["b14_768x6_flat", "x14_768x6_flat", "b14_plant_escape"]
    jobs, data, expect, out_bytes = _lay_out(names, 0x5A, lambda k: 3)
    jobs[0].in_bytes -= 1
    IO = abi.RSX_ERR_IO
    bad_st, bad_strips, _ = F.expected(names[2])
    assert bad_st not in (F.OK, IO) and bad_strips == [bad_st] and F.expected(names[1])[0] == F.OK
    inp = torch.from_numpy(data).cuda()
    out = torch.full((out_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
    plan = gpu.fuji_plan(jobs)
    plan.run(inp.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    rc, st, _ = plan.results()
    assert st == [IO, F.OK, bad_st] and rc == bad_st
    assert plan.strip_status(0, 1)[0] == abi.RSX_ERR_INVALID_ARG
    assert plan.strip_status(2, 1) == (abi.RSX_OK, bad_strips)
    plan.close()
    host = out.cpu().numpy()
    rect = np.lib.stride_tricks.as_strided
    outside = np.ones(host.size, bool)
    for name, off, pitch, w, h in expect[1:]:  # (job 1: every pixel; job 2: its whole lines)
        px = np.ascontiguousarray(rect(host[off:], (h, 2 * w), (pitch, 1))).view(np.uint16)
        F.check_pixels(name, px, 0xA5A5)
        assert name != names[1] or np.array_equal(px, F.expected(name)[2])
        rect(outside[off:], (h, 2 * w), (pitch, 1))[:] = False
    assert (host[outside] == 0xA5).all(), "bytes outside the two images were written"


def _lay_out(names, gap, gap_len, share=False):
    """the cases as jobs of one plan: every job its own image rectangle at its own pitch class;
    the inputs one behind the other with gap_len(k) bytes of `gap` between them (share: the jobs
    of one case read one copy) -> (jobs, input bytes, [(name, image offset, pitch, w, h)], output
    bytes)"""
    jobs, expect, where = [], [], {}
    parts = [np.full(5, gap, np.uint8)]
    in_off, img_off = 5, 0
    for k, name in enumerate(names):
        b = F.build_case(name)
        c = b["case"]
        w, h = c["width"], c["height"]
        pitch = (2 * w + 15) // 16 * 16 + 2 * (k % 11)
        if not (share and name in where):
            where[name] = in_off
            parts += [np.frombuffer(b["data"], np.uint8), np.full(gap_len(k), gap, np.uint8)]
            in_off += len(b["data"]) + gap_len(k)
        j = abi.FujiJob()
        j.desc = _desc(b["data"])
        j.in_offset, j.in_bytes, j.img_offset = where[name], len(b["data"]), img_off
        j.img = abi.Image(None, pitch, w, h, 1, 1)
        jobs.append(j)
        expect.append((name, img_off, pitch, w, h))
        img_off += pitch * h + 6
    return jobs, np.concatenate(parts), expect, img_off


def _check_plan(plan, st, host, expect):
    """every job's status, the strip statuses of the failing ones, every rectangle against the
    model, 0xA5 outside the rectangles"""
    covered = np.zeros(host.size, bool)
    for k, (name, off, pitch, w, h) in enumerate(expect):
        want, sts, px = F.expected(name)
        assert st[k] == want, (k, name)
        if want != F.OK:
            assert plan.strip_status(k, len(sts)) == (abi.RSX_OK, sts), (k, name)
        rows = np.lib.stride_tricks.as_strided(host[off:], (h, 2 * w), (pitch, 1))
        F.check_pixels(name, np.ascontiguousarray(rows).view(np.uint16), 0xA5A5)
        np.lib.stride_tricks.as_strided(covered[off:], (h, 2 * w), (pitch, 1))[:] = True
    assert (host[~covered] == 0xA5).all(), "bytes outside the jobs' rectangles were written"


def test_bytes_behind_a_strip_are_not_read_as_data(gpu):
    """Bytes behind a strip read as zero, whatever lies there: every strip that ends early --
    cut, 3 bytes, all zero, a zero tail that leaves the window, and those with the next strip's
    bytes behind them -- decodes as the model says with 64 bytes of 0xFF directly behind the
    container (in the tensor, outside in_bytes), and as jobs of one plan with 0xFF between the
    jobs' inputs."""
    names = [c["name"] for c in F.case_list()
             if c["fault"] and c["fault"][0] in ("cut", "cut_to", "zero", "zero_tail")]
    assert len(names) == 4 * (5 + 1 + 1 + 4 + 5)
    for k, name in enumerate(names):
        b = F.build_case(name)
        w, h = b["case"]["width"], b["case"]["height"]
        rc, sts, px = F.expected(name)
        st, ss, got = _device_call(gpu, b["data"], w, h, (2 * w + 15) // 16 * 16, lead=k % 4,
                                   behind=b"\xff" * 64)
        assert (st, ss) == (rc, sts), name
        F.check_pixels(name, got, 0xA5A5)
    jobs, data, expect, out_bytes = _lay_out(names, 0xFF, lambda k: 64 + k % 4)
    inp = torch.from_numpy(data).cuda()
    out = torch.full((out_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
    plan = gpu.fuji_plan(jobs)
    plan.run(inp.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    rc, st, _ = plan.results()
    _check_plan(plan, st, out.cpu().numpy(), expect)
    plan.close()


def test_plan_past_residency(gpu):
    """1561 strips in one launch, more than the 1280 a device of 256 CUs holds at once (five a
    CU): 97 jobs of one 16-strip frame reading one copy of its bytes, and three frames with
    failing strips at different job indices; twice."""
    good = next(n for n in NAMES if n.startswith("x14_12288x6_"))
    names = [good] * 100
    for k, tag in ((3, "b16"), (50, "x14"), (99, "b14")):
        names[k] = tag + "_multi"
    jobs, data, expect, out_bytes = _lay_out(names, 0x5A, lambda k: 3 + k % 5, share=True)
    assert sum(j.desc.n_strips for j in jobs) == 1561 > 1280
    inp = torch.from_numpy(data).cuda()
    out = torch.full((out_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
    plan = gpu.fuji_plan(jobs)
    for _ in range(2):
        out.fill_(0xA5)
        plan.run(inp.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        rc, st, _ = plan.results()
        assert rc != 0 and sum(s != 0 for s in st) == 3
        _check_plan(plan, st, out.cpu().numpy(), expect)
    plan.close()


def test_plan_timing_names_the_kernel(gpu):
    b = F.build_case("x14_768x6_flat")
    j = abi.FujiJob()
    j.desc = _desc(b["data"])
    j.in_offset, j.in_bytes, j.img_offset = 0, len(b["data"]), 0
    j.img = abi.Image(None, 2 * 768, 768, 6, 1, 1)
    inp = torch.from_numpy(np.frombuffer(b["data"], np.uint8).copy()).cuda()
    out = torch.zeros(2 * 768 * 6, dtype=torch.uint8, device="cuda")
    plan = gpu.fuji_plan([j])
    plan.set_timing(True)
    plan.run(inp.data_ptr(), out.data_ptr())
    assert plan.results()[0] == 0
    names = [n for n, _ in plan.kernel_table()[0]]
    plan.close()
    assert names == ["fuji_strip_kernel"]
    assert np.array_equal(out.cpu().numpy().view(np.uint16).reshape(6, 768),
                          F.expected("x14_768x6_flat")[2])


def test_mixed_pointers_and_strips_outside_the_input_are_refused(gpu):
    b = F.build_case("b14_768x6_flat")
    d = _desc(b["data"])
    out = HostImage(768, 6)
    inp = torch.from_numpy(np.frombuffer(b["data"], np.uint8).copy()).cuda()
    st, _ = gpu.fuji_decompress(d, None, out.view(), in_ptr=inp.data_ptr(), in_bytes=inp.numel())
    assert st == abi.RSX_ERR_INVALID_ARG
    st, _ = gpu.fuji_decompress(d, b["data"][:-1], out.view())
    assert st == abi.RSX_ERR_IO and (out.buf == 0xA5).all()
