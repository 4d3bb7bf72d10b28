"""KodakDecompressor on the device (rsx_kodak_*, rawspeed_amd/csrc/rsx_kodak.hip) through the
C-ABI: every case of tests/kodak_files.py through rsx_kodak_decompress with device pointers and
with host pointers under each of the three table modes, and through plans of many jobs; pixels
against the model bit for bit, hashes against the reference's recorded ones
(tests/golden/kodak_ref.json: uncorrected = no table, corrected = the dither table), statuses
identical.  Every image buffer starts as 0xA5: the bytes of a row past 2 dim_x, in front of
img_offset and behind the last row must stay as they were, and a failing host-pointer call leaves
the whole image as it was.  Behind every stream lie 16 bytes of 0xFF that belong to nobody:
truncated and out-of-range streams are ordinary inputs whose reads the kernels bound by in_bytes."""
import numpy as np
import pytest
import torch

import kodak_files as F
from oracle_lib import HostImage
from rawspeed_amd import abi, capi

pytestmark = pytest.mark.gpu

NAMES = F.names()
MODES = (F.NONE, F.PLAIN, F.DITHER)
ROUTE = {F.NONE: "uncorrected", F.DITHER: "corrected"}
LEAD, TAIL = 6, 10  # canary bytes around a device image
BEHIND = b"\xff" * 16


@pytest.fixture(scope="module")
def gpu():
    import gpu_util
    return gpu_util.ctx()


@pytest.fixture(scope="module")
def golden():
    return F.golden()


def _pitch(name, w):
    # off and on the 16-byte grid, never below 2 w
    return 2 * w + (0, 2, 14, 16)[len(name) % 4]


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


def _check(name, mode, golden, st, got):
    """status and pixels of one decode against the model and the reference's record"""
    want_st, want = F.expected(name, mode)
    assert st == want_st
    if mode in ROUTE:
        assert golden[name][ROUTE[mode]][0] == st
    if st == F.OK:
        assert np.array_equal(got, want), np.argwhere(got != want)[:5]
        if mode in ROUTE:
            assert F.sha_rows(got) == golden[name][ROUTE[mode]][1]


@pytest.mark.parametrize("name", NAMES)
def test_case_device_and_host_pointers(gpu, golden, name):
    c, b = F.case(name), F.build_case(name)
    w, h, bps, data = c["width"], c["height"], c["bps"], b["data"]
    pitch = _pitch(name, w)
    lead_in = 1 + len(name) % 4  # (the stream at any address)
    inp = torch.from_numpy(np.frombuffer(bytes(lead_in) + data + BEHIND, np.uint8).copy()).cuda()
    for mode in MODES:
        table = F.table_for(mode, b["curve"])
        assert capi.kodak_validate(bps, mode, table, abi.Image(None, pitch, w, h, 1, 1),
                                   len(data)) == F.validate(w, h, bps, len(data), pitch)
        out = torch.full((LEAD + pitch * h + TAIL,), 0xA5, dtype=torch.uint8, device="cuda")
        view = abi.Image(out.data_ptr() + LEAD, pitch, w, h, 1, 1)
        st = gpu.kodak_decompress(bps, mode, table, None, view, in_ptr=inp.data_ptr() + lead_in,
                                  in_bytes=len(data))
        torch.cuda.synchronize()
        host = out.cpu().numpy()
        _check(name, mode, golden, st, _rows(host, LEAD, pitch, w, h))
        if F.validate(w, h, bps, len(data)) != F.OK:
            assert (host == 0xA5).all(), "a refused call wrote"
        _check_canaries(host, [(LEAD, pitch, w, h)])
        # host pointers: a failing call leaves the caller's image as it was
        img = HostImage(w, h, pitch=pitch)
        st = gpu.kodak_decompress(bps, mode, table, data, img.view())
        _check(name, mode, golden, st, img.pixels())
        if st == F.OK:
            assert (img.buf.reshape(h, pitch)[:, 2 * w:] == 0xA5).all()
        else:
            assert (img.buf == 0xA5).all(), "a failed decode wrote into the caller's image"


def _plan_of(gpu, names, mode_of=lambda k: MODES[k % 3]):
    """-> (plan, input tensor, output size, [(name, mode, img_offset, pitch, w, h)], keep-alive);
    the streams lie at staggered offsets of one input buffer with gaps of 0x5A between them, the
    images at even offsets of one output buffer"""
    jobs, parts, where, keep = [], [], [], []
    in_off, img_off = 0, 4
    for k, name in enumerate(names):
        c, b = F.case(name), F.build_case(name)
        w, h, data = c["width"], c["height"], b["data"]
        gap = 1 + k % 5
        parts += [np.full(gap, 0x5A, np.uint8), np.frombuffer(data, np.uint8)]
        in_off += gap
        pitch = _pitch(name, w) + 2 * (k % 3)
        j = abi.KodakJob()
        j.desc, arr = abi.kodak_desc(c["bps"], mode_of(k), F.table_for(mode_of(k), b["curve"]))
        keep.append(arr)
        j.in_offset, j.in_bytes, j.img_offset = in_off, len(data), img_off
        j.img = abi.Image(None, pitch, w, h, 1, 1)
        jobs.append(j)
        where.append((name, mode_of(k), img_off, pitch, w, h))
        in_off += len(data)
        img_off += pitch * h + 6 + 2 * (k % 2)
    inp = torch.from_numpy(np.concatenate(parts + [np.frombuffer(BEHIND, np.uint8)])).cuda()
    return gpu.kodak_plan(jobs), inp, img_off, where, keep


def _run(plan, inp, out_bytes):
    out = torch.full((out_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
    plan.run(inp.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    rc, st, _ = plan.results()
    return rc, st, out.cpu().numpy()


def _check_plan(golden, where, st, host):
    for (name, mode, off, pitch, w, h), status in zip(where, st):
        _check(name, mode, golden, status, _rows(host, off, pitch, w, h))
    _check_canaries(host, [x[2:] for x in where])


def test_plan_of_every_case(gpu, golden):
    """mixed geometry, depth, table mode and verdict in one plan: every job has its own status,
    and a failing job does not disturb its neighbours"""
    plan, inp, n, where, keep = _plan_of(gpu, NAMES)
    rc, st, host = _run(plan, inp, n)
    plan.close()
    want = [F.expected(name, mode)[0] for name, mode, *_ in where]
    assert st == want
    assert {F.OK, F.ERR_IO, F.ERR_VALUE_RANGE} <= set(want)
    assert rc == [s for s in want if s != F.OK][-1], "the status of the last failing job"
    _check_plan(golden, where, st, host)
    for (name, mode, off, pitch, w, h), status in zip(where, st):
        if F.validate(w, h, F.case(name)["bps"], len(F.build_case(name)["data"])) != F.OK:
            assert (_rows(host, off, pitch, w, h) == 0xA5A5).all(), "a refused job was written"


@pytest.mark.parametrize("mode", MODES)
def test_plan_of_every_case_under_one_mode(gpu, golden, mode):
    plan, inp, n, where, keep = _plan_of(gpu, NAMES[::-1], lambda k: mode)
    rc, st, host = _run(plan, inp, n)
    plan.close()
    _check_plan(golden, where, st, host)


def test_a_plan_run_twice_gives_the_same_bytes(gpu, golden):
    names = ["g_516x65", "t_read4", "g_260x130", "v_tail_high", "g_4516x3", "z_12x2", "g_12x65"]
    plan, inp, n, where, keep = _plan_of(gpu, names)
    out = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
    hosts, sts = [], []
    for _ in range(2):
        plan.run(inp.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        sts.append(plan.results()[1])
        hosts.append(out.cpu().numpy())
    plan.close()
    assert sts[0] == sts[1] == [F.expected(name, mode)[0] for name, mode, *_ in where]
    assert np.array_equal(hosts[0], hosts[1])
    _check_plan(golden, where, sts[1], hosts[1])


def test_plan_timing_names_the_map_kernels_and_the_decode_kernel(gpu):
    """the composed route ran: successor maps, the row map, its doubling, the segment starts"""
    plan, inp, n, where, keep = _plan_of(gpu, ["g_516x130"])
    plan.set_timing(True)
    out = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
    plan.run(inp.data_ptr(), out.data_ptr())
    assert plan.results()[0] == 0
    names = [k for k, _ in plan.kernel_table()[0]]
    plan.close()
    assert names == ["kodak_succ_kernel", "kodak_row_map_kernel", "kodak_row_double_kernel",
                     "kodak_seg_kernel", "kodak_decode_kernel"]


def test_the_host_pointer_call_keeps_its_plan_and_takes_each_call_s_table(gpu):
    """same geometry, size, depth and mode twice with different tables: the second call reuses the
    first one's plan and must decode through its own table"""
    name = "g_260x65"
    c, b = F.case(name), F.build_case(name)
    w, h, bps = c["width"], c["height"], c["bps"]
    for kind in ("camera", "wild", "camera"):
        cv = F.curve(kind, bps)
        img = HostImage(w, h)
        st = gpu.kodak_decompress(bps, F.DITHER, F.dither_table(cv), b["data"], img.view())
        assert st == F.OK
        assert np.array_equal(img.pixels(), F.apply_table(F.model_values(name)[1], F.DITHER, cv))


def test_refusals_of_the_call(gpu):
    name = "g_12x2"
    c, b = F.case(name), F.build_case(name)
    w, h, bps, data = c["width"], c["height"], c["bps"], b["data"]
    out = HostImage(w, h)
    inp = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    # host and device pointers mixed
    st = gpu.kodak_decompress(bps, F.NONE, None, None, out.view(), in_ptr=inp.data_ptr(),
                              in_bytes=len(data))
    assert st == abi.RSX_ERR_INVALID_ARG
    # a pitch below 2 dim_x, and an odd one
    for pitch in (2 * w - 2, 2 * w + 1):
        v = out.view()
        v.pitch_bytes = pitch
        assert gpu.kodak_decompress(bps, F.NONE, None, data, v) == abi.RSX_ERR_INVALID_ARG
    # a table mode without a table, an unknown mode, another depth
    assert gpu.kodak_decompress(bps, F.PLAIN, None, data, out.view()) == abi.RSX_ERR_INVALID_ARG
    assert gpu.kodak_decompress(bps, 3, None, data, out.view()) == abi.RSX_ERR_INVALID_ARG
    assert gpu.kodak_decompress(11, F.NONE, None, data, out.view()) == abi.RSX_ERR_INVALID_ARG
    assert (out.buf == 0xA5).all()
    # an odd image offset in a plan
    j = abi.KodakJob()
    j.desc, _ = abi.kodak_desc(bps, F.NONE)
    j.in_offset, j.in_bytes, j.img_offset = 0, len(data), 1
    j.img = abi.Image(None, 2 * w, w, h, 1, 1)
    plan = gpu.kodak_plan([j])
    assert plan.results()[1] == [abi.RSX_ERR_INVALID_ARG]
    plan.close()
