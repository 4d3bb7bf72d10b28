"""CrwDecompressor on the device (rsx_crw_*, rawspeed_amd/csrc/rsx_crw.hip) through the C-ABI:
every case of tests/crw_files.py through rsx_crw_decompress with device pointers and with host
pointers, with and without low bits, and through plans of many jobs; pixels against the model bit
for bit, hashes against the reference's recorded ones (tests/golden/crw_ref.json holds the route
with low bits), statuses identical.  Every image buffer starts as 0xA5: the bytes of a row past
2 dim_x, in front of img_offset and behind the last row must stay as they were, and a failing
host-pointer call leaves the whole image as it was.  The streams lie at odd addresses, and behind
every stream lie 16 bytes of 0xFF that belong to nobody: a stream that ends early is an ordinary
input whose reads the kernels bound by in_bytes.  The same cases run on a context created with
RSX_CRW_SPEC_ROUNDS=0, where the settling kernel does all the work behind the first pass."""
import os

import numpy as np
import pytest
import torch

import crw_files as F
from oracle_lib import HostImage
from rawspeed_amd import abi, capi

pytestmark = pytest.mark.gpu

NAMES = F.case_names()
LEAD, TAIL = 6, 10  # canary bytes around a device image
BEHIND = b"\xff" * 16
KERNELS = ["crw_zero_kernel", "crw_count_kernel", "crw_compact_kernel", "crw_parse_kernel",
           "crw_settle_kernel", "crw_scan_kernel", "crw_write_kernel", "crw_carry_kernel",
           "crw_recon_kernel"]


@pytest.fixture(scope="module")
def gpu():
    import gpu_util
    return gpu_util.ctx()


@pytest.fixture(scope="module")
def gpu_no_rounds():
    """a context whose CRW plans run no speculative round behind the first pass"""
    os.environ["RSX_CRW_SPEC_ROUNDS"] = "0"
    try:
        ctx = capi.Context(0)
    finally:
        del os.environ["RSX_CRW_SPEC_ROUNDS"]
    return ctx


@pytest.fixture(scope="module")
def golden():
    return F.golden()["cases"]


def _pitch(name, w):
    # off and on the 16-byte grid, never below 2 w
    return 2 * w + (0, 2, 14, 16)[len(name) % 4]


def _rows(host, off, pitch, w, h):
    return np.stack([host[off + r * pitch:off + r * pitch + 2 * w].view(np.uint16)
                     for r in range(h)])


def _check_canaries(host, rects):
    covered = np.zeros(host.size, bool)
    for off, pitch, w, h in rects:
        for r in range(h):
            covered[off + r * pitch:off + r * pitch + 2 * w] = True
    assert (host[~covered] == 0xA5).all(), "bytes outside the images' rows were written"


def _check(name, lowbits, golden, st, got):
    want_st, want = F.expected(name, lowbits)
    assert st == want_st, (name, lowbits, st, want_st)
    if lowbits:
        assert golden[name]["lowbits"][0] == st
    if st == F.OK:
        assert np.array_equal(got, want), (name, lowbits, np.argwhere(got != want)[:5])
        if lowbits:
            assert F.sha_rows(got) == golden[name]["lowbits"][1]


def _both_pointers(ctx, golden, name):
    c = F.build_case(name)
    w, h, table, data, low = c["width"], c["height"], c["table"], c["data"], c["low"]
    pitch = _pitch(name, w)
    lead_in = 1 + len(name) % 4  # (the stream at any address)
    inp = torch.from_numpy(np.frombuffer(bytes(lead_in) + data + BEHIND, np.uint8).copy()).cuda()
    lowd = torch.from_numpy(np.frombuffer(bytes(3) + low + BEHIND, np.uint8).copy()).cuda()
    for lowbits in (True, False):
        assert capi.crw_validate(table, lowbits, abi.Image(None, pitch, w, h, 1, 1), len(data),
                                 len(low)) == F.validate(w, h, table, lowbits, len(low), len(data),
                                                         1, pitch)
        out = torch.full((LEAD + pitch * h + TAIL,), 0xA5, dtype=torch.uint8, device="cuda")
        view = abi.Image(out.data_ptr() + LEAD, pitch, w, h, 1, 1)
        st = ctx.crw_decompress(table, None, None, view, in_ptr=inp.data_ptr() + lead_in,
                                in_bytes=len(data),
                                low_ptr=lowd.data_ptr() + 3 if lowbits else None,
                                low_bytes=len(low) if lowbits else 0)
        torch.cuda.synchronize()
        host = out.cpu().numpy()
        _check(name, lowbits, golden, st, _rows(host, LEAD, pitch, w, h))
        if len(data) < 8:
            assert (host == 0xA5).all(), "a refused call wrote"
        _check_canaries(host, [(LEAD, pitch, w, h)])
        # host pointers: a failing call leaves the caller's image as it was
        img = HostImage(w, h, pitch=pitch)
        st = ctx.crw_decompress(table, data, low if lowbits else None, img.view())
        _check(name, lowbits, golden, st, img.pixels())
        if st == F.OK:
            assert (img.buf.reshape(h, pitch)[:, 2 * w:] == 0xA5).all()
        else:
            assert (img.buf == 0xA5).all(), "a failed decode wrote into the caller's image"


@pytest.mark.parametrize("name", NAMES)
def test_case_device_and_host_pointers(gpu, golden, name):
    _both_pointers(gpu, golden, name)


def _plan_of(ctx, names, lowbits_of=lambda k: k % 3 != 2):
    """-> (plan, input tensor, output size, [(name, lowbits, img_offset, pitch, w, h)]); the scans
    and the low bits lie at staggered offsets of one input buffer with gaps of 0x5A between them,
    the images at even offsets of one output buffer"""
    jobs, parts, where = [], [], []
    in_off, img_off = 0, 4
    for k, name in enumerate(names):
        c = F.build_case(name)
        w, h, data, low = c["width"], c["height"], c["data"], c["low"]
        j = abi.CrwJob()
        j.desc = abi.crw_desc(c["table"], lowbits_of(k))
        for what, blob in (("low", low), ("in", data)):
            gap = 1 + k % 5
            parts += [np.full(gap, 0x5A, np.uint8), np.frombuffer(blob, np.uint8)]
            in_off += gap
            setattr(j, what + "_offset", in_off)
            setattr(j, what + "_bytes", len(blob))
            in_off += len(blob)
        pitch = _pitch(name, w) + 2 * (k % 3)
        j.img_offset = img_off
        j.img = abi.Image(None, pitch, w, h, 1, 1)
        jobs.append(j)
        where.append((name, lowbits_of(k), img_off, pitch, w, h))
        img_off += pitch * h + 6 + 2 * (k % 2)
    inp = torch.from_numpy(np.concatenate(parts + [np.frombuffer(BEHIND, np.uint8)])).cuda()
    return ctx.crw_plan(jobs), inp, img_off, where


def _run(plan, inp, out_bytes):
    out = torch.full((out_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
    plan.run(inp.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    rc, st, _ = plan.results()
    return rc, st, out.cpu().numpy()


def _check_plan(golden, where, st, host):
    for (name, lowbits, off, pitch, w, h), status in zip(where, st):
        _check(name, lowbits, golden, status, _rows(host, off, pitch, w, h))
    _check_canaries(host, [x[2:] for x in where])


def _plan_of_every_case(ctx, golden):
    plan, inp, n, where = _plan_of(ctx, NAMES)
    rc, st, host = _run(plan, inp, n)
    stats = [plan.stats(k) for k in range(len(NAMES))]
    plan.close()
    want = [F.expected(name, lowbits)[0] for name, lowbits, *_ in where]
    assert st == want
    assert {F.OK, F.ERR_IO, F.ERR_BAD_CODE, F.ERR_OVERFLOW, F.ERR_VALUE_RANGE} <= set(want)
    assert rc == [s for s in want if s != F.OK][-1], "the status of the last failing job"
    _check_plan(golden, where, st, host)
    for (name, lowbits, off, pitch, w, h), status in zip(where, st):
        if status == F.ERR_IO:
            assert (_rows(host, off, pitch, w, h) == 0xA5A5).all(), "a refused job was written"
    return dict(zip(NAMES, stats))


def test_plan_of_every_case(gpu, golden):
    """mixed geometry, table, low bits and verdict in one plan: every job has its own status, and
    a failing job does not disturb its neighbours"""
    stats = _plan_of_every_case(gpu, golden)
    # the three-window noise case: at least three windows at the shipped window size, and the
    # speculative rounds suffice
    for t in range(3):
        windows, inner, outer, settle = stats["noise_1024x256_t%d" % t]
        assert windows >= 3 and settle == 0, stats["noise_1024x256_t%d" % t]
    # the stream without a 00 is exact (checked above); what it took is a finding, not a threshold
    print("nonzero_1024x256: windows, inner rounds, outer rounds, settling work =",
          stats["nonzero_1024x256"])
    print("noise_1024x256_t0:", stats["noise_1024x256_t0"])


def test_plan_of_every_case_without_speculative_rounds(gpu_no_rounds, golden):
    stats = _plan_of_every_case(gpu_no_rounds, golden)
    assert all(s[2] == 0 for s in stats.values()), "no round behind the first pass was asked for"
    # the first pass enters every window behind the first from a guess: some window of the long
    # streams needs the settling kernel
    assert stats["noise_1024x256_t0"][3] == 1 and stats["nonzero_1024x256"][3] == 1


@pytest.mark.parametrize("name", ["noise_1024x256_t1", "nonzero_1024x256", "edge_code_straddles_window",
                                  "reader_ff_across_window_edge", "reader_marker_15_into_zeros",
                                  "reader_zero_tail_15_short", "verdict_both_in_one_block"])
def test_case_without_speculative_rounds(gpu_no_rounds, golden, name):
    _both_pointers(gpu_no_rounds, golden, name)


def test_a_plan_run_twice_gives_the_same_bytes(gpu, golden):
    names = ["geom_68x16", "verdict_bad_code_middle", "noise_1024x256_t2", "reader_marker_mid_frame",
             "geom_2672x4_plus2", "verdict_carry_1024", "reader_ff_across_window_edge"]
    plan, inp, n, where = _plan_of(gpu, names)
    out = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
    hosts, sts = [], []
    for _ in range(2):
        plan.run(inp.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        sts.append(plan.results()[1])
        hosts.append(out.cpu().numpy())
    plan.close()
    assert sts[0] == sts[1] == [F.expected(name, lowbits)[0] for name, lowbits, *_ in where]
    assert np.array_equal(hosts[0], hosts[1])
    _check_plan(golden, where, sts[1], hosts[1])


def test_plan_timing_names_the_kernels_in_order(gpu, gpu_no_rounds):
    for ctx in (gpu, gpu_no_rounds):
        plan, inp, n, where = _plan_of(ctx, ["geom_68x16"])
        plan.set_timing(True)
        out = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
        plan.run(inp.data_ptr(), out.data_ptr())
        assert plan.results()[0] == 0
        names = [k for k, _ in plan.kernel_table()[0]]
        plan.close()
        assert names == KERNELS, names  # (the table folds the launches of one name into one row)


def test_refusals_of_the_call(gpu):
    name = "geom_8x8"
    c = F.build_case(name)
    w, h, data, low = c["width"], c["height"], c["data"], c["low"]
    out = HostImage(w, h)
    inp = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    lowd = torch.from_numpy(np.frombuffer(low, np.uint8).copy()).cuda()
    # host and device pointers mixed: the scan, and the low bits
    st = gpu.crw_decompress(c["table"], None, None, out.view(), in_ptr=inp.data_ptr(),
                            in_bytes=len(data))
    assert st == abi.RSX_ERR_INVALID_ARG
    dev = torch.full((2 * w * h,), 0xA5, dtype=torch.uint8, device="cuda")
    hostlow = np.frombuffer(low, np.uint8).copy()
    st = gpu.crw_decompress(c["table"], None, None, abi.Image(dev.data_ptr(), 2 * w, w, h, 1, 1),
                            in_ptr=inp.data_ptr(), in_bytes=len(data),
                            low_ptr=hostlow.ctypes.data, low_bytes=len(low))
    assert st == abi.RSX_ERR_INVALID_ARG
    del lowd
    # a pitch below 2 dim_x, and an odd one
    for pitch in (2 * w - 2, 2 * w + 1):
        v = out.view()
        v.pitch_bytes = pitch
        assert gpu.crw_decompress(c["table"], data, low, v) == abi.RSX_ERR_INVALID_ARG
    # table 3, one low-bit byte too few, fewer than 8 bytes
    assert gpu.crw_decompress(3, data, low, out.view()) == abi.RSX_ERR_INVALID_ARG
    assert gpu.crw_decompress(c["table"], data, low[:-1], out.view()) == abi.RSX_ERR_INVALID_ARG
    assert gpu.crw_decompress(c["table"], data[:7], low, out.view()) == abi.RSX_ERR_IO
    assert (out.buf == 0xA5).all()
    # an odd image offset in a plan
    j = abi.CrwJob()
    j.desc = abi.crw_desc(c["table"], False)
    j.in_offset, j.in_bytes, j.img_offset = 0, len(data), 1
    j.img = abi.Image(None, 2 * w, w, h, 1, 1)
    plan = gpu.crw_plan([j])
    assert plan.results()[1] == [abi.RSX_ERR_INVALID_ARG]
    plan.close()
