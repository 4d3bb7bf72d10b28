"""PanasonicV5 / V6 / V7Decompressor on the device (rsx_panasonic_*, rawspeed_amd/csrc/
rsx_panasonic.hip) through the C-ABI, against the model tests/rw2_files.py (which
tests/test_panasonic_model.py pins against the reference and against recorded hashes) and, where
oracle/_ref is built, against the reference's whole-file decode of the same RW2 file."""
import threading

import numpy as np
import pytest
import torch

import rw2_files as P
from oracle_lib import HostImage, Ref
from rawspeed_amd import abi

pytestmark = pytest.mark.gpu

OK, INV = abi.RSX_OK, abi.RSX_ERR_INVALID_ARG
FILL = 0xA5


@pytest.fixture(scope="module")
def gpu():
    import gpu_util
    return gpu_util.ctx()


@pytest.fixture(scope="module")
def ref():
    return Ref() if Ref.available() else None


def _host(gpu, version, bps, data, w, h, pitch=None):
    out = HostImage(w, h, pitch=pitch)
    return gpu.panasonic_decompress(version, bps, data, out.view()), out


def _job(version, bps, w, h, in_off, in_bytes, img_off, pitch):
    j = abi.PanasonicJob()
    j.desc = abi.PanasonicDesc(version, bps)
    j.in_offset, j.in_bytes, j.img_offset = in_off, in_bytes, img_off
    j.img = abi.Image(None, pitch, w, h, 1, 1)
    return j


def _plan_case(specs, in_lead=0):
    """specs: (version, bps, w, h, bytes in front of the job's input, bytes behind it, pitch
    pad, bytes in front of the image) -> jobs, the plan's input, what to expect, output bytes"""
    jobs, parts, expect = [], [np.full(in_lead, 0x5A, np.uint8)], []
    in_off, img_off = in_lead, 0
    for k, (version, bps, w, h, lead, gap, pad, img_lead) in enumerate(specs):
        rng = np.random.default_rng([0x9A, k, version, bps, w, h])
        data = P.random_stream(rng, version, bps, w, h, zero_half=bool(k & 1))
        pitch = 2 * w + pad
        in_off += lead
        img_off += img_lead
        jobs.append(_job(version, bps, w, h, in_off, data.size + gap, img_off, pitch))
        parts += [np.full(lead, 0x5A, np.uint8), data, np.full(gap, 0x5A, np.uint8)]
        expect.append((img_off, pitch, w, h, P.model_decode(version, bps, w, h, data), data.size))
        in_off += data.size + gap
        img_off += pitch * h
    return jobs, np.concatenate(parts), expect, img_off


def _run_plan(gpu, jobs, inp, out_bytes, times=1):
    din = torch.from_numpy(inp).cuda()
    outs = []
    plan = gpu.panasonic_plan(jobs)
    for _ in range(times):
        out = torch.full((out_bytes + 64,), FILL, dtype=torch.uint8, device="cuda")
        plan.run(din.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        res = plan.results()
        outs.append((res, out.cpu().numpy()))
    plan.close()
    return outs


def _check_plan(outs, expect):
    covered = np.zeros(outs[0][1].size, bool)
    for (off, pitch, w, h, img, size) in expect:
        for r in range(h):
            covered[off + r * pitch:off + r * pitch + 2 * w] = True
    for (rc, st, cons), host in outs:
        assert rc == OK and st == [OK] * len(expect)
        assert cons == [e[5] for e in expect]
        assert (host[~covered] == FILL).all()  # nothing outside the images is written
        for (off, pitch, w, h, img, size) in expect:
            px = np.stack([host[off + r * pitch:off + r * pitch + 2 * w].view(np.uint16)
                           for r in range(h)])
            assert np.array_equal(px, img), (w, h, np.argwhere(px != img)[:4])
    assert all(np.array_equal(outs[0][1], o[1]) for o in outs)


SHAPES = [(1, 1), (1, 7), (3, 5), (41, 7), (130, 33), (668, 9), (257, 8), (1024, 3), (1025, 2)]


@pytest.mark.parametrize("version,bps", P.LAYOUTS)
def test_parity_with_the_model_and_the_reference(gpu, ref, version, bps):
    """the host-pointer call and a one-job device plan, small and odd shapes (packets a row,
    rows)"""
    n = P.PIXELS[(version, bps)]
    for k, (pw, h) in enumerate(SHAPES):
        w = n * pw
        rng = np.random.default_rng([0x70, version, bps, pw, h])
        data = P.random_stream(rng, version, bps, w, h, zero_half=bool(k & 1))
        img = P.model_decode(version, bps, w, h, data)
        st, out = _host(gpu, version, bps, data, w, h)
        assert st == OK and np.array_equal(out.pixels(), img), (w, h)
        assert (out.u16()[:, w:].view(np.uint8) == FILL).all()  # the pitch's padding
        if ref is not None:
            rst, dec = ref.decode_file(P.rw2_file(w, h, version, bps, data))
            assert rst == 0 and np.array_equal(dec.u16()[:h, :w], out.pixels())
        jobs = [_job(version, bps, w, h, 0, data.size, 0, 2 * w)]
        (res, host), = _run_plan(gpu, jobs, data, 2 * w * h)
        assert res == (OK, [OK], [P.consumed(version, bps, w, h)])
        assert np.array_equal(host[:2 * w * h].view(np.uint16).reshape(h, w), img), (w, h)
        assert (host[2 * w * h:] == FILL).all()


FULL = {(5, 12): (8320, 5640), (5, 14): (8316, 5640), (6, 12): (8316, 5640), (6, 14): (8316, 5640),
        (7, 14): (8316, 5640)}


@pytest.mark.parametrize("version,bps", P.LAYOUTS)
def test_full_size_frame(gpu, ref, version, bps):
    """about 47 MP through the host-pointer call (the RawImage's own pitch, roundUp(2 w, 16))"""
    w, h = FULL[(version, bps)]
    rng = np.random.default_rng([47, version, bps])
    data = P.random_stream(rng, version, bps, w, h, zero_half=version == 6)
    st, out = _host(gpu, version, bps, data, w, h)
    assert st == OK
    if ref is not None:
        rst, dec = ref.decode_file(P.rw2_file(w, h, version, bps, data), threads=16)
        assert rst == 0 and np.array_equal(dec.u16()[:h, :w], out.pixels())
        del dec
    img = P.model_decode(version, bps, w, h, data)
    assert np.array_equal(out.pixels(), img)
    assert (out.u16()[:, w:].view(np.uint8) == FILL).all()
    # the same frame through a device plan, rows at 2 w (not on the 16-byte grid for 8316)
    jobs = [_job(version, bps, w, h, 0, data.size, 0, 2 * w)]
    (res, host), = _run_plan(gpu, jobs, data, 2 * w * h)
    assert res == (OK, [OK], [P.consumed(version, bps, w, h)])
    assert np.array_equal(host[:2 * w * h].view(np.uint16).reshape(h, w), img)
    assert (host[2 * w * h:] == FILL).all()


@pytest.mark.parametrize("bps", [12, 14])
@pytest.mark.parametrize("packets", [1, 511, 512, 513, 1023, 1025, 2049, 3000])
def test_v5_partial_last_block(gpu, bps, packets):
    n = P.PIXELS[(5, bps)]
    rng = np.random.default_rng([5, bps, packets])
    for w, h in ((n * packets, 1), (n, packets)):
        data = P.random_stream(rng, 5, bps, w, h)
        st, out = _host(gpu, 5, bps, data, w, h)
        assert st == OK and np.array_equal(out.pixels(), P.model_decode(5, bps, w, h, data)), (w, h)


def test_input_at_every_byte_offset(gpu):
    """a job's input at the byte offsets 0 .. 17 and 0x1FF8 - 1, 0x1FF8, 0x1FF8 + 1"""
    offsets = list(range(18)) + [0x1FF7, 0x1FF8, 0x1FF9]
    for version, bps in P.LAYOUTS:
        n = P.PIXELS[(version, bps)]
        w, h = 70 * n, 17  # 1190 packets: V5 reads the wrapping packet and a partial block
        rng = np.random.default_rng([0x0F, version, bps])
        data = P.random_stream(rng, version, bps, w, h)
        img = P.model_decode(version, bps, w, h, data)
        jobs, parts, pos = [], [], 0
        for k, off in enumerate(offsets):
            start = (pos + 63) // 64 * 64 + off  # (64-byte grid + off)
            parts.append(np.full(start - pos, 0x5A, np.uint8))
            parts.append(data)
            jobs.append(_job(version, bps, w, h, start, data.size, 2 * w * h * k, 2 * w))
            pos = start + data.size
        (res, host), = _run_plan(gpu, jobs, np.concatenate(parts), 2 * w * h * len(offsets))
        assert res[0] == OK and res[2] == [data.size] * len(offsets)
        got = host[:2 * w * h * len(offsets)].view(np.uint16).reshape(len(offsets), h, w)
        for k, off in enumerate(offsets):
            assert np.array_equal(got[k], img), (version, bps, off)


def test_padded_pitches_and_image_offsets(gpu):
    """pitches and image offsets that break the 16-byte alignment of the rows (and the 4-byte
    one); the bytes around every image rectangle keep their fill"""
    specs = []
    pads = [0, 2, 4, 6, 8, 14, 16, 34]
    leads = [0, 2, 6, 16, 10, 4]
    k = 0
    for version, bps in P.LAYOUTS:
        n = P.PIXELS[(version, bps)]
        for pw, h in ((1, 9), (5, 6), (37, 5), (300, 4)):
            specs.append((version, bps, n * pw, h, k % 3, k % 2, pads[k % len(pads)],
                          leads[k % len(leads)]))
            k += 1
    jobs, inp, expect, out_bytes = _plan_case(specs, in_lead=1)
    assert {j.img.pitch_bytes % 16 for j in jobs} >= {0, 2, 4, 6, 8, 10, 12, 14}
    _check_plan(_run_plan(gpu, jobs, inp, out_bytes, times=2), expect)


def test_a_plan_mixes_versions_depths_and_geometries(gpu):
    specs = [(7, 14, 6012, 40, 0, 0, 8, 0),
             (5, 12, 6000, 33, 0, 5, 0, 0),
             (6, 14, 11, 700, 3, 0, 2, 2),
             (6, 12, 6006, 21, 0, 16, 4, 0),
             (5, 14, 8316, 9, 8, 1, 0, 6),
             (7, 14, 9, 1, 0, 0, 0, 0),
             (6, 12, 14 * 1024, 5, 1, 0, 0, 0),
             (5, 12, 10, 2051, 0, 0, 12, 0)]
    jobs, inp, expect, out_bytes = _plan_case(specs)
    outs = _run_plan(gpu, jobs, inp, out_bytes, times=2)
    _check_plan(outs, expect)
    assert outs[0][0][2] == [P.consumed(s[0], s[1], s[2], s[3]) for s in specs]


def test_a_plan_reports_an_invalid_job(gpu):
    """A job the validation refuses gets its status and consumes nothing; the others decode."""
    specs = [(7, 14, 90, 4, 0, 0, 0, 0), (6, 12, 140, 4, 0, 0, 0, 0), (5, 14, 90, 4, 0, 0, 0, 0)]
    jobs, inp, expect, out_bytes = _plan_case(specs)
    jobs[1].in_bytes -= 1  # "Insufficient count of input blocks"
    (res, host), = _run_plan(gpu, jobs, inp, out_bytes)
    rc, st, cons = res
    assert rc == INV and st == [OK, INV, OK]
    assert cons == [expect[0][5], 0, expect[2][5]]
    for k in (0, 2):
        off, pitch, w, h, img, _ = expect[k]
        assert np.array_equal(host[off:off + pitch * h].view(np.uint16).reshape(h, w), img)
    off, pitch, w, h, _, _ = expect[1]
    assert (host[off:off + pitch * h] == FILL).all()  # the refused job's image is not touched
    # a job with an odd pitch or image offset is refused as well
    jobs, inp, expect, out_bytes = _plan_case(specs)
    jobs[0].img.pitch_bytes += 1
    jobs[2].img_offset += 1
    (res, host), = _run_plan(gpu, jobs, inp, out_bytes)
    assert res[0] == INV and res[1] == [INV, OK, INV]


def test_the_host_call_rejects_what_validate_rejects(gpu):
    out = HostImage(90, 4, fill=0x3C)
    before = out.buf.copy()
    data = np.zeros(16 * 40, np.uint8)
    assert gpu.panasonic_decompress(7, 14, data[:-1], out.view()) == INV
    assert gpu.panasonic_decompress(7, 12, data, out.view()) == INV
    assert gpu.panasonic_decompress(4, 12, data, out.view()) == INV
    assert np.array_equal(out.buf, before)
    assert gpu.panasonic_decompress(7, 14, data, out.view()) == OK
    assert (out.pixels() == 0).all()


def test_consecutive_host_calls_alternate_versions(gpu):
    """Equal geometry, another version or depth: the lane's cached plan is keyed by all three
    (V5/12 and V6/12 share w = 70 k, V5/14 and V7/14 share every geometry)"""
    w, h = 630, 40  # 630 = 9 * 70 = 10 * 63 = 14 * 45
    cases = []
    for k, (version, bps) in enumerate([(5, 12), (6, 12), (5, 14), (7, 14)]):
        rng = np.random.default_rng([0xA1, k])
        data = rng.integers(0, 256, size=0x4000 * 4, dtype=np.uint8)  # (enough for each of them)
        cases.append((version, bps, data, P.model_decode(version, bps, w, h, data)))
    imgs = [c[3] for c in cases]
    assert not any(np.array_equal(imgs[a], imgs[b]) for a in range(4) for b in range(a))
    for rnd in range(3):
        for version, bps, data, img in cases + cases[::-1]:
            st, out = _host(gpu, version, bps, data, w, h)
            assert st == OK and np.array_equal(out.pixels(), img), (rnd, version, bps)


def test_two_threads_share_a_context(gpu):
    cases = []
    for t, (version, bps, w, h) in enumerate([(6, 14, 6006, 40), (5, 12, 3200, 57)]):
        rng = np.random.default_rng([11, t])
        data = P.random_stream(rng, version, bps, w, h)
        cases.append((version, bps, w, h, data, P.model_decode(version, bps, w, h, data)))
    results = [None, None]

    def work(t):
        version, bps, w, h, data, img = cases[t]
        ok = True
        for _ in range(6):
            st, out = _host(gpu, version, bps, data, w, h)
            ok &= st == OK and np.array_equal(out.pixels(), img)
        results[t] = ok

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert results == [True, True]


def test_host_calls_are_counted(gpu):
    data = np.zeros(16 * 10, np.uint8)
    before = gpu.host_calls()
    for k in range(3):
        out = HostImage(90, 1)
        assert gpu.panasonic_decompress(7, 14, data, out.view()) == OK
    out = HostImage(91, 1)
    assert gpu.panasonic_decompress(7, 14, data, out.view()) == INV  # (a refused call counts too)
    assert gpu.host_calls() == before + 4


def test_kernel_table_names_the_panasonic_kernel(gpu):
    specs = [(7, 14, 6012, 16, 0, 0, 0, 0), (6, 12, 6006, 16, 0, 0, 0, 0)]
    jobs, inp, expect, out_bytes = _plan_case(specs)
    din = torch.from_numpy(inp).cuda()
    out = torch.zeros(out_bytes, dtype=torch.uint8, device="cuda")
    plan = gpu.panasonic_plan(jobs)
    plan.set_timing(True)
    s = torch.cuda.current_stream().cuda_stream
    for _ in range(3):
        plan.run(din.data_ptr(), out.data_ptr(), s)
    rc, st, _ = plan.results()
    table, runs = plan.kernel_table()
    plan.close()
    assert rc == OK and runs == 3
    assert [n for n, _ in table] == ["panasonic_kernel"] and table[0][1] > 0
