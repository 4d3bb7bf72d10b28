"""PanasonicV4Decompressor on the device (rsx_panasonic_v4_*, rawspeed_amd/csrc/
rsx_panasonic_v4.hip) through the C-ABI, against the model tests/rw2_v4_files.py (which
tests/test_panasonic_v4_model.py pins against the reference and against recorded hashes) and,
where oracle/_ref is built, against the reference's whole-file decode of the same RW2 file.  The
zero-pixel list is held against the model's, which is the set of zero pixels of the image."""
import numpy as np
import pytest
import torch

import rw2_v4_files as V
from oracle_lib import HostImage, Ref
from rawspeed_amd import abi, capi

pytestmark = pytest.mark.gpu

OK, INV, UNS = abi.RSX_OK, abi.RSX_ERR_INVALID_ARG, abi.RSX_ERR_UNSUPPORTED
FILL = 0xA5
# packets a row, rows: one packet; rows of 28 bytes; 287 packets; 1170 = two blocks (a partial one
# for split 0, packet 512's wrap for 0x1FF8) and three workgroups; 2051 = two blocks and three packets
SHAPES = [(1, 1), (2, 3), (41, 7), (130, 9), (293, 7)]


@pytest.fixture(scope="module")
def gpu():
    import gpu_util
    return gpu_util.ctx()


@pytest.fixture(scope="module")
def ref():
    return Ref() if Ref.available() else None


@pytest.fixture(scope="module")
def cases():
    """(split, w, h, kind) -> (data, the model's image, the model's list), computed once"""
    out = {}
    for split in V.SPLITS:
        for pw, h in SHAPES:
            for k, kind in enumerate(V.KINDS):
                rng = np.random.default_rng([0x74, split, pw, h, k])
                w = V.N * pw
                data = V.random_stream(rng, split, w, h, kind)
                out[(split, w, h, kind)] = (data,) + V.model_decode(split, w, h, data)
    return out


def _host(gpu, split, data, w, h, zero_is_bad=1, bad_cap=None, pitch=None):
    out = HostImage(w, h, pitch=pitch)
    res = gpu.panasonic_v4_decompress(split, zero_is_bad, data, out.view(),
                                      w * h if bad_cap is None else bad_cap)
    return res, out


def _job(split, flag, w, h, in_off, in_bytes, img_off, pitch, bad_cap):
    j = abi.PanasonicV4Job()
    j.desc = abi.PanasonicV4Desc(split, flag)
    j.in_offset, j.in_bytes, j.img_offset = in_off, in_bytes, img_off
    j.img = abi.Image(None, pitch, w, h, 1, 1)
    j.bad_cap = bad_cap
    return j


@pytest.mark.parametrize("kind", V.KINDS)
@pytest.mark.parametrize("split", V.SPLITS)
def test_parity_with_the_model_and_the_reference(gpu, ref, cases, split, kind):
    """the host-pointer call: the image, the padding of its pitch, the count and the sorted list"""
    for pw, h in SHAPES:
        w = V.N * pw
        data, img, zeros = cases[(split, w, h, kind)]
        (st, n_bad, bad), out = _host(gpu, split, data, w, h)
        assert st == OK and np.array_equal(out.pixels(), img), (w, h, np.argwhere(out.pixels() != img)[:4])
        assert (out.u16()[:, w:].view(np.uint8) == FILL).all()  # the pitch's padding
        assert n_bad == len(zeros) and np.array_equal(bad, zeros), (w, h)
        if ref is not None:
            rst, dec = ref.decode_file(V.v4_file(split, w, h, data))
            assert rst == 0 and np.array_equal(dec.u16()[:h, :w], out.pixels())
            assert np.array_equal(bad, V.zero_list(dec.u16()[:h, :w]))


@pytest.mark.parametrize("split", V.SPLITS)
def test_the_list_s_capacity(gpu, cases, split):
    """exactly enough room is enough; one entry less, or none, is RSX_ERR_UNSUPPORTED with the
    image complete and the count exact; the flag off collects nothing and changes no pixel"""
    w, h = V.N * 130, 9
    data, img, zeros = cases[(split, w, h, "sparse")]
    n = len(zeros)
    assert 30 < n < w * h
    (st, n_bad, bad), out = _host(gpu, split, data, w, h, bad_cap=n)
    assert (st, n_bad) == (OK, n) and np.array_equal(bad, zeros) and np.array_equal(out.pixels(), img)
    for cap in (n - 1, 7, 0):
        (st, n_bad, bad), out = _host(gpu, split, data, w, h, bad_cap=cap)
        assert (st, n_bad, bad) == (UNS, n, None), cap
        assert np.array_equal(out.pixels(), img), cap
    (st, n_bad, bad), out = _host(gpu, split, data, w, h, zero_is_bad=0, bad_cap=0)
    assert (st, n_bad) == (OK, 0) and len(bad) == 0 and np.array_equal(out.pixels(), img)
    (st, n_bad, bad), out = _host(gpu, split, data, w, h, zero_is_bad=0, bad_cap=n)
    assert (st, n_bad) == (OK, 0) and len(bad) == 0 and np.array_equal(out.pixels(), img)
    # a frame without a zero pixel needs no room
    data = np.full(V.consumed(split, w, h), 0x11, np.uint8)
    img, zeros = V.model_decode(split, w, h, data)
    assert len(zeros) == 0
    (st, n_bad, bad), out = _host(gpu, split, data, w, h, bad_cap=0)
    assert (st, n_bad) == (OK, 0) and np.array_equal(out.pixels(), img)


@pytest.mark.parametrize("split", V.SPLITS)
def test_an_all_zero_input_lists_every_pixel(gpu, split):
    w, h = V.N * 130, 9
    data = np.zeros(V.consumed(split, w, h), np.uint8)
    (st, n_bad, bad), out = _host(gpu, split, data, w, h)
    assert st == OK and n_bad == w * h and (out.pixels() == 0).all()
    rows, cols = np.divmod(np.arange(w * h, dtype=np.uint32), w)
    assert np.array_equal(bad, rows << 16 | cols)
    (st, n_bad, bad), out = _host(gpu, split, data, w, h, bad_cap=w * h - 1)
    assert (st, n_bad) == (UNS, w * h) and (out.pixels() == 0).all()


def _plan_case(specs, in_lead=0):
    """specs: (split, flag, w, h, kind, bytes in front of the job's input, bytes behind it, pitch
    pad, the image's offset mod 16, bad_cap or None for enough) -> jobs, the plan's input, what
    to expect, output bytes"""
    jobs, parts, expect = [], [np.full(in_lead, 0x5A, np.uint8)], []
    in_off, img_off = in_lead, 0
    for k, (split, flag, w, h, kind, lead, gap, pad, img_mod, cap) in enumerate(specs):
        rng = np.random.default_rng([0x9B, k, split, w, h])
        data = V.random_stream(rng, split, w, h, kind)
        img, zeros = V.model_decode(split, w, h, data)
        if not flag:
            zeros = zeros[:0]
        cap = len(zeros) if cap is None else cap
        pitch = 2 * w + pad
        in_off += lead
        img_off += (img_mod - img_off) % 16
        jobs.append(_job(split, flag, w, h, in_off, data.size + gap, img_off, pitch, cap))
        parts += [np.full(lead, 0x5A, np.uint8), data, np.full(gap, 0x5A, np.uint8)]
        expect.append((img_off, pitch, w, h, img, data.size, zeros, cap))
        in_off += data.size + gap
        img_off += pitch * h
    return jobs, np.concatenate(parts), expect, img_off


def _run_plan(gpu, jobs, inp, out_bytes, times=1):
    din = torch.from_numpy(inp).cuda()
    outs = []
    plan = gpu.panasonic_v4_plan(jobs)
    for _ in range(times):
        out = torch.full((out_bytes + 64,), FILL, dtype=torch.uint8, device="cuda")
        plan.run(din.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        res = plan.results()
        lists = [plan.bad_pixels(k, j.bad_cap) for k, j in enumerate(jobs)]
        outs.append((res, out.cpu().numpy(), lists))
    plan.close()
    return outs


def _check_plan(outs, expect):
    covered = np.zeros(outs[0][1].size, bool)
    for (off, pitch, w, h, *_rest) in expect:
        for r in range(h):
            covered[off + r * pitch:off + r * pitch + 2 * w] = True
    want_st = [OK if len(e[6]) <= e[7] else UNS for e in expect]
    for (rc, st, cons), host, lists in outs:
        assert st == want_st and rc == ([s for s in want_st if s != OK] or [OK])[-1]
        assert cons == [e[5] for e in expect]
        assert (host[~covered] == FILL).all()  # nothing outside the images is written
        for (off, pitch, w, h, img, size, zeros, cap), (lst, n_bad, bad) in zip(expect, lists):
            px = np.stack([host[off + r * pitch:off + r * pitch + 2 * w].view(np.uint16)
                           for r in range(h)])
            assert np.array_equal(px, img), (w, h, np.argwhere(px != img)[:4])
            assert n_bad == len(zeros)
            if len(zeros) <= cap:
                assert lst == OK and np.array_equal(bad, zeros), (w, h)
            else:
                assert lst == UNS
    assert all(np.array_equal(outs[0][1], o[1]) for o in outs)


def test_padded_pitches_image_offsets_and_input_offsets(gpu):
    """pitches and image offsets that break the 16-byte alignment of the rows (w = 14: 28-byte
    rows), the image 2 and 14 bytes in, the input 1 and 8 bytes in; the bytes around every image
    rectangle keep their fill"""
    specs = []
    pads = [0, 2, 4, 6, 8, 14, 16, 34]
    img_mods = [0, 2, 14, 8, 10, 4]
    in_leads = [0, 1, 8, 3, 7, 16]
    k = 0
    for split in V.SPLITS:
        for pw, h in ((1, 9), (5, 6), (37, 5), (300, 5)):
            specs.append((split, 1, V.N * pw, h, V.KINDS[k % 3], in_leads[k % len(in_leads)], k % 2,
                          pads[k % len(pads)], img_mods[k % len(img_mods)], None))
            k += 1
    jobs, inp, expect, out_bytes = _plan_case(specs, in_lead=1)
    assert {2, 14} <= {j.img_offset % 16 for j in jobs} and {1, 8} <= {s[5] for s in specs}
    assert len({j.in_offset % 16 for j in jobs}) >= 5
    _check_plan(_run_plan(gpu, jobs, inp, out_bytes, times=2), expect)


def test_a_plan_mixes_splits_flags_and_geometries_and_runs_twice(gpu):
    """six jobs; the second run's images, counts and lists are the first's: the counters start
    from zero in every run"""
    S = V.SPLIT
    specs = [(S, 1, 14 * 130, 9, "sparse", 0, 0, 8, 0, None),
             (0, 1, 14 * 130, 9, "half", 0, 5, 0, 0, None),
             (S, 0, 14, 700, "sparse", 3, 0, 2, 2, 0),
             (0, 1, 14 * 429, 5, "sparse", 0, 16, 4, 0, 3),   # its list does not fit
             (0, 0, 14 * 41, 7, "uniform", 8, 1, 0, 6, 100),
             (S, 1, 14 * 1024, 3, "sparse", 1, 0, 0, 0, None)]
    jobs, inp, expect, out_bytes = _plan_case(specs)
    assert len(expect[3][6]) > 3 and all(len(expect[k][6]) > 0 for k in (0, 1, 5))
    outs = _run_plan(gpu, jobs, inp, out_bytes, times=2)
    _check_plan(outs, expect)
    assert outs[0][0] == outs[1][0]
    for a, b in zip(outs[0][2], outs[1][2]):
        assert a[:2] == b[:2] and (a[2] is None) == (b[2] is None)
        assert a[2] is None or np.array_equal(a[2], b[2])
    assert outs[0][0][2] == [V.consumed(s[0], s[2], s[3]) for s in specs]


def test_a_plan_reports_an_invalid_job_and_guards_the_list_call(gpu):
    specs = [(0, 1, 140, 4, "half", 0, 0, 0, 0, None), (V.SPLIT, 1, 140, 4, "half", 0, 0, 0, 0, None),
             (0, 1, 140, 4, "sparse", 0, 0, 0, 0, None)]
    jobs, inp, expect, out_bytes = _plan_case(specs)
    jobs[1].in_bytes -= 1  # peekStream
    din = torch.from_numpy(inp).cuda()
    out = torch.full((out_bytes + 64,), FILL, dtype=torch.uint8, device="cuda")
    plan = gpu.panasonic_v4_plan(jobs)
    assert plan.bad_pixels(0, 100)[0] == INV  # before a run's results
    plan.run(din.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    rc, st, cons = plan.results()
    assert rc == abi.RSX_ERR_IO and st == [OK, abi.RSX_ERR_IO, OK]
    assert cons == [expect[0][5], 0, expect[2][5]]
    host = out.cpu().numpy()
    for k in (0, 2):
        off, pitch, w, h, img, _, zeros, cap = expect[k]
        assert np.array_equal(host[off:off + pitch * h].view(np.uint16).reshape(h, w), img)
        lst, n_bad, bad = plan.bad_pixels(k, cap)
        assert lst == OK and np.array_equal(bad, zeros)
        if len(zeros):
            assert plan.bad_pixels(k, len(zeros) - 1)[:2] == (UNS, len(zeros))
    off, pitch, w, h = expect[1][:4]
    assert (host[off:off + pitch * h] == FILL).all()  # the refused job's image is not touched
    assert plan.bad_pixels(1, 100)[0] == INV and plan.bad_pixels(3, 100)[0] == INV
    assert plan.bad_pixels(-1, 100)[0] == INV
    plan.close()
    # the list call belongs to V4 plans
    other = gpu.panasonic_plan([abi.PanasonicJob(abi.PanasonicDesc(7, 14), 0, 160, 0,
                                                 abi.Image(None, 180, 90, 1, 1, 1))])
    n = capi.C.c_uint64(5)
    assert capi.lib().rsx_panasonic_v4_plan_bad_pixels(other._h, 0, None, 0, capi.C.byref(n)) == INV
    other.close()


def test_the_host_call_rejects_what_validate_rejects(gpu):
    out = HostImage(140, 4, fill=0x3C)
    before = out.buf.copy()
    data = np.zeros(16 * 40, np.uint8)
    assert gpu.panasonic_v4_decompress(0, 1, data[:-1], out.view(), 10)[0] == abi.RSX_ERR_IO
    assert gpu.panasonic_v4_decompress(V.SPLIT, 1, data, out.view(), 10)[0] == abi.RSX_ERR_IO
    assert gpu.panasonic_v4_decompress(0x2000, 1, np.zeros(0x4000, np.uint8), out.view(), 10)[0] == UNS
    assert gpu.panasonic_v4_decompress(0x4001, 1, np.zeros(0x4000, np.uint8), out.view(), 10)[0] == INV
    assert np.array_equal(out.buf, before)
    st, n_bad, bad = gpu.panasonic_v4_decompress(0, 1, data, out.view(), 560)
    assert (st, n_bad) == (OK, 560) and (out.pixels() == 0).all()
    # the entry points of section 3j keep refusing version 4
    assert capi.panasonic_validate(4, 12, out.view(), 1 << 20) == INV
    assert gpu.panasonic_decompress(4, 12, data, out.view()) == INV


def test_kernel_time_names_the_v4_kernel(gpu):
    specs = [(V.SPLIT, 1, 14 * 429, 16, "half", 0, 0, 0, 0, None), (0, 0, 14 * 429, 16, "uniform", 0, 0, 0, 0, 0)]
    jobs, inp, expect, out_bytes = _plan_case(specs)
    din = torch.from_numpy(inp).cuda()
    out = torch.zeros(out_bytes, dtype=torch.uint8, device="cuda")
    plan = gpu.panasonic_v4_plan(jobs)
    plan.set_timing(True)
    s = torch.cuda.current_stream().cuda_stream
    for _ in range(3):
        plan.run(din.data_ptr(), out.data_ptr(), s)
    rc, st, _ = plan.results()
    table, runs = plan.kernel_table()
    name, ms, n = plan.kernel_time()
    plan.close()
    assert rc == OK and runs == 3
    assert [t[0] for t in table] == ["panasonic_v4_kernel"] and table[0][1] > 0
    assert name == "panasonic_v4_kernel" and ms > 0 and n == 3
