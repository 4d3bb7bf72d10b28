"""SonyArw2Decompressor on the device (rsx_sony_arw2_*, rawspeed_amd/csrc/rsx_sony_arw2.hip)
through the C-ABI, in all three table modes, against the model tests/arw2_files.py (which
tests/test_arw2_model.py pins against the reference) and, where oracle/_ref is built, against
the reference's whole-file decode of the same ARW2 file (NONE: uncorrectedRawValues; DITHER:
the curve the file carries; a PLAIN table is not reachable through a whole file)."""
import threading

import numpy as np
import pytest
import torch

import arw2_files as A
from oracle_lib import HostImage, Ref
from rawspeed_amd import abi

pytestmark = pytest.mark.gpu

OK, TILE, INV = abi.RSX_OK, abi.RSX_ERR_TILE_ERRORS, abi.RSX_ERR_INVALID_ARG
MODES = {"none": A.NONE, "plain": A.PLAIN, "dither": A.DITHER}


@pytest.fixture(scope="module")
def gpu():
    import gpu_util
    return gpu_util.ctx()


@pytest.fixture(scope="module")
def ref():
    return Ref() if Ref.available() else None


def _table(mode, points):
    curve = A.decode_curve(points)
    return {A.NONE: None, A.PLAIN: A.table_plain(curve), A.DITHER: A.table_dither(curve)}[mode]


def _host(gpu, mode, table, data, w, h, pitch=None):
    out = HostImage(w, h, pitch=pitch)
    st, rows = gpu.sony_arw2_decompress(mode, table, data, out.view())
    return st, rows, out


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("w,h", [(32, 2), (64, 6), (96, 10), (1024, 4), (6048, 8), (9600, 4),
                                 (2880, 33)])
def test_parity_with_the_model_and_the_reference(gpu, ref, mode, w, h):
    m = MODES[mode]
    rng = np.random.default_rng([0xA2, w, h, m])
    points = A.random_monotone_points(rng) if w % 64 else A.REALISTIC_CURVE
    table = _table(m, points)
    data = A.random_stream(rng, w, h)
    st, rows, out = _host(gpu, m, table, data, w, h)
    mst, img, mrows = A.model_decode(data, w, h, m, table)
    assert st == OK == mst and rows == mrows == [0] * h
    assert np.array_equal(out.pixels(), img)
    if ref is not None and m != A.PLAIN and h % 2 == 0:
        rst, dec = ref.decode_file(A.arw2_file(w, h, data, points), uncorrected=m == A.NONE)
        assert rst == 0 and np.array_equal(dec.u16()[:h, :w], out.pixels())


def test_largest_frame(gpu, ref):
    w, h = 9600, 6376
    rng = np.random.default_rng(61)
    data = A.random_stream(rng, w, h)
    table = _table(A.DITHER, A.REALISTIC_CURVE)
    st, rows, out = _host(gpu, A.DITHER, table, data, w, h)
    assert st == OK and rows == [0] * h
    _, img, _ = A.model_decode(data, w, h, A.DITHER, table)
    assert np.array_equal(out.pixels(), img)
    if ref is not None:
        rst, dec = ref.decode_file(A.arw2_file(w, h, data, A.REALISTIC_CURVE), threads=16)
        assert rst == 0 and np.array_equal(dec.u16()[:h, :w], out.pixels())


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("where", [(0, 0), (0, -1), (-1, 0), (-1, -1), (5, 7)])
def test_damaged_rows(gpu, ref, mode, where):
    """A block with imax == imin: the call fails with the reference's whole-file status, the
    row statuses name the damaged rows, and the caller's image keeps its bytes."""
    m = MODES[mode]
    w, h = 640, 12
    y, b = where[0] % h, where[1] % (w // 16)
    rng = np.random.default_rng([7, m, y, b])
    data = A.set_block(A.random_stream(rng, w, h), w, y, b, A.pack_block(700, 3, 9, 9, [5] * 14))
    data = A.set_block(data, w, (y + 3) % h, 1, A.pack_block(0, 0, 0, 0, [0] * 14))
    table = _table(m, A.REALISTIC_CURVE)
    out = HostImage(w, h, fill=0x3C)
    before = out.buf.copy()
    st, rows = gpu.sony_arw2_decompress(m, table, data, out.view())
    assert st == TILE
    assert rows == [INV if r in (y, (y + 3) % h) else OK for r in range(h)]
    assert np.array_equal(out.buf, before)
    if ref is not None and m != A.PLAIN:
        rst, _ = ref.decode_file(A.arw2_file(w, h, data, A.REALISTIC_CURVE),
                                 uncorrected=m == A.NONE)
        assert rst == st


def _plan_case(specs, in_lead=0):
    """specs: (w, h, mode, points, damaged row or None, input gap, pitch pad, image gap)"""
    jobs, keep, parts, expect = [], [], [np.full(in_lead, 0x5A, np.uint8)], []
    in_off, img_off = in_lead, 0
    for k, (w, h, mode, points, bad, gap, pad, img_gap) in enumerate(specs):
        rng = np.random.default_rng([0x3A2, k, w, h])
        data = A.random_stream(rng, w, h)
        if bad is not None:
            data = A.set_block(data, w, bad, w // 16 - 1, A.pack_block(1, 2, 4, 4, [0] * 14))
        table = _table(mode, points)
        d, arr = abi.sony_arw2_desc(mode, table)
        keep.append(arr)
        pitch = 2 * w + pad
        j = abi.SonyArw2Job()
        j.desc = d
        j.in_offset, j.in_bytes, j.img_offset = in_off, w * h + gap, img_off
        j.img = abi.Image(None, pitch, w, h, 1, 1)
        jobs.append(j)
        parts.append(data)
        parts.append(np.full(gap, 0x5A, np.uint8))  # (bytes behind the job: not read)
        _, img, _ = A.model_decode(data, w, h, mode, table)
        expect.append((img_off, pitch, w, h, img, TILE if bad is not None else OK))
        in_off += w * h + gap
        img_off += pitch * h + img_gap
    return jobs, keep, np.concatenate(parts), expect, img_off


def _run_plan(gpu, jobs, inp, out_bytes, times=1):
    din = torch.from_numpy(inp).cuda()
    outs = []
    plan = gpu.sony_arw2_plan(jobs)
    for _ in range(times):
        out = torch.full((out_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
        plan.run(din.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        res = plan.results()
        outs.append((res, out.cpu().numpy()))
    plan.close()
    return outs


def _check_plan(outs, expect, jobs):
    want_rc = TILE if any(e[5] for e in expect) else OK
    covered = np.zeros(outs[0][1].size, bool)
    for (off, pitch, w, h, img, want) in expect:
        for r in range(h):
            covered[off + r * pitch:off + r * pitch + 2 * w] = True
    for (rc, st, cons), host in outs:
        assert rc == want_rc
        assert st == [e[5] for e in expect]
        assert cons == [j.img.dim_x * j.img.dim_y for j in jobs]
        assert (host[~covered] == 0xA5).all()  # nothing outside the images is written
        for (off, pitch, w, h, img, want) in expect:
            if want:
                continue
            px = np.stack([host[off + r * pitch:off + r * pitch + 2 * w].view(np.uint16)
                           for r in range(h)])
            assert np.array_equal(px, img)
    # (every byte the kernel writes is a function of the input: a second run repeats the first)
    assert all(np.array_equal(outs[0][1], o[1]) for o in outs)


def test_input_offsets_and_padded_pitches(gpu):
    """Rows that start at every byte offset mod 16, pitches and image offsets that are not
    multiples of 16 (and not of 4)."""
    specs = []
    for k in range(16):
        w = 32 * (1 + k % 5)
        specs.append((w, 3 + k % 3, [A.NONE, A.PLAIN, A.DITHER][k % 3], A.REALISTIC_CURVE, None,
                      1, [0, 2, 4, 6, 16, 34][k % 6], [0, 2, 6, 16][k % 4]))
    jobs, keep, inp, expect, out_bytes = _plan_case(specs, in_lead=1)
    assert sorted(j.in_offset % 16 for j in jobs) == list(range(16))
    _check_plan(_run_plan(gpu, jobs, inp, out_bytes), expect, jobs)


def test_plans_mix_geometries_tables_and_damage(gpu):
    rng = np.random.default_rng(5)
    specs = [(9600, 5, A.DITHER, A.REALISTIC_CURVE, None, 0, 0, 0),
             (64, 7, A.PLAIN, A.random_monotone_points(rng), None, 3, 2, 2),
             (6048, 4, A.DITHER, A.random_monotone_points(rng), 2, 16, 16, 0),
             (32, 600, A.NONE, (0, 0, 0, 0), None, 0, 0, 6),
             (2016, 9, A.DITHER, (0, 0, 0, 0), None, 7, 4, 0),
             (480, 3, A.NONE, (0, 0, 0, 0), 0, 1, 0, 0),
             (1024, 8, A.PLAIN, A.REALISTIC_CURVE, None, 0, 0, 0)]
    jobs, keep, inp, expect, out_bytes = _plan_case(specs)
    _check_plan(_run_plan(gpu, jobs, inp, out_bytes, times=2), expect, jobs)


def test_plan_rejects_jobs_it_cannot_run(gpu):
    """A job the validation refuses gets its status and consumes nothing; the others decode."""
    specs = [(64, 4, A.DITHER, A.REALISTIC_CURVE, None, 0, 0, 0),
             (96, 4, A.NONE, (0, 0, 0, 0), None, 0, 0, 0)]
    jobs, keep, inp, expect, out_bytes = _plan_case(specs)
    jobs[1].in_bytes = 96 * 4 - 1
    outs = _run_plan(gpu, jobs, inp, out_bytes)
    (rc, st, cons), host = outs[0]
    assert st == [OK, abi.RSX_ERR_IO] and cons == [64 * 4, 0] and rc == abi.RSX_ERR_IO
    off, pitch, w, h, img, _ = expect[0]
    px = np.stack([host[off + r * pitch:off + r * pitch + 2 * w].view(np.uint16) for r in range(h)])
    assert np.array_equal(px, img)


def test_plan_returns_the_last_failing_jobs_status(gpu):
    """Three 32 x 2 jobs: the host refuses job 0 (in_bytes one short of w * h), job 1 decodes,
    row 1 of job 2 fails on the device with another status.  Every job gets its own status and
    results() returns job 2's, the last failing job's; the row statuses of a refused job are not
    to be had, those of job 2 name the row."""
    import gpu_util
    specs = [(32, 2, A.NONE, (0, 0, 0, 0), None, 0, 2, 6),
             (32, 2, A.DITHER, A.REALISTIC_CURVE, None, 0, 2, 6),
             (32, 2, A.PLAIN, A.REALISTIC_CURVE, 1, 0, 2, 6)]
    jobs, keep, inp, expect, out_bytes = _plan_case(specs)
    jobs[0].in_bytes = 32 * 2 - 1
    IO = abi.RSX_ERR_IO
    din = torch.from_numpy(inp).cuda()
    out = torch.full((out_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
    plan = gpu.sony_arw2_plan(jobs)
    plan.run(din.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    rc, st, cons = plan.results()
    assert IO != TILE and st == [IO, OK, TILE] and rc == TILE and cons == [0, 64, 64]
    assert gpu_util.plan_row_status(plan, 0, 2)[0] == INV
    assert gpu_util.plan_row_status(plan, 2, 2) == (OK, [OK, INV])
    plan.close()
    host = out.cpu().numpy()
    rect = np.lib.stride_tricks.as_strided
    off, pitch, w, h, img, _ = expect[1]
    px = np.ascontiguousarray(rect(host[off:], (h, 2 * w), (pitch, 1)))
    assert np.array_equal(px.view(np.uint16), img)
    outside = np.ones(host.size, bool)
    for off, pitch, w, h, _, _ in expect[1:]:
        rect(outside[off:], (h, 2 * w), (pitch, 1))[:] = False
    assert (host[outside] == 0xA5).all(), "bytes outside the two images were written"


def test_kernel_table_names_the_arw2_kernel(gpu):
    specs = [(6048, 16, A.DITHER, A.REALISTIC_CURVE, None, 0, 0, 0),
             (6048, 16, A.NONE, (0, 0, 0, 0), None, 0, 0, 0)]
    jobs, keep, inp, expect, out_bytes = _plan_case(specs)
    din = torch.from_numpy(inp).cuda()
    out = torch.zeros(out_bytes, dtype=torch.uint8, device="cuda")
    plan = gpu.sony_arw2_plan(jobs)
    plan.set_timing(True)
    s = torch.cuda.current_stream().cuda_stream
    for _ in range(3):
        plan.run(din.data_ptr(), out.data_ptr(), s)
    rc, st, _ = plan.results()
    table, runs = plan.kernel_table()
    plan.close()
    assert rc == OK and runs == 3
    assert [n for n, _ in table] == ["arw2_kernel"] and table[0][1] > 0


def test_consecutive_host_calls_with_different_curves(gpu):
    """Same geometry, same mode, another curve: the table is call data, not part of the
    cached plan."""
    w, h = 2048, 6
    rng = np.random.default_rng(9)
    data = A.random_stream(rng, w, h)
    for m in (A.DITHER, A.PLAIN):
        for points in (A.REALISTIC_CURVE, (0, 0, 0, 0), A.random_monotone_points(rng),
                       A.REALISTIC_CURVE):
            table = _table(m, points)
            st, rows, out = _host(gpu, m, table, data, w, h)
            _, img, _ = A.model_decode(data, w, h, m, table)
            assert st == OK and np.array_equal(out.pixels(), img), (m, points)


def test_two_threads_share_a_context(gpu):
    cases = []
    for t, (w, h, m) in enumerate([(6048, 40, A.DITHER), (3200, 57, A.PLAIN)]):
        rng = np.random.default_rng([11, t])
        data = A.random_stream(rng, w, h)
        table = _table(m, A.random_monotone_points(rng))
        cases.append((w, h, m, table, data, A.model_decode(data, w, h, m, table)[1]))
    results = [None, None]

    def work(t):
        w, h, m, table, data, img = cases[t]
        ok = True
        for _ in range(6):
            st, _, out = _host(gpu, m, table, data, w, h)
            ok &= st == OK and np.array_equal(out.pixels(), img)
        results[t] = ok

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert results == [True, True]
