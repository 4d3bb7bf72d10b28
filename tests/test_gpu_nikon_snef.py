"""NefDecoder::DecodeNikonSNef on the device (rsx_nikon_snef_*, rawspeed_amd/csrc/
rsx_nikon_snef.hip) through the C-ABI -- the host-pointer call and plans -- against the model
tests/snef_files.py (which tests/test_snef_model.py pins against the reference's whole-file
decode) and against tests/golden/snef_ref.json, the reference's recorded curve and images."""
import numpy as np
import pytest
import torch

import snef_files as S
from oracle_lib import HostImage
from rawspeed_amd import abi

pytestmark = pytest.mark.gpu

OK, INV, IO = abi.RSX_OK, abi.RSX_ERR_INVALID_ARG, abi.RSX_ERR_IO
WIDTHS = [6, 8, 10, 22, 66, 170, 1026, 3680]  # every w / 2 mod 4; one round, two rounds, two items
WBS = [(S.INV_WB_MIN, S.INV_WB_MAX), (S.INV_WB_MAX, S.INV_WB_MIN), (512, 682), (1000, 333)]


@pytest.fixture(scope="module")
def gpu():
    import gpu_util
    return gpu_util.ctx()


@pytest.fixture(scope="module")
def golden():
    curve, cases = S.load_golden()
    return S.host_table(curve), cases


def _host(gpu, wb, table, data, w, h, pitch=None):
    out = HostImage(w, h, cpp=3, is_cfa=False, pitch=pitch)
    st = gpu.nikon_snef_decompress(wb, table, data, out.view())
    return st, out


def _padding_kept(out):
    return (out.buf.reshape(out.dim_y, out.pitch)[:, 6 * out.dim_x:] == 0xA5).all()


def _data(rng, w, h, zero_seed_row=None):
    data = rng.integers(0, 256, 3 * w * h, dtype=np.uint8)
    for k in range(6):  # the clamps of all six expressions, last group included
        S.set_group(data, w, k % h, (w // 2 - 1 - k) % (w // 2), *S.CLAMP_GROUPS[k])
    if zero_seed_row is not None:
        data[3 * w * zero_seed_row:3 * w * zero_seed_row + 3] = 0
    return data


@pytest.mark.parametrize("h", [1, 2, 3])
@pytest.mark.parametrize("w", WIDTHS)
def test_host_call_matches_the_model(gpu, golden, w, h):
    rng = np.random.default_rng([0x5E, w, h])
    table = golden[0] if (w // 2 + h) % 2 else S.arbitrary_table(rng)
    wb = WBS[(w // 2 + h) % 4]
    data = _data(rng, w, h, zero_seed_row=h - 1 if w % 4 == 2 else None)
    pitch = None if h != 2 else 6 * w + [2, 4, 10, 16][(w // 2) % 4]  # (also off the 4- and 16-byte grid)
    st, out = _host(gpu, wb, table, data, w, h, pitch)
    assert st == OK
    assert np.array_equal(out.pixels(), S.model_decode(data, w, h, wb[0], wb[1], table))
    assert _padding_kept(out)


def test_tall_narrow_image(gpu, golden):
    w, h = 16, S.MAX_H
    rng = np.random.default_rng(16)
    data = _data(rng, w, h, zero_seed_row=1234)
    st, out = _host(gpu, WBS[2], golden[0], data, w, h)
    assert st == OK
    assert np.array_equal(out.pixels(), S.model_decode(data, w, h, WBS[2][0], WBS[2][1], golden[0]))


def test_recorded_reference_images(gpu, golden):
    """the reference's own answers (SHA-256), with the curve the reference agreed with"""
    table, cases = golden
    for name, w, h, wb_r, wb_b, data in S.golden_cases():
        c = cases[name]
        st, out = _host(gpu, c["inv_wb"], table, data, w, h)
        assert st == OK and S.sha(out.pixels()) == c["image"], name
        assert _padding_kept(out)


def test_planted_fma_pairs_decode_to_the_unfused_values(gpu, golden):
    """34 chroma pairs x 7 luma values at which fused operations change the green value
    (tests/test_snef_model.py: test_planted_pairs_tell_fused_from_unfused)"""
    w, h, data = S.fma_case()
    table = np.zeros(8192, np.uint16)
    table[0::2] = np.arange(4096) * 8  # base 8 v, delta 0: the stored green is 8 v
    st, out = _host(gpu, WBS[2], table, data, w, h)
    assert st == OK
    v = S.model_values(data, w, h)
    assert np.array_equal(out.pixels()[:, 1::3], 8 * v[:, 1::3])
    # the issue's two examples
    d = np.zeros(3 * 6, np.uint8)
    S.set_group(d, 6, 0, 0, 2047, 0, 396, 3764)
    S.set_group(d, 6, 0, 2, 2047, 0, 3011, 3469)
    st, out = _host(gpu, WBS[2], table, d, 6, 1)
    assert st == OK and out.pixels()[0, 1] == 8 * 1406 and out.pixels()[0, 13] == 8 * 730


def test_arbitrary_table_wraps_modulo_2_16_and_both_clamps_bite(gpu):
    rng = np.random.default_rng(77)
    w, h = 170, 3
    table = S.arbitrary_table(rng)
    data = _data(rng, w, h)
    v = S.model_values(data, w, h).astype(np.int64)
    r = S.states_by_jump(S.row_seeds(data, w, h), 3 * w)
    t = table.astype(np.int64)
    raw = t[2 * v] + ((t[2 * v + 1] * (r & 2047) + 1024) >> 12)
    assert (raw > 65535).any()  # base + dither passes 65535 somewhere: the store is modulo 2^16
    wb = (S.INV_WB_MAX, S.INV_WB_MAX)
    want = S.model_decode(data, w, h, wb[0], wb[1], table)
    assert (want[:, 0::3] == 32767).any() and (want[:, 2::3] == 32767).any()
    assert (want[:, 0::3] < 32767).any() and (want[:, 2::3] < 32767).any()
    st, out = _host(gpu, wb, table, data, w, h)
    assert st == OK and np.array_equal(out.pixels(), want)


def test_seed_zero_rows(gpu, golden):
    w, h = 66, 3
    rng = np.random.default_rng(8)
    data = rng.integers(0, 256, 3 * w * h, dtype=np.uint8)
    for y in range(h):
        data[3 * w * y:3 * w * y + 3] = 0
    assert not S.states_by_jump(S.row_seeds(data, w, h), 3 * w).any()
    table = S.arbitrary_table(rng)
    st, out = _host(gpu, WBS[3], table, data, w, h)
    assert st == OK and np.array_equal(out.pixels(), S.model_decode(data, w, h, WBS[3][0], WBS[3][1], table))


def test_consecutive_host_calls_with_other_tables_and_white_balances(gpu, golden):
    """same geometry: the table is call data, the white balance part of the cached plan's key"""
    w, h = 1026, 2
    rng = np.random.default_rng(9)
    data = _data(rng, w, h)
    tables = [golden[0], S.arbitrary_table(rng), golden[0], S.arbitrary_table(rng)]
    for k, table in enumerate(tables + tables):
        wb = WBS[2] if k < 4 else WBS[k % 4]
        st, out = _host(gpu, wb, table, data, w, h)
        assert st == OK and np.array_equal(out.pixels(), S.model_decode(data, w, h, wb[0], wb[1], table)), k


def test_host_call_rejections_leave_the_image_alone(gpu, golden):
    data = np.zeros(3 * 8 * 2, np.uint8)
    for wb, w, n, want in (((101, 512), 8, 48, INV), ((512, 512), 8, 47, IO), ((512, 512), 4, 24, IO)):
        out = HostImage(w, 2, cpp=3, is_cfa=False)
        a = np.zeros(n, np.uint8)
        assert gpu.nikon_snef_decompress(wb, golden[0], a, out.view()) == want
        assert (out.buf == 0xA5).all()
    out = HostImage(8, 2, cpp=1)
    assert gpu.nikon_snef_decompress((512, 512), golden[0], data, out.view()) == INV


# ---------------------------------------------------------------------------- plans
def _plan_case(specs, tables, in_lead=0):
    """specs: (w, h, table index, white balance, input gap, pitch pad, image gap)"""
    jobs, keep, parts, expect = [], [], [np.full(in_lead, 0x5A, np.uint8)], []
    in_off, img_off = in_lead, 0
    for k, (w, h, ti, wb, gap, pad, img_gap) in enumerate(specs):
        rng = np.random.default_rng([0x3EF, k, w, h])
        data = _data(rng, w, h, zero_seed_row=0 if k % 3 == 0 else None)
        d, arr = abi.nikon_snef_desc(wb[0], wb[1], tables[ti])
        keep.append(arr)
        pitch = 6 * w + pad
        j = abi.NikonSnefJob()
        j.desc = d
        j.in_offset, j.in_bytes, j.img_offset = in_off, 3 * w * h + gap, img_off
        j.img = abi.Image(None, pitch, w, h, 3, 0)
        jobs.append(j)
        parts.append(data)
        parts.append(np.full(gap, 0x5A, np.uint8))  # (bytes between jobs that belong to nobody)
        expect.append((img_off, pitch, w, h, S.model_decode(data, w, h, wb[0], wb[1], tables[ti])))
        in_off += 3 * w * h + gap
        img_off += pitch * h + img_gap
    return jobs, keep, np.concatenate(parts), expect, img_off


def _run_plan(gpu, jobs, inp, out_bytes, times=1):
    din = torch.from_numpy(inp).cuda()
    outs = []
    plan = gpu.nikon_snef_plan(jobs)
    for _ in range(times):
        out = torch.full((out_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
        plan.run(din.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        res = plan.results()
        outs.append((res, out.cpu().numpy()))
    plan.close()
    return outs


def _check_plan(outs, expect, jobs):
    covered = np.zeros(outs[0][1].size, bool)
    for (off, pitch, w, h, img) in expect:
        for r in range(h):
            covered[off + r * pitch:off + r * pitch + 6 * w] = True
    for (rc, st, cons), host in outs:
        assert rc == OK and st == [OK] * len(jobs)
        assert cons == [3 * j.img.dim_x * j.img.dim_y for j in jobs]
        assert (host[~covered] == 0xA5).all()  # pitch padding and everything outside the images
        for (off, pitch, w, h, img) in expect:
            px = np.stack([host[off + r * pitch:off + r * pitch + 6 * w].view(np.uint16)
                           for r in range(h)])
            assert np.array_equal(px, img), (w, h)
    assert all(np.array_equal(outs[0][1], o[1]) for o in outs)  # a second run repeats the first


def test_plan_every_width_and_height(gpu, golden):
    """every shape of the host test in one plan, at odd and even input offsets, with padded
    pitches and image offsets on and off the 4- and 16-byte grids"""
    rng = np.random.default_rng(21)
    tables = [golden[0], S.arbitrary_table(rng)]
    specs = []
    for k, (w, h) in enumerate([(w, h) for w in WIDTHS for h in (1, 2, 3)]):
        specs.append((w, h, k % 2, WBS[k % 4], [1, 0, 3, 2, 7][k % 5], [0, 2, 4, 10, 16][k % 5],
                      [0, 2, 6, 16][k % 4]))
    jobs, keep, inp, expect, out_bytes = _plan_case(specs, tables, in_lead=1)
    assert {j.in_offset % 4 for j in jobs} == {0, 1, 2, 3}
    _check_plan(_run_plan(gpu, jobs, inp, out_bytes, times=2), expect, jobs)


def test_plan_mixes_geometries_tables_and_white_balances(gpu, golden):
    rng = np.random.default_rng(5)
    tables = [golden[0], S.arbitrary_table(rng)]
    specs = [(3680, 5, 0, WBS[0], 0, 0, 0), (16, 700, 1, WBS[1], 3, 2, 2),
             (1026, 4, 1, WBS[2], 5, 16, 0), (6, 1, 0, WBS[3], 1, 0, 6),
             (2050, 9, 0, WBS[2], 7, 4, 0), (170, 3, 1, WBS[0], 0, 0, 0)]
    jobs, keep, inp, expect, out_bytes = _plan_case(specs, tables)
    _check_plan(_run_plan(gpu, jobs, inp, out_bytes, times=2), expect, jobs)


def test_plan_rejects_jobs_it_cannot_run(gpu, golden):
    """a job the validation refuses gets its status and consumes nothing; the others decode"""
    specs = [(66, 4, 0, WBS[2], 0, 0, 0), (22, 4, 0, WBS[2], 0, 0, 0), (10, 2, 0, WBS[2], 0, 0, 0)]
    jobs, keep, inp, expect, out_bytes = _plan_case(specs, [golden[0]])
    jobs[1].in_bytes = 3 * 22 * 4 - 1
    jobs[2].img.pitch_bytes = 6 * 10 + 1  # odd pitch
    outs = _run_plan(gpu, jobs, inp, out_bytes)
    (rc, st, cons), host = outs[0]
    assert st == [OK, IO, INV] and cons == [3 * 66 * 4, 0, 3 * 10 * 2] and rc != OK
    off, pitch, w, h, img = expect[0]
    px = np.stack([host[off + r * pitch:off + r * pitch + 6 * w].view(np.uint16) for r in range(h)])
    assert np.array_equal(px, img)
    assert (host[off + h * pitch:] == 0xA5).all()


def test_kernel_table_names_the_snef_kernel(gpu, golden):
    specs = [(3680, 16, 0, WBS[2], 0, 0, 0)]
    jobs, keep, inp, expect, out_bytes = _plan_case(specs, [golden[0]])
    din = torch.from_numpy(inp).cuda()
    out = torch.zeros(out_bytes, dtype=torch.uint8, device="cuda")
    plan = gpu.nikon_snef_plan(jobs)
    plan.set_timing(True)
    s = torch.cuda.current_stream().cuda_stream
    for _ in range(3):
        plan.run(din.data_ptr(), out.data_ptr(), s)
    rc, st, _ = plan.results()
    table, runs = plan.kernel_table()
    plan.close()
    assert rc == OK and runs == 3
    assert [n for n, _ in table] == ["nikon_snef_kernel"] and table[0][1] > 0
