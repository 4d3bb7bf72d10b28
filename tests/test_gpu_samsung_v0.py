"""SamsungV0Decompressor on the device (rsx_samsung_v0_*, rawspeed_amd/csrc/rsx_samsung_v0.hip)
through the C-ABI: the host-pointer call and device plans against the model of
tests/srw_v0_files.py, which tests/test_samsung_v0_model.py pins against the reference; with the
reference's own decode of the same file where oracle/_ref is built, and with the results recorded
from it in tests/golden/samsung_v0_ref.json everywhere."""
import hashlib
import json
import threading

import numpy as np
import pytest
import torch

import srw_v0_files as S
import test_samsung_v0_model as M
from oracle_lib import HostImage, Ref
from rawspeed_amd import abi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import gpu_util
    return gpu_util.ctx()


@pytest.fixture(scope="module")
def ref():
    return Ref() if Ref.available() else None


@pytest.fixture(scope="module")
def golden():
    with open(M.GOLDEN) as f:
        return json.load(f)


def _decode(gpu, w, h, rows, pitch=None, lead=0):
    """`lead` bytes in front of the first row: the strip need not start at its first row"""
    strip, offs = S.strip_and_offsets(rows)
    if lead:
        strip = np.concatenate([np.full(lead, 0x5A, np.uint8), strip])
        offs = [o + lead for o in offs]
    out = HostImage(w, h, pitch=pitch)
    st, rs = gpu.samsung_v0_decompress(strip, offs, out.view())
    return st, rs, out


def _check_padding(out):
    pad = out.buf.reshape(out.dim_y, out.pitch)[:, 2 * out.dim_x:]
    assert (pad == 0xA5).all(), "the pitch padding was written"


def _check_ok(gpu, ref, w, h, rows, pitch=None, lead=0):
    mst, _, img = S.model_decode(w, h, rows)
    assert mst == S.OK
    st, rs, out = _decode(gpu, w, h, rows, pitch, lead)
    assert st == abi.RSX_OK and rs == [0] * h, (st, rs[:8])
    assert np.array_equal(out.pixels(), img), (w, h, np.argwhere(out.pixels() != img)[:5])
    _check_padding(out)
    if ref is not None:
        rst, dec = ref.decode_file(S.rows_file(w, h, rows))
        assert rst == 0 and np.array_equal(dec.u16()[:h, :w], out.pixels())


@pytest.mark.parametrize("seed", range(12))
def test_random_files(gpu, ref, seed):
    w, h, rows = M.random_case(seed)
    pitch = (2 * w + 15) // 16 * 16 + 16 * (seed % 2) + 2 * (seed % 3 == 2)
    _check_ok(gpu, ref, w, h, rows, pitch=pitch, lead=seed % 4)


# one block, one more pixel, around two blocks, a row of every kind of height (no pair, one pair,
# a pair and a single row, rows past the four the reconstruction loads ahead), the widest rows
SHAPES = [(16, 1), (16, 2), (17, 3), (31, 4), (32, 5), (33, 6), (47, 9), (400, 7), (1023, 8),
          (5536, 5), (5546, 6), (5545, 3)]


@pytest.mark.parametrize("w,h", SHAPES)
def test_shapes(gpu, ref, w, h):
    rng = np.random.default_rng([0x5B, w, h])
    rows = S.random_rows(rng, w, h, p_up=0.4, plant=True)
    _check_ok(gpu, ref, w, h, rows)
    _check_ok(gpu, ref, w, h, rows, pitch=(2 * w + 15) // 16 * 16 + 18)


def test_largest_frame(gpu, golden):
    """5546 x 3714, the largest frame the reference accepts, with a partial last block: against
    the model and against the hash recorded from the reference"""
    w, h, rows = M.large_case()
    assert M._sha_rows(rows) == golden["large"]["input_sha256"]
    st, rs, out = _decode(gpu, w, h, rows)
    assert st == abi.RSX_OK and not any(rs)
    _check_padding(out)
    got = hashlib.sha256(np.ascontiguousarray(out.pixels(), dtype="<u2").tobytes()).hexdigest()
    assert got == golden["large"]["image_sha256"]
    mst, _, img = S.model_decode(w, h, rows, cache={})
    assert mst == S.OK and np.array_equal(out.pixels(), img)


@pytest.mark.parametrize("kind", M.PLANTED)
def test_planted_rows(gpu, ref, golden, kind):
    w, h, rows, bad, want, _ = M.planted(kind)
    mst, mrows, _ = S.model_decode(w, h, rows)
    st, rs, out = _decode(gpu, w, h, rows)
    assert (st, rs) == (mst, mrows) and st == want and rs[bad] == want, (st, rs)
    assert (out.buf == 0xA5).all(), "a failed decode wrote into the caller's image"
    assert golden["planted"][kind]["ok"] is False
    assert golden["planted"][kind]["input_sha256"] == M._sha_rows(rows)
    if ref is not None:
        assert ref.decode_file(S.rows_file(w, h, rows))[0] != 0


def test_truncated_rows(gpu, golden):
    """the last row cut at every size: ok / fail as recorded from the reference, the statuses and
    the image as the model's"""
    cut = M.truncated_cases()
    assert len(cut) == len(golden["truncated"])
    n_bad = 0
    for (w, h, rows), ref_ok in zip(cut, golden["truncated"]):
        if w != 50 and len(rows[-1]) % 5:
            continue  # (every size of the first frame, every fifth of the others)
        mst, mrows, img = S.model_decode(w, h, rows)
        st, rs, out = _decode(gpu, w, h, rows)
        assert (st == abi.RSX_OK) == ref_ok, (w, len(rows[-1]))
        assert (st, rs) == (mst, mrows)
        if ref_ok:
            assert np.array_equal(out.pixels(), img)
        else:
            n_bad += 1
            assert st in (abi.RSX_ERR_INPUT_OVERFLOW, abi.RSX_ERR_IO)
            assert (out.buf == 0xA5).all(), "a failed decode wrote into the caller's image"
    assert n_bad > 20


def test_lowest_failing_row_wins(gpu):
    """two damaged rows of different kinds: the call returns the lower one's status"""
    w, h, rows, bad, want, _ = M.planted("len_above_16")
    rows = list(rows) + [rows[0][:2]]  # (and a two-byte row behind it)
    st, rs, out = _decode(gpu, w, h + 1, rows)
    assert st == want == abi.RSX_ERR_VALUE_RANGE
    assert rs == [0, 0, want, abi.RSX_ERR_IO]
    assert (out.buf == 0xA5).all()


def test_plan_jobs_of_different_geometry(gpu):
    """One plan, five jobs at device pointers: strips at odd byte offsets of the input, images at
    different offsets and pitches, a damaged job and a rejected one with their own statuses."""
    jobs, keep, parts, expect = [], [], [], []
    in_off, img_off = 3, 0
    shapes = [(130, 5, None), (16, 3, None), (1002, 4, "len_below_0"), (66, 7, None), (40, 4, "reject")]
    for k, (w, h, how) in enumerate(shapes):
        rng = np.random.default_rng([0x9A, k])
        rows = S.random_rows(rng, w, h, p_up=0.4)
        want = 0
        if how == "len_below_0":
            rows[2] = M.planted(how)[2][2]
            want = abi.RSX_ERR_VALUE_RANGE
        strip, offs = S.strip_and_offsets(rows)
        if how == "reject":
            offs[2] = offs[1]
            want = abi.RSX_ERR_INVALID_ARG
        _, _, img = S.model_decode(w, h, rows)
        arr = abi.samsung_v0_offsets(offs)
        keep.append(arr)
        pitch = (2 * w + 15) // 16 * 16 + 2 * k
        j = abi.SamsungV0Job()
        j.row_offsets = arr
        j.n_offsets = len(offs)
        j.in_offset, j.in_bytes, j.img_offset = in_off, len(strip), img_off
        j.img = abi.Image(None, pitch, w, h, 1, 1)
        jobs.append(j)
        parts.append(strip)
        parts.append(np.full(5 + k, 0x5A, np.uint8))  # (bytes between the jobs: nobody's)
        expect.append((img_off, pitch, w, h, img, want))
        in_off += len(strip) + 5 + k
        img_off += pitch * h + 6
    inp = torch.from_numpy(np.concatenate([np.full(3, 0x5A, np.uint8)] + parts)).cuda()
    out = torch.full((img_off,), 0xA5, dtype=torch.uint8, device="cuda")
    plan = gpu.samsung_v0_plan(jobs)
    for _ in range(2):  # (a plan runs again on the same scratch)
        out.fill_(0xA5)
        plan.run(inp.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        rc, st, _ = plan.results()
        assert rc != 0
        host = out.cpu().numpy()
        covered = np.zeros(host.size, bool)
        for (off, pitch, w, h, img, want), got_st in zip(expect, st):
            assert got_st == want
            if want:
                if want != abi.RSX_ERR_INVALID_ARG:
                    for r in range(h):
                        covered[off + r * pitch:off + r * pitch + 2 * w] = True
                continue
            px = np.stack([host[off + r * pitch:off + r * pitch + 2 * w].view(np.uint16) for r in range(h)])
            assert np.array_equal(px, img)
            for r in range(h):
                covered[off + r * pitch:off + r * pitch + 2 * w] = True
        assert (host[~covered] == 0xA5).all(), "bytes outside the jobs' rectangles were written"
    plan.close()


def test_plan_returns_the_last_failing_jobs_status(gpu):
    """Three 48 x 3 jobs: the host refuses job 0 (its in_bytes end inside row 0), job 1 decodes,
    row 2 of job 2 fails on the device with another status.  Every job gets its own status and
    results() returns job 2's, the last failing job's; the row statuses of a refused job are not
    to be had, those of job 2 name the row."""
    import gpu_util
    w, h, planted, bad, bad_st, _ = M.planted("len_below_0")
    good = S.random_rows(np.random.default_rng(0x9B), w, h, p_up=0.0)
    _, bad_rows, _ = S.model_decode(w, h, planted)
    mst, _, img = S.model_decode(w, h, good)
    IO = abi.RSX_ERR_IO
    assert mst == S.OK and bad_st == abi.RSX_ERR_VALUE_RANGE != IO and bad_rows[bad] == bad_st
    pitch = 2 * w + 2
    jobs, keep, parts = [], [], []
    in_off = 0
    for k, rows in enumerate([good, good, planted]):
        strip, offs = S.strip_and_offsets(rows)
        keep.append(abi.samsung_v0_offsets(offs))
        j = abi.SamsungV0Job()
        j.row_offsets = keep[-1]
        j.n_offsets = len(offs)
        j.in_offset, j.img_offset = in_off, k * (pitch * h + 6)
        j.in_bytes = offs[1] - 1 if k == 0 else len(strip)
        j.img = abi.Image(None, pitch, w, h, 1, 1)
        jobs.append(j)
        parts.append(strip)
        in_off += len(strip)
    inp = torch.from_numpy(np.concatenate(parts)).cuda()
    out = torch.full((3 * (pitch * h + 6),), 0xA5, dtype=torch.uint8, device="cuda")
    plan = gpu.samsung_v0_plan(jobs)
    plan.run(inp.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    rc, st, _ = plan.results()
    assert st == [IO, abi.RSX_OK, bad_st] and rc == bad_st
    assert gpu_util.plan_row_status(plan, 0, h)[0] == abi.RSX_ERR_INVALID_ARG
    assert gpu_util.plan_row_status(plan, 2, h) == (abi.RSX_OK, bad_rows)
    plan.close()
    host = out.cpu().numpy()
    rect = np.lib.stride_tricks.as_strided
    px = np.ascontiguousarray(rect(host[jobs[1].img_offset:], (h, 2 * w), (pitch, 1)))
    assert np.array_equal(px.view(np.uint16), img)
    outside = np.ones(host.size, bool)
    for k in (1, 2):
        rect(outside[jobs[k].img_offset:], (h, 2 * w), (pitch, 1))[:] = False
    assert (host[outside] == 0xA5).all(), "bytes outside the two images were written"


def test_plan_timing_names_both_kernels(gpu):
    rng = np.random.default_rng(0x71)
    w, h = 200, 9
    rows = S.random_rows(rng, w, h)
    strip, offs = S.strip_and_offsets(rows)
    arr = abi.samsung_v0_offsets(offs)
    j = abi.SamsungV0Job()
    j.row_offsets, j.n_offsets = arr, len(offs)
    j.in_offset, j.in_bytes, j.img_offset = 0, len(strip), 0
    j.img = abi.Image(None, 2 * w, w, h, 1, 1)
    inp = torch.from_numpy(strip.copy()).cuda()
    out = torch.zeros(2 * w * h, dtype=torch.uint8, device="cuda")
    plan = gpu.samsung_v0_plan([j])
    plan.set_timing(True)
    plan.run(inp.data_ptr(), out.data_ptr())
    assert plan.results()[0] == 0
    names = [n for n, _ in plan.kernel_table()[0]]
    plan.close()
    assert names == ["sv0_parse_kernel", "sv0_recon_kernel"]
    _, _, img = S.model_decode(w, h, rows)
    assert np.array_equal(out.cpu().numpy().view(np.uint16).reshape(h, w), img)


def test_two_threads_share_a_context(gpu):
    files = []
    for t, (w, h) in enumerate([(2000, 40), (1338, 57)]):
        rng = np.random.default_rng([0x77, t])
        rows = S.tiled_rows(rng, w, h, pool=6)
        files.append((w, h, rows, S.model_decode(w, h, rows, cache={})[2]))
    results = [None, None]

    def work(t):
        w, h, rows, img = files[t]
        ok = True
        for _ in range(6):
            st, _, out = _decode(gpu, w, h, rows)
            ok &= st == 0 and np.array_equal(out.pixels(), img)
        results[t] = ok

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert results == [True, True]
