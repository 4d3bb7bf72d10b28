"""PhaseOneDecompressor on the device (rsx_phase_one_*, rawspeed_amd/csrc/rsx_phase_one.hip)
through the C-ABI.  Whole IIQ files (tests/iiq_files.py) are cut into strips the way
IiqDecoder::computeSripes does; the decode is compared with the image the file was written
from (the encoder is lossless), with the reference's own decode of the same file where
oracle/_ref is built, and -- for damaged files -- with the per-row statuses of the model that
tests/test_phase_one_model.py pins against the reference."""
import threading

import numpy as np
import pytest
import torch

import iiq_files as I
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


def _file(seed, w, h, gap_max=9, choices=(0.25, 0.1, 0.4)):
    rng = np.random.default_rng([0x9F1, seed, w, h])
    img = I.sample_image(rng, w, h)
    rows = I.encode(img, seed, choices)
    return img, rows, I.iiq_file(rows, w, rng, gap_max=gap_max, tail_gap=int(rng.integers(0, 7))), rng


def _decode(gpu, blob, pitch=None):
    raw, strips, w, h = I.iiq_strips(blob)
    out = HostImage(w, h, pitch=pitch)
    st, rows = gpu.phase_one_decompress(np.frombuffer(raw, np.uint8), strips, out.view())
    return st, rows, out


def _check_padding(out):
    pad = out.buf.reshape(out.dim_y, out.pitch)[:, 2 * out.dim_x:]
    assert (pad == 0xA5).all(), "the pitch padding was written"


SHAPES = [(2, 1), (2, 5), (4, 3), (6, 4), (8, 1), (10, 3), (14, 7), (62, 2), (64, 3), (66, 4),
          (70, 2), (126, 5), (128, 3), (130, 2), (1000, 6), (1022, 3), (4096, 4), (6002, 3),
          (11974, 2), (11976, 3)]


@pytest.mark.parametrize("w,h", SHAPES)
def test_parity_with_the_source_and_the_reference(gpu, ref, w, h):
    for seed, choices in enumerate([(0.0, 0.0, 0.0), (0.25, 0.1, 0.4), (0.6, 0.3, 0.9)]):
        img, rows, blob, _ = _file(seed, w, h, choices=choices)
        pitch = (2 * w + 15) // 16 * 16 + 16 * (seed % 2) + 2 * (seed == 2)
        st, srow, out = _decode(gpu, blob, pitch=pitch)
        assert st == abi.RSX_OK and srow == [0] * h, (st, srow[:8])
        assert np.array_equal(out.pixels(), img), (w, h, seed)
        _check_padding(out)
        if ref is not None:
            rst, dec = ref.decode_file(blob)
            assert rst == 0 and np.array_equal(dec.u16()[:h, :w], out.pixels())


def test_largest_frame(gpu, ref):
    """11976 x 8854, the largest frame the reference accepts (PhaseOneDecompressor.cpp:52-56)"""
    w, h = I.MAX_W, I.MAX_H
    img, rows, blob, _ = _file(5, w, h, gap_max=4)
    st, srow, out = _decode(gpu, blob)
    assert st == abi.RSX_OK and not any(srow)
    assert np.array_equal(out.pixels(), img)
    _check_padding(out)
    if ref is not None:
        rst, dec = ref.decode_file(blob, threads=8)
        assert rst == 0 and np.array_equal(dec.u16()[:h, :w], out.pixels())


@pytest.mark.parametrize("how", ["truncate", "col0", "short"])
def test_damaged_files(gpu, ref, how):
    for seed in range(4):
        rng = np.random.default_rng([0xDA2, seed])
        w, h = 2 * int(rng.integers(24, 700)), int(rng.integers(2, 9))
        img = I.sample_image(rng, w, h)
        bad = sorted({int(x) for x in rng.integers(0, h, size=1 + seed % 2)})
        rows = I.encode(img, seed)
        for b in bad:
            rows = I.damage(rows, b, how, rng)
        blob = I.iiq_file(rows, w, rng, gap_max=0 if how == "short" else 5)
        mst, _, mrows = I.model_file(blob)
        assert mst != 0
        st, srow, out = _decode(gpu, blob)
        assert (st, srow) == (mst, mrows), (seed, bad)
        assert (out.buf == 0xA5).all(), "a failed decode wrote into the caller's image"
        if ref is not None:
            assert ref.decode_file(blob)[0] != 0


def test_plan_jobs_of_different_geometry(gpu):
    """One plan, four jobs at device pointers: strips at odd byte offsets of the input,
    images at different offsets and pitches, one damaged job with its own status."""
    jobs, keep, parts, expect = [], [], [], []
    in_off, img_off = 3, 0
    shapes = [(130, 5, None), (8, 3, None), (1002, 4, "col0"), (66, 6, None)]
    for k, (w, h, how) in enumerate(shapes):
        img, rows, blob, rng = _file(40 + k, w, h)
        if how:
            rows = I.damage(rows, 1, how, rng)
            blob = I.iiq_file(rows, w, rng)
        raw, strips, _, _ = I.iiq_strips(blob)
        arr = abi.phase_one_strips(strips)
        keep.append(arr)
        pitch = (2 * w + 15) // 16 * 16 + 2 * k
        j = abi.PhaseOneJob()
        j.strips = arr
        j.n_strips = len(strips)
        j.in_offset, j.in_bytes, j.img_offset = in_off, len(raw), img_off
        j.img = abi.Image(None, pitch, w, h, 1, 1)
        jobs.append(j)
        parts.append(np.frombuffer(raw, np.uint8))
        parts.append(np.full(5 + k, 0x5A, np.uint8))  # (bytes between the jobs: nobody's)
        expect.append((img_off, pitch, w, h, img, I.RSX_ERR_BAD_HUFFMAN_CODE if how else 0))
        in_off += len(raw) + 5 + k
        img_off += pitch * h + 6
    inp = torch.from_numpy(np.concatenate([np.full(3, 0x5A, np.uint8)] + parts)).cuda()
    out = torch.full((img_off,), 0xA5, dtype=torch.uint8, device="cuda")
    plan = gpu.phase_one_plan(jobs)
    plan.run(inp.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    rc, st, _ = plan.results()
    plan.close()
    assert rc == I.RSX_ERR_BAD_HUFFMAN_CODE
    host = out.cpu().numpy()
    for (off, pitch, w, h, img, want), got_st in zip(expect, st):
        assert got_st == want
        if want:
            continue
        px = np.stack([host[off + r * pitch:off + r * pitch + 2 * w].view(np.uint16) for r in range(h)])
        assert np.array_equal(px, img)


def test_plan_returns_the_last_failing_jobs_status(gpu):
    """Three 8 x 3 jobs: the host refuses job 0 (a strip ends behind its in_bytes), job 1 decodes,
    row 1 of job 2 fails on the device with another status.  Every job gets its own status and
    results() returns job 2's, the last failing job's; the row statuses of a refused job are not
    to be had, those of job 2 name the row."""
    import gpu_util
    w, h, pitch = 8, 3, 2 * 8 + 2
    jobs, keep, parts, imgs = [], [], [], []
    in_off = 0
    for k in range(3):
        img, rows, blob, rng = _file(90 + k, w, h)
        if k == 2:
            blob = I.iiq_file(I.damage(rows, 1, "col0", rng), w, rng)
            bad_st, _, bad_rows = I.model_file(blob)
        raw, strips, _, _ = I.iiq_strips(blob)
        keep.append(abi.phase_one_strips(strips))
        j = abi.PhaseOneJob()
        j.strips = keep[-1]
        j.n_strips = len(strips)
        j.in_offset, j.in_bytes, j.img_offset = in_off, len(raw) - (k == 0), k * (pitch * h + 6)
        j.img = abi.Image(None, pitch, w, h, 1, 1)
        jobs.append(j)
        parts.append(np.frombuffer(raw, np.uint8))
        imgs.append(img)
        in_off += len(raw)
    INV = abi.RSX_ERR_INVALID_ARG
    assert bad_st == I.RSX_ERR_BAD_HUFFMAN_CODE != INV and bad_rows == [0, bad_st, 0]
    inp = torch.from_numpy(np.concatenate(parts)).cuda()
    out = torch.full((3 * (pitch * h + 6),), 0xA5, dtype=torch.uint8, device="cuda")
    plan = gpu.phase_one_plan(jobs)
    plan.run(inp.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    rc, st, _ = plan.results()
    assert st == [INV, abi.RSX_OK, bad_st] and rc == bad_st
    assert gpu_util.plan_row_status(plan, 0, h)[0] == INV
    assert gpu_util.plan_row_status(plan, 2, h) == (abi.RSX_OK, bad_rows)
    plan.close()
    host = out.cpu().numpy()
    rect = np.lib.stride_tricks.as_strided
    px = np.ascontiguousarray(rect(host[jobs[1].img_offset:], (h, 2 * w), (pitch, 1)))
    assert np.array_equal(px.view(np.uint16), imgs[1])
    outside = np.ones(host.size, bool)
    for k in (1, 2):
        rect(outside[jobs[k].img_offset:], (h, 2 * w), (pitch, 1))[:] = False
    assert (host[outside] == 0xA5).all(), "bytes outside the two images were written"


def test_two_threads_share_a_context(gpu):
    files = [_file(70 + t, w, h) for t, (w, h) in enumerate([(2000, 40), (1338, 57)])]
    results = [None, None]

    def work(t):
        img, _, blob, _ = files[t]
        ok = True
        for _ in range(6):
            st, _, out = _decode(gpu, blob)
            ok &= st == 0 and np.array_equal(out.pixels(), img)
        results[t] = ok

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert results == [True, True]
