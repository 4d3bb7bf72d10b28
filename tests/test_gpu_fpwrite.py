"""The F32 writers on the device (rsx_fpwrite_*, rawspeed_amd/csrc/rsx_fpwrite_pack.hip) through the
C-ABI, held byte for byte against the host build of their core (tests/fpwrite_files.py, which
tests/test_fpwrite_host.py pins to the numpy model and the oracle's unpack).  Every output buffer
starts as a guard pattern and is compared whole.  Random inputs are seeded from their names."""
import numpy as np
import pytest
import torch

import fpwrite_files as F
from oracle_lib import HostImage
from rawspeed_amd import abi

pytestmark = pytest.mark.gpu

GUARD = 0x5A


@pytest.fixture(scope="module")
def gpu():
    import gpu_util
    return gpu_util.ctx()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(n):
    return torch.full((n,), GUARD, dtype=torch.uint8, device="cuda")


def _result(r):
    return int(r.bytes_written), int(r.stream_bytes), int(r.inexact)


@pytest.mark.parametrize("case", F.pack_cases(), ids=lambda c: c[0])
def test_pack_equals_the_host_core_and_unpacks_to_the_image(gpu, case):
    """host pointers and device pointers (the output 1 byte into its buffer where the stream has
    more than one row) against the host build; then rsx_unpack_f32 gives the image back"""
    d, img = F.pack_case(case)
    st, want, hr = F.host_pack(d, img)
    assert st == F.OK
    n = int(hr.bytes_written)
    out = np.full(len(want), GUARD, np.uint8)
    st, r = gpu.fpwrite_pack(d, img.view(), out.ctypes.data, n)
    assert st == F.OK and _result(r) == _result(hr)
    assert np.array_equal(out, want)
    lead = 1 if d.crop_h > 1 else 0
    dimg, dout = _dev(img.buf), _guarded(lead + len(want))
    st, r = gpu.fpwrite_pack(d, img.view(dimg.data_ptr()), dout.data_ptr() + lead, n)
    assert st == F.OK and _result(r) == _result(hr)
    back = dout.cpu().numpy()
    assert (back[:lead] == GUARD).all() and np.array_equal(back[lead:], want)
    got = HostImage(img.dim_x, img.dim_y, img.cpp, fill=0, bpc=4)
    assert gpu.unpack_f32(d, want[:n], got.view()) == F.OK
    x0 = F.first_sample(d, img.cpp)
    win = got.u32()[d.crop_y:d.crop_y + d.crop_h, x0:x0 + d.crop_w * img.cpp]
    assert np.array_equal(win, F.window_of(d, img))


def _plan_inputs():
    """jobs of every width and order, odd output offsets; job 2 holds inexact samples (one in the
    last row and column of its window), job 4 is refused by the validation"""
    imgs, jobs, wants, results = [], [], [], []
    img_off, out_off = 0, 3
    names = ("odd16m", "cpp224l", "short16l", "block24m", "cpp332l", "one24m")
    cases = {c[0]: c for c in F.pack_cases()}
    for k, name in enumerate(names):
        d, img = F.pack_case(cases[name])
        if k == 2:
            px = img.px.copy()
            x0 = F.first_sample(d, img.cpp)
            px[d.crop_y, x0 + 1] = 0x3F800001
            px[d.crop_y + d.crop_h - 1, x0 + d.crop_w * img.cpp - 1] = 0x00000001
            img = F.Img32(px, cpp=img.cpp, pad=img.pitch - 4 * px.shape[1])
        st, want, hr = F.host_pack(d, img)
        n = F.round_up4(d.crop_h * d.input_pitch_bytes)
        assert st == (F.VALUE_RANGE if k == 2 else F.OK)
        if k == 4:
            d = F.pack_desc(d.crop_x, d.crop_y + 2, d.crop_w, d.crop_h, d.input_pitch_bytes,
                            d.bits_per_pixel, d.bit_order)  # rows past the image
            st, hr = F.INVALID_ARG, abi.FpWritePackResult()
        jobs.append(abi.fpwrite_pack_job(d, img_off, out_off, n, img.dim_x, img.dim_y, img.cpp,
                                         img.pitch))
        # an inexact job may write its range; a refused one writes nothing
        wants.append((out_off, n, want[:n] if st == F.OK else None, st == F.VALUE_RANGE))
        results.append((st, _result(hr)))
        imgs.append((img_off, img.buf))
        img_off += (len(img.buf) + 15) // 16 * 16
        out_off += n + 5
    src = np.zeros(img_off, np.uint8)
    for off, buf in imgs:
        src[off:off + len(buf)] = buf
    return src, jobs, wants, results, out_off + 16


def test_plan_of_mixed_jobs_with_an_inexact_and_a_refused_one(gpu):
    src, jobs, wants, results, total = _plan_inputs()
    dsrc = _dev(src)
    plan = gpu.fpwrite_pack_plan(jobs)
    runs = []
    for _ in range(2):
        dout = _guarded(total)
        plan.run(dsrc.data_ptr(), dout.data_ptr())
        rc, st, cons = plan.results()
        assert st == [r[0] for r in results] and rc == F.INVALID_ARG  # (the last failing job's)
        assert cons == [r[1][0] for r in results]
        for k, (want_st, want_r) in enumerate(results):
            got_st, r = plan.result(k)
            assert got_st == want_st and _result(r) == want_r, k
        back = dout.cpu().numpy()
        keep = np.ones(total, bool)
        for off, n, w, may_write in wants:
            if w is not None:
                assert np.array_equal(back[off:off + n], w)
            if w is not None or may_write:
                keep[off:off + n] = False
        assert (back[keep] == GUARD).all()  # nothing outside the jobs' ranges, none past out_cap
        runs.append(back)
    assert np.array_equal(runs[0], runs[1])


def test_inexact_call_reports_nothing_written(gpu):
    d, img = F.pack_case([c for c in F.pack_cases() if c[0] == "odd24m"][0])
    px = img.px.copy()
    x0 = F.first_sample(d, img.cpp)
    px[d.crop_y + d.crop_h - 1, x0 + d.crop_w - 1] = 0x3F800001
    px[d.crop_y, x0] = 0x7F800001  # a NaN payload below the narrow fraction
    bad = F.Img32(px)
    n = F.round_up4(d.crop_h * d.input_pitch_bytes)
    out = np.full(n + 16, GUARD, np.uint8)
    st, r = gpu.fpwrite_pack(d, bad.view(), out.ctypes.data, n)
    assert st == F.VALUE_RANGE and _result(r) == (0, d.crop_h * d.input_pitch_bytes, 2)
    assert (out[n:] == GUARD).all()
    dimg, dout = _dev(bad.buf), _guarded(n + 16)
    st, r = gpu.fpwrite_pack(d, bad.view(dimg.data_ptr()), dout.data_ptr(), n)
    assert st == F.VALUE_RANGE and _result(r) == (0, d.crop_h * d.input_pitch_bytes, 2)
    assert (dout.cpu().numpy()[n:] == GUARD).all()
    # a host image with a device output is refused
    assert gpu.fpwrite_pack(d, img.view(), dout.data_ptr(), n)[0] == F.INVALID_ARG


def test_fit_against_the_model(gpu):
    """windows that are all-16, all-24 and all-32, windows made 32 (or 24) by one sample in their
    last row and column, a window of more than one piece and one wider than a workgroup's lanes;
    through a host and a device pointer"""
    piece = F.fit_block_samples()
    w, h = 300, (3 * piece) // 300 + 7
    px = np.empty((h, w), np.uint32)
    px[:, :100] = F.exact_samples("fit16", 16, h, 100)
    px[:, 100:200] = F.exact_samples("fit24", 24, h, 100)
    px[:, 200:] = F.exact_samples("fit32", 32, h, 100)
    px[:, 100:200][F.model_narrow(px[:, 100:200], 16)[1]] = 0x3F800080  # no binary16 value among them
    px[h - 1, 99] = 0x3F800001   # 32 in the last row and column of the first block of columns
    px[20, 59] = 0x3F800080      # 24 in the last row and column of (40, 10, 20, 11)
    wins = [(0, 0, 40, h - 1), (100, 0, 100, h), (200, 0, 100, h), (0, 0, 100, h),
            (40, 10, 20, 11), (40, 10, 19, 11), (40, 10, 20, 10), (0, 0, w, h), (0, 0, 99, h),
            (99, h - 1, 1, 1), (0, 3, 1, 1)]
    want = [F.model_fit(px[y:y + wh, x:x + ww]) for x, y, ww, wh in wins]
    assert want[:7] == [16, 24, 32, 32, 24, 16, 16] and want[7:] == [32, 24, 32, 16]
    for pad in (0, 16):
        img = F.Img32(px, pad=pad)
        assert F.host_fit(img, wins) == (F.OK, want)
        assert gpu.fpwrite_fit(img.view(), wins) == (F.OK, want)
        dimg = _dev(img.buf)
        assert gpu.fpwrite_fit(img.view(dimg.data_ptr()), wins) == (F.OK, want)
    # a contiguous all-16 image of many pieces
    flat = F.Img32(F.exact_samples("flat", 16, 64, 1024))
    assert gpu.fpwrite_fit(flat.view(), [(0, 0, 1024, 64)]) == (F.OK, [16])
    assert gpu.fpwrite_fit(flat.view(), [(0, 0, 1025, 1)])[0] == F.INVALID_ARG
    assert gpu.fpwrite_fit(flat.view(), [])[0] == F.INVALID_ARG


def test_every_binary24_pattern_narrows_on_the_device(gpu):
    """the 2^24 widened binary24 patterns as one image, packed at 24 bits in one launch: the stream
    is the patterns, big-endian"""
    p = np.arange(1 << 24, dtype=np.uint32)
    img = F.Img32(F.model_widen(p, 24).reshape(4096, 4096))
    d = F.pack_desc(0, 0, 4096, 4096, 3 * 4096, 24, abi.ORDER_MSB)
    dimg, dout = _dev(img.buf), _guarded(3 * (1 << 24) + 16)
    st, r = gpu.fpwrite_pack(d, img.view(dimg.data_ptr()), dout.data_ptr(), 3 * (1 << 24))
    assert st == F.OK and _result(r) == (3 << 24, 3 << 24, 0)
    back = dout.cpu().numpy()
    assert (back[3 << 24:] == GUARD).all()
    b = back[:3 << 24].reshape(-1, 3).astype(np.uint32)
    assert np.array_equal((b[:, 0] << 16) | (b[:, 1] << 8) | b[:, 2], p)
    assert gpu.fpwrite_fit(img.view(dimg.data_ptr()), [(0, 0, 4096, 4096)]) == (F.OK, [24])


# ---------------------------------------------------------------------------------------------
# deflate tiles: the device stream is the host core's stream
# ---------------------------------------------------------------------------------------------
import dng_deflate_files as DF  # noqa: E402


def _res(r):
    return int(r.status), int(r.adler), int(r.bytes), int(r.blocks), int(r.stored_blocks)


def _job(d, geom, img, img_off, out_off, cap):
    return abi.FpWriteDeflateJob(d, *geom, img_off, out_off, cap,
                                 abi.Image(None, img.pitch, img.dim_x, img.dim_y, img.cpp, 0))


@pytest.mark.parametrize("case", F.deflate_cases(), ids=lambda c: c[0])
def test_deflate_equals_the_host_core(gpu, case):
    d, geom, img, tile = F.deflate_case(case)
    hst, want, hr = F.host_deflate(d, geom, img)
    cap = len(want) - 16
    assert hst == F.OK
    out = np.full(len(want), GUARD, np.uint8)
    rc, res = gpu.fpwrite_deflate(d, [F.deflate_tile(geom, out.ctypes.data, cap)], img.view())
    assert rc == F.OK and _res(res[0]) == _res(hr)
    n = int(hr.bytes)
    assert np.array_equal(out[:n], want[:n]) and (out[n:] == GUARD).all()
    lead = 1 + len(case[0]) % 3
    dimg, dout = _dev(img.buf), _guarded(lead + len(want))
    t = F.deflate_tile(geom, dout.data_ptr() + lead, cap)
    rc, res = gpu.fpwrite_deflate(d, [t], img.view(dimg.data_ptr()))
    assert rc == F.OK and _res(res[0]) == _res(hr)
    back = dout.cpu().numpy()
    assert (back[:lead] == GUARD).all() and np.array_equal(back[lead:lead + n], want[:n])
    assert (back[lead + n:] == GUARD).all()


def test_deflate_plan_of_all_cases_twice(gpu):
    """every case of the shape list as the jobs of one plan, odd output offsets, with one job an
    output byte short and one holding an inexact sample among them: the good jobs' streams are the
    host core's, nothing is written for the two, the guard bytes stay, and a second run equals the
    first"""
    imgs, jobs, wants = [], [], []
    img_off, out_off = 0, 5
    cases = F.deflate_cases()
    for k, case in enumerate(cases + cases[-8:-6]):
        d, geom, img, tile = F.deflate_case(case)
        if k == len(cases) + 1:
            px = img.px.copy()
            px[geom[3] + geom[5] - 1, geom[2] + geom[4] - 1] = 0x3F800001
            img = F.Img32(px, cpp=img.cpp, pad=img.pitch - 4 * px.shape[1])
        hst, want, hr = F.host_deflate(d, geom, img)
        cap = len(want) - 16
        if k == len(cases):
            cap = int(hr.bytes) - 1
            hst, want, hr = F.host_deflate(d, geom, img, cap=cap)
            assert hst == F.INPUT_OVERFLOW
        jobs.append(_job(d, geom, img, img_off, out_off, cap))
        wants.append((out_off, want[:int(hr.bytes)], _res(hr)))
        imgs.append((img_off, img.buf))
        img_off += (len(img.buf) + 15) // 16 * 16
        out_off += cap + 3
    assert wants[-1][2][0] == F.VALUE_RANGE and wants[-2][2][0] == F.INPUT_OVERFLOW
    src = np.zeros(img_off, np.uint8)
    for off, buf in imgs:
        src[off:off + len(buf)] = buf
    want = np.full(out_off + 16, GUARD, np.uint8)
    for off, w, _ in wants:
        want[off:off + len(w)] = w
    dsrc = _dev(src)
    plan = gpu.fpwrite_deflate_plan(jobs)
    for _ in range(2):
        dout = _guarded(len(want))
        plan.run(dsrc.data_ptr(), dout.data_ptr())
        rc, st, cons = plan.results()
        assert rc == F.VALUE_RANGE and st == [w[2][0] for w in wants]
        assert cons == [w[2][2] for w in wants]
        for k, w in enumerate(wants):
            got_st, r = plan.result(k)
            assert got_st == w[2][0] and _res(r) == w[2], k
        assert np.array_equal(dout.cpu().numpy(), want)


@pytest.mark.parametrize("pred", sorted(DF.PREDICTORS))
@pytest.mark.parametrize("bps", F.BPS)
def test_deflate_round_trip_on_the_device(gpu, bps, pred):
    """one plan writes the 3 x 2 tiles of an image with ragged right and bottom tiles;
    rsx_dng_decompress_deflate over the written streams gives the image back bit for bit"""
    tw, th, W, H = 40, 24, 100, 40
    rng = np.random.default_rng([bps, pred])
    px = F.model_widen(DF.random_samples(rng, bps, H, W, "mixed"), bps)
    img = F.Img32(px, pad=8)
    d = abi.DngDeflateDesc(bps, pred)
    geoms = [(tw, th, x, y, min(tw, W - x), min(th, H - y)) for y in range(0, H, th)
             for x in range(0, W, tw)]
    assert len(geoms) == 6
    bound = F.bound_model(tw * th * bps // 8)
    jobs = [_job(d, g, img, 0, k * (bound + 7), bound) for k, g in enumerate(geoms)]
    dimg, dout = _dev(img.buf), _guarded(6 * (bound + 7))
    plan = gpu.fpwrite_deflate_plan(jobs)
    plan.run(dimg.data_ptr(), dout.data_ptr())
    rc, st, cons = plan.results()
    assert rc == F.OK and st == [0] * 6
    back = dout.cpu().numpy()
    datas = [back[k * (bound + 7):k * (bound + 7) + cons[k]].copy() for k in range(6)]
    for k in range(6):
        assert (back[k * (bound + 7) + cons[k]:(k + 1) * (bound + 7)] == GUARD).all()
    got = HostImage(W, H, 1, fill=0, bpc=4)
    rc, st = gpu.dng_decompress_deflate(bps, pred, geoms, datas, got.view())
    assert rc == F.OK and st == [F.OK] * 6
    assert np.array_equal(got.u32()[:, :W], px)
