"""RawImageData::scaleBlackWhite on the device (rsx_scale_black_white, rsx_scale_plan_create;
rawspeed_amd/csrc/rsx_scale.hip) through the C-ABI, byte for byte against the numpy model
tests/scale_files.py and, for every recorded case, against the reference's own hash in
tests/golden/scale_ref.json.  Every case goes through host pointers and through device pointers,
at the row's own pitch and at a wider one whose padding holds a sentinel that must survive (the
wider pitch also takes the rows off the 16-byte grid); the rows outside the crop are part of the
comparison, so nothing but the pass's samples may change; a refused case must leave its image as
it was.  F32 images are compared as bit patterns."""
import ctypes as C

import numpy as np
import pytest
import torch

import scale_files as S
from rawspeed_amd import abi, capi

pytestmark = pytest.mark.gpu

OK = abi.RSX_OK
NAMES = [c.name for c in S.cases()]


@pytest.fixture(scope="module")
def gpu():
    import gpu_util
    return gpu_util.ctx()


@pytest.fixture(scope="module")
def golden():
    return S.load_golden()


def _fill(dtype):
    return 0x5A5A if dtype == np.uint16 else np.float32(-7.25)


def padded(c, pad):
    buf = np.full((c.h, c.w * c.cpp + pad), _fill(c.img.dtype), c.img.dtype)
    buf[:, :c.w * c.cpp] = c.img
    return buf


def desc(c):
    return abi.scale_desc(c.crop, c.black, c.white, c.sep, c.areas, c.dither, c.sse2, c.is_f32)


def _on_host(gpu, c, pad):
    buf = padded(c, pad)
    d, keep = desc(c)
    st, r = gpu.scale_black_white(d, abi.Image(buf.ctypes.data, buf.strides[0], c.w, c.h, c.cpp, int(c.cfa)))
    return st, buf, r


def _on_device(gpu, c, pad):
    host = padded(c, pad)
    dev = torch.from_numpy(host.view(np.uint8).reshape(-1).copy()).cuda()
    d, keep = desc(c)
    st, r = gpu.scale_black_white(d, abi.Image(dev.data_ptr(), host.strides[0], c.w, c.h, c.cpp, int(c.cfa)))
    back = dev.cpu().numpy().view(c.img.dtype).reshape(host.shape)
    return st, back, r


def _check_result(r, st, res, what):
    if st != OK:
        assert bytes(r) == bytes(C.sizeof(abi.ScaleResult)), what
        return
    assert (r.estimated, r.skipped, r.variant, r.n_wrapped) == \
        (res["estimated"], res["skipped"], res["variant"], res["n_wrapped"]), what
    assert r.levels() == (res["black"], res["white"], res["sep"]), what


def _same(got, c, golden, what):
    st, buf, r = got
    want_st, want, res = S.expected(c.name)
    ws = c.w * c.cpp
    assert st == want_st, what
    assert buf[:, :ws].tobytes() == want.tobytes(), what
    assert buf[:, ws:].tobytes() == np.full((c.h, buf.shape[1] - ws), _fill(buf.dtype), buf.dtype).tobytes(), \
        ("the pitch padding was written", what)
    _check_result(r, st, res, what)
    if c.ref:
        assert golden[c.name]["image"] == S.sha(buf[:, :ws]), ("against the reference", what)


@pytest.mark.parametrize("name", NAMES)
def test_cases_through_host_pointers(gpu, golden, name):
    for pad in (0, 3):
        _same(_on_host(gpu, S.case(name), pad), S.case(name), golden, ("host", pad))


@pytest.mark.parametrize("name", NAMES)
def test_cases_through_device_pointers(gpu, golden, name):
    for pad in (0, 3):
        _same(_on_device(gpu, S.case(name), pad), S.case(name), golden, ("device", pad))


def test_a_plain_row_seed_past_int_is_refused_and_the_image_untouched(gpu):
    # crop_x + y 36969 leaves int at y = 58088: refused for the plain variant only
    img = np.full((58090, 8), 700, np.uint16)
    for sse2, want in ((False, abi.RSX_ERR_UNSUPPORTED), (True, OK)):
        buf = img.copy()
        d, keep = abi.scale_desc((0, 0, 8, 58090), 10, 4000, host_sse2=sse2)
        st, r = gpu.scale_black_white(d, abi.Image(buf.ctypes.data, 16, 8, 58090, 1, 1))
        assert st == want
        assert np.array_equal(buf, img) == (want != OK)
    d, keep = abi.scale_desc((0, 0, 8, 58088), 10, 4000, host_sse2=False, dither=False)
    buf = img.copy()
    st, r = gpu.scale_black_white(d, abi.Image(buf.ctypes.data, 16, 8, 58090, 1, 1))
    assert st == OK and r.variant == S.PLAIN
    assert (buf[:58088] == (690 * (16384 * 65535 // 3990) + 8192) >> 14).all() and (buf[58088:] == 700).all()


PLAN_CASES = ("sse2_wide_dither", "plain_no_sse2_dither", "f32_pass", "areas_both_not_cfa",
              "white_below_level", "estimate_window", "skip", "crop_1_2_sse2", "f32_estimate_nan",
              "plain_wrapped")


def test_a_plan_of_mixed_variants_run_twice(gpu, golden):
    jobs, keeps, layout, parts = [], [], [], []
    off = 0
    for i, name in enumerate(PLAN_CASES):
        c = S.case(name)
        rows = padded(c, i % 3)
        off += (2 * i + 2) * c.img.itemsize  # (rows off the 16-byte grid, a gap of sentinels)
        off += -off % c.img.itemsize
        d, keep = desc(c)
        keeps.append(keep)
        j = abi.ScaleJob()
        j.desc, j.img_offset = d, off
        j.img = abi.Image(0, rows.strides[0], c.w, c.h, c.cpp, int(c.cfa))
        jobs.append(j)
        layout.append((c, rows.shape, off))
        parts.append((off, rows.view(np.uint8).reshape(-1)))
        off += rows.nbytes
    before = np.full(off + 64, 0xA5, np.uint8)
    for o, b in parts:
        before[o:o + b.size] = b
    plan = gpu.scale_plan(jobs)
    want_status = [S.expected(n)[0] for n in PLAN_CASES]
    assert OK in want_status and abi.RSX_ERR_UNSUPPORTED in want_status
    for _ in range(2):
        dout = torch.from_numpy(before).cuda()
        torch.cuda.synchronize()
        plan.run(dout.data_ptr(), dout.data_ptr())
        rc, st, _ = plan.results()
        assert st == want_status and rc == abi.RSX_ERR_UNSUPPORTED
        back = dout.cpu().numpy()
        mask = np.ones_like(back, bool)
        for i, (c, shape, o) in enumerate(layout):
            n = shape[0] * shape[1] * c.img.itemsize
            rows = back[o:o + n].view(c.img.dtype).reshape(shape)
            mask[o:o + n] = False
            _, want, res = S.expected(c.name)
            ws = c.w * c.cpp
            assert rows[:, :ws].tobytes() == want.tobytes(), c.name
            assert rows[:, ws:].tobytes() == \
                np.full((c.h, shape[1] - ws), _fill(c.img.dtype), c.img.dtype).tobytes(), c.name
            rs, r = plan.result(i)
            assert rs == OK
            _check_result(r, st[i], res, c.name)
            if c.ref:
                assert golden[c.name]["image"] == S.sha(rows[:, :ws])
        assert np.array_equal(back[mask], before[mask]), "bytes outside the images were written"
    plan.close()


def test_plan_creation_refuses_what_validate_refuses(gpu):
    d, keep = abi.scale_desc((0, 0, 41, 4), 10, 1000)
    j = abi.ScaleJob()
    j.desc, j.img = d, abi.Image(0, 80, 40, 4, 1, 1)
    with pytest.raises(capi.RsxError) as e:
        gpu.scale_plan([j])
    assert e.value.status == abi.RSX_ERR_INVALID_ARG
    d, keep = abi.scale_desc((0, 0, 40, 4), 10, None, is_f32=True)
    j.desc, j.img = d, abi.Image(0, 160, 40, 4, 1, 1)
    with pytest.raises(capi.RsxError) as e:
        gpu.scale_plan([j])
    assert e.value.status == abi.RSX_ERR_UNSUPPORTED
    d, keep = abi.scale_desc((0, 0, 40, 4), 10, 1000)
    j.desc, j.img, j.img_offset = d, abi.Image(0, 80, 40, 4, 1, 1), 3
    with pytest.raises(capi.RsxError) as e:
        gpu.scale_plan([j])
    assert e.value.status == abi.RSX_ERR_INVALID_ARG


def test_nulls(gpu):
    d, keep = abi.scale_desc((0, 0, 40, 4), 10, 1000)
    st, r = gpu.scale_black_white(d, abi.Image(0, 80, 40, 4, 1, 1))
    assert st == abi.RSX_ERR_INVALID_ARG
