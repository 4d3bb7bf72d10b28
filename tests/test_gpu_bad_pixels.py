"""RawImageData::fixBadPixels on the device (rsx_bad_pixels_fix, rsx_bad_pixels_plan_create;
rawspeed_amd/csrc/rsx_bad_pixels.hip) through the C-ABI, byte for byte against the numpy model
tests/bad_pixels_files.py -- which tests/test_bad_pixels_model.py pins against the answers recorded
from the reference.  Every model case goes through host pointers and through device pointers, at
the row's own pitch and at a wider one whose padding holds a sentinel that must survive; F32
images are compared as bit patterns."""
import ctypes as C

import numpy as np
import pytest
import torch

import bad_pixels_files as B
from rawspeed_amd import abi, capi

pytestmark = pytest.mark.gpu

OK = abi.RSX_OK
NAMES = [c[0] for c in B.cases()]
CASES = {c[0]: c for c in B.cases()}


@pytest.fixture(scope="module")
def gpu():
    import gpu_util
    return gpu_util.ctx()


def _fill(dtype):
    return 0x5A5A if dtype == np.uint16 else 0x5A5A5A5A


def _on_host(gpu, case, pad):
    _, cfa, f32, img, positions, m = case
    h, w = img.shape
    buf = B.padded(img, pad, _fill(img.dtype))
    d, keep, map_out = abi.bad_pixels_desc(positions, (w, h), m, f32)
    st, r = gpu.bad_pixels_fix(d, abi.Image(buf.ctypes.data, buf.strides[0], w, h, 1, int(cfa)))
    return st, buf, map_out, r


def _on_device(gpu, case, pad):
    _, cfa, f32, img, positions, m = case
    h, w = img.shape
    host = B.padded(img, pad, _fill(img.dtype))
    dev = torch.from_numpy(host.view(np.uint8).reshape(-1).copy()).cuda()
    d, keep, map_out = abi.bad_pixels_desc(positions, (w, h), m, f32)
    st, r = gpu.bad_pixels_fix(d, abi.Image(dev.data_ptr(), host.strides[0], w, h, 1, int(cfa)))
    back = dev.cpu().numpy().view(img.dtype).reshape(host.shape)
    return st, back, map_out, r


def _same(got, name, what):
    st, buf, map_out, r = got
    want, wmap, n_bad, n_fixed = B.expected(name)
    w = want.shape[1]
    assert st == OK, what
    assert buf[:, :w].tobytes() == want.tobytes(), what
    assert (buf[:, w:] == _fill(buf.dtype)).all(), ("the pitch padding was written", what)
    assert (r.n_bad, r.n_fixed, r.map_made) == (n_bad, n_fixed, int(wmap is not None)), what
    if wmap is None:
        assert (map_out == 0xA5).all(), what
    else:
        assert map_out.tobytes() == wmap.tobytes(), what


@pytest.mark.parametrize("name", NAMES)
def test_model_cases_through_host_pointers(gpu, name):
    for pad in (0, 3):
        _same(_on_host(gpu, CASES[name], pad), name, ("host", pad))


@pytest.mark.parametrize("name", NAMES)
def test_model_cases_through_device_pointers(gpu, name):
    for pad in (0, 3):
        _same(_on_device(gpu, CASES[name], pad), name, ("device", pad))


def test_refused_calls_leave_the_image_untouched(gpu):
    _, cfa, f32, img, positions, m = CASES["interior_cfa"]
    h, w = img.shape
    for pos_list, kw, cpp in (((B.pos(w, 0),), {}, 1), ((B.pos(0, h),), {}, 1),
                              ((B.pos(3, 2),), dict(map_pitch=48), 1), ((B.pos(1, 1),), {}, 3)):
        buf = img.copy()
        d, keep, map_out = abi.bad_pixels_desc(pos_list, (w // cpp, h), None, False, **kw)
        st, r = gpu.bad_pixels_fix(d, abi.Image(buf.ctypes.data, buf.strides[0], w // cpp, h, cpp, 1))
        assert st == (abi.RSX_ERR_UNSUPPORTED if cpp == 3 else abi.RSX_ERR_INVALID_ARG)
        assert np.array_equal(buf, img) and (map_out == 0xA5).all()
        assert (r.n_bad, r.n_fixed, r.map_made) == (0, 0, 0)


def test_the_empty_call_does_nothing(gpu):
    _, cfa, f32, img, positions, m = CASES["interior_cfa"]
    h, w = img.shape
    buf = img.copy()
    d, keep, map_out = abi.bad_pixels_desc((), (w, h))
    st, r = gpu.bad_pixels_fix(d, abi.Image(buf.ctypes.data, buf.strides[0], w, h, 1, 1))
    assert st == OK and (r.n_bad, r.n_fixed, r.map_made) == (0, 0, 0)
    assert np.array_equal(buf, img) and (map_out == 0xA5).all()


PLAN_JOBS = (("u16 cfa", 130, 66, True, False, 0.05), ("u16 plain", 49, 8, False, False, 0.2),
             ("f32", 96, 34, True, True, 0.1))


def _plan_buffers(rng, bad_position=None):
    """three jobs in one input and one output buffer: (jobs, input bytes, output bytes, layout)"""
    jobs, layout = [], []
    inp, out = [], []
    in_off = out_off = 0
    for i, (_, w, h, cfa, f32, density) in enumerate(PLAN_JOBS):
        img = B._image(900 + i, w, h, f32)
        positions = B._random_positions(910 + i, w, h, density)
        positions += positions[:3]  # (duplicates)
        if bad_position is not None and i == bad_position:
            positions[len(positions) // 2] = B.pos(w, 0)
        pad = 2 * i
        rows = B.padded(img, pad, _fill(img.dtype))
        p = np.asarray(positions, np.uint32)
        in_off += 12  # (any multiple of 4)
        inp.append((in_off, p.view(np.uint8)))
        out_off += 8 * img.itemsize
        out.append((out_off, rows.view(np.uint8).reshape(-1)))
        j = abi.BadPixelsJob()
        j.in_offset, j.n_positions, j.is_f32 = in_off, p.size, int(f32)
        j.img_offset = out_off
        j.img = abi.Image(0, rows.strides[0], w, h, 1, int(cfa))
        jobs.append(j)
        layout.append((img, positions, cfa, rows.shape, out_off))
        in_off += p.nbytes
        out_off += rows.nbytes
    hin = np.full(in_off + 16, 0xEE, np.uint8)
    hout = np.full(out_off + 32, 0xA5, np.uint8)
    for off, b in inp:
        hin[off:off + b.size] = b
    for off, b in out:
        hout[off:off + b.size] = b
    return jobs, hin, hout, layout


def _check_plan_output(back, before, layout, skip=None):
    mask = np.ones_like(back, bool)
    for i, (img, positions, cfa, shape, off) in enumerate(layout):
        rows = back[off:off + shape[0] * shape[1] * img.itemsize].view(img.dtype).reshape(shape)
        mask[off:off + shape[0] * shape[1] * img.itemsize] = False
        h, w = img.shape
        if i == skip:
            assert np.array_equal(rows[:, :w], img), "a refused job touched its image"
        else:
            want, _, _, _ = B.model_fix(img, cfa, positions)
            assert rows[:, :w].tobytes() == want.tobytes(), PLAN_JOBS[i][0]
        assert (rows[:, w:] == _fill(img.dtype)).all(), "the pitch padding was written"
    assert np.array_equal(back[mask], before[mask]), "bytes outside the images were written"


def test_a_plan_of_three_jobs_run_twice(gpu):
    jobs, hin, hout, layout = _plan_buffers(np.random.default_rng(5))
    plan = gpu.bad_pixels_plan(jobs)
    din = torch.from_numpy(hin).cuda()
    for _ in range(2):
        dout = torch.from_numpy(hout).cuda()
        torch.cuda.synchronize()
        plan.run(din.data_ptr(), dout.data_ptr())
        rc, st, _ = plan.results()
        assert rc == OK and st == [OK] * 3
        _check_plan_output(dout.cpu().numpy(), hout, layout)
        for i, (img, positions, cfa, _, _) in enumerate(layout):
            _, _, n_bad, n_fixed = B.model_fix(img, cfa, positions)
            rs, r = plan.result(i)
            assert rs == OK and (r.n_bad, r.n_fixed, r.map_made) == (n_bad, n_fixed, 1)
    # once more on the fixed images: the stage reads only unmarked pixels
    plan.run(din.data_ptr(), dout.data_ptr())
    assert plan.results()[0] == OK
    _check_plan_output(dout.cpu().numpy(), hout, layout)
    plan.close()


def test_a_plan_job_with_a_position_outside_is_refused_on_the_device(gpu):
    jobs, hin, hout, layout = _plan_buffers(np.random.default_rng(6), bad_position=1)
    plan = gpu.bad_pixels_plan(jobs)
    din, dout = torch.from_numpy(hin).cuda(), torch.from_numpy(hout).cuda()
    torch.cuda.synchronize()
    plan.run(din.data_ptr(), dout.data_ptr())
    rc, st, _ = plan.results()
    assert rc == abi.RSX_ERR_INVALID_ARG and st == [OK, abi.RSX_ERR_INVALID_ARG, OK]
    _check_plan_output(dout.cpu().numpy(), hout, layout, skip=1)
    plan.close()


def test_plan_creation_refuses_what_validate_refuses(gpu):
    j = abi.BadPixelsJob()
    j.n_positions, j.img = 1, abi.Image(0, 80, 40, 4, 3, 1)
    with pytest.raises(capi.RsxError) as e:
        gpu.bad_pixels_plan([j])
    assert e.value.status == abi.RSX_ERR_INVALID_ARG  # (a pitch too small for three components)
    j.img = abi.Image(0, 240, 40, 4, 3, 1)
    with pytest.raises(capi.RsxError) as e:
        gpu.bad_pixels_plan([j])
    assert e.value.status == abi.RSX_ERR_UNSUPPORTED
    j.img = abi.Image(0, 80, 40, 4, 1, 1)
    j.map_pitch = 32
    with pytest.raises(capi.RsxError) as e:
        gpu.bad_pixels_plan([j])
    assert e.value.status == abi.RSX_ERR_INVALID_ARG
