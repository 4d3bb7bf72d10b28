"""The SuperCCD rotation on the device (rsx_raf_rotate*, rawspeed_amd/csrc/rsx_fuji_rotate.hip)
through the C-ABI: every geometry of tests/fuji_rotate_files.py under both layouts, at four crops
inside a larger source, into destinations with and without pitch padding, through device pointers,
host pointers and plans; against the model of the reference's loop byte for byte over the WHOLE
destination buffer.  Every destination starts as 0xA5: pitch padding and the bytes around the image
must keep it, the corners nothing lands on must be 0, and a refused descriptor must leave it all.

The normal layout with odd H is a refusal (the reference throws there, tests/
test_fuji_rotate_model.py); those sizes of the list check the status and the untouched buffer."""
import numpy as np
import pytest
import torch

import fuji_rotate_files as F
from oracle_lib import HostImage
from rawspeed_amd import abi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import gpu_util
    return gpu_util.ctx()


def _dst_layouts(R):
    """(lead bytes, pitch): on the 16-byte grid with padding, and off it without"""
    return [(16, (2 * R + 15) // 16 * 16 + 16), (6, 2 * R)]


def _expected(want, lead, pitch, tail=10):
    """the whole destination buffer: 0xA5 but for the R samples of every row"""
    rows, R = want.shape
    buf = np.full(lead + pitch * rows + tail, 0xA5, np.uint8)
    for r in range(rows):
        buf[lead + r * pitch:lead + r * pitch + 2 * R] = want[r].view(np.uint8)
    return buf


def _source(W, H, cx, cy, seed):
    """(2-D array, padded bytes, pitch): the crop inside a larger image"""
    src = F.source(W + cx + 2, H + cy + 3, seed)
    pitch = F.src_pitch(src.shape[1])
    return src, F.padded(src, pitch), pitch


def _device_call(gpu, W, H, alt, cx, cy, lead, pitch, seed=1):
    """rsx_raf_rotate with device pointers -> (status, the whole destination buffer, expected)"""
    src, sbytes, sp = _source(W, H, cx, cy, seed)
    R = F.rotated_size(W, H, alt)[0]
    d_src = torch.from_numpy(sbytes).cuda()
    out = torch.full((lead + pitch * (R - 1) + 10,), 0xA5, dtype=torch.uint8, device="cuda")
    st = gpu.fuji_rotate(abi.fuji_rotate_desc((cx, cy), (W, H), alt),
                         abi.Image(d_src.data_ptr(), sp, src.shape[1], src.shape[0], 1, 1),
                         abi.Image(out.data_ptr() + lead, pitch, R, R - 1, 1, 1))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    if F.refusal(W, H, alt) != F.OK:
        return st, got, np.full(got.size, 0xA5, np.uint8)
    return st, got, _expected(F.rotate_scatter(src, cx, cy, W, H, alt), lead, pitch)


@pytest.mark.parametrize("W,H,alt", F.cases())
def test_device_pointers_every_crop_and_pitch(gpu, W, H, alt):
    R = F.rotated_size(W, H, alt)[0]
    for k, (cx, cy) in enumerate(F.CROPS):
        for lead, pitch in _dst_layouts(R):
            st, got, want = _device_call(gpu, W, H, alt, cx, cy, lead, pitch, seed=k + 1)
            assert st == F.refusal(W, H, alt), (cx, cy, pitch)
            assert np.array_equal(got, want), (cx, cy, pitch, np.flatnonzero(got != want)[:8])


@pytest.mark.parametrize("W,H,alt", F.cases())
def test_host_pointers(gpu, W, H, alt):
    cx, cy = 3, 5
    src, sbytes, sp = _source(W, H, cx, cy, 7)
    R = F.rotated_size(W, H, alt)[0]
    for padded in (True, False):
        dst = HostImage(R, max(R - 1, 1), pitch=None if padded else 2 * R)
        st = gpu.fuji_rotate(abi.fuji_rotate_desc((cx, cy), (W, H), alt),
                             F.image_of(sbytes, sp, src.shape[1], src.shape[0]), dst.view())
        assert st == F.refusal(W, H, alt)
        if st != F.OK:
            assert (dst.buf == 0xA5).all(), "a refused call wrote"
            continue
        want = _expected(F.rotate_scatter(src, cx, cy, W, H, alt), 0, dst.pitch, tail=0)
        assert np.array_equal(dst.buf, want)
    assert (sbytes.reshape(-1, sp)[:, 2 * src.shape[1]:] == 0x5A).all()


def _job(W, H, alt, cx, cy, src, sp, in_off, img_off, pitch):
    R = F.rotated_size(W, H, alt)[0]
    j = abi.FujiRotateJob()
    j.desc = abi.fuji_rotate_desc((cx, cy), (W, H), alt)
    j.in_offset, j.img_offset = in_off, img_off
    j.in_ = abi.Image(None, sp, src.shape[1], src.shape[0], 1, 1)
    j.img = abi.Image(None, pitch, R, max(R - 1, 1), 1, 1)
    return j


def test_plan_of_three_geometries_both_layouts_and_a_refused_job(gpu):
    specs = [(65, 64, 0, 1, 0), (130, 67, 1, 3, 5), (9, 16, 0, 0, 1), (63, 65, 0, 0, 0)]
    jobs, parts, where = [], [], []
    in_off, img_off = 2, 4
    for k, (W, H, alt, cx, cy) in enumerate(specs):
        src, sbytes, sp = _source(W, H, cx, cy, 20 + k)
        R = F.rotated_size(W, H, alt)[0]
        pitch = 2 * R + 2 * (k % 3)
        parts += [np.full(in_off - sum(p.size for p in parts), 0x5A, np.uint8), sbytes]
        jobs.append(_job(W, H, alt, cx, cy, src, sp, in_off, img_off, pitch))
        where.append((W, H, alt, cx, cy, src, img_off, pitch, R))
        in_off += sbytes.size + 2 + 4 * k
        img_off += pitch * (R - 1) + 6
    inp = torch.from_numpy(np.concatenate(parts)).cuda()
    out = torch.full((img_off,), 0xA5, dtype=torch.uint8, device="cuda")
    plan = gpu.fuji_rotate_plan(jobs)
    plan.set_timing(True)
    plan.run(inp.data_ptr(), out.data_ptr())
    rc, st, cons = plan.results()
    names = [n for n, _ in plan.kernel_table()[0]]
    plan.close()
    assert st == [F.OK, F.OK, F.OK, F.INVALID_ARG] and rc == F.INVALID_ARG and cons == [0] * 4
    assert len(names) == 1 and names[0] in ("fuji_rotate_kernel", "fuji_rotate_lds_kernel")
    want = np.full(img_off, 0xA5, np.uint8)
    for (W, H, alt, cx, cy, src, off, pitch, R), s in zip(where, st):
        if s == F.OK:
            rows = F.rotate_scatter(src, cx, cy, W, H, alt)
            for r in range(R - 1):
                want[off + r * pitch:off + r * pitch + 2 * R] = rows[r].view(np.uint8)
    got = out.cpu().numpy()
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]


@pytest.mark.parametrize("W,H,alt", [(4000, 3000, 0), (4352, 1446, 1)])
def test_camera_sized_frame(gpu, W, H, alt):
    R = F.rotated_size(W, H, alt)[0]
    lead, pitch = _dst_layouts(R)[0]
    st, got, want = _device_call(gpu, W, H, alt, 4, 2, lead, pitch)
    assert st == F.OK
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]


def test_both_kernels_give_the_same_bytes(gpu, monkeypatch):
    """RSX_FUJI_ROTATE_KERNEL picks the direct gather or the one staged through LDS when a plan is
    made; whichever is the default, the other must write the same buffer"""
    for W, H, alt in [(130, 68, 0), (130, 67, 1), (9, 16, 0), (200, 4, 0), (64, 64, 1)]:
        R = F.rotated_size(W, H, alt)[0]
        for which in ("direct", "lds"):
            monkeypatch.setenv("RSX_FUJI_ROTATE_KERNEL", which)
            for lead, pitch in _dst_layouts(R):
                st, got, want = _device_call(gpu, W, H, alt, 3, 5, lead, pitch)
                assert st == F.OK
                assert np.array_equal(got, want), (which, W, H, alt, pitch)
        monkeypatch.delenv("RSX_FUJI_ROTATE_KERNEL")


def test_unpack_plan_feeds_a_rotate_plan_with_one_download(gpu):
    """the flow of a device-resident caller: 16-bit LSB rows of twice the width are unpacked into
    a device image, the rotation reads that image where it lies, and only the rotated image comes
    back"""
    W, H, alt, cx, cy = 130, 68, 0, 2, 1
    dim_x, dim_y = 2 * 70, H + 2  # the unpacked image: double width
    raw = F.source(dim_x, dim_y, 31)
    mid_pitch = (2 * dim_x + 15) // 16 * 16
    u = abi.UnpackJob()
    u.desc = abi.UnpackDesc(0, 0, dim_x, dim_y, 2 * dim_x, 16, abi.ORDER_LSB)
    u.in_offset, u.in_bytes, u.img_offset = 0, raw.nbytes, 0
    u.img = abi.Image(None, mid_pitch, dim_x, dim_y, 1, 1)
    R = F.rotated_size(W, H, alt)[0]
    pitch = (2 * R + 15) // 16 * 16
    j = abi.FujiRotateJob()
    j.desc = abi.fuji_rotate_desc((cx, cy), (W, H), alt)
    j.in_ = abi.Image(None, mid_pitch, dim_x, dim_y, 1, 1)
    j.img = abi.Image(None, pitch, R, R - 1, 1, 1)
    d_raw = torch.from_numpy(raw.view(np.uint8).reshape(-1).copy()).cuda()
    d_mid = torch.full((mid_pitch * dim_y,), 0xA5, dtype=torch.uint8, device="cuda")
    d_out = torch.full((pitch * (R - 1),), 0xA5, dtype=torch.uint8, device="cuda")
    up, rot = gpu.unpack_plan([u]), gpu.fuji_rotate_plan([j])
    s = torch.cuda.current_stream().cuda_stream
    up.run(d_raw.data_ptr(), d_mid.data_ptr(), s)
    rot.run(d_mid.data_ptr(), d_out.data_ptr(), s)
    assert up.results()[0] == F.OK and rot.results()[0] == F.OK
    got = d_out.cpu().numpy()  # the one download
    up.close()
    rot.close()
    want = _expected(F.rotate_scatter(raw, cx, cy, W, H, alt), 0, pitch, tail=0)
    assert np.array_equal(got, want)


def test_refused_descriptors_leave_dst_untouched(gpu):
    W, H = 8, 6
    src, sbytes, sp = _source(W, H, 1, 2, 3)
    d_src = torch.from_numpy(sbytes).cuda()
    sv = abi.Image(d_src.data_ptr(), sp, src.shape[1], src.shape[0], 1, 1)
    R = F.rotated_size(W, H, 0)[0]
    out = torch.full((2 * R * (R - 1) + 64,), 0xA5, dtype=torch.uint8, device="cuda")

    def dv(dx=R, dy=R - 1, pitch=2 * R):
        return abi.Image(out.data_ptr(), pitch, dx, dy, 1, 1)

    d = abi.fuji_rotate_desc
    refused = [
        (d((1, 2), (8, 7), 0), sv, dv(11, 10), F.INVALID_ARG),      # odd H, normal
        (d((1, 2), (7, 6), 1), sv, dv(9, 8, 18), F.UNSUPPORTED),    # odd W, alt
        (d((1, 2), (W, H), 0), sv, dv(R + 1, R - 1, 2 * R + 2), F.INVALID_ARG),  # dst size
        (d((1, 2), (W, H), 0), sv, dv(pitch=2 * R + 1), F.INVALID_ARG),          # odd pitch
        (d((4, 2), (W, H), 0), sv, dv(), F.INVALID_ARG),            # crop past the source
        (d((-1, 2), (W, H), 0), sv, dv(), F.INVALID_ARG),
        (d((1, 2), (W, H), 0), sv, abi.Image(d_src.data_ptr() + 8, 2 * R, R, R - 1, 1, 1),
         F.INVALID_ARG),                                            # overlapping images
        (None, sv, dv(), F.INVALID_ARG),
    ]
    for desc, s, t, want in refused:
        assert gpu.fuji_rotate(desc, s, t) == want
    # host and device pointers mixed
    host = HostImage(R, R - 1)
    assert gpu.fuji_rotate(d((1, 2), (W, H), 0), sv, host.view()) == F.INVALID_ARG
    assert (host.buf == 0xA5).all()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xA5).all()
    assert np.array_equal(d_src.cpu().numpy(), sbytes)
    # odd offsets in a plan
    for in_off, img_off in ((1, 0), (0, 1)):
        plan = gpu.fuji_rotate_plan([_job(W, H, 0, 1, 2, src, sp, in_off, img_off, 2 * R)])
        assert plan.results()[1] == [F.INVALID_ARG]
        plan.close()
    # ... and the good call on the same buffers works
    assert gpu.fuji_rotate(d((1, 2), (W, H), 0), sv, dv()) == F.OK
    torch.cuda.synchronize()
    got = out.cpu().numpy()[:2 * R * (R - 1)].view(np.uint16).reshape(R - 1, R)
    assert np.array_equal(got, F.rotate_scatter(src, 1, 2, W, H, 0))
