"""ArwDecoder::SonyDecrypt and decodeSRF on the device (rsx_sony_decrypt, rsx_sony_srf_*,
rawspeed_amd/csrc/rsx_sony_srf.hip) through the C-ABI: the generator over buffers around the pad
and the chunk length with host pointers, device pointers and in place, at addresses on and off the
16-byte grid; SRF frames with padded and unpadded pitch through both kinds of pointers and a plan;
against the model (tests/sony_srf_files.py) byte for byte over the whole output buffer, which
starts as 0xA5.  The full 3360 x 2460 frame takes its expectation from the host build of the core,
which tests/test_sony_srf_model.py pins to the model."""
import numpy as np
import pytest
import torch

import sony_srf_files as F
from oracle_lib import HostImage
from rawspeed_amd import abi

pytestmark = pytest.mark.gpu

SIZES = F.N_WORDS + F.N_WORDS_CHUNK


@pytest.fixture(scope="module")
def gpu():
    import gpu_util
    return gpu_util.ctx()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("key", F.KEYS)
def test_decrypt_host_pointers(gpu, key):
    for n in SIZES:
        data = F.payload(4 * n, seed=n)
        st, got = gpu.sony_decrypt(data.tobytes(), key)
        assert st == F.OK
        assert np.array_equal(got, F.decrypt(data, key)), n


@pytest.mark.parametrize("key", F.KEYS)
def test_decrypt_device_pointers_on_and_off_the_grid(gpu, key):
    for n in SIZES:
        data = F.payload(4 * n, seed=n + 1)
        want = F.decrypt(data, key)
        for lead_in, lead_out in ((0, 0), (16, 32), (1, 3), (4, 16)):
            inp = _dev(np.concatenate([np.full(lead_in, 0x5A, np.uint8), data,
                                       np.full(16, 0xFF, np.uint8)]))
            out = torch.full((lead_out + 4 * n + 20,), 0xA5, dtype=torch.uint8, device="cuda")
            st = gpu.sony_decrypt(None, key, in_ptr=inp.data_ptr() + lead_in,
                                  out_ptr=out.data_ptr() + lead_out, n_words=n)
            assert st == F.OK
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert np.array_equal(got[lead_out:lead_out + 4 * n], want), (n, lead_in, lead_out)
            assert (got[:lead_out] == 0xA5).all() and (got[lead_out + 4 * n:] == 0xA5).all()


@pytest.mark.parametrize("key", F.KEYS)
def test_decrypt_in_place(gpu, key):
    for n in SIZES:
        data = F.payload(4 * n, seed=n + 2)
        for lead in (0, 2):
            buf = _dev(np.concatenate([np.full(lead, 0xA5, np.uint8), data,
                                       np.full(12, 0xA5, np.uint8)]))
            p = buf.data_ptr() + lead
            assert gpu.sony_decrypt(None, key, in_ptr=p, out_ptr=p, n_words=n) == F.OK
            torch.cuda.synchronize()
            got = buf.cpu().numpy()
            assert np.array_equal(got[lead:lead + 4 * n], F.decrypt(data, key)), (n, lead)
            assert (got[:lead] == 0xA5).all() and (got[lead + 4 * n:] == 0xA5).all()
            # ... and once more gives the input back
            assert gpu.sony_decrypt(None, key, in_ptr=p, out_ptr=p, n_words=n) == F.OK
            torch.cuda.synchronize()
            assert np.array_equal(buf.cpu().numpy()[lead:lead + 4 * n], data)


def test_decrypt_of_nothing_and_refusals(gpu):
    assert gpu.sony_decrypt(b"", 5)[0] == F.OK
    buf = torch.full((64,), 0xA5, dtype=torch.uint8, device="cuda")
    assert gpu.sony_decrypt(None, 5, in_ptr=buf.data_ptr(), out_ptr=buf.data_ptr(), n_words=0) == F.OK
    assert gpu.sony_decrypt(None, 5, in_ptr=0, out_ptr=0, n_words=0) == F.OK
    assert gpu.sony_decrypt(None, 5, in_ptr=0, out_ptr=buf.data_ptr(), n_words=4) == F.INVALID_ARG
    assert gpu.sony_decrypt(None, 5, in_ptr=buf.data_ptr(), out_ptr=0, n_words=4) == F.INVALID_ARG
    host = np.zeros(64, np.uint8)
    assert gpu.sony_decrypt(None, 5, in_ptr=host.ctypes.data, out_ptr=buf.data_ptr(),
                            n_words=4) == F.INVALID_ARG  # host and device pointers mixed
    assert gpu.sony_decrypt(None, 5, in_ptr=buf.data_ptr(), out_ptr=buf.data_ptr(),
                            n_words=1 << 32) == F.UNSUPPORTED
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0xA5).all()


def _pitches(w):
    return [2 * w, (2 * w + 15) // 16 * 16 + 16]


@pytest.mark.parametrize("w,h", F.IMAGES)
def test_srf_device_and_host_pointers(gpu, w, h):
    key = 0x9E3779B9 ^ w
    data = F.payload(2 * w * h + 5, seed=w + h)
    want = F.decode_srf(data, key, w, h)
    assert F.host_decode(data, key, w, h)[0] == F.OK
    for pitch in _pitches(w):
        for lead_in, lead_out in ((0, 16), (3, 6)):
            inp = _dev(np.concatenate([np.full(lead_in, 0x5A, np.uint8), data]))
            out = torch.full((lead_out + pitch * h + 10,), 0xA5, dtype=torch.uint8, device="cuda")
            view = abi.Image(out.data_ptr() + lead_out, pitch, w, h, 1, 1)
            st = gpu.sony_srf_decompress(None, key, view, in_ptr=inp.data_ptr() + lead_in,
                                         in_bytes=len(data))
            assert st == F.OK
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            exp = np.full(got.size, 0xA5, np.uint8)
            for r in range(h):
                exp[lead_out + r * pitch:lead_out + r * pitch + 2 * w] = want[r].view(np.uint8)
            assert np.array_equal(got, exp), (pitch, lead_in, np.flatnonzero(got != exp)[:8])
        img = HostImage(w, h, pitch=pitch)
        assert gpu.sony_srf_decompress(data.tobytes(), key, img.view()) == F.OK
        assert np.array_equal(img.pixels(), want)
        assert (img.buf.reshape(h, pitch)[:, 2 * w:] == 0xA5).all()


def test_srf_full_frame(gpu):
    w, h, key = 3360, 2460, 0x1234ABCD
    data = F.payload(2 * w * h, seed=11)
    st, want = F.host_decode(data, key, w, h)
    assert st == F.OK
    pitch = 2 * w + 32
    inp = _dev(data)
    out = torch.full((pitch * h,), 0xA5, dtype=torch.uint8, device="cuda")
    view = abi.Image(out.data_ptr(), pitch, w, h, 1, 1)
    assert gpu.sony_srf_decompress(None, key, view, in_ptr=inp.data_ptr(), in_bytes=len(data)) == F.OK
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(h, pitch)
    assert np.array_equal(got[:, :2 * w].copy().view(np.uint16), want)
    assert (got[:, 2 * w:] == 0xA5).all()
    img = HostImage(w, h)
    assert gpu.sony_srf_decompress(data.tobytes(), key, img.view()) == F.OK
    assert np.array_equal(img.pixels(), want)


def test_srf_plan_of_two_jobs_and_refused_ones(gpu):
    # (w, h, key, bytes withheld from in_bytes); the third has an odd area, the fourth is short
    specs = [(254, 4, 0xDEADBEEF, 0), (63, 2, 7, 0), (63, 65, 9, 0), (4, 3, 1, 1)]
    jobs, parts, where = [], [], []
    in_off, img_off = 1, 2
    for k, (w, h, key, cut) in enumerate(specs):
        data = F.payload(2 * w * h, seed=40 + k)
        pitch = 2 * w + 2 * k
        parts += [np.full(in_off - sum(p.size for p in parts), 0x5A, np.uint8), data]
        j = abi.SonySrfJob()
        j.in_offset, j.img_offset, j.key = in_off, img_off, key
        j.in_bytes = len(data) - cut
        j.img = abi.Image(None, pitch, w, h, 1, 1)
        jobs.append(j)
        where.append((w, h, key, data, img_off, pitch))
        in_off += len(data) + 1 + 2 * k
        img_off += pitch * h + 4
    inp = _dev(np.concatenate(parts + [np.full(16, 0xFF, np.uint8)]))
    out = torch.full((img_off,), 0xA5, dtype=torch.uint8, device="cuda")
    plan = gpu.sony_srf_plan(jobs)
    plan.set_timing(True)
    plan.run(inp.data_ptr(), out.data_ptr())
    rc, st, cons = plan.results()
    names = [n for n, _ in plan.kernel_table()[0]]
    plan.close()
    assert st == [F.OK, F.OK, F.UNSUPPORTED, F.IO] and rc == F.IO and cons == [0] * 4
    assert names == ["sony_srf_kernel"]
    want = np.full(img_off, 0xA5, np.uint8)
    for (w, h, key, data, off, pitch), s in zip(where, st):
        if s == F.OK:
            rows = F.decode_srf(data, key, w, h)
            for r in range(h):
                want[off + r * pitch:off + r * pitch + 2 * w] = rows[r].view(np.uint8)
    got = out.cpu().numpy()
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]


def test_srf_refusals_leave_the_image_untouched(gpu):
    w, h = 63, 2
    data = F.payload(2 * w * h)
    for pointers in ("host", "device"):
        for ww, hh, n, want in [(w, h, 2 * w * h - 1, F.IO), (63, 1, 126, F.UNSUPPORTED),
                                (w, h, 0, F.IO), (3361, 2, 1 << 20, F.INVALID_ARG)]:
            if pointers == "host":
                img = HostImage(ww, hh)
                a = np.ascontiguousarray(data)
                st = gpu.sony_srf_decompress(None, 3, img.view(), in_ptr=a.ctypes.data, in_bytes=n)
                assert st == want
                assert (img.buf == 0xA5).all()
            else:
                inp = _dev(data)
                out = torch.full((2 * ww * hh + 16,), 0xA5, dtype=torch.uint8, device="cuda")
                st = gpu.sony_srf_decompress(None, 3, abi.Image(out.data_ptr(), 2 * ww, ww, hh, 1, 1),
                                             in_ptr=inp.data_ptr(), in_bytes=n)
                assert st == want
                torch.cuda.synchronize()
                assert (out.cpu().numpy() == 0xA5).all()
    # host and device pointers mixed
    inp = _dev(data)
    img = HostImage(w, h)
    assert gpu.sony_srf_decompress(None, 3, img.view(), in_ptr=inp.data_ptr(),
                                   in_bytes=len(data)) == F.INVALID_ARG
    assert (img.buf == 0xA5).all()
    # an odd image offset in a plan
    j = abi.SonySrfJob()
    j.in_offset, j.in_bytes, j.img_offset, j.key = 0, len(data), 1, 3
    j.img = abi.Image(None, 2 * w, w, h, 1, 1)
    plan = gpu.sony_srf_plan([j])
    assert plan.results()[1] == [F.INVALID_ARG]
    plan.close()
