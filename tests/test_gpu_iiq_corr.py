"""IiqDecoder::CorrectPhaseOneC's pixel passes on the device (rsx_iiq_correct, rsx_phase_one_
decompress_corrected, rsx_iiq_correct_plan_create; rawspeed_amd/csrc/rsx_iiq_corr.hip) through the
C-ABI, against the numpy model tests/iiq_corr_files.py -- which tests/test_iiq_corr_model.py pins
against the reference's whole-file decode for luma and the quadrant curves, and which is the only
yardstick of chroma.  Images of 64 x 40 and 72 x 38 (a row is several 8-pixel vectors, an odd
number of them), a pitch off the 16-byte grid and an odd img_offset / 2 for the halves path."""
import numpy as np
import pytest
import torch

import iiq_corr_files as K
import iiq_files as F
from oracle_lib import HostImage
from rawspeed_amd import abi, capi

pytestmark = pytest.mark.gpu

OK = abi.RSX_OK
SIZES = ((64, 40), (72, 38))
RGGB, GRBG, CFA_2X4 = (2, 2, (0, 1, 1, 2)), (2, 2, (1, 0, 2, 1)), (2, 4, (0, 1, 1, 2, 2, 1, 1, 0))
# head[0..5]: 1 x 1 cells; 7 x 5 (divides neither dimension) at offset (3, 2): a vector starts in
# front of the area and ends inside; 13 x 11 reaching past the image on both axes; a cell wider than
# the image; wide == 1; high == 1; a head field of 0; head[5] above the image height
HEADS = {"1x1": (0, 0, 60, 30, 1, 1), "7x5": (3, 2, 56, 30, 7, 5), "13x11": (5, 3, 130, 121, 13, 11),
         "8x8": (0, 0, 72, 40, 8, 8), "wide_cell": (0, 0, 400, 40, 200, 4), "wide_1": (0, 0, 8, 40, 8, 4),
         "high_1": (0, 0, 64, 8, 8, 8), "zero": (0, 0, 64, 40, 0, 8), "tall": (2, 1, 60, 300, 6, 100),
         # cells wider than 32 columns: lanes start from the start values kept every 32 columns
         "70x8": (1, 0, 140, 40, 70, 8), "33x8": (0, 0, 99, 40, 33, 8), "64x32": (3, 1, 128, 64, 64, 32)}


@pytest.fixture(scope="module")
def gpu():
    import gpu_util
    return gpu_util.ctx()


@pytest.fixture(scope="module")
def curves():
    return K.random_curves(np.random.default_rng(0x431))


def _image(rng, w, h):
    img = rng.integers(0, 65536, size=(h, w)).astype(np.uint16)
    img[::3, ::5] = 65535
    return img


def _payload(rng, head, planes=1, **kw):
    if K.ff_shape(head) is None:
        return K.ff_payload(head, [])
    return K.ff_random(rng, head, planes, **kw)


def _on_host(gpu, img, ops, cfa=None, pitch=None):
    h, w = img.shape
    out = HostImage(w, h, pitch=pitch)
    out.pixels()[:] = img
    before = out.buf.copy()
    d, keep = abi.iiq_corr(ops, cfa)
    st = gpu.iiq_correct(d, out.view())
    assert (out.buf.reshape(h, out.pitch)[:, 2 * w:] == 0xA5).all(), "the pitch padding was written"
    if st != OK:
        assert np.array_equal(out.buf, before), "a refused list touched the image"
    return st, out.pixels().copy()


def _on_device(gpu, img, ops, cfa=None, pitch=None, offset=0):
    """through a device pointer: the image at byte `offset` of a buffer filled with 0xA5"""
    h, w = img.shape
    pitch = pitch or 2 * w
    host = np.full(offset + pitch * h + 32, 0xA5, np.uint8)
    rows = host[offset:offset + pitch * h].reshape(h, pitch)
    rows[:, :2 * w] = img.view(np.uint8).reshape(h, 2 * w)
    dev = torch.from_numpy(host.copy()).cuda()
    d, keep = abi.iiq_corr(ops, cfa)
    st = gpu.iiq_correct(d, abi.Image(dev.data_ptr() + offset, pitch, w, h, 1, 1))
    back = dev.cpu().numpy()
    got = back[offset:offset + pitch * h].reshape(h, pitch)
    mask = np.ones_like(back, bool)
    mask[offset:offset + pitch * h].reshape(h, pitch)[:, :2 * w] = False
    assert (back[mask] == 0xA5).all(), "bytes outside the image were written"
    return st, got[:, :2 * w].copy().view(np.uint16)


def _check(gpu, img, ops, cfa=None):
    st, want = K.apply(img, ops, cfa)
    assert st == K.OK
    h, w = img.shape
    for pitch in (None, 2 * w + 6):
        got_st, got = _on_host(gpu, img, ops, cfa, pitch)
        assert got_st == OK and np.array_equal(got, want), ("host", pitch)
    for pitch, off in ((2 * w, 0), (2 * w + 6, 0), (2 * w, 6)):
        got_st, got = _on_device(gpu, img, ops, cfa, pitch, off)
        assert got_st == OK and np.array_equal(got, want), ("device", pitch, off)
    return want


@pytest.mark.parametrize("name", sorted(HEADS))
@pytest.mark.parametrize("w,h", SIZES)
def test_luma_cells(gpu, w, h, name):
    rng = np.random.default_rng([1, w, len(name)])
    img = _image(rng, w, h)
    want = _check(gpu, img, [("ff", _payload(rng, HEADS[name]), 0)])
    if name in ("wide_1", "high_1", "zero"):
        assert np.array_equal(want, img)  # (nothing is written)
    else:
        assert (want != img).sum() > 20


@pytest.mark.parametrize("w,h", SIZES)
def test_luma_values(gpu, w, h):
    rng = np.random.default_rng([2, w])
    img = _image(rng, w, h)
    head = HEADS["8x8"]
    wide, high = K.ff_shape(head)
    same = _check(gpu, img, [("ff", K.ff_payload(head, np.full((high, wide), 32768)), 0)])
    assert np.array_equal(same, img)  # x 1.0
    top = _check(gpu, np.full((h, w), 65535, np.uint16),
                 [("ff", K.ff_payload(head, np.full((high, wide), 65535)), 0)])
    assert (top[:min(h, 32), :min(w, 64)] == 65535).all()  # 65535 x 1.99997 clamps
    zero = _check(gpu, img, [("ff", K.ff_payload(head, np.zeros((high, wide))), 0)])
    assert (zero[:32, :64] == 0).all()
    # targets that return to 0: the running sums end a hair above or below it, and a product in
    # (-1, 0) truncates to 0
    v = np.where((np.arange(high)[:, None] + np.arange(wide)[None, :]) % 2 == 0, 0, 3)
    drift = K.ff_payload((0, 0, 72, 40, 9, 13), v[:4, :8] + np.arange(8)[None, :] % 3)
    _check(gpu, np.full((h, w), 65535, np.uint16), [("ff", drift, 0)])
    _check(gpu, img, [("ff", _payload(rng, HEADS["7x5"], lo=0, hi=65535), 0)])


@pytest.mark.parametrize("cfa", [RGGB, GRBG, CFA_2X4], ids=["rggb", "grbg", "2x4"])
@pytest.mark.parametrize("w,h", SIZES)
def test_chroma(gpu, w, h, cfa):
    rng = np.random.default_rng([3, w, len(cfa[2])])
    img = _image(rng, w, h)
    for name in ("1x1", "7x5", "13x11", "8x8", "tall", "70x8", "33x8"):
        want = _check(gpu, img, [("ff", _payload(rng, HEADS[name], 2, lo=36000, hi=50000), 1)], cfa)
        assert (want != img).sum() > 20
    if cfa is GRBG:
        # an untransposed lookup corrects the wrong pixels of a GRBG image
        p = _payload(rng, HEADS["8x8"], 2, lo=36000, hi=50000)
        cw, ch, c = cfa
        swapped = (ch, cw, [c[x + y * cw] for x in range(cw) for y in range(ch)])
        st, got = _on_host(gpu, img, [("ff", p, 1)], cfa)
        assert np.array_equal(got, K.flat_field(img, p, True, cfa)[1])
        assert (got != K.flat_field(img, p, True, swapped)[1]).sum() > 100


@pytest.mark.parametrize("w,h", SIZES)
def test_quadrant(gpu, curves, w, h):
    rng = np.random.default_rng([4, w])
    img = _image(rng, w, h)
    img[1, :8] = (999, 1000, 1001, 0, 65535, 1000, 999, 1001)  # below, at and above the black level
    for split_row, split_col in ((0, 0), (h, w), (h // 2 + 1, 29), (1, w - 1)):
        for black in (0, 1000, 70000):
            want = _check(gpu, img, [("quad", curves, split_row, split_col, black)])
    # a sum that wraps past 65535: the curve's top value above a black level
    wrap = curves.copy()
    wrap[:, :16] = 65535
    want = _check(gpu, img, [("quad", wrap, h // 2, w // 2, 1000)])
    assert want[1, 1] == (65535 + 1000) & 0xFFFF


@pytest.mark.parametrize("w,h", SIZES)
def test_four_ops_fused(gpu, curves, w, h):
    rng = np.random.default_rng([5, w])
    img = _image(rng, w, h)
    ops = [("ff", _payload(rng, HEADS["7x5"]), 0),
           ("ff", _payload(rng, HEADS["13x11"], 2), 1),
           ("quad", curves, h // 2 - 1, w // 2 + 3, 1500),
           ("ff", _payload(rng, HEADS["8x8"]), 0)]
    step = img
    for op in ops:  # op by op
        st, step = K.apply(step, [op], GRBG)
    want = _check(gpu, img, ops, GRBG)
    assert np.array_equal(want, step)


def test_an_empty_list_writes_nothing(gpu):
    img = _image(np.random.default_rng(6), 64, 40)
    st, got = _on_host(gpu, img, [])
    assert st == OK and np.array_equal(got, img)


def _iiq(rng, w, h, seed):
    img = F.sample_image(rng, w, h)
    rows = F.encode(img, seed, (0.25, 0.1, 0.4))
    return img, rows, F.iiq_file(rows, w, rng, gap_max=5)


@pytest.mark.parametrize("w,h", SIZES)
def test_decode_and_correct_in_one_call(gpu, curves, w, h):
    rng = np.random.default_rng([7, w])
    img, rows, blob = _iiq(rng, w, h, 3)
    raw, strips, _, _ = F.iiq_strips(blob)
    ops = [("ff", _payload(rng, HEADS["7x5"]), 0), ("ff", _payload(rng, HEADS["8x8"], 2), 1),
           ("quad", curves, 17, 29, 1200)]
    st, want = K.apply(img, ops, RGGB)
    for pitch in (None, 2 * w + 6):
        out = HostImage(w, h, pitch=pitch)
        d, keep = abi.iiq_corr(ops, RGGB)
        got_st, row_st = gpu.phase_one_decompress_corrected(np.frombuffer(raw, np.uint8), strips, d, out.view())
        assert got_st == OK and not any(row_st)
        assert np.array_equal(out.pixels(), want)
        assert (out.buf.reshape(h, out.pitch)[:, 2 * w:] == 0xA5).all()
    # an empty list: the plain decode
    out = HostImage(w, h)
    d, keep = abi.iiq_corr([])
    got_st, _ = gpu.phase_one_decompress_corrected(np.frombuffer(raw, np.uint8), strips, d, out.view())
    assert got_st == OK and np.array_equal(out.pixels(), img)
    # a refused list, and a failing strip: the caller's image stays as it was
    d, keep = abi.iiq_corr([("ff", ops[0][1][:-1], 0)])
    out = HostImage(w, h)
    got_st, _ = gpu.phase_one_decompress_corrected(np.frombuffer(raw, np.uint8), strips, d, out.view())
    assert got_st == abi.RSX_ERR_IO and (out.buf == 0xA5).all()
    bad = F.iiq_file(F.damage(rows, h // 2, "col0", rng), w, rng, gap_max=5)
    raw, strips, _, _ = F.iiq_strips(bad)
    d, keep = abi.iiq_corr(ops, RGGB)
    got_st, row_st = gpu.phase_one_decompress_corrected(np.frombuffer(raw, np.uint8), strips, d, out.view())
    assert got_st == F.RSX_ERR_BAD_HUFFMAN_CODE and row_st[h // 2] == got_st
    assert (out.buf == 0xA5).all()


def _plan_jobs(curves, short=False):
    """two jobs of different geometry and different lists, behind one another in one buffer; job 1
    at an odd img_offset / 2 with a pitch off the 16-byte grid"""
    rng = np.random.default_rng(8)
    specs = [(64, 40, 128, [("ff", _payload(rng, HEADS["7x5"]), 0), ("quad", curves, 20, 33, 900)], None),
             (72, 38, 150, [("ff", _payload(rng, HEADS["13x11"], 2), 1), ("ff", _payload(rng, HEADS["8x8"]), 0)], GRBG)]
    jobs, keeps, layout = [], [], []
    off = 6
    for k, (w, h, pitch, ops, cfa) in enumerate(specs):
        if short and k == 1:
            ops = [ops[0], ("ff", ops[1][1][:-1], 0)]
        d, keep = abi.iiq_corr(ops, cfa)
        j = abi.IiqCorrectJob()
        j.corr = d
        j.img_offset = off
        j.img = abi.Image(None, pitch, w, h, 1, 1)
        jobs.append(j)
        keeps.append(keep)
        layout.append((off, pitch, w, h, _image(rng, w, h), ops, cfa))
        off += pitch * h + 10
    return jobs, keeps, layout, off


def _buffer(layout, total):
    host = np.full(total, 0xA5, np.uint8)
    for off, pitch, w, h, img, _, _ in layout:
        host[off:off + pitch * h].reshape(h, pitch)[:, :2 * w] = img.view(np.uint8).reshape(h, 2 * w)
    return host


def test_plan_of_two_jobs(gpu, curves):
    jobs, keeps, layout, total = _plan_jobs(curves)
    host = _buffer(layout, total)
    dev = torch.from_numpy(host.copy()).cuda()
    plan = gpu.iiq_correct_plan(jobs)
    plan.run(dev.data_ptr(), dev.data_ptr(), torch.cuda.current_stream().cuda_stream)
    rc, st, _ = plan.results()
    plan.close()
    assert rc == OK and st == [OK, OK]
    back = dev.cpu().numpy()
    want = host.copy()
    for off, pitch, w, h, img, ops, cfa in layout:
        # against the separate call, and against the model
        st1, alone = _on_device(gpu, img, ops, cfa, pitch, 6)
        st2, model = K.apply(img, ops, cfa)
        assert st1 == OK and st2 == K.OK and np.array_equal(alone, model)
        want[off:off + pitch * h].reshape(h, pitch)[:, :2 * w] = model.view(np.uint8).reshape(h, 2 * w)
    assert np.array_equal(back, want)  # (every byte between and around the images as it was)


def test_plan_with_a_short_payload_touches_no_image(gpu, curves):
    jobs, keeps, layout, total = _plan_jobs(curves, short=True)
    with pytest.raises(capi.RsxError) as e:
        gpu.iiq_correct_plan(jobs)
    assert e.value.status == abi.RSX_ERR_IO
    # (no plan, so nothing can run: both images are what they were; the separate call of job 0
    # still works)
    off, pitch, w, h, img, ops, cfa = layout[0]
    st, got = _on_device(gpu, img, ops, cfa, pitch, 6)
    assert st == OK and np.array_equal(got, K.apply(img, ops, cfa)[1])
    st, got = _on_device(gpu, layout[1][4], [layout[1][5][0], ("ff", layout[1][5][1][1][:-1], 0)], GRBG, 150, 6)
    assert st == abi.RSX_ERR_IO and np.array_equal(got, layout[1][4])
