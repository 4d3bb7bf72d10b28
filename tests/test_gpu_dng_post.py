"""DngDecoder's stage behind the tiles on the device (rsx_dng_post, the two _post fan-outs,
rsx_dng_post_plan_create; rawspeed_amd/csrc/rsx_dng_post.hip) through the C-ABI, against the numpy
model tests/dng_post_files.py -- which tests/test_dng_post_model.py pins against the reference's
whole-file decode, and which the host build of the same core matches on every case there.  The
position lists have no reference run (its shim does not hand them out): model only.

Shapes for the lane layout (a lane owns 8 uint16 samples, 4 floats): rows of 2, 6, 8, 10, 66, 520
and 1030 samples (cpp 1) and of 6, 9, 66, 519 and 1029 (cpp 3), heights 1, 2 and 37, an image base
and a pitch off the 16-byte grid with sentinel bytes around."""
import numpy as np
import pytest
import torch

import cases as C
import dng_post_files as K
from oracle_lib import HostImage
from rawspeed_amd import abi, capi

pytestmark = pytest.mark.gpu

OK = abi.RSX_OK
f32 = np.float32


@pytest.fixture(scope="module")
def gpu():
    import gpu_util
    return gpu_util.ctx()


def _on_host(gpu, img, cpp, crop, opcodes, table, pitch=None, bad_cap=1 << 16):
    img = np.asarray(img)
    bpc = img.dtype.itemsize
    h, ws = img.shape
    out = HostImage(ws // cpp, h, cpp=cpp, pitch=pitch, bpc=bpc)
    rows = out.buf.reshape(h, out.pitch)
    rows[:, :ws * bpc] = img.view(np.uint8).reshape(h, -1)
    before = out.buf.copy()
    d, keep = abi.dng_post_desc(opcodes, table, crop, bpc == 4)
    st, r, bad = gpu.dng_post(d, out.view(), bad_cap)
    assert (rows[:, ws * bpc:] == 0xA5).all(), "the pitch padding was written"
    if st not in (OK, K.UNSUPPORTED):
        assert np.array_equal(out.buf, before), "a refused list touched the image"
    return st, rows[:, :ws * bpc].copy().view(img.dtype), r, bad


def _on_device(gpu, img, cpp, crop, opcodes, table, pitch=None, offset=0, bad_cap=1 << 16):
    """through a device pointer: the image at byte `offset` of a buffer filled with 0xA5"""
    img = np.asarray(img)
    bpc = img.dtype.itemsize
    h, ws = img.shape
    pitch = pitch or ws * bpc
    host = np.full(offset + pitch * h + 32, 0xA5, np.uint8)
    rows = host[offset:offset + pitch * h].reshape(h, pitch)
    rows[:, :ws * bpc] = img.view(np.uint8).reshape(h, -1)
    dev = torch.from_numpy(host.copy()).cuda()
    d, keep = abi.dng_post_desc(opcodes, table, crop, bpc == 4)
    st, r, bad = gpu.dng_post(d, abi.Image(dev.data_ptr() + offset, pitch, ws // cpp, h, cpp, 1), bad_cap)
    back = dev.cpu().numpy()
    got = back[offset:offset + pitch * h].reshape(h, pitch)
    mask = np.ones_like(back, bool)
    mask[offset:offset + pitch * h].reshape(h, pitch)[:, :ws * bpc] = False
    assert (back[mask] == 0xA5).all(), "bytes outside the image were written"
    return st, got[:, :ws * bpc].copy().view(img.dtype), r, bad


def _same(got, want, what):
    st, px, r, bad = got
    mst, mimg, info = want
    assert st == mst, what
    assert px.tobytes() == mimg.tobytes(), what
    if st == OK:
        assert (r.list_status, r.list_reason, r.n_applied, r.crop()) == \
            (info["list_status"], info["reason"], info["n_applied"], info["crop"]), what
        assert bad == info["bad"], what
        assert r.n_bad == len(info["bad"]), what


def _check(gpu, img, cpp, crop, opcodes, table, ways="all"):
    want = K.apply(img, cpp, crop, opcodes, table)
    bpc = np.asarray(img).dtype.itemsize
    row = img.shape[1] * bpc
    odd = 6 if bpc == 2 else 4
    for pitch in (None, row + odd):
        _same(_on_host(gpu, img, cpp, crop, opcodes, table, pitch), want, ("host", pitch))
    for pitch, off in ((row, 0), (row + odd, 0), (row, odd), (row + odd, odd)):
        _same(_on_device(gpu, img, cpp, crop, opcodes, table, pitch, off), want, ("device", pitch, off))
    return want


@pytest.mark.parametrize("name", [c[0] for c in K.file_cases()])
def test_reference_cases(gpu, name):
    case = {c[0]: c for c in K.file_cases()}[name]
    _, img, cpp, opcodes, table, aa = case
    _check(gpu, img, cpp, K.case_crop(case), opcodes, table)


def _random_list(rng, w, h, cpp, n_ops, codes=(7, 10, 11, 12, 13)):
    """ops inside a w x h crop: odd offsets, pitches 1..3, plane windows"""
    ops = []
    for _ in range(n_ops):
        code = int(rng.choice(codes))
        left = int(rng.integers(0, max(1, w // 2)))
        top = int(rng.integers(0, max(1, h // 2)))
        right = int(rng.integers(left + 1, w + 1))
        bottom = int(rng.integers(top + 1, h + 1))
        roi = (top, left, bottom, right)
        first = int(rng.integers(0, cpp))
        planes = (first, int(rng.integers(1, cpp - first + 1)))
        pitch = (int(rng.integers(1, min(3, bottom - top) + 1)), int(rng.integers(1, min(3, right - left) + 1)))
        if code == 7:
            ops.append(K.op_table(roi, rng.integers(0, 65536, size=int(rng.integers(1, 600))), planes, pitch))
        else:
            extent, p = (right - left, pitch[1]) if code in (11, 13) else (bottom - top, pitch[0])
            lo, hi = (-1.0, 1.0) if code <= 11 else (0.0, 3.0)
            ops.append(K.op_delta(code, roi, rng.uniform(lo, hi, size=-(-extent // p)).astype(f32), planes, pitch))
    return ops


SHAPES = [(1, ws) for ws in (2, 6, 8, 10, 66, 520, 1030)] + [(3, ws) for ws in (6, 9, 66, 519, 1029)]


@pytest.mark.parametrize("h", (1, 2, 37))
@pytest.mark.parametrize("cpp,ws", SHAPES)
def test_lane_layout_shapes(gpu, cpp, ws, h):
    rng = np.random.default_rng([3, cpp, ws, h])
    w = ws // cpp
    img = rng.integers(0, 65536, size=(h, ws)).astype(np.uint16)
    img[::3, ::5] = 9
    ops = _random_list(rng, w, h, cpp, 5)
    if cpp == 1:
        ops.insert(3, K.op_bad_constant(9))
    table = np.sort(rng.integers(0, 65536, size=700)).astype(np.uint16)
    want = _check(gpu, img, cpp, (0, 0, w, h), K.opcode_list(ops), table)
    assert want[2]["n_applied"] == len(ops)


@pytest.mark.parametrize("cpp,ws", [(1, 66), (3, 66), (1, 10)])
def test_f32_shapes(gpu, cpp, ws):
    rng = np.random.default_rng([4, cpp, ws])
    w, h = ws // cpp, 7
    img = rng.uniform(-2, 2, size=(h, ws)).astype(f32)
    ops = _random_list(rng, w, h, cpp, 5, codes=(10, 11, 12, 13))
    want = _check(gpu, img, cpp, (0, 0, w, h), K.opcode_list(ops), None)
    assert (want[1] != img).sum() > 5


def test_crop_offsets_move_every_opcode(gpu):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 65536, size=(37, 66)).astype(np.uint16)
    ops = _random_list(rng, 50, 30, 1, 4) + [K.op_trim((3, 5, 27, 45))] + _random_list(rng, 40, 24, 1, 3)
    table = rng.integers(0, 65536, size=65536).astype(np.uint16)
    want = _check(gpu, img, 1, (7, 2, 50, 30), K.opcode_list(ops), table)
    assert want[2]["crop"] == (12, 5, 40, 24)


def test_sixteen_opcodes_and_one_more(gpu):
    rng = np.random.default_rng(6)
    img = rng.integers(0, 65536, size=(20, 70)).astype(np.uint16)
    ops = _random_list(rng, 70, 20, 1, 16)
    _check(gpu, img, 1, (0, 0, 70, 20), K.opcode_list(ops), None)
    # TrimBounds and FixBadPixelsList are no pixel opcodes: the cap counts the sixteen alone
    more = ops[:8] + [K.op_trim((0, 0, 20, 70)), K.op_bad_list([(1, 1)])] + ops[8:]
    _check(gpu, img, 1, (0, 0, 70, 20), K.opcode_list(more), None)
    st, px, r, bad = _on_host(gpu, img, 1, (0, 0, 70, 20), K.opcode_list(ops + ops[:1]), None)
    assert st == K.UNSUPPORTED and np.array_equal(px, img)


@pytest.mark.parametrize("hits", ["none", "one", "everywhere"])
def test_bad_constant_hits(gpu, hits):
    """no hit, one hit, hits in every workgroup (600 x 30 is 9 workgroups of 256 lanes)"""
    rng = np.random.default_rng(7)
    img = rng.integers(100, 65536, size=(30, 600)).astype(np.uint16)
    if hits == "one":
        img[17, 333] = 5
    elif hits == "everywhere":
        img[:, ::7] = 5
    ops = [K.op_bad_constant(5), K.op_table((0, 0, 30, 600), [5]), K.op_bad_constant(5)]
    want = _check(gpu, img, 1, (0, 0, 600, 30), K.opcode_list(ops), None)
    first = {"none": 0, "one": 1, "everywhere": 30 * 86}[hits]
    assert len(want[2]["bad"]) == first + 30 * 600  # (behind the table every pixel is 5)
    assert want[2]["bad"][:first] == sorted(want[2]["bad"][:first])


def test_bad_constant_past_the_capacity(gpu):
    rng = np.random.default_rng(8)
    img = rng.integers(100, 65536, size=(30, 600)).astype(np.uint16)
    img[:, ::7] = 5
    ops = K.opcode_list([K.op_bad_list([(2, 2)]), K.op_bad_constant(5), K.op_delta(10, (0, 0, 30, 600), [0.5] * 30)])
    st, want, info = K.apply(img, 1, (0, 0, 600, 30), ops, None)
    n = len(info["bad"])
    assert n == 1 + 30 * 86
    for run in (_on_host, _on_device):
        got = run(gpu, img, 1, (0, 0, 600, 30), ops, None, bad_cap=n)
        _same(got, (st, want, info), run.__name__)
        st2, px, r, bad = run(gpu, img, 1, (0, 0, 600, 30), ops, None, bad_cap=n - 1)
        # the image is complete, the count exact, the list is not handed out
        assert st2 == K.UNSUPPORTED and r.n_bad == n and bad is None
        assert np.array_equal(px, want)
        st3, px, r, bad = run(gpu, img, 1, (0, 0, 600, 30), ops, None, bad_cap=0)
        assert st3 == K.UNSUPPORTED and r.n_bad == n and np.array_equal(px, want)


def test_plan_of_three_jobs(gpu):
    """three images in one buffer, different lists, tables, geometry and sample type"""
    rng = np.random.default_rng(9)
    specs = [(1, 66, 37, np.uint16), (3, 519, 5, np.uint16), (1, 10, 9, f32)]
    jobs, wants, keep, placed = [], [], [], []
    offset = 6
    for k, (cpp, ws, h, dt) in enumerate(specs):
        w = ws // cpp
        if dt is f32:
            img = rng.uniform(-1, 1, size=(h, ws)).astype(f32)
            ops = _random_list(rng, w, h, cpp, 3, codes=(10, 13))
            table = None
            offset += -offset % 4
        else:
            img = rng.integers(0, 65536, size=(h, ws)).astype(np.uint16)
            img[::2, ::3] = 11
            ops = _random_list(rng, w, h, cpp, 4) + ([K.op_bad_constant(11)] if cpp == 1 else [])
            table = rng.integers(0, 65536, size=300 + k).astype(np.uint16)
        opcodes = K.opcode_list(ops)
        pitch = ws * img.itemsize + (6 if dt is not f32 else 4)
        d, kp = abi.dng_post_desc(opcodes, table, (0, 0, w, h), dt is f32)
        keep.append(kp)
        j = abi.DngPostJob()
        j.desc, j.img_offset, j.bad_cap = d, offset, 1 << 16
        j.img = abi.Image(None, pitch, w, h, cpp, 1)
        jobs.append(j)
        wants.append(K.apply(img, cpp, (0, 0, w, h), opcodes, table))
        placed.append((offset, pitch, img))
        offset += pitch * h + 10
    host = np.full(offset + 32, 0xA5, np.uint8)
    mask = np.ones_like(host, bool)
    for off, pitch, img in placed:
        h, ws = img.shape
        rows = host[off:off + pitch * h].reshape(h, pitch)
        rows[:, :ws * img.itemsize] = img.view(np.uint8).reshape(h, -1)
        mask[off:off + pitch * h].reshape(h, pitch)[:, :ws * img.itemsize] = False
    dev = torch.from_numpy(host.copy()).cuda()
    plan = gpu.dng_post_plan(jobs)
    plan.run(dev.data_ptr(), dev.data_ptr(), torch.cuda.current_stream().cuda_stream)
    rc, st, _ = plan.results()
    assert rc == OK and st == [OK] * 3
    back = dev.cpu().numpy()
    assert (back[mask] == 0xA5).all(), "bytes outside the images were written"
    for k, ((off, pitch, img), (mst, mimg, info)) in enumerate(zip(placed, wants)):
        h, ws = img.shape
        got = back[off:off + pitch * h].reshape(h, pitch)[:, :ws * img.itemsize]
        assert got.tobytes() == mimg.tobytes(), k
        rst, r = plan.result(k)
        assert rst == OK and (r.n_applied, r.crop()) == (info["n_applied"], info["crop"]), k
        bst, n, bad = plan.bad_pixels(k, 1 << 16)
        assert (bst, n, bad) == (OK, len(info["bad"]), info["bad"]), k
    assert len(wants[0][2]["bad"]) > 0
    plan.close()


def test_a_refused_job_fails_plan_creation(gpu):
    d, keep = abi.dng_post_desc(K.opcode_list([K.op_bad_constant(1)])[:-3], None, (0, 0, 8, 6))
    j = abi.DngPostJob()
    j.desc, j.img = d, abi.Image(None, 16, 8, 6, 1, 1)
    with pytest.raises(capi.RsxError) as e:
        gpu.dng_post_plan([j])
    assert e.value.status == K.IO


def test_wide_rows_share_workgroups_and_jump_past_65536_samples(gpu):
    """70000 samples x 3 rows: 35 workgroups a row, the generator jumped up to 69992 steps"""
    rng = np.random.default_rng(10)
    img = rng.integers(0, 65536, size=(3, 70000)).astype(np.uint16)
    table = np.sort(rng.integers(0, 65536, size=4096)).astype(np.uint16)
    ops = K.opcode_list([K.op_delta(13, (0, 1, 3, 69999), rng.uniform(0, 2, size=34999).astype(f32),
                                    pitch=(1, 2))])
    want = K.apply(img, 1, (0, 0, 70000, 3), ops, table)
    _same(_on_device(gpu, img, 1, (0, 0, 70000, 3), ops, table), want, "device")
    _same(_on_host(gpu, img, 1, (0, 0, 70000, 3), ops, table), want, "host")


def test_the_row_whose_seed_ends_in_ffff(gpu):
    """dim_x + 13 y = 0xBA7B: the seed's low half is 65535 and the state after its first step is
    not below the modulus (rsx_dng_post_core.h) -- the lane of sample 0 must step the seed itself"""
    w = 0xBA7B - 13 * 2
    rng = np.random.default_rng(11)
    img = rng.integers(0, 65536, size=(4, w)).astype(np.uint16)
    table = np.sort(rng.integers(0, 65536, size=4096)).astype(np.uint16)
    assert (K.dither_states(w, [2], 1)[0, 0]) >= 15700 * 65536 - 1
    want = K.apply(img, 1, (0, 0, w, 4), None, table)
    _same(_on_device(gpu, img, 1, (0, 0, w, 4), None, table), want, "device")


# ---------------------------------------------------------------------------------------
# the fan-outs
# ---------------------------------------------------------------------------------------
def _ljpeg_tiles(rng, W, H, tw, th):
    descs, datas = [], []
    for ty in range(2):
        for tx in range(2):
            d, data, _, _ = C.make_ljpeg_case(rng, img_w=W, img_h=H, cpp=1,
                                              tile=(tx * tw, ty * th, min(tw, W - tx * tw), min(th, H - ty * th)),
                                              mcu=(2, 1), frame=(tw // 2, th))
            descs.append(d)
            datas.append(data)
    return descs, datas


def _ljpeg_grid(rng, W, H, tw, th):
    descs, datas = [], []
    for ty in range(-(-H // th)):
        for tx in range(-(-W // tw)):
            d, data, _, _ = C.make_ljpeg_case(rng, img_w=W, img_h=H, cpp=1,
                                              tile=(tx * tw, ty * th, min(tw, W - tx * tw), min(th, H - ty * th)),
                                              mcu=(2, 1), frame=(tw // 2, th))
            descs.append(d)
            datas.append(data)
    return descs, datas


def _post_list(rng, W, H):
    ops = _random_list(rng, W, H, 1, 4) + [K.op_bad_constant(3), K.op_trim((1, 2, H - 1, W - 2))]
    return K.opcode_list(ops), np.sort(rng.integers(0, 65536, size=1000)).astype(np.uint16)


def test_ljpeg_fan_out_with_the_pass(gpu):
    """2 x 2 LJPEG tiles: the _post call against the plain call followed by the model"""
    rng = np.random.default_rng(12)
    W, H = 250, 61
    descs, datas = _ljpeg_tiles(rng, W, H, 128, 32)
    plain = HostImage(W, H)
    rc, st, _ = gpu.dng_decompress_ljpeg(descs, datas, plain.view())
    assert rc == OK
    opcodes, table = _post_list(rng, W, H)
    mst, want, info = K.apply(plain.pixels(), 1, (0, 0, W, H), opcodes, table)
    d, keep = abi.dng_post_desc(opcodes, table, (0, 0, W, H))
    got = HostImage(W, H)
    rc, st, r, bad = gpu.dng_decompress_ljpeg_post(descs, datas, d, got.view())
    assert rc == OK and not any(st)
    assert np.array_equal(got.pixels(), want)
    assert (got.u16()[:, W:] == 0xA5A5).all()
    assert (r.n_applied, r.crop(), bad) == (info["n_applied"], info["crop"], info["bad"])
    assert r.crop() == (2, 1, W - 4, H - 2)


def test_ljpeg_fan_out_with_more_tiles_than_the_download_merges(gpu):
    """9 x 8 = 72 tiles (the plain call merges up to 64 rectangles into one download; the pass
    does not depend on that): decoded, processed, one download"""
    rng = np.random.default_rng(17)
    W, H = 270, 120
    descs, datas = _ljpeg_grid(rng, W, H, 32, 16)
    assert len(descs) == 72
    plain = HostImage(W, H)
    rc, st, _ = gpu.dng_decompress_ljpeg(descs, datas, plain.view())
    assert rc == OK
    opcodes, table = _post_list(rng, W, H)
    mst, want, info = K.apply(plain.pixels(), 1, (0, 0, W, H), opcodes, table)
    d, keep = abi.dng_post_desc(opcodes, table, (0, 0, W, H))
    got = HostImage(W, H)
    rc, st, r, bad = gpu.dng_decompress_ljpeg_post(descs, datas, d, got.view())
    assert rc == OK and st == [OK] * 72
    assert np.array_equal(got.pixels(), want)
    assert (got.u16()[:, W:] == 0xA5A5).all()
    assert (r.n_applied, r.crop(), bad) == (info["n_applied"], info["crop"], info["bad"])


@pytest.mark.parametrize("how", ["missing", "twice", "overlap"])
def test_ljpeg_fan_out_refuses_tiles_that_do_not_tile_the_image(gpu, how):
    """refused before anything is decoded: the image and the statuses stay as the caller set them"""
    rng = np.random.default_rng(18)
    W, H = 270, 120
    descs, datas = _ljpeg_grid(rng, W, H, 32, 16)
    if how == "missing":
        del descs[40], datas[40]
    elif how == "twice":  # (the right number of tiles and the right area, one place empty)
        descs[40], datas[40] = descs[41], datas[41]
    else:
        descs[40].tile_x -= 2
    opcodes, table = _post_list(rng, W, H)
    d, keep = abi.dng_post_desc(opcodes, table, (0, 0, W, H))
    got = HostImage(W, H)
    rc, st, r, bad = gpu.dng_decompress_ljpeg_post(descs, datas, d, got.view())
    assert rc == K.UNSUPPORTED and st == [-1] * len(descs)
    assert (got.buf == 0xA5).all()


def test_ljpeg_fan_out_with_a_failing_tile_is_the_plain_call(gpu):
    rng = np.random.default_rng(13)
    W, H = 250, 61
    descs, datas = _ljpeg_tiles(rng, W, H, 128, 32)
    datas[2] = datas[2][:len(datas[2]) // 3]
    plain = HostImage(W, H)
    prc, pst, _ = gpu.dng_decompress_ljpeg(descs, datas, plain.view())
    assert prc != OK and pst[2] != OK
    opcodes, table = _post_list(rng, W, H)
    d, keep = abi.dng_post_desc(opcodes, table, (0, 0, W, H))
    got = HostImage(W, H)
    rc, st, r, bad = gpu.dng_decompress_ljpeg_post(descs, datas, d, got.view())
    assert (rc, st) == (prc, pst)
    assert np.array_equal(got.buf, plain.buf)  # (nothing of the list or the look-up)


def test_ljpeg_fan_out_refuses_a_list_that_fails_the_file(gpu):
    rng = np.random.default_rng(14)
    W, H = 250, 61
    descs, datas = _ljpeg_tiles(rng, W, H, 128, 32)
    opcodes, table = _post_list(rng, W, H)
    d, keep = abi.dng_post_desc(opcodes[:-5], table, (0, 0, W, H))
    got = HostImage(W, H)
    rc, st, r, bad = gpu.dng_decompress_ljpeg_post(descs, datas, d, got.view())
    assert rc == K.IO and (got.buf == 0xA5).all() and st == [-1] * 4


def test_uncompressed_fan_out_with_the_pass(gpu):
    """packed 12-bit strips, and 2 x 2 tiles of 16-bit samples"""
    rng = np.random.default_rng(15)
    for W, H, tw, th, bps, order in ((40, 13, 40, 8, 12, abi.ORDER_MSB), (40, 13, 24, 8, 16, abi.ORDER_LSB)):
        descs, datas = [], []
        for ty in range(2):
            for tx in range(-(-W // tw)):
                pitch = tw * bps // 8
                datas.append(rng.integers(0, 256, size=th * pitch, dtype=np.uint8))
                descs.append(abi.UnpackDesc(tx * tw, ty * th, min(tw, W - tx * tw), min(th, H - ty * th),
                                            pitch, bps, order))
        plain = HostImage(W, H)
        rc, st = gpu.dng_decompress_uncompressed(descs, datas, plain.view())
        assert rc == OK
        opcodes, table = _post_list(rng, W, H)
        mst, want, info = K.apply(plain.pixels(), 1, (0, 0, W, H), opcodes, table)
        d, keep = abi.dng_post_desc(opcodes, table, (0, 0, W, H))
        got = HostImage(W, H)
        rc, st, r, bad = gpu.dng_decompress_uncompressed_post(descs, datas, d, got.view())
        assert rc == OK and not any(st), bps
        assert np.array_equal(got.pixels(), want), bps
        assert (got.u16()[:, W:] == 0xA5A5).all()
        assert (r.n_applied, r.crop(), bad) == (info["n_applied"], info["crop"], info["bad"])
        # a failing tile: the plain call's status and image
        descs[1] = abi.UnpackDesc(descs[1].crop_x, descs[1].crop_y, descs[1].crop_w, 8, 5, bps, order)
        plain, got = HostImage(W, H), HostImage(W, H)
        prc, pst = gpu.dng_decompress_uncompressed(descs, datas, plain.view())
        rc, st, r, bad = gpu.dng_decompress_uncompressed_post(descs, datas, d, got.view())
        assert prc != OK and (rc, st) == (prc, pst) and np.array_equal(got.buf, plain.buf), bps


def test_uncompressed_fan_out_refuses_packed_tiles_side_by_side(gpu):
    """the reference writes a packed tile from column 0 whatever its offset: only the plain call
    keeps the order in which such tiles land on each other"""
    rng = np.random.default_rng(16)
    descs = [abi.UnpackDesc(tx * 24, 0, min(24, 40 - tx * 24), 13, 36, 12, abi.ORDER_MSB) for tx in range(2)]
    datas = [rng.integers(0, 256, size=13 * 36, dtype=np.uint8) for _ in range(2)]
    d, keep = abi.dng_post_desc(None, [1, 2, 3], (0, 0, 40, 13))
    got = HostImage(40, 13)
    rc, st, r, bad = gpu.dng_decompress_uncompressed_post(descs, datas, d, got.view())
    assert rc == K.UNSUPPORTED and (got.buf == 0xA5).all() and st == [-1, -1]


def test_uncompressed_fan_out_refuses_tiles_that_overlap_with_the_right_area(gpu):
    """two 20-column tiles of 16-bit samples on a 40-column image, one of them 4 columns off its
    place: the areas add up to the image, the tiles share columns and leave others out"""
    rng = np.random.default_rng(19)
    d, keep = abi.dng_post_desc(None, [1, 2, 3], (0, 0, 40, 13))
    for xs in ((0, 16), (4, 20)):
        descs = [abi.UnpackDesc(x, 0, 20, 13, 40, 16, abi.ORDER_LSB) for x in xs]
        datas = [rng.integers(0, 256, size=13 * 40, dtype=np.uint8) for _ in range(2)]
        got = HostImage(40, 13)
        rc, st, r, bad = gpu.dng_decompress_uncompressed_post(descs, datas, d, got.view())
        assert rc == K.UNSUPPORTED and (got.buf == 0xA5).all() and st == [-1, -1], xs
