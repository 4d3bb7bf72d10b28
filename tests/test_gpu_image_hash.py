"""rstest's image hash and identify's sums on the device (rsx_image_hash*, rawspeed_amd/csrc/
rsx_image_hash.hip) through the C-ABI.  Every expectation comes from hashlib and numpy on the host
(tests/image_hash_files.py); every output buffer starts as 0xA5 and is compared whole.  Row lengths
around MD5's padding edge, heights around the wavefront, pitches and base offsets that take each of
the kernel's three load paths, both kinds of pointers, a plan of mixed jobs with a refused one, the
hash plan chained behind an unpack plan against hashes recorded from the reference, and the edges of
the plan layout: an image based past 4 GiB, one whose rows cross 4 GiB, 65 537 jobs."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import golden_cases as G
import image_hash_files as F
from oracle_lib import HostImage
from rawspeed_amd import abi, capi

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(__file__), "golden", "golden_hashes.json")) as f:
    GOLD = json.load(f)


@pytest.fixture(scope="module")
def gpu():
    import gpu_util
    return gpu_util.ctx()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _on_device(gpu, L, lines=True):
    """rsx_image_hash on a device copy of the layout's buffer (exactly its bytes)"""
    buf = _dev(L.buf)
    assert buf.data_ptr() % 256 == 0
    out = gpu.image_hash(L.view(buf.data_ptr()), L.sample_bytes, lines)
    return out, buf


class kernel_choice:
    """RSX_IMAGE_HASH_KERNEL for the block (read when a plan is made): None or "direct" for the row
    kernel that ships, "lds" for the variant that stages the blocks through LDS."""

    def __init__(self, which):
        self.which = which

    def __enter__(self):
        if self.which:
            os.environ["RSX_IMAGE_HASH_KERNEL"] = self.which

    def __exit__(self, *a):
        os.environ.pop("RSX_IMAGE_HASH_KERNEL", None)


KERNELS = [None, "lds"]


def _check_layouts(gpu, w, cpp, sb, heights, kernel=None):
    with kernel_choice(kernel):
        return _check_layouts_now(gpu, w, cpp, sb, heights)


def _check_layouts_now(gpu, w, cpp, sb, heights):
    rng = np.random.default_rng([7, w, cpp, sb])
    # tight, row_bytes + 2 (+ 4: an F32 pitch is a multiple of 4), row_bytes + 16;
    # base offsets 0, 2 and 14 (0, 4 and 12)
    pads = (0, 2, 16) if sb == 2 else (0, 4, 16)
    leads = (0, 2, 14) if sb == 2 else (0, 4, 12)
    paths = set()
    for h in heights:
        for pad in pads:
            for lead in leads:
                L = F.Layout(rng, w, h, cpp, sb, pad=pad, lead=lead)
                want = L.want()
                (st, r, lines), buf = _on_device(gpu, L)
                assert st == F.OK and lines == want[0] and F.same(r, want), (h, pad, lead)
                # the padding rewritten: the same results from the same device buffer
                L.rewrite_padding()
                buf.copy_(torch.from_numpy(L.buf))
                st, r, lines = gpu.image_hash(L.view(buf.data_ptr()), sb, False)
                assert st == F.OK and lines is None and F.same(r, want), (h, pad, lead)
                # ... and through host pointers
                st, r, lines = gpu.image_hash(L.view(), sb)
                assert st == F.OK and lines == want[0] and F.same(r, want), (h, pad, lead)
                grid = lead | L.pitch
                paths.add(16 if grid % 16 == 0 else 4 if grid % 4 == 0 else 2)
    return paths


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("w", F.WIDTHS_U16)
def test_u16_rows_around_the_padding_edge(gpu, w, kernel):
    assert 2 in _check_layouts(gpu, w, 1, 2, F.HEIGHTS, kernel)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("w", F.WIDTHS_U16_CPP3)
def test_u16_three_samples_a_pixel(gpu, w, kernel):
    _check_layouts(gpu, w, 3, 2, F.HEIGHTS, kernel)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("w", F.WIDTHS_F32)
def test_f32_rows(gpu, w, kernel):
    assert _check_layouts(gpu, w, 1, 4, F.HEIGHTS, kernel) >= {4}


@pytest.mark.parametrize("kernel", KERNELS + ["direct"])
def test_every_load_path_is_taken(gpu, kernel):
    # width 32: row_bytes 64, so pitch 64 / 80 on base 0 is the 16-byte path (the one the staged
    # kernel replaces), 66 the 2-byte one, base 2 or 14 the 2-byte one; width 30 with pitch 60 + 0 /
    # 4 on base 0 the 4-byte one
    assert _check_layouts(gpu, 32, 1, 2, F.HEIGHTS, kernel) == {16, 2}
    assert 4 in _check_layouts(gpu, 30, 1, 2, (65,), kernel)
    assert _check_layouts(gpu, 16, 1, 4, F.HEIGHTS, kernel) == {16, 4}


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("w,sb", [(4099, 2), (32768, 2), (4099, 4)])
def test_long_rows(gpu, w, sb, kernel):
    _check_layouts(gpu, w, 1, sb, (1, 65), kernel)


@pytest.mark.parametrize("sb", (2, 4))
def test_sums(gpu, sb):
    rng = np.random.default_rng(8)
    w, h = 2056, 130
    for value in (0xFF, None):
        L = F.Layout(rng, w, h, 1, sb, pad=16, value=value)
        want = L.want()
        (st, r, lines), _ = _on_device(gpu, L)
        assert st == F.OK and lines == want[0] and F.same(r, want)
        if value is not None:
            assert r.byte_sum == 255 * w * sb * h
        assert r.sample_sum == ((0xFFFF * w * h if value else want[3]) if sb == 2 else 0)
        assert (r.sample_sum != 0) == (sb == 2)


def test_both_pointer_kinds_count_as_one_host_call_each(gpu):
    rng = np.random.default_rng(9)
    L = F.Layout(rng, 29, 65, 1, 2, pad=2, lead=2)
    want = L.want()
    buf = _dev(L.buf)
    for view in (L.view(), L.view(buf.data_ptr())):
        for with_lines in (True, False):
            before = gpu.host_calls()
            st, r, lines = gpu.image_hash(view, 2, with_lines)
            assert gpu.host_calls() == before + 1
            assert st == F.OK and F.same(r, want)
            assert lines == (want[0] if with_lines else None)


def test_refusals_write_nothing(gpu):
    rng = np.random.default_rng(10)
    L = F.Layout(rng, 8, 4, 1, 4)
    buf = _dev(L.buf)
    r = abi.ImageHashResult()
    lib = capi.lib()
    for base in (L.buf.ctypes.data, buf.data_ptr()):
        for view, sb, want in [(abi.Image(base, 30, 8, 4, 1, 0), 4, F.INVALID_ARG),
                               (abi.Image(base, 32, 8, 4, 1, 0), 3, F.INVALID_ARG),
                               (abi.Image(base, 32, 8, 0, 1, 0), 4, F.INVALID_ARG),
                               (abi.Image(base + 2, 32, 7, 4, 1, 0), 4, F.INVALID_ARG),
                               (abi.Image(base + 1, 32, 8, 4, 1, 0), 2, F.INVALID_ARG),
                               (abi.Image(None, 32, 8, 4, 1, 0), 4, F.INVALID_ARG),
                               (abi.Image(base, 1 << 28, 1 << 27, 1, 1, 0), 2, F.UNSUPPORTED)]:
            before = gpu.host_calls()
            st, res, lines = gpu.image_hash(view, sb)
            assert st == want
            assert bytes(res) == b"\xa5" * 32 and lines == b"\xa5" * max(16, 16 * view.dim_y)
            assert gpu.host_calls() == before + (0 if view.data is None else 1)
        v = abi.Image(base, 32, 8, 4, 1, 0)
        assert lib.rsx_image_hash(gpu._h, C.byref(v), 4, None, None) == F.INVALID_ARG
        assert lib.rsx_image_hash(gpu._h, None, 4, None, C.byref(r)) == F.INVALID_ARG


class Packed:
    """Jobs of a plan packed into one input and one output buffer: images one behind the other at
    offsets on their own grids, digests and results likewise; the expected output buffer alongside."""

    def __init__(self, rng):
        self.rng, self.jobs, self.parts, self.in_size = rng, [], [], 0
        self.out_size, self.places = 0, []

    def add(self, w, h, cpp, sb, pad=0, gap=0, refuse=None):
        L = F.Layout(self.rng, w, h, cpp, sb, pad=pad)
        img_off = (self.in_size + gap + sb - 1) // sb * sb
        self.parts.append(self.rng.integers(0, 256, img_off - self.in_size, dtype=np.uint8))
        self.parts.append(L.buf)
        self.in_size = img_off + L.size
        lines_off = (self.out_size + 15) // 16 * 16 + (16 if gap else 0)
        result_off = lines_off + 16 * h + (8 if (gap // sb) % 2 else 0)
        self.out_size = result_off + 32
        j = abi.image_hash_job(img_off, lines_off, result_off, sb, w, h, cpp, L.pitch)
        if refuse == "pitch":
            j.img.pitch_bytes = L.row_bytes - sb
        elif refuse == "lines":
            j.lines_offset += 8
        elif refuse == "result":
            j.result_offset += 4
        elif refuse == "image":
            j.img_offset += sb // 2
        elif refuse == "rows":
            j.img.dim_y = 1 << 24
        self.jobs.append(j)
        self.places.append((L, lines_off, result_off, refuse))
        return L

    def input(self):
        return np.concatenate(self.parts)

    def want(self, size=None):
        out = np.full(self.out_size if size is None else size, 0xA5, np.uint8)
        for L, lines_off, result_off, refuse in self.places:
            if refuse:
                continue
            lines, md5, bs, ss = L.want()
            out[lines_off:lines_off + len(lines)] = np.frombuffer(lines, np.uint8)
            out[result_off:result_off + 32] = np.frombuffer(F.result_bytes(md5, bs, ss), np.uint8)
        return out


@pytest.mark.parametrize("kernel", KERNELS)
def test_plan_of_70_mixed_jobs_with_refused_ones(gpu, kernel):
    with kernel_choice(kernel):
        _plan_of_70(gpu)


def _plan_of_70(gpu):
    rng = np.random.default_rng(11)
    P = Packed(rng)
    refusals = {17: ("pitch", F.INVALID_ARG), 30: ("rows", F.UNSUPPORTED),
                41: ("lines", F.INVALID_ARG), 42: ("result", F.INVALID_ARG),
                43: ("image", F.INVALID_ARG)}
    shapes = [(1, 1), (27, 63), (28, 64), (29, 65), (31, 130), (32, 3), (91, 7), (96, 66), (301, 5)]
    for k in range(70):
        w, h = shapes[k % len(shapes)]
        sb = 4 if k % 3 == 1 else 2
        cpp = 3 if k % 7 == 2 else 1
        P.add(w, h, cpp, sb, pad=(0, sb, 16, 3 * sb)[k % 4], gap=(0, 1, 6, 21)[k % 4] * sb,
              refuse=refusals.get(k, (None,))[0])
    inp = _dev(P.input())
    want = P.want(P.out_size + 48)
    outs = []
    plan = gpu.image_hash_plan(P.jobs)
    plan.set_timing(True)
    for run in range(2):
        out = torch.full((P.out_size + 48,), 0xA5, dtype=torch.uint8, device="cuda")
        plan.run(inp.data_ptr(), out.data_ptr())
        rc, st, cons = plan.results()
        assert st == [refusals.get(k, (None, F.OK))[1] for k in range(70)]
        assert rc == F.INVALID_ARG and cons == [0] * 70
        outs.append(out.cpu().numpy())
        assert np.array_equal(outs[-1], want), np.flatnonzero(outs[-1] != want)[:8]
    names = [n for n, _ in plan.kernel_table()[0]]
    plan.close()
    assert names == ["image_hash_rows_kernel", "image_hash_finish_kernel"]
    # 65 jobs go to the device: the finish kernel spans two wavefronts
    assert sum(1 for s in st if s == F.OK) == 65


def test_a_plan_whose_every_job_is_refused_and_bases_off_their_grids(gpu):
    rng = np.random.default_rng(12)
    P = Packed(rng)
    P.add(8, 2, 1, 2, refuse="pitch")
    out = torch.full((P.out_size,), 0xA5, dtype=torch.uint8, device="cuda")
    inp = _dev(P.input())
    plan = gpu.image_hash_plan(P.jobs)
    plan.run(inp.data_ptr(), out.data_ptr())
    assert plan.results() == (F.INVALID_ARG, [F.INVALID_ARG], [0])
    plan.close()
    assert (out.cpu().numpy() == 0xA5).all()
    P = Packed(rng)
    P.add(8, 2, 1, 4)
    inp = _dev(np.concatenate([P.input(), np.zeros(16, np.uint8)]))
    out = torch.full((P.out_size + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    plan = gpu.image_hash_plan(P.jobs)
    for din, dout in ((2, 0), (1, 0), (0, 8), (0, 4)):
        with pytest.raises(capi.RsxError) as e:
            plan.run(inp.data_ptr() + din, out.data_ptr() + dout)
        assert e.value.status == F.INVALID_ARG
    plan.close()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xA5).all()


UNPACK_2056 = [i for i, c in enumerate(G.UNPACK_CASES) if c["w"] == 2056]


def test_chained_behind_an_unpack_plan(gpu):
    """the golden unpack cases of width 2056 decoded by one plan, hashed by another right behind it
    on the same stream and in the same buffer, no host wait in between: the hex-joined hashes are
    the ones recorded from the reference"""
    import gpu_util
    ujobs, hjobs, chunks, in_off, out_off, metas = [], [], [], 0, 0, []
    for i in UNPACK_2056:
        d, data, (w, h, cpp) = G.build_unpack(G.UNPACK_CASES[i])
        img = HostImage(w, h, cpp)
        j = abi.UnpackJob()
        j.desc = d
        j.in_offset, j.in_bytes, j.img_offset = in_off, data.size, out_off
        j.img = gpu_util.image_job_view(w, h, cpp, img.pitch)
        ujobs.append(j)
        chunks.append(data)
        metas.append((i, out_off, w, h, cpp, img.pitch))
        in_off += data.size
        out_off += img.buf.size
    at = out_off
    for i, img_off, w, h, cpp, pitch in metas:
        hjobs.append(abi.image_hash_job(img_off, at, at + 16 * h, 2, w, h, cpp, pitch))
        at += 16 * h + 32
    inp = gpu_util.to_dev(np.concatenate(chunks + [np.zeros(64, np.uint8)]))
    out = torch.full((at,), 0xA5, dtype=torch.uint8, device="cuda")
    uplan, hplan = gpu.unpack_plan(ujobs), gpu.image_hash_plan(hjobs)
    stream = torch.cuda.current_stream().cuda_stream
    uplan.run(inp.data_ptr(), out.data_ptr(), stream)
    hplan.run(out.data_ptr(), out.data_ptr(), stream)
    rc, st, _ = hplan.results()
    assert rc == F.OK and not any(st)
    assert uplan.results()[0] == F.OK
    got = out.cpu().numpy()
    uplan.close()
    hplan.close()
    for (i, img_off, w, h, cpp, pitch), hj in zip(metas, hjobs):
        g = GOLD["unpack"][str(i)]
        lines = got[hj.lines_offset:hj.lines_offset + 16 * h].tobytes()
        assert abi.hex_joined_hash(lines) == g["hash"], i
        rows = got[img_off:img_off + pitch * h].reshape(h, pitch)[:, :2 * w * cpp]
        assert got[hj.result_offset:hj.result_offset + 32].tobytes() == \
            F.result_bytes(*F.expect(rows, 2)[1:]), i


TALL_PITCH, TALL_ROWS = (1 << 20) + 16, 4100


def test_an_image_past_4g_and_one_whose_rows_cross_4g(gpu):
    """one allocation of 4100 x (1 MiB + 16) bytes holds a tall image of short rows at that pitch
    (its rows 4096 .. 4099 start past 2^32), a small image based just past 2^32 between two of its
    rows, and every output in the gap behind row 4096"""
    rng = np.random.default_rng(13)
    big = torch.empty(TALL_PITCH * TALL_ROWS, dtype=torch.uint8, device="cuda")
    tall = F.Layout(rng, 29, TALL_ROWS, 1, 2)       # rows as the device holds them: compact here
    rows = tall.rows()
    torch.as_strided(big, (TALL_ROWS, tall.row_bytes), (TALL_PITCH, 1), 0).copy_(_dev(rows))
    small = F.Layout(rng, 27, 65, 3, 2, pad=2)
    small_off = (1 << 32) + 50
    assert 4095 * TALL_PITCH + tall.row_bytes < small_off
    assert small_off + small.size < 4096 * TALL_PITCH
    big[small_off:small_off + small.size].copy_(_dev(small.buf))
    gap0, gap1 = 4096 * TALL_PITCH + 4096, 4097 * TALL_PITCH
    assert gap0 > 1 << 32 and gap0 % 16 == 0
    big[gap0:gap1].fill_(0xA5)
    t_lines = gap0 + 32
    t_res = t_lines + 16 * TALL_ROWS + 8
    s_lines = (t_res + 32 + 15) // 16 * 16 + 16
    s_res = s_lines + 16 * 65
    jobs = [abi.image_hash_job(0, t_lines, t_res, 2, 29, TALL_ROWS, 1, TALL_PITCH),
            abi.image_hash_job(small_off, s_lines, s_res, 2, 27, 65, 3, small.pitch)]
    plan = gpu.image_hash_plan(jobs)
    plan.run(big.data_ptr(), big.data_ptr())
    assert plan.results()[:2] == (F.OK, [F.OK, F.OK])
    plan.close()
    got = big[gap0:gap1].cpu().numpy()
    want = np.full(gap1 - gap0, 0xA5, np.uint8)
    for (lines, md5, bs, ss), lo, ro in ((F.expect(rows, 2), t_lines, t_res),
                                        (small.want(), s_lines, s_res)):
        want[lo - gap0:lo - gap0 + len(lines)] = np.frombuffer(lines, np.uint8)
        want[ro - gap0:ro - gap0 + 32] = np.frombuffer(F.result_bytes(md5, bs, ss), np.uint8)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    del big
    torch.cuda.empty_cache()


def test_plan_of_65537_jobs(gpu):
    """one to three rows each: more jobs than a grid axis has rows, every result exact"""
    rng = np.random.default_rng(14)
    n = 65537
    data = rng.integers(0, 256, 1 << 20, dtype=np.uint8)
    raw = data.tobytes()
    jobs = (abi.ImageHashJob * n)()
    parts = []
    at = out_at = 0
    for k in range(n):
        h, sb = 1 + k % 3, (2, 4)[(k // 3) % 2]
        w = 1 + (k * 7) % 23
        rb = w * sb
        pitch = rb + sb * (k % 2)
        size = pitch * (h - 1) + rb
        if at + size > len(raw):
            at = (k % 5) * 4
        j = jobs[k]
        j.img_offset, j.lines_offset, j.result_offset = at, out_at, out_at + 16 * h
        j.sample_bytes = sb
        j.img = abi.Image(None, pitch, w, h, 1, 0)
        rows = [raw[at + y * pitch:at + y * pitch + rb] for y in range(h)]
        lines = b"".join(hashlib.md5(r).digest() for r in rows)
        samples = sum(sum(memoryview(r).cast("H")) for r in rows) if sb == 2 else 0
        parts.append(lines)
        parts.append(F.result_bytes(hashlib.md5(lines).digest(), sum(map(sum, rows)), samples))
        at += (size + 3) // 4 * 4
        out_at += 16 * h + 32
    want = np.frombuffer(b"".join(parts) + b"\xa5" * 16, np.uint8)
    inp = _dev(data)
    out = torch.full((want.size,), 0xA5, dtype=torch.uint8, device="cuda")
    h_plan = C.c_void_p()
    assert capi.lib().rsx_image_hash_plan_create(gpu._h, n, jobs, C.byref(h_plan)) == F.OK
    try:
        assert capi.lib().rsx_plan_run(h_plan, C.c_void_p(inp.data_ptr()),
                                       C.c_void_p(out.data_ptr()), None) == F.OK
        st = (C.c_int32 * n)()
        assert capi.lib().rsx_plan_results(h_plan, st, None) == F.OK
        assert not any(st)
    finally:
        capi.lib().rsx_plan_destroy(h_plan)
    got = out.cpu().numpy()
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
