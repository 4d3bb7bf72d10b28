"""The segmented scans of p1_row_kernel (rsx_phase_one.hip, steps 3-5) and sv0_parse_kernel
(rsx_samsung_v0.hip, steps 4-5) over long runs without a reset, bit-exactly.

Both scans are a shuffle ladder inside a wave (d = 1 .. 32), per-wave totals in LDS, a loop over
the waves (and the pass) before the lane's own, and a carry in front of the lane's first reset.
On the random inputs of test_gpu_phase_one.py and test_gpu_samsung_v0.py a reset comes every few
elements -- the longest run without one is 123 groups of 1496 (15 of 188 lanes; 18 .. 39 groups
with the non-zero `choices`) and 19 blocks of 347 (27 in the largest frame) --, so a flag in the
nearer operand wins every combine of the ladder's upper steps, of the totals and of the pass
carry, and their arithmetic decides nothing.  Here the resets are planned (tests/long_runs.py):
runs as long as the row (1497 groups at w = 11976, 347 blocks at w = 5546), single resets at the
first and last lane of a wave and in the middle of a lane, one early reset whose sum then travels
across both wave boundaries, sums that wrap 2^16 every 16 pixels.  test_long_runs_structure.py
holds the inputs to their plans on the CPU; tests/golden/long_runs_ref.json holds the reference's
image of each, test_phase_one_model.py and test_samsung_v0_model.py pin the models on them."""
import functools

import numpy as np
import pytest
import torch

import iiq_files as I
import long_runs as L
import srw_v0_files as S
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
    return L.golden()


def _check_padding(out):
    pad = out.buf.reshape(out.dim_y, out.pitch)[:, 2 * out.dim_x:]
    assert (pad == 0xA5).all(), "the pitch padding was written"


def _rect(host, off, pitch, w, h):
    return np.stack([host[off + r * pitch:off + r * pitch + 2 * w].view(np.uint16) for r in range(h)])


def _check_outside(host, rects):
    covered = np.zeros(host.size, bool)
    for off, pitch, w, h in rects:
        for r in range(h):
            covered[off + r * pitch:off + r * pitch + 2 * w] = True
    assert (host[~covered] == 0xA5).all(), "bytes outside the jobs' rectangles were written"


# ---- Phase One ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.p1_files(), ids=lambda c: c[0])
def test_phase_one_long_runs(gpu, ref, golden, case):
    """One file per width and value pattern, one row (one workgroup) per reset plan, through the
    host-pointer call: the source image (the codec is lossless), model_row, the reference's
    recorded hash, and the reference itself where it is built."""
    name, w, pattern, keep, plans = case
    img, rows, blob = L.p1_build(case)
    h = len(rows)
    assert L.sha_rows(rows)[:16] == golden["phase_one"][name]["input"]
    raw, strips, fw, fh = I.iiq_strips(blob)
    assert (fw, fh) == (w, h)
    out = HostImage(w, h, pitch=(2 * w + 15) // 16 * 16 + 16 * (len(name) % 2) + 2 * (w % 3 == 0))
    st, srow = gpu.phase_one_decompress(np.frombuffer(raw, np.uint8), strips, out.view())
    assert st == abi.RSX_OK and srow == [0] * h, (st, srow)
    got = out.pixels()
    bad = [plans[r][0] for r in range(h) if not np.array_equal(got[r], img[r])]
    assert not bad, (name, bad, [int(np.flatnonzero(got[r] != img[r])[0]) for r in range(h)
                                 if not np.array_equal(got[r], img[r])])
    _check_padding(out)
    mst, mimg, mrows = I.model_file(blob)
    assert mst == 0 and not any(mrows) and np.array_equal(got, mimg)
    assert L.sha(got) == golden["phase_one"][name]["image"]
    if ref is not None:
        rst, dec = ref.decode_file(blob)
        assert rst == 0 and np.array_equal(dec.u16()[:h, :w], got)


def test_phase_one_plan_of_long_runs(gpu):
    """One plan at device pointers: rows of different widths, plans and patterns as jobs of their
    own, strips at odd byte offsets of the input, images at pitches off the 16-byte grid."""
    picks = [(11976, "none", "plus4096", False), (11974, "early", "small", False),
             (8256, "even_512", "minus4095", False), (4160, "odd_511", "small", False),
             (11966, "mid3_even", "plus4096", False), (11976, "none", "small", True),
             (8192, "odd_1023", "minus4095", False), (11974, "none", "minus4095", False)]
    jobs, keep_alive, parts, expect = [], [], [], []
    in_off, img_off = 3, 0
    for k, (w, plan_name, pattern, keep) in enumerate(picks):
        plan = dict(L.p1_plans(w))[plan_name]
        img, rows = I.planned_rows(w, [plan, plan], pattern, seed=50 + k, keep=keep)
        h = 2 - k % 2
        img, rows = img[:h], rows[:h]
        for r in range(h):
            st, px = I.model_row(rows[r], w)
            assert st == 0 and np.array_equal(px, img[r])
        raw, strips, _, _ = I.iiq_strips(I.iiq_file(rows, w, np.random.default_rng(k), gap_max=3))
        arr = abi.phase_one_strips(strips)
        keep_alive.append(arr)
        pitch = (2 * w + 15) // 16 * 16 + 2 * (k % 7 + 1)
        j = abi.PhaseOneJob()
        j.strips = arr
        j.n_strips = len(strips)
        j.in_offset, j.in_bytes, j.img_offset = in_off, len(raw), img_off
        j.img = abi.Image(None, pitch, w, h, 1, 1)
        jobs.append(j)
        parts.append(np.frombuffer(raw, np.uint8))
        parts.append(np.full(5 + k, 0x5A, np.uint8))  # (bytes between the jobs: nobody's)
        expect.append((img_off, pitch, w, h, img))
        in_off += len(raw) + 5 + k
        img_off += pitch * h + 6
    assert any(e[0] % 4 == 2 for e in expect) and all(e[1] % 16 for e in expect)
    inp = torch.from_numpy(np.concatenate([np.full(3, 0x5A, np.uint8)] + parts)).cuda()
    out = torch.full((img_off,), 0xA5, dtype=torch.uint8, device="cuda")
    plan = gpu.phase_one_plan(jobs)
    plan.run(inp.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    rc, st, _ = plan.results()
    plan.close()
    assert rc == 0 and list(st) == [0] * len(jobs)
    host = out.cpu().numpy()
    for k, (off, pitch, w, h, img) in enumerate(expect):
        assert np.array_equal(_rect(host, off, pitch, w, h), img), picks[k]
    _check_outside(host, [e[:4] for e in expect])


# ---- Samsung V0 -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _v0_frame(name):
    """(w, h, rows, the model's image): built once, shared, never written"""
    case = next(c for c in L.v0_frames() if c[0] == name)
    _, w, h, _ = case
    rows = L.v0_build(case)
    mst, _, img = S.model_decode(w, h, rows)
    assert mst == S.OK
    img.setflags(write=False)
    return w, h, rows, img


def _v0_kind(name):
    part = name.split("_")[2]
    return part if part in ("row2", "row3") else "rows"


@pytest.mark.parametrize("kind", ["rows", "row2", "row3"])
@pytest.mark.parametrize("w", L.V0_WIDTHS)
def test_samsung_v0_long_runs(gpu, ref, golden, w, kind):
    """Frames whose upward blocks are planned, through the host-pointer call: "rows" -- none in
    any row, every eligible block, two blocks 200 apart --, "row2" / "row3" -- a single one in that
    row at block 0, 1, 63, 64, 127, 128, 191, 192, 193, nblk - 2, none in the rows behind it.
    Against model_decode (np.cumsum and np.maximum.accumulate, no scan of the kernel's kind), the
    reference's recorded hash, and the reference itself where it is built."""
    names = [c[0] for c in L.v0_frames() if c[1] == w and _v0_kind(c[0]) == kind]
    assert names
    for name in names:
        fw, h, rows, img = _v0_frame(name)
        assert L.sha_rows(rows)[:16] == golden["samsung_v0"][name]["input"]
        strip, offs = S.strip_and_offsets(rows)
        out = HostImage(w, h, pitch=(2 * w + 15) // 16 * 16 + 18 * (len(name) % 2))
        st, rs = gpu.samsung_v0_decompress(strip, offs, out.view())
        assert st == abi.RSX_OK and rs == [0] * h, (name, st, rs)
        got = out.pixels()
        assert np.array_equal(got, img), (name, np.argwhere(got != img)[:5])
        _check_padding(out)
        assert L.sha(got) == golden["samsung_v0"][name]["image"], name
        if ref is not None:
            rst, dec = ref.decode_file(S.rows_file(w, h, rows))
            assert rst == 0 and np.array_equal(dec.u16()[:h, :w], got)


def test_samsung_v0_plan_of_long_runs_runs_twice(gpu):
    """One plan at device pointers with two frames, run twice on the same scratch plane and root
    codes.  The direction bit does not change a row's size, so the two runs decode frames of the
    same geometry with different upward blocks: first every eligible block (every root code says
    "upward") and none, then two blocks 200 apart and a single one at block 191, the last of pass
    0 -- what the first run left in the scratch must not show in the second."""
    frames = [(5546, 6, [{y: tuple(range(346)) for y in range(2, 6)},
                         {2: (5, 205), 3: (140, 340), 4: (0, 200), 5: (63, 263)}]),
              (3088, 5, [{}, {2: (191,)}])]
    runs = [[], []]
    for k, (w, h, plans) in enumerate(frames):
        for run, plan in zip(runs, plans):
            rows = S.random_rows(np.random.default_rng([0x2A, k]), w, h, dirs=S.planned_dirs(w, h, plan))
            mst, _, img = S.model_decode(w, h, rows)
            assert mst == S.OK
            run.append((rows, img))
        assert [len(r) for r in runs[0][k][0]] == [len(r) for r in runs[1][k][0]]
        assert not np.array_equal(runs[0][k][1], runs[1][k][1])
    jobs, keep_alive, expect, inputs = [], [], [], [[np.full(3, 0x5A, np.uint8)], [np.full(3, 0x5A, np.uint8)]]
    in_off, img_off = 3, 0
    for k, (w, h, _) in enumerate(frames):
        strip, offs = S.strip_and_offsets(runs[0][k][0])
        arr = abi.samsung_v0_offsets(offs)
        keep_alive.append(arr)
        pitch = (2 * w + 15) // 16 * 16 + 2 * (k + 1)
        j = abi.SamsungV0Job()
        j.row_offsets = arr
        j.n_offsets = len(offs)
        j.in_offset, j.in_bytes, j.img_offset = in_off, len(strip), img_off
        j.img = abi.Image(None, pitch, w, h, 1, 1)
        jobs.append(j)
        for run, parts in zip(runs, inputs):
            parts.append(S.strip_and_offsets(run[k][0])[0])
            parts.append(np.full(5 + k, 0x5A, np.uint8))  # (bytes between the jobs: nobody's)
        expect.append((img_off, pitch, w, h))
        in_off += len(strip) + 5 + k
        img_off += pitch * h + 6
    inps = [torch.from_numpy(np.concatenate(parts)).cuda() for parts in inputs]
    out = torch.full((img_off,), 0xA5, dtype=torch.uint8, device="cuda")
    plan = gpu.samsung_v0_plan(jobs)
    for run, inp in zip(runs, inps):
        out.fill_(0xA5)
        plan.run(inp.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        rc, st, _ = plan.results()
        assert rc == 0 and list(st) == [0, 0]
        host = out.cpu().numpy()
        for (off, pitch, w, h), (_, img) in zip(expect, run):
            got = _rect(host, off, pitch, w, h)
            assert np.array_equal(got, img), (w, np.argwhere(got != img)[:5])
        _check_outside(host, expect)
    plan.close()
