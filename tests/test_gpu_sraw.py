"""sraw_kernel<0|1|2> (rsx_sraw.hip) at every width class and value edge.

One lane handles 4 groups with 16-byte loads and stores when all 4 exist and a scalar tail
otherwise; a workgroup covers 1024 groups, and the last lane's right neighbour lies across the
workgroup boundary.  sraw_cases.WIDTHS has every residue mod 4 in one lane, in two, on both
sides of that seam and in a third workgroup; its value classes reach every clamp outcome, the
values next to the clamps, negative odd sums under the shifts, and products that wrap.

Truth is the oracle, which tests/test_sraw_model.py pins to a numpy model written from the
reference's source and to the compiled reference, on exactly these inputs.  A plan's whole
output buffer is compared: every job's pixels, and 0xA5 in every other byte -- the row padding
(the full-lane path writes 48 bytes per row per lane; the tail must not) and the gaps between
the jobs."""
import threading

import numpy as np
import pytest
import torch

from rawspeed_amd import abi

import sraw_cases as S
from oracle_lib import HostImage

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import gpu_util
    return gpu_util.ctx()


_TRUTH = {}


def truth(oracle, c, take=0):
    """the oracle's output pixels for image `take` of the case (computed once)"""
    if (c, take) not in _TRUTH:
        d, px = S.images(c)[take]
        ow, oh = S.out_dims(c)
        src = HostImage(px.shape[1], c.rows, 1, is_cfa=False)
        dst = HostImage(ow, oh, 3, is_cfa=False)
        src.pixels()[:] = px
        assert oracle.sraw(d, src, dst) == 0
        want = dst.pixels().copy()
        want.flags.writeable = False
        _TRUTH[(c, take)] = want
    return _TRUTH[(c, take)]


def layout_of(cases):
    """every image of every case as a job: pitches roundUp(row bytes, 16) plus 0, 16 or 32
    (input and output cycle apart: all nine combinations), gaps of 0, 16 or 48 bytes"""
    lay, by_name = S.PlanLayout(), {}
    for c in cases:
        for take in range(len(S.images(c))):
            i = len(lay.entries)
            d, px = S.images(c)[take]
            e = lay.add("%s/%d" % (S.case_id(c), take), d, px, c.ysf, in_extra=16 * (i % 3),
                        out_extra=16 * (i // 3 % 3), gap=(0, 16, 48)[i // 2 % 3])
            by_name[e.name] = (c, take)
    return lay, by_name


def run_twice(gpu, lay, want, want_rc=0):
    """the plan, run twice into 0xA5-filled buffers: statuses, pixels, every other byte"""
    import gpu_util
    plan = gpu.sraw_plan(lay.jobs())
    d_in = gpu_util.to_dev(lay.in_host())
    for run in range(2):
        d_out = torch.full((lay.out_bytes(),), 0xA5, dtype=torch.uint8, device="cuda")
        plan.run(d_in.data_ptr(), d_out.data_ptr())
        rc, status, _ = plan.results()
        assert rc == want_rc, (run, rc)
        lay.check(d_out.cpu().numpy(), status, want)
    plan.close()


def matrix_cases():
    return S.cases("full")


def class_cases(cls):
    return S.cases(cls, S.SEAM, rows="max")


def test_width_and_row_matrix_in_one_plan(gpu, oracle):
    """every (subsampling, version) x WIDTHS x ROWS of the full class in ONE plan: a few hundred
    jobs, all three kernels in one launch, both group sizes, the block -> job search over a
    long table"""
    lay, by_name = layout_of(matrix_cases())
    assert len(lay.entries) == 3 * 17 * 3 + 2 * 17 * 4
    assert {e.desc.version for e in lay.entries} == {0, 1, 2}
    want = lay.render(lambda e: truth(oracle, *by_name[e.name]))
    run_twice(gpu, lay, want)


@pytest.mark.parametrize("cls", ["sensor", "boundary", "rounding", "wrap"])
def test_value_classes(gpu, oracle, cls):
    """the five pairs at 2, 3, 5 groups and around the seam, the largest row count, one plan per
    class (boundary: 18 images per shape, rounding: 2)"""
    lay, by_name = layout_of(class_cases(cls))
    want = lay.render(lambda e: truth(oracle, *by_name[e.name]))
    run_twice(gpu, lay, want)


PADS = (2, 6, 18)


def host_call_cases():
    return S.cases("full", (3, 5, 1025), rows="max")


def check_host_image(got, want, name):
    """the caller's output image after a host-pointer call: its pixels, and its row padding"""
    assert np.array_equal(got.pixels(), want), name
    assert (got.u16()[:, want.shape[1]:] == 0xA5A5).all(), "%s: row padding written" % name


def test_host_pointer_call_pitches(gpu, oracle):
    """rsx_sraw_interpolate repacks the caller's rows to a compact pitch: callers' pitches that
    are no multiple of 16 (row bytes + 2, 6, 18; input and output independently)"""
    for c in host_call_cases():
        (d, px), = S.images(c)
        ow, oh = S.out_dims(c)
        want = truth(oracle, c)
        for pad_in in PADS:
            src = HostImage(px.shape[1], c.rows, 1, is_cfa=False, pitch=2 * px.shape[1] + pad_in)
            src.pixels()[:] = px
            for pad_out in PADS:
                got = HostImage(ow, oh, 3, is_cfa=False, pitch=6 * ow + pad_out)
                assert gpu.sraw_interpolate(d, src.view(), got.view()) == 0
                check_host_image(got, want, "%s +%d +%d" % (S.case_id(c), pad_in, pad_out))


def refusal_layout(good):
    """good jobs (when asked for) interleaved with jobs that each carry one defect"""
    lay, by_name = S.PlanLayout(), {}
    goods = iter([S.Case("full", 1, 0, 5, 3), S.Case("full", 2, 1, 1025, 4),
                  S.Case("full", 1, 2, 1027, 2), S.Case("full", 2, 2, 3, 1),
                  S.Case("full", 1, 1, 1024, 3), S.Case("full", 2, 2, 1026, 2),
                  S.Case("full", 1, 1, 2, 1), S.Case("full", 2, 1, 6, 3)])

    def add_good():
        if good:
            c = next(goods)
            (d, px), = S.images(c)
            by_name[lay.add(S.case_id(c), d, px, c.ysf).name] = (c, 0)

    c422, c420 = S.Case("full", 1, 1, 1025, 3), S.Case("full", 2, 2, 7, 2)
    (d422, px422), = S.images(c422)
    (d420, px420), = S.images(c420)
    bad = abi.RSX_ERR_INVALID_ARG
    add_good()
    lay.add("input pitch % 16 = 8", d422, px422, 1, in_extra=8, want_status=bad)
    add_good()
    lay.add("output pitch % 16 = 4", d420, px420, 2, out_extra=4, want_status=bad)
    add_good()
    lay.add("in_offset % 16 = 2", d420, px420, 2, in_shift=2, want_status=bad)
    add_good()
    lay.add("img_offset % 16 = 8", d422, px422, 1, out_shift=8, want_status=bad)
    add_good()
    lay.add("version 0 with 4:2:0", abi.SrawDesc.make(0, 2, [1024, 1024, 1024], 0), px420, 2,
            want_status=bad)
    add_good()
    lay.add("a one-group row", d420, px420[:, :6], 2, want_status=bad)
    add_good()
    lay.add("output width off by 2", d422, px422, 1, out_w=2 * 1025 + 2, want_status=bad)
    add_good()
    return lay, by_name


def test_plan_refuses_what_the_kernel_cannot_move(gpu, oracle):
    """a job whose pitches or offsets are no multiples of 16, or that the reference would not
    take, reports RSX_ERR_INVALID_ARG and its window stays untouched; its neighbours decode"""
    lay, by_name = refusal_layout(good=True)
    assert sum(e.want_status == 0 for e in lay.entries) == 8
    want = lay.render(lambda e: truth(oracle, *by_name[e.name]))
    run_twice(gpu, lay, want, want_rc=abi.RSX_ERR_INVALID_ARG)
    # every job refused: the plan is made, runs, and writes nothing
    lay, _ = refusal_layout(good=False)
    assert len(lay.entries) == 7 and all(e.want_status for e in lay.entries)
    run_twice(gpu, lay, lay.render(None), want_rc=abi.RSX_ERR_INVALID_ARG)


def thread_cases():
    return ([S.Case("full", 1, v, 1027, r) for v in (0, 1, 2) for r in (2, 3)],
            [S.Case("full", 2, v, 1025, r) for v in (1, 2) for r in (2, 3, 4)])


def test_two_threads_share_a_context(gpu, oracle):
    """two threads, six host-pointer calls each on one context: 4:2:2 at 1027 groups against
    4:2:0 at 1025"""
    work = [[(c, truth(oracle, c)) for c in cs] for cs in thread_cases()]
    failures, barrier = [], threading.Barrier(2)

    def worker(items):
        try:
            barrier.wait()
            for c, want in items:
                (d, px), = S.images(c)
                ow, oh = S.out_dims(c)
                src = HostImage(px.shape[1], c.rows, 1, is_cfa=False)
                src.pixels()[:] = px
                got = HostImage(ow, oh, 3, is_cfa=False)
                assert gpu.sraw_interpolate(d, src.view(), got.view()) == 0
                check_host_image(got, want, S.case_id(c))
        except BaseException as e:  # (an assertion in a thread would otherwise go unseen)
            failures.append(e)
            barrier.abort()

    ts = [threading.Thread(target=worker, args=(w,)) for w in work]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not failures, failures
