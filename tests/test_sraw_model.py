"""Cr2sRawInterpolator: the numpy model (sraw_cases.model, written from the reference's
source), the oracle and the compiled reference agree sample for sample on the inputs that
tests/test_gpu_sraw.py then holds the kernel to; and those inputs are what they claim to be:
the conditions on them are asserted on the model's pre-clamp values.

The `wrap` class is held to the model and the oracle only: its products overflow int, which is
undefined in the reference."""
import numpy as np
import pytest

import sraw_cases as S
from oracle_lib import HostImage


def run_oracle(oracle, c, d, px):
    ow, oh = S.out_dims(c)
    src, dst = HostImage(px.shape[1], c.rows, 1, is_cfa=False), HostImage(ow, oh, 3, is_cfa=False)
    src.pixels()[:] = px
    assert oracle.sraw(d, src, dst) == 0
    return dst


def agree(oracle, ref, c):
    """model == oracle (== ref, the whole buffer: the reference writes no padding either) for
    every image of the case; returns the models.  Outside the full class the reference is
    asked at S.NARROW; the two widths before the seam are held to the model alone."""
    models = []
    if c.cls != "full" and c.groups not in S.NARROW:
        ref = None
    for d, px in S.images(c):
        m = S.model(d, px)
        dst = run_oracle(oracle, c, d, px)
        assert np.array_equal(m.out, dst.pixels()), S.case_id(c)
        if ref is not None:
            ow, oh = S.out_dims(c)
            rsrc, rdst = ref.image(px.shape[1], c.rows, 1, False), ref.image(ow, oh, 3, False)
            rsrc.set_pixels(px)
            assert ref.sraw(d, rsrc, rdst) == 0, ref.last_error()
            assert np.array_equal(dst.u16(), rdst.u16()), S.case_id(c)
        models.append(m)
    return models


@pytest.mark.parametrize("groups", S.WIDTHS)
@pytest.mark.parametrize("pair", S.PAIRS, ids=lambda p: "42%d_v%d" % (4 - 2 * p[0], p[1]))
def test_full_class(oracle, ref, pair, groups):
    for c in S.cases("full", (groups,), pairs=(pair,)):
        for m in agree(oracle, ref, c):
            assert m.max_product < 2 ** 31, S.case_id(c)  # the reference's multiply is defined


@pytest.mark.parametrize("pair", S.PAIRS, ids=lambda p: "42%d_v%d" % (4 - 2 * p[0], p[1]))
def test_full_class_clamps_both_ways_in_every_channel(pair):
    """over the class, per channel: clamped to 0, clamped to 65535 and unclamped each hold at
    least 0.5 % of the samples (a numpy draw of 200 000 samples per version gives 0.9 % at the
    least: version 1, blue, coefficient 4096)"""
    counts = np.zeros((3, 3), np.int64)
    for c in S.cases("full", pairs=(pair,)):
        (d, px), = S.images(c)
        pre = S.model(d, px).pre.reshape(-1, 3)
        counts += np.stack([(pre < 0).sum(0), (pre > 65535).sum(0),
                            ((pre >= 0) & (pre <= 65535)).sum(0)])
    frac = counts / counts.sum(0)
    print("clamped to 0 / to 65535 / unclamped, per channel:\n", frac)
    assert frac.min() >= 0.005, frac


@pytest.mark.parametrize("pair", S.PAIRS, ids=lambda p: "42%d_v%d" % (4 - 2 * p[0], p[1]))
def test_sensor_class(oracle, ref, pair):
    for c in S.cases("sensor", S.SEAM, pairs=(pair,)):
        agree(oracle, ref, c)


@pytest.mark.parametrize("pair", S.PAIRS, ids=lambda p: "42%d_v%d" % (4 - 2 * p[0], p[1]))
def test_boundary_class(oracle, ref, pair):
    """every target, in every channel, at every kind of pixel: at one whose chroma is a mean
    wherever the shape has such a pixel of that kind (a one-row 4:2:0 image has only copies in
    its second line)"""
    for c in S.cases("boundary", S.SEAM, pairs=(pair,)):
        models = agree(oracle, ref, c)
        kinds = (S.FULL, S.HORIZ) if c.ysf == 1 else (S.FULL, S.HORIZ, S.VERT, S.DIAG)
        for kind in kinds:
            at = models[0].kind == kind
            if kind != S.FULL and (at & models[0].interp).any():
                at &= models[0].interp
            assert at.any()
            pre = np.stack([m.pre.reshape(at.shape + (3,))[at] for m in models])
            for ch in range(3):
                for t in S.TARGETS:
                    assert (pre[..., ch] == t).any(), (S.case_id(c), kind, ch, t)


@pytest.mark.parametrize("pair", S.PAIRS, ids=lambda p: "42%d_v%d" % (4 - 2 * p[0], p[1]))
def test_rounding_class(oracle, ref, pair):
    """a kernel that divided towards zero, or rounded as dcraw does, would differ in every
    output row of every image; so would one that divided only the >> 12 terms towards zero,
    in the channels that have such a term"""
    for c in S.cases("rounding", S.SEAM, pairs=(pair,)):
        models = agree(oracle, ref, c)
        for take, ((d, px), m) in enumerate(zip(S.images(c), models)):
            for wrong in ("trunc", "round"):
                w = S.model(d, px, mean=wrong)
                assert (w.out != m.out).any(axis=1).all(), (S.case_id(c), take, wrong)
            w = S.model(d, px, shift12="trunc").out.reshape(-1, 3)
            differs = (w != m.out.reshape(-1, 3)).any(axis=0)
            # take 0: version 1's r and b; take 1: every version's g
            want = [c.version == 1, False, c.version == 1] if take == 0 else [False, True, False]
            assert (differs >= want).all(), (S.case_id(c), take, differs)


@pytest.mark.parametrize("pair", S.PAIRS, ids=lambda p: "42%d_v%d" % (4 - 2 * p[0], p[1]))
def test_wrap_class(oracle, pair):
    wrapped = 0
    for c in S.cases("wrap", S.SEAM, pairs=(pair,)):
        for m in agree(oracle, None, c):
            wrapped += m.max_product >= 2 ** 31
    assert wrapped  # (the class is about products that leave 32 bits)


def test_wrong_models_are_wrong():
    """the variants that stand in for a wrong kernel differ from the model where they should,
    and only there"""
    c = S.Case("full", 2, 2, 5, 3)
    (d, px), = S.images(c)
    m = S.model(d, px)
    zero = S.model(d, px, edge="zero")
    last = np.zeros(m.kind.shape, bool)
    last[:, -1] = True  # the second pixel of the last group
    diff = (zero.out != m.out).reshape(m.kind.shape + (3,)).any(axis=2)
    assert diff.any() and not (diff & ~last).any()
    low = S.model(d, px, top=65534)
    assert np.array_equal(low.out != m.out, m.pre >= 65535) and (m.pre >= 65535).any()
