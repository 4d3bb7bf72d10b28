"""SamsungV2Decompressor: the Python model (samsung_v2_cases.decode_model, written from the
reference's source), the oracle and the compiled reference agree pixel for pixel on the
streams that tests/test_gpu_samsung_v2.py then holds the kernels to; those streams are what
they claim to be (the conditions on them are asserted from the writer's own counts); and a
decoder that is wrong in one of the ways of samsung_v2_cases.VARIANTS differs from the oracle
on the class named for it."""
import numpy as np
import pytest

import samsung_v2_cases as V2
from oracle_lib import HostImage


@pytest.fixture(scope="module")
def ref(ref):
    if hasattr(ref, "lib") and not hasattr(ref.lib, "ref_samsung_v2_decompress"):
        pytest.skip("oracle/_ref predates the SamsungV2 entry point")
    return ref


def run_oracle(oracle, bits, w, h, data):
    host = HostImage(w, h)
    return oracle.samsung_v2(bits, data, host), host


def agree(oracle, ref, bits, w, h, data, model=True):
    """oracle == reference (status; where it is 0 the whole buffer, padding included) and, if
    asked, == model.  Returns (status, the oracle's image)."""
    st, host = run_oracle(oracle, bits, w, h, data)
    img = ref.image(w, h)
    assert ref.samsung_v2(bits, data, img) == st, ref.last_error()
    if st == 0:
        assert np.array_equal(img.u16(), host.u16())
    if model:
        ms, mi = V2.decode_model(data, bits, w, h)
        assert ms == st
        if st == 0:
            assert np.array_equal(mi, host.pixels())
    return st, host


@pytest.mark.parametrize("optflags", range(8))
@pytest.mark.parametrize("bits", [12, 14])
@pytest.mark.parametrize("cls", V2.CLASSES)
def test_value_class(oracle, ref, cls, bits, optflags):
    c = V2.value_case(cls, bits, optflags)
    st, host = agree(oracle, ref, bits, c.w, c.h, c.data)
    assert st == 0
    if c.want is not None:  # (the writer tracked the image)
        assert np.array_equal(c.want, host.pixels())
    hi = (1 << bits) - 1
    scaled = not (optflags & 4)  # (QP: the stream has no scale fields)
    if cls == "extremes":
        assert c.stats["below"] > 100 and c.stats["above"] > 100, c.stats
        assert (host.pixels() == 0).sum() > 1000 and (host.pixels() == hi).sum() > 1000
        assert not scaled or c.stats["max_scale"] >= 4095
    elif cls == "floor":
        assert c.stats["below"] > 1000, c.stats
        assert (host.pixels() == 0).sum() > c.w * c.h // 2
    elif cls == "ceiling":
        assert c.stats["above"] > 1000, c.stats
        assert (host.pixels() == hi).sum() > c.w * c.h // 2
    elif cls == "negative_scale":
        assert not scaled or c.stats["min_scale"] < 0, c.stats
    elif cls == "max_len":
        assert c.stats["max_len"] == bits + 1
        assert (host.pixels() == 0).sum() > 1000 and (host.pixels() == hi).sum() > 1000


def test_floor_skips_blocks_under_a_scale():
    """skipped blocks at a scale other than 0 (they still add the scale, :307), in every flag
    set that has both the skip bit and scale fields"""
    for bits in (12, 14):
        for optflags in (0, 2):
            assert V2.value_case("floor", bits, optflags).stats["skipped_scaled"] > 10


def test_negative_scale_by_hand(oracle, ref):
    data, rows = V2.negative_scale_rows()
    assert all(r.min_scale == -2 for r in rows)
    st, host = agree(oracle, ref, 12, 32, 4, data)
    assert st == 0
    assert (host.pixels()[:, :16] == 95).all() and (host.pixels()[:, 16:] == 93).all()


# the class whose streams tell each wrong decoder from the right one
CAUGHT_BY = {
    "no_clamp_hi": "ceiling",
    "clamp_hi_minus_1": "ceiling",
    "no_clamp_0": "floor",
    "truncating_average": "sensor",
    "skip_without_scale": "floor",
    "odd_shuffle_on_even_rows": "sensor",
    "scale_unsigned_16": "negative_scale",
    "left_neighbour_col_minus_1": "sensor",
    "init_val_in_every_block_0": "sensor",
}


@pytest.mark.parametrize("variant", V2.VARIANTS)
def test_wrong_decoder_is_caught(oracle, variant):
    """per depth: the variant's image differs from the oracle's on the named class (flag set 0,
    the one every field exists in)"""
    cls = CAUGHT_BY[variant]
    for bits in (12, 14):
        c = V2.value_case(cls, bits, 0)
        st, host = run_oracle(oracle, bits, c.w, c.h, c.data)
        ms, mi = V2.decode_model(c.data, bits, c.w, c.h, variant)
        assert st == 0
        assert ms != 0 or not np.array_equal(mi, host.pixels()), (variant, cls, bits)


def test_every_variant_has_a_class():
    assert set(CAUGHT_BY) == set(V2.VARIANTS)
    assert set(CAUGHT_BY.values()) <= set(V2.CLASSES)


def test_scale_variant_only_differs_under_a_negative_scale(oracle):
    """(the variants are wrong in one way each: this one is right wherever no scale is below 0)"""
    c = V2.value_case("extremes", 12, 0)
    st, host = run_oracle(oracle, 12, c.w, c.h, c.data)
    ms, mi = V2.decode_model(c.data, 12, c.w, c.h, "scale_unsigned_16")
    assert (st, ms) == (0, 0) and np.array_equal(mi, host.pixels())


def test_directed_motions(oracle, ref):
    """every motion at either end of an even and an odd row, and in rows 0 and 1: the status is
    the reference's, and only the motions its edge checks name are refused"""
    bad = set()
    for d in V2.motion_cases():
        st, _ = agree(oracle, ref, d.bits, d.w, d.h, d.data)
        assert st in (0, 1), d.name
        if st:
            bad.add(d.name)
    want = {"row%d_blk%d_motion%d" % (r, b, m) for r in (0, 1) for b in (0, 1) for m in range(7)}
    # :214-217 -- left edge: a slide to the left; right edge: to the right, or an average
    # whose second pixel lies two columns further
    want |= {"row%d_blk0_motion%d" % (r, m) for r in (2, 3) for m in (0, 1, 2)}
    want |= {"row%d_blk1_motion%d" % (r, m) for r in (2, 3) for m in (4, 5, 6)}
    assert bad == want


def test_directed_lengths(oracle, ref):
    for d in V2.length_cases():
        st, _ = agree(oracle, ref, d.bits, d.w, d.h, d.data)
        refused = "underflow" in d.name.replace("no_underflow", "") or "too_long" in d.name \
            or "explicit_15" in d.name
        assert st == (1 if refused else 0), d.name


def test_repeated_rows_are_a_valid_frame(oracle, ref):
    """the tall-frame builder: rows 2.. of a short frame over and over keep a frame valid;
    reference == oracle == model on one of them (48 x 67: row 66 starts a third hop)"""
    bits, w, h = 12, 48, 67
    data, init_val, rows = V2.short_frame(bits, w, 0)
    tall = V2.repeat_rows(bits, w, h, 0, init_val, rows)
    st, _ = agree(oracle, ref, bits, w, h, tall)
    assert st == 0
