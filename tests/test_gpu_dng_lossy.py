"""The lossy-DNG chain on the device (rsx_dng_lossy_decompress, include/rsx.h section 4f) through
the C-ABI.  Every case is held against two yardsticks: the composed model of
tests/dng_lossy_files.py, and the sequence of the stand-alone calls -- rsx_dng_decompress_jpeg,
rsx_dng_post, rsx_scale_black_white, rsx_dng_post, rsx_bad_pixels_fix -- on the same inputs,
results and statuses included.  Every image has a padded pitch, and the padding must stay."""
import numpy as np
import pytest

import dng_jpeg_files as J
import dng_lossy_files as F
import dng_post_files as P
from oracle_lib import HostImage
from rawspeed_amd import abi, capi

pytestmark = pytest.mark.gpu
OK, UNSUPPORTED, TILE_ERRORS = F.OK, F.UNSUPPORTED, F.TILE_ERRORS
FILL = 0xA5A5


@pytest.fixture(scope="module")
def gpu():
    import gpu_util
    return gpu_util.ctx()


def _image(dim_x, dim_y, cpp):
    pitch = (2 * cpp * dim_x + 15) // 16 * 16 + 6
    return HostImage(dim_x, dim_y, cpp, pitch=pitch, is_cfa=cpp == 1)


def _padding_untouched(img):
    rows = img.buf.reshape(img.dim_y, img.pitch)
    assert (rows[:, 2 * img.cpp * img.dim_x:] == 0xA5).all(), "the pitch padding was written"


def _fields(r):
    """a ctypes result as plain values"""
    out = []
    for name, _ in r._fields_:
        v = getattr(r, name)
        out.append(tuple(v) if hasattr(v, "__len__") else v)
    return tuple(out)


def _chained(gpu, c, streams=None, offsets=None, dims=None):
    s = c.shape
    dim_x, dim_y = dims or (s.dim_x, s.dim_y)
    img = _image(dim_x, dim_y, s.cpp)
    d, keep = F.desc(c, abi)
    before = gpu.host_calls()
    rc, st, r, bad, m = gpu.dng_lossy_decompress(streams or s.streams(), offsets or s.offsets(), d,
                                                 img.view(), c.bad_cap)
    assert gpu.host_calls() == before + 1, "the chained call is one host call"
    _padding_untouched(img)
    return rc, st, r, bad, m, img.pixels().copy()


def _sequence(gpu, c):
    """the stand-alone calls one after the other, each a round trip: what a caller does today.
    Returns a dict shaped like dng_lossy_files.compose()'s plus the calls' own results."""
    s = c.shape
    img = _image(s.dim_x, s.dim_y, s.cpp)
    v = img.view()
    out = dict(stages=0, r1=None, r2=None, rs=None, rf=None, bad=None, map=None)
    rc, st = gpu.dng_decompress_jpeg(s.streams(), s.offsets(), v)
    assert rc == OK, st
    d1, keep1 = abi.dng_post_desc(c.list1, c.table, c.crop)
    rc, out["r1"], bad1 = gpu.dng_post(d1, v)
    assert rc == OK
    out["stages"] = F.STAGE1
    bad2, f2, status = [], 0, OK
    if c.list2 is not None:
        ds, keeps = F.scale_desc(c, abi, out["r1"].crop())
        rc, rs = gpu.scale_black_white(ds, v)
        if rc == UNSUPPORTED:
            status = UNSUPPORTED
        else:
            assert rc == OK
            out["rs"] = rs
            out["stages"] |= F.SCALED
            d2, keep2 = abi.dng_post_desc(c.list2, None, out["r1"].crop())
            st2, r2v, fixed2 = capi.dng_post_validate(d2, v)
            assert st2 == OK
            f2 = len(fixed2)
            rc, out["r2"], bad2 = gpu.dng_post(d2, v)
            assert rc == OK
            out["stages"] |= F.LIST2
    merged = F.merge(bad1, bad2, f2)
    if len(merged) <= c.bad_cap:
        out["bad"] = merged
        if c.fix and status == OK:
            if merged:
                db, keepb, m = abi.bad_pixels_desc(merged, (s.dim_x, s.dim_y))
                rc, out["rf"] = gpu.bad_pixels_fix(db, v)
                assert rc == OK
                out["map"] = m
            out["stages"] |= F.FIXED
    else:
        status = UNSUPPORTED
    _padding_untouched(img)
    out.update(status=status, img=img.pixels().copy())
    return out


def _check_list(r, info, n_bad):
    assert (r.list_status, r.list_reason, r.n_applied, r.crop(), r.n_bad) == \
        (info["list_status"], info["reason"], info["n_applied"], tuple(info["crop"]), n_bad)


def _check_case(gpu, c):
    """the chained call against the composed model and against the sequence"""
    s = c.shape
    want = F.expected(c.name)
    rc, st, r, bad, m, got = _chained(gpu, c)
    # --- the model
    assert rc == want["status"], (c.name, rc, gpu.last_error())
    assert st == [OK] * len(s.tiles)
    assert r.stages == want["stages"], c.name
    assert np.array_equal(got, want["img"]), (c.name, np.argwhere(got != want["img"])[:4])
    _check_list(r.list1, want["info1"], want["n_bad1"])
    if c.list2 is not None:
        _check_list(r.list2, want["info2"], want["n_bad2"])  # (0 where list 2 did not run)
    else:
        assert _fields(r.list2) == _fields(abi.DngPostResult())
    if want["scale"] is not None:
        res = want["scale"]
        assert (r.scale.levels(), r.scale.estimated, r.scale.skipped, r.scale.variant,
                r.scale.n_wrapped) == ((res["black"], res["white"], tuple(res["sep"])),
                                       res["estimated"], res["skipped"], res["variant"],
                                       res["n_wrapped"]), c.name
    else:
        assert _fields(r.scale) == _fields(abi.ScaleResult())
    assert bad == want["bad"], c.name
    n_bad, n_fixed, wmap = want["fixed"]
    assert (r.fixed.n_bad, r.fixed.n_fixed, r.fixed.map_made) == (n_bad, n_fixed, int(wmap is not None))
    if wmap is not None:
        assert np.array_equal(m, wmap), "the map"
    else:
        assert (m == 0xA5).all(), "map_out was written without a map"
    # --- the sequence of the stand-alone calls
    seq = _sequence(gpu, c)
    assert (rc, r.stages) == (seq["status"], seq["stages"]), c.name
    assert np.array_equal(got, seq["img"]), (c.name, np.argwhere(got != seq["img"])[:4])
    assert _fields(r.list1) == _fields(seq["r1"])
    if seq["r2"] is not None:
        assert _fields(r.list2) == _fields(seq["r2"])
    if seq["rs"] is not None:
        assert _fields(r.scale) == _fields(seq["rs"])
    assert bad == seq["bad"]
    if seq["rf"] is not None:
        assert _fields(r.fixed) == _fields(seq["rf"])
        assert np.array_equal(m, seq["map"])
    else:
        assert _fields(r.fixed) == _fields(abi.BadPixelsResult())
    return want, r, bad, got


@pytest.mark.parametrize("name", [c.name for c in F.cases()])
def test_case_equals_the_model_and_the_sequence(gpu, name):
    _check_case(gpu, F.case(name))


def test_the_case_table_covers_what_it_promises(gpu):
    """the variants, the skip rule, the moved crop and the positions, read from the results"""
    E = F.expected
    S = F.S
    assert E("post_rgb")["stages"] == F.STAGE1 and E("finish_cfa")["stages"] == F.STAGE1 | F.FIXED
    assert E("finish_cfa")["fixed"][1] > 0 and E("finish_segments_no_positions")["fixed"][2] is None
    all_stages = F.STAGE1 | F.SCALED | F.LIST2
    for name, variant in (("maptable_sse2_dither", S.SSE2), ("deltarow_sse2_plain_rows", S.SSE2),
                          ("cfa_sse2_row_tail", S.SSE2), ("trim_scalecol_plain_dither", S.PLAIN),
                          ("trim_scalecol_plain_cfa", S.PLAIN), ("app_scale_plain", S.PLAIN),
                          ("app_scale_plain_dither", S.PLAIN), ("separate_levels", S.SSE2),
                          ("black_area", S.SSE2)):
        e = E(name)
        assert (e["status"], e["stages"]) == (OK, all_stages), name
        assert e["scale"]["variant"] == variant and not e["scale"]["skipped"], name
    assert F.case("app_scale_plain").sse2 and F.case("app_scale_plain_dither").sse2
    assert E("trim_scalecol_plain_dither")["info1"]["crop"] == (5, 2, 87, 139)
    assert E("black_area")["scale"]["sep"] != (0, 0, 0, 0)
    assert E("skip_rule")["scale"]["skipped"] == 1 and E("skip_rule")["stages"] == all_stages
    # the constant of list 2 hits a value that exists only behind the scaling
    e = E("const2_fix")
    st, lookup, _ = P.apply(F.decoded("66x100x1"), 1, (0, 0, 66, 100), None, F.case("const2_fix").table)
    assert not (lookup == 65535).any() and e["n_bad2"] > 14 and e["n_bad1"] > 3
    assert e["stages"] == all_stages | F.FIXED and e["fixed"][1] > 0
    assert E("const2_no_fix")["stages"] == all_stages and E("const2_no_fix")["n_bad2"] > 2
    e = E("const2_cap_too_small")
    assert (e["status"], e["stages"], e["bad"]) == (UNSUPPORTED, all_stages, None)
    assert np.array_equal(e["img"], E("const2_no_fix")["img"]), "complete, unfixed"
    assert E("list2_fails_constructed")["info2"]["n_applied"] == 0
    assert E("list2_stops_at_setup")["info2"]["n_applied"] == 1
    e = E("scale_refuses")
    assert (e["status"], e["stages"], e["scale"]) == (UNSUPPORTED, F.STAGE1, None)


def test_a_scale_that_refuses_leaves_what_the_post_equivalent_gives(gpu):
    c = F.case("scale_refuses")
    rc, st, r, bad, m, got = _chained(gpu, c)
    assert (rc, r.stages) == (UNSUPPORTED, F.STAGE1) and st == [OK] * 4
    post = F.Case("x", c.shape.name, c.list1, c.table)
    rc2, st2, r2, bad2, m2, got2 = _chained(gpu, post)
    assert (rc2, r2.stages) == (OK, F.STAGE1)
    assert np.array_equal(got, got2) and bad == bad2 and bad
    assert _fields(r.list1) == _fields(r2.list1)
    assert (m == 0xA5).all() and r.fixed.map_made == 0


@pytest.mark.parametrize("fix", [True, False])
def test_a_scale_that_refuses_hands_out_list1s_positions_alone(gpu, fix):
    """list 2 carries a FixBadPixelsList and never runs: `bad` is list 1's positions, list2.n_bad
    is 0, and a capacity of exactly list 1's count is enough"""
    c = F.case("scale_refuses_list2_positions" if fix else "scale_refuses_list2_positions_no_fix")
    post = F.Case("x", c.shape.name, c.list1, c.table)
    rc1, _, r1, bad1, _, got1 = _chained(gpu, post)
    assert rc1 == OK and len(bad1) == r1.list1.n_bad > 3
    for cap in (1 << 16, len(bad1)):
        tight = F.Case("x", c.shape.name, c.list1, c.table, None, c.list2, c.black, c.white,
                       areas=c.areas, fix=fix, bad_cap=cap)
        rc, st, r, bad, m, got = _chained(gpu, tight)
        assert (rc, r.stages, st) == (UNSUPPORTED, F.STAGE1, [OK] * 4)
        assert bad == bad1 and (r.list1.n_bad, r.list2.n_bad) == (len(bad1), 0)
        assert (r.list2.list_status, r.list2.n_opcodes, r.list2.n_applied) == (OK, 2, 2)
        assert np.array_equal(got, got1) and (m == 0xA5).all()
        assert _fields(r.fixed) == _fields(abi.BadPixelsResult())
    # one position less room: the image as stage 1 left it, the positions do not fit
    short = F.Case("x", c.shape.name, c.list1, c.table, None, c.list2, c.black, c.white,
                   areas=c.areas, fix=fix, bad_cap=len(bad1) - 1)
    rc, st, r, bad, m, got = _chained(gpu, short)
    assert (rc, r.stages, bad) == (UNSUPPORTED, F.STAGE1, None)
    assert (r.list1.n_bad, r.list2.n_bad) == (len(bad1), 0) and np.array_equal(got, got1)


def test_a_damaged_tile_makes_it_the_plain_call(gpu):
    damaged = next(c for c in J.damaged() if c["name"].endswith("restart3_420_64x96/rst_renumbered"))
    good = J.case("444_48x72")["stream"]
    streams = [damaged["stream"], good, good]
    offsets = [(0, 0), (0, 96), (48, 96)]
    base = F.case("maptable_sse2_dither")
    list2 = P.opcode_list([P.op_table((0, 0, 168, 64), np.arange(65536) ^ 1, planes=(0, 3))])
    c = F.Case("x", "96x144x3", None, base.table, (0, 0, 64, 168), list2, 256, 16383)
    rc, st, r, bad, m, got = _chained(gpu, c, streams, offsets, (64, 168))
    plain = _image(64, 168, 3)
    prc, pst = gpu.dng_decompress_jpeg(streams, offsets, plain.view())
    assert prc == TILE_ERRORS and pst[0] != OK and pst[1:] == [OK, OK]
    assert (rc, st) == (prc, pst)
    assert np.array_equal(got, plain.pixels())
    assert (got[:96] == FILL).all() and not (got[96:] == FILL).all()
    assert r.stages == 0 and bad is None and (m == 0xA5).all()
    # the results carry the parses alone
    assert (r.list2.n_opcodes, r.list2.n_applied, r.list2.crop()) == (1, 1, (0, 0, 64, 168))
    assert _fields(r.scale) == _fields(abi.ScaleResult())
    # the same grid undamaged: the chain runs
    streams[0] = J.case("restart3_420_64x96")["stream"]
    rc, st, r, bad, m, got = _chained(gpu, c, streams, offsets, (64, 168))
    assert (rc, st, r.stages) == (OK, [OK] * 3, F.STAGE1 | F.SCALED | F.LIST2)


@pytest.mark.parametrize("how", ["one_missing", "one_twice"])
def test_tiles_that_do_not_tile_the_image_write_nothing(gpu, how):
    c = F.case("maptable_sse2_dither")
    streams, offsets = c.shape.streams(), c.shape.offsets()
    if how == "one_missing":
        streams, offsets = streams[:3], offsets[:3]
    else:
        offsets = offsets[:3] + [offsets[2]]
    rc, st, r, bad, m, got = _chained(gpu, c, streams, offsets)
    assert rc == UNSUPPORTED
    assert (got == FILL).all() and st == [-1] * len(streams) and r.stages == 0
    # (the plain call takes them)
    img = _image(96, 144, 3)
    assert gpu.dng_decompress_jpeg(streams, offsets, img.view())[0] == OK


def test_a_check_that_fails_ends_the_call_before_anything_is_decoded(gpu):
    c = F.case("maptable_sse2_dither")
    for bad_case, want in ((F.Case("x", c.shape.name, None, c.table, None, b"", 256, 16383), F.IO),
                           (F.Case("x", c.shape.name, None, c.table, None, c.list2, 256, 16383,
                                   scale_crop=(0, 0, 96, 143)), F.INVALID_ARG),
                           (F.Case("x", c.shape.name, P.opcode_list([P.op_bad_list([(1, 1)])]), c.table,
                                   fix=True), UNSUPPORTED)):
        rc, st, r, bad, m, got = _chained(gpu, bad_case)
        assert rc == want
        assert (got == FILL).all() and st == [-1] * 4 and r.stages == 0
