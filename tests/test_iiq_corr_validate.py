"""rsx_iiq_correct_validate: every row of the table in include/rsx.h section 3n, in its order (a
list that earns two refusals gets the earlier one), the accepted corners, and the image untouched
after each refusal -- the last through the host build of the core, whose validation is the same
function.  Host code only: no GPU needed."""
import ctypes as C

import numpy as np
import pytest

import iiq_corr_files as K
from oracle_lib import HostImage
from rawspeed_amd import abi, build, capi

OK, INV, IO, UNS = abi.RSX_OK, abi.RSX_ERR_INVALID_ARG, abi.RSX_ERR_IO, abi.RSX_ERR_UNSUPPORTED
RNG = np.random.default_rng(7)
W, H = 64, 40
LUMA = K.ff_random(RNG, (0, 0, 64, 40, 8, 8))
CHROMA = K.ff_random(RNG, (0, 0, 64, 40, 8, 8), planes=2)
CURVES = K.random_curves(RNG)
RGGB = (2, 2, (0, 1, 1, 2))
QUAD = ("quad", CURVES, 20, 32, 100)

# (name, ops, cfa, image overrides, n_ops override, status), in the table's order: every list
# also carries the defects of the rows BELOW its own
BAD_IMAGE = dict(cpp=2)
LATER = [("ff", LUMA[:-1], 0), ("ff", CHROMA, 1), ("quad", CURVES, H + 1, 0, 0)]
ROWS = [
    ("cpp", LATER, None, dict(cpp=2), None, INV),
    ("pitch", LATER, None, dict(pitch=2 * W - 2), None, INV),
    ("dim", LATER, None, dict(w=0), None, INV),
    ("n_ops 17", LATER, None, {}, 17, INV),
    ("n_ops -1", LATER, None, {}, -1, INV),
    ("kind", [("kind", 2)] + LATER, None, {}, None, INV),
    ("null payload", [("ff", None, 0)] + LATER, None, {}, None, INV),
    ("null curves", [("quad", None, 0, 0, 0)] + LATER, None, {}, None, INV),
    ("short head", [("ff", LUMA[:15], 0), ("ff", CHROMA, 1), LATER[2]], None, {}, None, IO),
    ("short payload", LATER, None, {}, None, IO),
    ("short chroma payload", [("ff", CHROMA[:-2], 1), LATER[2]], None, {}, None, IO),
    ("no cfa", [("ff", CHROMA, 1), LATER[2]], None, {}, None, INV),
    ("cfa 0 x 2", [("ff", CHROMA, 1), LATER[2]], (0, 2, (0, 1, 1, 2)), {}, None, INV),
    ("cfa of 65", [("ff", CHROMA, 1)], (5, 13, [1] * 64), {}, None, INV),
    ("colour 4", [("ff", CHROMA, 1), LATER[2]], (2, 2, (0, 1, 4, 2)), {}, None, UNS),
    ("split_row", [("ff", CHROMA, 1), LATER[2]], RGGB, {}, None, INV),
    ("split_col", [("quad", CURVES, 0, W + 1, 0)], None, {}, None, INV),
]


def _view(w=W, h=H, cpp=1, pitch=None, data=None):
    return abi.Image(data, 2 * w if pitch is None else pitch, w, h, cpp, 1)


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_refusals_in_table_order(row):
    name, ops, cfa, image, n_ops, want = row
    d, keep = abi.iiq_corr(ops, cfa, n_ops)
    assert capi.iiq_correct_validate(d, _view(**image)) == want


def test_null_arguments():
    d, keep = abi.iiq_corr([QUAD])
    assert capi.iiq_correct_validate(None, _view()) == INV
    assert capi.lib().rsx_iiq_correct_validate(C.byref(d), None) == INV


def _big_table(wide):
    # touched rows 8192, `wide` cell columns of width 1, two values a column
    head = (0, 0, wide, 16384, 1, 8192)
    return K.ff_payload(head, np.full((2, wide), 32768))


def test_table_bound_is_the_last_check():
    """8192 rows x 8193 cell columns = 2^26 + 8192 floats: refused; 8192 x 8192: accepted"""
    img = dict(w=9000, h=8192)
    d, keep = abi.iiq_corr([("ff", _big_table(8193), 0)])
    assert capi.iiq_correct_validate(d, _view(**img)) == UNS
    d, keep = abi.iiq_corr([("ff", _big_table(8192), 0)])
    assert capi.iiq_correct_validate(d, _view(**img)) == OK
    # (the cells in reach of the image count: a narrower image needs a narrower table)
    d, keep = abi.iiq_corr([("ff", _big_table(8193), 0)])
    assert capi.iiq_correct_validate(d, _view(w=4000, h=8192)) == OK
    # ... and a bad split in the same list is found first
    d, keep = abi.iiq_corr([("ff", _big_table(8193), 0), ("quad", CURVES, 0, 9001, 0)])
    assert capi.iiq_correct_validate(d, _view(**img)) == INV


def test_accepted_corners():
    ok = [
        ([], None, {}),                                      # an empty list
        ([("ff", K.ff_payload((0, 0, 64, 0, 8, 8), []), 0)], None, {}),  # a head field of 0: 16 bytes do
        ([("ff", K.ff_payload((0, 0, 0, 40, 8, 8), []), 1)], RGGB, {}),
        ([("ff", LUMA + b"\0\0\0", 0)], None, {}),         # bytes behind the values
        ([("ff", CHROMA, 1)], (2, 2, (0, 1, 3, 5)), {}),   # odd colours are skipped, not refused
        ([("ff", CHROMA, 1)], (8, 8, [0, 1, 1, 2] * 16), {}),
        ([("ff", LUMA, 0)], (2, 2, (0, 1, 4, 2)), {}),     # the CFA only matters to chroma
        ([("quad", CURVES, H, W, 1 << 30)], None, {}),     # splits at the full dimensions
        ([QUAD] * 16, None, {}),
        ([QUAD], None, dict(pitch=2 * W + 6)),
        ([("ff", K.ff_random(RNG, (60000, 60000, 64, 40, 8, 8)), 0)], None, {}),  # outside the image
    ]
    for ops, cfa, image in ok:
        d, keep = abi.iiq_corr(ops, cfa)
        assert capi.iiq_correct_validate(d, _view(**image)) == OK, (len(ops), cfa, image)


@pytest.fixture(scope="module")
def host():
    lib_path, _ = build.build_iiq_corr_host()
    L = C.CDLL(lib_path)
    L.rsx_iiq_corr_host_apply.argtypes = [C.c_void_p, C.c_void_p]
    L.rsx_iiq_corr_host_validate.argtypes = [C.c_void_p, C.c_void_p]
    return L


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_host_core_agrees_and_leaves_the_image_untouched(host, row):
    name, ops, cfa, image, n_ops, want = row
    d, keep = abi.iiq_corr(ops, cfa, n_ops)
    out = HostImage(W, H, pitch=2 * W + 16)
    out.pixels()[:] = RNG.integers(0, 65536, size=(H, W))
    before = out.buf.copy()
    v = out.view()
    if "w" in image:
        v.dim_x = image["w"]
    if "cpp" in image:
        v.cpp = image["cpp"]
    if "pitch" in image:
        v.pitch_bytes = image["pitch"]
    assert host.rsx_iiq_corr_host_validate(C.byref(d), C.byref(v)) == want
    assert host.rsx_iiq_corr_host_apply(C.byref(d), C.byref(v)) == want
    assert np.array_equal(out.buf, before)
