"""The host build of rsx_dctwrite_core.h (rawspeed_amd/librsx_dctwrite_host.so) against the
recorded streams of Pillow's encoder and the numpy model: every fixture with and without APP0,
images with pitch padding, the result fields, the capacity edge, the value range, the bound under
noise at tables of ones, and restart intervals the fixtures do not have.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import dctwrite_files as D
import dng_jpeg_files as J
from rawspeed_amd import abi

REQUIRED = ["size_%s_%s" % (s, m) for s in ("1x1", "8x8", "16x16", "17x16", "33x17")
            for m in ("grey", "c444", "c422", "c420")] + ["c420_oversize", "grey_oversize_ri2",
                                                          "c422_oversize"]


def test_the_named_frames_are_fixtures():
    names = {c["name"] for c in D.cases()}
    assert set(REQUIRED) <= names
    over = D.case("c420_oversize")
    assert over["frame"][0] + over["frame"][2] > over["dim_x"]
    assert over["frame"][1] + over["frame"][3] > over["dim_y"]


@pytest.mark.parametrize("c", D.cases(), ids=lambda c: c["name"])
def test_host_stream_is_the_recorded_stream(c):
    img = D.Img(c["pixels"], c["cpp"], pad=3)
    stats = {}
    D.model_case(c, stats=stats)
    st, got, r, intact = D.host_encode(D.desc_of(c), img)
    assert st == D.OK and intact and got.tobytes() == c["stream"]
    assert (r.status, r.bytes, r.scan_bytes, r.symbol_bits) == \
        (D.OK, len(c["stream"]), stats["scan_bytes"], stats["symbol_bits"])
    st, got, r, intact = D.host_encode(D.desc_of(c, jfif=False), img)
    assert st == D.OK and intact and got.tobytes() == J.without_marker(c["stream"], 0xE0)


@pytest.mark.parametrize("name", ["c444_noise_q100_ri5", "c420_40x37_noise_q95_ri2",
                                  "c422_40x21_noise_q60", "grey_oversize_ri2"])
@pytest.mark.parametrize("restart", [0, 1, 3, 7, 65535])
def test_host_follows_the_model_at_other_restart_intervals(name, restart):
    c = D.case(name)
    st, got, r, _ = D.host_encode(D.desc_of(c, restart=restart), D.Img(c["pixels"], c["cpp"]))
    assert st == D.OK and got.tobytes() == D.model_case(c, restart=restart)


def test_capacity_edge_and_value_range():
    c = D.case("c420_40x37_noise_q95_ri2")
    img, d = D.Img(c["pixels"], c["cpp"]), D.desc_of(c)
    n = len(c["stream"])
    st, got, r, intact = D.host_encode(d, img, cap=n)
    assert st == D.OK and intact and got.tobytes() == c["stream"]
    st, got, r, intact = D.host_encode(d, img, cap=n - 1)
    assert st == D.OVERFLOW and intact and (r.status, r.bytes, r.scan_bytes) == (D.OVERFLOW, 0, 0)
    px = c["pixels"].astype(np.uint16)
    px[36, 39, 2] = 256  # the last sample of the image
    st, got, r, intact = D.host_encode(d, D.Img(px, 3))
    assert st == D.VALUE_RANGE and intact and r.bytes == 0
    px[36, 39, 2] = 255
    assert D.host_encode(d, D.Img(px, 3))[0] == D.OK


def test_value_range_looks_only_at_samples_the_frame_reads():
    c = D.case("grey_oversize_ri2")  # frame (5, 0, 24, 29) of a 19 x 21 image
    px = c["pixels"].astype(np.uint16)
    px[0, 4] = 0xFFFF  # left of the frame
    st, got, _, _ = D.host_encode(D.desc_of(c), D.Img(px, 1))
    assert st == D.OK and got.tobytes() == c["stream"]
    px[20, 18] = 256  # the corner sample the frame replicates
    assert D.host_encode(D.desc_of(c), D.Img(px, 1))[0] == D.VALUE_RANGE


@pytest.mark.parametrize("sub", [0, 1, 2])
def test_noise_at_tables_of_ones_stays_under_the_bound(sub):
    """the worst input the fixtures' generator makes: LCG noise, every table entry 1, an interval an
    MCU.  The bound is a closed form of the geometry (include/rsx.h 7e)."""
    c = D.case("c444_noise_q100_ri5")
    hs, vs = D.SAMPLINGS[sub]
    d = abi.dctwrite_desc(0, 0, 64, 48, 3, hs, vs, [1] * 64, [1] * 64, 1)
    img = D.Img(c["pixels"], 3)
    L = D.host_lib()
    view = img.view()
    bound = int(L.rsx_dctwrite_host_bound(C.byref(d), C.byref(view)))
    assert bound == D.model_bound([0, 0, 64, 48], 3, hs, vs, 1, True)
    st, got, r, intact = D.host_encode(d, img)
    print("bound", bound, "bytes", r.bytes)
    assert st == D.OK and intact and 0 < r.bytes <= bound
    stats = {}
    want = D.model_stream(c["pixels"], 3, [0, 0, 64, 48], hs, vs, ([1] * 64, [1] * 64), 1, True, stats)
    assert got.tobytes() == want and r.symbol_bits == stats["symbol_bits"]


def test_quality_tables_of_the_host_build():
    L = D.host_lib()
    lu, ch = (C.c_uint16 * 64)(), (C.c_uint16 * 64)()
    for q in range(1, 101):
        assert L.rsx_dctwrite_host_quality_tables(q, lu, ch) == D.OK
        assert (list(lu), list(ch)) == D.model_quality_tables(q)
    for q in (0, 101, -5):
        assert L.rsx_dctwrite_host_quality_tables(q, lu, ch) == D.INVALID_ARG
