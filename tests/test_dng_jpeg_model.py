"""The numpy model of tests/dng_jpeg_files.py and the host build of rsx_jpeg_core.h
(rawspeed_amd/librsx_jpeg_host.so) against every hash recorded from libjpeg-turbo's decoder
(tests/golden/dng_jpeg_ref.json), and -- only where Pillow imports -- against Pillow live on 200
further seeded images across the sampling modes and sizes 1 .. 40."""
import ctypes as C
import io

import numpy as np
import pytest

import dng_jpeg_files as J
from rawspeed_amd import abi, build

FILL = 0xA5A5


@pytest.fixture(scope="module")
def host():
    L = C.CDLL(build.build_jpeg_host()[0])

    def decode(stream, w, h, cpp, off=(0, 0)):
        tiles, keep = abi.dng_jpeg_tiles([stream], [off])
        out = np.full((h, w * cpp + 3), FILL, np.uint16)
        img = abi.Image(out.ctypes.data, out.strides[0], w, h, cpp, 0)
        st = L.rsx_jpeg_host_decode(tiles, C.byref(img))
        assert (out[:, w * cpp:] == FILL).all(), "the pitch padding was written"
        return st, out[:, :w * cpp]
    return decode


@pytest.mark.parametrize("name", [c["name"] for c in J.cases()])
def test_fixture_against_the_recorded_hash(host, name):
    c = J.case(name)
    st, got = J.model_decode(c["stream"], c["cpp"])
    assert st == J.OK and got.shape == (c["height"], c["width"] * c["cpp"])
    assert J.sha(got) == c["sha256"], "the model"
    st, got = host(c["stream"], c["width"], c["height"], c["cpp"])
    assert st == J.OK and J.sha(got) == c["sha256"], "the host core"


@pytest.mark.parametrize("c", J.damaged() + J.forged(), ids=lambda c: c["name"])
def test_damaged_is_refused_or_equal(host, c):
    st, got = J.model_decode(c["stream"], c["cpp"])
    w, h = (c["width"], c["height"]) if c["sha256"] else (64, 96)
    hst, hgot = host(c["stream"], w, h, c["cpp"])
    assert hst == st, "the model and the host core disagree about the verdict"
    if st == J.OK:
        assert c["sha256"] is not None, "libjpeg raised, the core decoded"
        assert J.sha(got) == c["sha256"] and J.sha(hgot) == c["sha256"]
    else:
        assert (hgot == FILL).all(), "a refused tile wrote into the image"


def test_the_damaged_set_holds_both_outcomes():
    verdicts = [J.model_decode(c["stream"], c["cpp"])[0] for c in J.damaged()]
    assert verdicts.count(J.OK) >= 10 and len(verdicts) - verdicts.count(J.OK) >= 10
    assert {J.BAD_CODE, J.RESTART, J.OVERFLOW, J.IO} <= set(verdicts)


def _segment_bounds(name):
    s = J.case(name)["stream"]
    return s, [(a, b) for _, _, a, b in J.segments(s, J.parse_header(s))]


def test_the_long_and_wide_fixtures_are_what_the_device_tests_take_them_for():
    """rsx_dng_jpeg.hip keeps 8192 bytes of a segment in LDS and reloads them once the walk is more
    than 4096 past their first; a workgroup of its finish kernel covers 1024 samples of a row.  The
    device tests cannot see a reload or a workgroup index: what makes them reach both is here."""
    s, ((a, b),) = _segment_bounds("long_grey_96x96")
    assert b - a >= 3 * 4096
    stuffed = [i - a for i in range(a, b - 1) if s[i] == 0xFF and s[i + 1] == 0]
    assert any(i < 4096 for i in stuffed) and any(i > 8192 for i in stuffed)
    _, ((a, b),) = _segment_bounds("long_420_64x64")
    assert b - a > 8192 and J.case("long_420_64x64")["cpp"] == 3
    _, segs = _segment_bounds("long_restart_grey_96x96")
    later = [b - a for a, b in segs[1:]]  # (they start deep inside the tile)
    assert max(later) > 4096 and min(later) < 4096 and segs[1][0] > 4096
    for name, samples in (("wide_grey_2064x8", 2064), ("wide_444_704x8", 2112),
                          ("wide_422_704x8", 2112), ("wide_420_704x16", 2112)):
        c = J.case(name)
        assert c["width"] * c["cpp"] == samples > 2 * 1024  # three workgroups a row
    H = J.parse_header(J.case("wide_422_704x8")["stream"])
    assert (H["hs"], H["vs"]) == (2, 1)
    H = J.parse_header(J.case("wide_420_704x16")["stream"])
    assert (H["hs"], H["vs"]) == (2, 2)
    # the fill runs: in front of a stuffed pair of the base, inside the first window and past 8192
    s, ((a, b),) = _segment_bounds("long_grey_96x96")
    fills = [c for c in J.damaged() if "repeat" in c]
    assert sorted((c["repeat"][1], c["head"] - a < 4096) for c in fills) == \
        sorted((n, near) for n in (1, 4095, 4096, 4097, 8192, 9000) for near in (True, False))
    for c in fills:
        at = c["head"]
        assert c["base"] == "long_grey_96x96" and c["repeat"][0] == 0xFF and s[at:at + 2] == b"\xff\x00"
        assert 16 <= at - a < 4096 or 8192 < at - a < b - a
        assert c["stream"] == s[:at] + b"\xff" * c["repeat"][1] + s[at:]
        assert c["sha256"] == J.case("long_grey_96x96")["sha256"]
    # the cuts: inside the second and the last 4096 bytes of the segment, and in front of EOI
    cuts = {c["name"].split("/")[1]: c for c in J.damaged() if c["name"].startswith("long_grey_96x96/cut")}
    assert a + 4096 < cuts["cut_at_6000"]["head"] < a + 8192
    assert b - 4096 < cuts["cut_at_12000"]["head"] < b
    assert cuts["cut_one_byte_before_eoi"]["stream"] == s[:-3]
    for k in ("cut_at_6000_eoi_kept", "cut_at_12000_eoi_kept"):  # (these reach the kernel)
        assert cuts[k]["stream"][-2:] == b"\xff\xd9"
        assert J.model_decode(cuts[k]["stream"], 1)[0] == J.OVERFLOW


def test_the_overshoot_fork():
    """the range limit saturates (libjpeg-turbo's SIMD code), it is not libjpeg's masked table;
    coefficients that leave 16 bits are refused"""
    by = {c["name"]: c for c in J.forged()}
    c = by["overshoot_moderate"]
    assert J.sha(J.model_decode(c["stream"], 1, "saturate")[1]) == c["sha256"]
    assert J.sha(J.model_decode(c["stream"], 1, "mask")[1]) != c["sha256"]
    assert J.model_decode(by["overshoot_extreme"]["stream"], 1)[0] == J.UNSUPPORTED


def test_window_of_the_host_core(host):
    c = J.case("420_47x71")
    _, frame = J.model_decode(c["stream"], 3)
    st, got = host(c["stream"], 29, 37, 3, off=(3, 5))
    want = np.full((37, 29 * 3), FILL, np.uint16)
    J.paste(want, frame, 3, 5, 3)
    assert st == J.OK and np.array_equal(got, want)


def test_200_random_images_live_against_pillow(host):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(20240607)
    modes = [("L", {}), ("RGB", {"subsampling": 0}), ("RGB", {"subsampling": 1}),
             ("RGB", {"subsampling": 2}), ("RGB", {"subsampling": 0, "keep_rgb": True})]
    for it in range(200):
        w, h = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        mode, kw = modes[it % len(modes)]
        kw = dict(kw, quality=int(rng.choice([1, 25, 50, 75, 90, 100])))
        if it % 3 == 0:
            kw["restart_marker_blocks"] = int(rng.integers(1, 5))
        if it % 4 == 1:
            kw["optimize"] = True
        y, x = np.mgrid[0:h, 0:w]
        px = 128 + 90 * np.sin(x / 4.0 + it) * np.cos(y / 6.0) + rng.normal(0, 25, (h, w))
        if mode == "RGB":
            px = px[..., None] + rng.normal(0, 25, (h, w, 3)) + np.array([20.0, -30.0, 10.0])
        b = io.BytesIO()
        Image.fromarray(np.clip(px, 0, 255).astype(np.uint8), mode).save(b, "JPEG", **kw)
        s = b.getvalue()
        cpp = 1 if mode == "L" else 3
        want = np.asarray(Image.open(io.BytesIO(s))).reshape(h, w * cpp).astype(np.uint16)
        st, got = J.model_decode(s, cpp)
        assert st == J.OK and np.array_equal(got, want), ("model", it, w, h, mode, kw)
        st, got = host(s, w, h, cpp)
        assert st == J.OK and np.array_equal(got, want), ("host core", it, w, h, mode, kw)
