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
