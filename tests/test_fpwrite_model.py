"""The numpy model of the F32 writers (tests/fpwrite_files.py) against the oracle: its widening is
the oracle's F32 unpack on every binary16 pattern and on a stride of the binary24 ones with all
edges, the narrowing inverts it, and a stream the model packs unpacks under the oracle's
decodePackedFP / copyPixels to the image.  No GPU and no library of the project's is needed."""
import numpy as np
import pytest

import dng_deflate_files as DF
import fpwrite_files as F
from oracle_lib import HostImage, Oracle
from rawspeed_amd import abi


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


def test_widening_of_every_binary16_pattern_is_the_oracles():
    p = np.arange(1 << 16, dtype=np.uint32)
    assert np.array_equal(F.model_widen(p, 16), DF.widen(p, 16))


def test_widening_of_binary24_patterns_is_the_oracles():
    """every subnormal exponent step, the patterns around every power of two, a stride of the rest"""
    frac = 16
    edges = [np.arange(0, 1 << 17, dtype=np.uint32)]  # subnormals and the first normals
    for e in range(1, 128):
        base = e << frac
        edges.append(np.array([base - 1, base, base + 1], dtype=np.uint32))
    p = np.concatenate(edges + [np.arange(0, 1 << 23, 509, dtype=np.uint32), F.specials(24)])
    p = np.concatenate([p, p | np.uint32(1 << 23)])
    assert np.array_equal(F.model_widen(p, 24), DF.widen(p, 24))


@pytest.mark.parametrize("bps", (16, 24))
def test_narrowing_inverts_the_widening_on_every_pattern(bps):
    p = np.arange(1 << bps, dtype=np.uint32)
    n, exact = F.model_narrow(F.model_widen(p, bps), bps)
    assert exact.all() and np.array_equal(n, p)


@pytest.mark.parametrize("bps", (16, 24))
def test_neighbours_subnormals_and_large_exponents_are_inexact(bps):
    frac, expw = F.FORMAT[bps]
    images = F.model_widen(np.arange(1 << bps, dtype=np.uint32), bps)
    member = np.sort(images)
    for y in (images + np.uint32(1), images - np.uint32(1)):
        is_image = member[np.minimum(np.searchsorted(member, y), member.size - 1)] == y
        assert not is_image.any()  # (an image's low 23 - frac bits are zero)
        assert not F.model_narrow(y, bps)[1].any()
    sub = np.concatenate([np.arange(1, 4096, dtype=np.uint32), np.array([0x7FFFFF], np.uint32)])
    for sign in (0, 1 << 31):
        assert not F.model_narrow(sub | np.uint32(sign), bps)[1].any()
        top = 127 + (1 << (expw - 1))  # one above the narrow maximum
        big = np.array([(e << 23) | f for e in range(top, 255) for f in (0, 1 << (23 - frac))],
                       dtype=np.uint32)
        assert not F.model_narrow(big | np.uint32(sign), bps)[1].any()
    assert F.model_narrow(np.array([0, 1 << 31], np.uint32), bps)[1].all()  # +-0


def test_fit_of_the_model():
    x = F.exact_samples("fit", 16, 3, 5)
    assert F.model_fit(x) == 16
    x[2, 4] = 0x3F800080  # 1 + 2^-16
    assert F.model_fit(x) == 24
    x[0, 0] = 0x3F800001
    assert F.model_fit(x) == 32


@pytest.mark.parametrize("case", F.pack_cases(), ids=lambda c: c[0])
def test_model_stream_unpacks_under_the_oracle_to_the_image(oracle, case):
    d, img = F.pack_case(case)
    stream, inexact = F.model_pack(d, img)
    assert inexact == 0 and len(stream) == F.round_up4(d.crop_h * d.input_pitch_bytes)
    got = HostImage(img.dim_x, img.dim_y, img.cpp, fill=0, bpc=4)
    assert oracle.unpack_f32(d, stream, got) == abi.RSX_OK
    x0 = F.first_sample(d, img.cpp)
    cols = d.crop_w * img.cpp
    win = got.u32()[d.crop_y:d.crop_y + d.crop_h, x0:x0 + cols]
    assert np.array_equal(win, F.window_of(d, img))
    # bytes of the pitch behind the samples and the tail are zero
    body = stream[:d.crop_h * d.input_pitch_bytes].reshape(d.crop_h, -1)
    assert not body[:, cols * d.bits_per_pixel // 8:].any()
    assert not stream[d.crop_h * d.input_pitch_bytes:].any()
