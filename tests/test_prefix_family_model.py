"""The value edges of PentaxDecompressor (isIntN(value, 16), PentaxDecompressor.cpp:155-177) and
SamsungV1Decompressor (isIntN(value, 12), SamsungV1Decompressor.cpp:123-137), without a GPU: the
plain int64 model (tests/nikon_cases.prefix_model), the oracle's C restatement and the reference
agree on the status and on every pixel.  The same images, several hundred workgroups large, are
what tests/test_gpu_prefix_family.py holds the device to."""
import numpy as np
import pytest

from rawspeed_amd import abi

import nikon_cases as N
from oracle_lib import HostImage

H, W = 160, 96  # (W: a multiple of 32 for SamsungV1)


def _cases():
    out = []
    for fam, (_, bits, _, _) in N.PREFIX_FAMILY.items():
        out += [(fam, v, p) for v, p in N.edge_cases(fam)]
        if bits == 16:
            out += [(fam, 40000, "plateau"), (fam, 65528, "plateau")]  # (+ 7: up to 65535)
    return out


@pytest.mark.parametrize("fam,value,place", _cases(), ids=lambda x: str(x))
def test_prefix_family_edges_model_oracle_ref(oracle, ref, fam, value, place):
    code, bits, _, maxv = N.PREFIX_FAMILY[fam]
    rng = np.random.default_rng([71, bits, maxv])
    base = N.smooth15(rng, H, W, maxv=maxv, sigma=30.0).astype(np.int64)
    img, at = N.edge_image(fam, base, value, place)
    data = N.encode_ints(img, [0, 0, 0, 0], code)
    model, fail = N.prefix_model(N.prefix_diffs(img, [0, 0, 0, 0]), bits)
    valid = 0 <= value < (1 << bits)
    # the model: the one value out of range is the first failure; a valid image decodes to itself
    assert fail == (None if valid else at), (fail, at)
    if valid:
        assert np.array_equal(model, img)
    hi, ri = HostImage(W, H), ref.image(W, H)
    if bits == 16:
        so, sr = oracle.pentax(N.pentax_desc(code), data, hi), ref.pentax(N.pentax_metadata(code), data, ri)
    else:
        so, sr = oracle.samsung_v1(abi.SamsungV1Desc.make(code), data, hi), ref.samsung_v1(12, data, ri)
    # (the reference reports the range error as a RawDecoderException: status 1)
    assert (so, sr) == ((0, 0) if valid else (abi.RSX_ERR_VALUE_RANGE, 1)), (so, sr, ref.last_error())
    if valid:
        assert np.array_equal(hi.pixels(), model)
        assert np.array_equal(ri.pixels(), model)
    else:
        assert "out of bounds" in ref.last_error()
        # what the oracle wrote in front of the failure is the model's
        y, x = fail
        assert np.array_equal(hi.pixels()[:y], model[:y])
        assert np.array_equal(hi.pixels()[y, :x], model[y, :x])
