"""rsx_dctwrite_validate (include/rsx.h section 7e): every refusal, in the documented order, from
the library, the host build of the core and the model of tests/dctwrite_files.py alike; the bound
of a refused descriptor is 0.  No GPU."""
import ctypes as C
import itertools

import pytest

import dctwrite_files as D
from rawspeed_amd import abi, capi


def _desc(**kw):
    f = dict(off_x=2, off_y=1, width=40, height=24, components=3, h_samp=2, v_samp=2,
             restart_interval=3, flags=D.JFIF, reserved=0, luma=[16] * 64, chroma=[17] * 64)
    f.update(kw)
    d = abi.dctwrite_desc(f["off_x"], f["off_y"], f["width"], f["height"], f["components"],
                          f["h_samp"], f["v_samp"], f["luma"], f["chroma"], f["restart_interval"],
                          f["flags"])
    d.reserved = f["reserved"]
    return d


def _img(**kw):
    f = dict(pitch_bytes=2 * 3 * 30 + 4, dim_x=30, dim_y=20, cpp=3)
    f.update(kw)
    return abi.Image(None, f["pitch_bytes"], f["dim_x"], f["dim_y"], f["cpp"], 0)


def _all(desc, img):
    """the three verdicts; they must agree"""
    L = D.host_lib()
    host = L.rsx_dctwrite_host_validate(C.byref(desc) if desc else None, C.byref(img) if img else None)
    lib = capi.dctwrite_validate(desc, img)
    model = D.model_validate(D.desc_dict(desc) if desc else None,
                             dict(dim_x=img.dim_x, dim_y=img.dim_y, cpp=img.cpp,
                                  pitch_bytes=img.pitch_bytes) if img else None)
    assert host == lib == model, (host, lib, model)
    if lib != D.OK:
        assert capi.dctwrite_bound(desc, img) == 0
    return lib


def _bad_table(t, i, v):
    tabs = {"luma": [16] * 64, "chroma": [17] * 64}
    tabs[t][i] = v
    return tabs


# (name, descriptor fields, image fields, status), in the order of the header comment
REFUSALS = [
    ("no pixels x", {}, dict(dim_x=0), D.INVALID_ARG),
    ("no pixels y", {}, dict(dim_y=0), D.INVALID_ARG),
    ("cpp 0", dict(components=0), dict(cpp=0), D.INVALID_ARG),
    ("odd pitch", {}, dict(pitch_bytes=2 * 3 * 30 + 1), D.INVALID_ARG),
    ("short pitch", {}, dict(pitch_bytes=2 * 3 * 30 - 2), D.INVALID_ARG),
    ("components != cpp", dict(components=1, h_samp=1, v_samp=1), {}, D.INVALID_ARG),
    ("cpp != components", {}, dict(cpp=1, pitch_bytes=64), D.INVALID_ARG),
    ("off_x", dict(off_x=30), {}, D.INVALID_ARG),
    ("off_y", dict(off_y=20), {}, D.INVALID_ARG),
    ("width 0", dict(width=0), {}, D.INVALID_ARG),
    ("height 0", dict(height=0), {}, D.INVALID_ARG),
    ("width 65536", dict(width=65536), {}, D.INVALID_ARG),
    ("height 65536", dict(height=65536), {}, D.INVALID_ARG),
    ("restart 65536", dict(restart_interval=65536), {}, D.INVALID_ARG),
    ("unknown flag", dict(flags=2), {}, D.INVALID_ARG),
    ("reserved", dict(reserved=1), {}, D.INVALID_ARG),
    ("luma entry 0", _bad_table("luma", 63, 0), {}, D.INVALID_ARG),
    ("luma entry 256", _bad_table("luma", 0, 256), {}, D.INVALID_ARG),
    ("chroma entry 0", _bad_table("chroma", 17, 0), {}, D.INVALID_ARG),
    ("chroma entry 256", _bad_table("chroma", 5, 256), {}, D.INVALID_ARG),
    ("two components", dict(components=2), dict(cpp=2), D.UNSUPPORTED),
    ("four components", dict(components=4), dict(cpp=4, pitch_bytes=2 * 4 * 30), D.UNSUPPORTED),
    ("sampling 1x2", dict(h_samp=1, v_samp=2), {}, D.UNSUPPORTED),
    ("sampling 4x1", dict(h_samp=4, v_samp=1), {}, D.UNSUPPORTED),
    ("sampling 0x0", dict(h_samp=0, v_samp=0), {}, D.UNSUPPORTED),
    ("grey 2x2", dict(components=1), dict(cpp=1, pitch_bytes=60), D.UNSUPPORTED),
]


def test_null_arguments():
    assert _all(None, _img()) == D.INVALID_ARG
    assert _all(_desc(), None) == D.INVALID_ARG


def test_accepted():
    assert _all(_desc(), _img()) == D.OK
    for hs, vs in ((1, 1), (2, 1), (2, 2)):
        assert _all(_desc(h_samp=hs, v_samp=vs), _img()) == D.OK
    assert _all(_desc(components=1, h_samp=1, v_samp=1, chroma=[0] * 64),
                _img(cpp=1, pitch_bytes=60)) == D.OK  # (grey reads one table)
    assert _all(_desc(width=65535, height=65535, restart_interval=65535, flags=0), _img()) == D.OK
    assert _all(_desc(off_x=29, off_y=19), _img()) == D.OK
    assert capi.dctwrite_bound(_desc(), _img()) == D.model_bound([2, 1, 40, 24], 3, 2, 2, 3, True)


@pytest.mark.parametrize("name,dkw,ikw,status", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal(name, dkw, ikw, status):
    assert _all(_desc(**dkw), _img(**ikw)) == status


def test_order_of_the_refusals():
    """two defects at once give the verdict of the one the header lists first: every
    RSX_ERR_INVALID_ARG check stands in front of the RSX_ERR_UNSUPPORTED ones, and the model, which
    states the order line by line, agrees on every pair"""
    for (na, da, ia, sa), (nb, db, ib, sb) in itertools.combinations(REFUSALS, 2):
        if set(da) & set(db) or set(ia) & set(ib):
            continue
        if (na, nb) == ("components != cpp", "cpp != components"):
            continue  # (together they are a grey image and a grey descriptor)
        got = _all(_desc(**da, **db), _img(**ia, **ib))
        assert got != D.OK, (na, nb)
        if sa == D.INVALID_ARG and sb == D.UNSUPPORTED and "cpp" not in ib:
            assert got == D.INVALID_ARG, (na, nb)
