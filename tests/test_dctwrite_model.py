"""The numpy model of the baseline-DCT JPEG writer (tests/dctwrite_files.py) against the recorded
streams of Pillow's encoder (tests/golden/dctwrite_ref.json): byte for byte with the APP0 segment
and without it, decodable by the model of the reader to the image Pillow's decoder made, the
quality scaling against the DQT segments Pillow wrote for every quality, and the coverage the
recorder asserted.  No GPU, no Pillow."""
import pytest

import dctwrite_files as D
import dng_jpeg_files as J


@pytest.mark.parametrize("c", D.cases(), ids=lambda c: c["name"])
def test_model_stream_is_the_recorded_stream(c):
    stats = {}
    with_app0 = D.model_case(c, jfif=True, stats=stats)
    assert with_app0 == c["stream"]
    assert D.model_case(c, jfif=False) == J.without_marker(c["stream"], 0xE0)
    assert stats["scan_bytes"] == len(c["stream"]) - len(D.model_header(
        c["frame"][2], c["frame"][3], c["cpp"], *D.SAMPLINGS[c["subsampling"]], D.tables_of(c),
        c["restart"], True)) - 2
    hs, vs = D.SAMPLINGS[c["subsampling"]]
    assert len(with_app0) <= D.model_bound(c["frame"], c["cpp"], hs, vs, c["restart"], True)


@pytest.mark.parametrize("c", D.cases(), ids=lambda c: c["name"])
def test_reader_model_decodes_the_stream_to_the_recorded_image(c):
    for jfif in (True, False):
        st, img = J.model_decode(D.model_case(c, jfif=jfif), c["cpp"])
        assert st == J.OK and J.sha(img) == c["sha256"]
        assert img.shape == (c["frame"][3], c["frame"][2] * c["cpp"])


def test_quality_tables_are_pillows_for_every_quality():
    for q in range(1, 101):
        lu, ch = D.model_quality_tables(q)
        want_lu, want_ch = D.quality_dqt(q)
        assert [lu[D.ZZ[i]] for i in range(64)] == want_lu, q
        assert [ch[D.ZZ[i]] for i in range(64)] == want_ch, q
    assert D.model_quality_tables(100) == ([1] * 64, [1] * 64)
    assert max(D.model_quality_tables(1)[0]) == 255  # (force_baseline)


def test_fixture_set_covers_what_the_recorder_asserted():
    g = D.golden()
    assert g["pillow"] and g["libjpeg_turbo"]
    assert set(D.COVERAGE) <= set(g["coverage"])
    per_case = set().union(*(set(c["flags"]) for c in g["cases"]))
    assert set(D.COVERAGE) <= per_case
    assert {"pad_%d" % k for k in range(8)} <= per_case  # every pad length
    # ... and the model sees the same pads and dummies in its own streams
    pads, dummies = set(), set()
    for c in g["cases"]:
        stats = {}
        D.model_case(c, stats=stats)
        pads |= set(stats["pads"])
        dummies |= {(d, D.SAMPLINGS[c["subsampling"]]) for d in stats["dummies"]}
    assert pads == set(range(8))
    assert dummies == {("right", (2, 1)), ("right", (2, 2)), ("bottom", (2, 2)), ("corner", (2, 2))}
    for c in g["cases"]:
        assert max(c["dim_x"], c["frame"][2]) <= 64 and max(c["dim_y"], c["frame"][3]) <= 48


def test_model_leaves_dummy_blocks_untransformed():
    """a dummy block is 6 bits of luma (DC difference 0, EOB) whatever lies beside the frame: the
    40-wide 4:2:0 fixture keeps its bytes when the image continues to the right of the frame"""
    import numpy as np
    c = D.case("c420_40x37_noise_q95_ri2")
    wide = np.concatenate([c["pixels"], 255 - c["pixels"][:, :8]], axis=1)
    d = dict(c, pixels=wide, dim_x=wide.shape[1])
    assert D.model_case(d) == c["stream"]
