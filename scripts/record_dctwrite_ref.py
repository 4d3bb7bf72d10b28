"""Records tests/golden/dctwrite_ref.json: small images, the JPEG stream Pillow's encoder
(libjpeg-turbo, every default left alone but quality / qtables, subsampling and
restart_marker_blocks) writes for each, and the SHA-256 of what Pillow's decoder makes of that
stream.  The images are stored with the streams; they come from the closed forms below (an LCG, a
few integer patterns), never from a library's random generator.

    python scripts/record_dctwrite_ref.py

Needs Pillow; the tests do not.  A second run writes the same file.  The recorder asserts that the
numpy model of tests/dctwrite_files.py reproduces every stream, and that the set covers what
dctwrite_files.COVERAGE lists; the flags are recorded with the file."""
import base64
import io
import json
import os
import sys

import numpy as np
from PIL import Image, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dng_jpeg_files as J  # noqa: E402
import dctwrite_files as D  # noqa: E402


def lcg(seed, n):
    """n bytes: the top byte of x <- 1664525 x + 1013904223 (mod 2^32), x0 = seed"""
    out, x = np.zeros(n, np.uint8), seed & 0xFFFFFFFF
    for i in range(n):
        x = (1664525 * x + 1013904223) & 0xFFFFFFFF
        out[i] = x >> 24
    return out


def content(kind, seed, w, h, cpp):
    y, x = np.mgrid[0:h, 0:w]
    if kind == "noise":
        px = lcg(seed, w * h * cpp).reshape(h, w, cpp)
    elif kind == "smooth":
        # a ramp with a slow triangle wave and a little noise
        tri = np.abs((x * 5 + y * 3 + seed) % 128 - 64)
        base = (40 + x + 2 * y + tri) % 256
        px = np.stack([(base + 37 * c) % 256 for c in range(cpp)], -1)
        px = (px + (lcg(seed, w * h * cpp).reshape(h, w, cpp) >> 6)) % 256
    elif kind == "extreme":
        # 8 x 8 blocks: all 0, all 255, a left/right step, a top/bottom step, a checkerboard
        k = ((x // 8) + 3 * (y // 8) + seed) % 5
        px = np.select([k == 0, k == 1, k == 2, k == 3],
                       [0 * x, 255 + 0 * x, 255 * ((x % 8) >= 4), 255 * ((y % 8) >= 4)],
                       255 * ((x + y) % 2))
        px = np.stack([px if c != 1 else 255 - px for c in range(cpp)], -1)
    elif kind == "sparse":
        # flat blocks with one fine diagonal ripple: long zero runs in front of a late coefficient
        px = 100 + 8 * (((x + y) % 2) * 2 - 1) * ((x // 8 + y // 8 + seed) % 2) + (x // 8) * 3
        px = np.stack([px + 5 * c for c in range(cpp)], -1)
    else:
        raise ValueError(kind)
    px = px.astype(np.uint8)
    return px[..., 0] if cpp == 1 else px


def pillow_stream(frame_px, cpp, sub, quality, qtables, restart):
    im = Image.fromarray(frame_px, "L" if cpp == 1 else "RGB")
    kw = {}
    if qtables:
        kw["qtables"] = [list(t) for t in qtables[:2 if cpp == 3 else 1]]
    else:
        kw["quality"] = quality
    if cpp == 3:
        kw["subsampling"] = sub
    if restart:
        kw["restart_marker_blocks"] = restart
    b = io.BytesIO()
    im.save(b, "JPEG", **kw)
    return b.getvalue()


def analyse(stream, cpp):
    """flags of one Pillow stream, from its own bits"""
    st, H = J.model_validate(stream, cpp)
    assert st == J.OK
    flags, pads = set(), []
    nb = [H["hs"] * H["vs"], 1, 1] if cpp == 3 else [1]
    segs = J.segments(stream, H)
    if len(segs) >= 9:
        flags.add("nine_intervals")
    if len(segs) > 1 and segs[-1][1] < segs[0][1]:
        flags.add("short_last_interval")
    for first, count, start, end in segs:
        B = J._Bits(stream, start, end)
        data = (B.v >> 32).to_bytes(B.n // 8, "big")
        for _ in range(count):
            for c in range(cpp):
                for _ in range(nb[c]):
                    dc, ac = H["dc"][c], H["ac"][c]
                    k = B.symbol(dc)
                    if k == 11:
                        flags.add("dc_category_11")
                    if k:
                        B.extend(k)
                    k, eob = 1, False
                    while k < 64:
                        rs = B.symbol(ac)
                        r, size = rs >> 4, rs & 15
                        if size:
                            k += r
                            B.extend(size)
                            if size == 10:
                                flags.add("ac_size_10")
                        elif r == 15:
                            k += 15
                            flags.add("zrl")
                        else:
                            eob = True
                            break
                        k += 1
                    if not eob:
                        flags.add("no_eob")
        pad = B.n - B.at
        assert 0 <= pad <= 7
        pads.append(pad)
        flags.add("pad_%d" % pad)
        body = data[:-1] if pad else data
        if 0xFF in body:
            flags.add("stuffed_ff_in_data")
        if pad and data[-1] == 0xFF:
            flags.add("stuffed_ff_in_padding")
    return flags, pads


CASES = []
for (w, h) in ((1, 1), (8, 8), (16, 16), (17, 16), (33, 17)):
    for mode, cpp, sub in (("grey", 1, 0), ("c444", 3, 0), ("c422", 3, 1), ("c420", 3, 2)):
        CASES.append(dict(name="size_%dx%d_%s" % (w, h, mode), kind="noise", seed=w * 100 + h + sub,
                          dim=(w, h), cpp=cpp, sub=sub, quality=90, restart=0))
CASES += [
    dict(name="grey_noise_q100_ri1", kind="noise", seed=1, dim=(64, 48), cpp=1, sub=0, quality=100, restart=1),
    dict(name="grey_smooth_q75", kind="smooth", seed=2, dim=(64, 48), cpp=1, sub=0, quality=75, restart=0),
    dict(name="c444_noise_q100_ri5", kind="noise", seed=3, dim=(64, 48), cpp=3, sub=0, quality=100, restart=5),
    dict(name="c420_smooth_q85_row", kind="smooth", seed=4, dim=(64, 40), cpp=3, sub=2, quality=85, restart=4),
    dict(name="c420_40x37_noise_q95_ri2", kind="noise", seed=5, dim=(40, 37), cpp=3, sub=2, quality=95, restart=2),
    dict(name="c422_40x21_noise_q60", kind="noise", seed=6, dim=(40, 21), cpp=3, sub=1, quality=60, restart=0),
    dict(name="c422_smooth_q92_ri3", kind="smooth", seed=7, dim=(56, 24), cpp=3, sub=1, quality=92, restart=3),
    dict(name="grey_extreme_q100", kind="extreme", seed=0, dim=(64, 48), cpp=1, sub=0, quality=100, restart=0),
    dict(name="c420_extreme_qtables", kind="extreme", seed=1, dim=(48, 32), cpp=3, sub=2,
         qtables=[[1 + (i % 3 == 0) for i in range(64)], [2 + (i // 8) for i in range(64)]], restart=1),
    dict(name="grey_sparse_q50", kind="sparse", seed=0, dim=(64, 48), cpp=1, sub=0, quality=50, restart=0),
    dict(name="c444_19x21_q30_ri3", kind="smooth", seed=8, dim=(19, 21), cpp=3, sub=0, quality=30, restart=3),
    dict(name="c420_oversize", kind="smooth", seed=9, dim=(19, 21), cpp=3, sub=2, quality=90, restart=0,
         frame=(3, 2, 32, 32)),
    dict(name="grey_oversize_ri2", kind="noise", seed=10, dim=(19, 21), cpp=1, sub=0, quality=80, restart=2,
         frame=(5, 0, 24, 29)),
    dict(name="c422_oversize", kind="noise", seed=11, dim=(21, 10), cpp=3, sub=1, quality=70, restart=0,
         frame=(0, 3, 40, 16)),
]


def record(c):
    w, h = c["dim"]
    px = content(c["kind"], c["seed"], w, h, c["cpp"])
    frame = list(c.get("frame", (0, 0, w, h)))
    cut = px[frame[1]:, frame[0]:]
    pad = ((0, max(0, frame[3] - cut.shape[0])), (0, max(0, frame[2] - cut.shape[1]))) + \
        (((0, 0),) if c["cpp"] == 3 else ())
    frame_px = np.ascontiguousarray(np.pad(cut, pad, mode="edge")[:frame[3], :frame[2]])
    stream = pillow_stream(frame_px, c["cpp"], c["sub"], c.get("quality"), c.get("qtables"), c["restart"])
    im = Image.open(io.BytesIO(stream))
    im.load()
    e = dict(name=c["name"], dim_x=w, dim_y=h, cpp=c["cpp"], frame=frame, subsampling=c["sub"],
             restart=c["restart"], pixels=base64.b64encode(px.tobytes()).decode(),
             stream=base64.b64encode(stream).decode(), sha256=J.sha(np.asarray(im)))
    if c.get("qtables"):
        e["qtables"] = c["qtables"]
    else:
        e["quality"] = c["quality"]
    return e, px, stream


def main():
    assert features.check_feature("libjpeg_turbo"), "Pillow must be built on libjpeg-turbo"
    # quality= selects jpeg_quality_scaling's tables: the DQT segments of 100 streams
    one = np.zeros((8, 8, 3), np.uint8)
    dqt = []
    for q in range(1, 101):
        s = pillow_stream(one, 3, 0, q, None, 0)
        lu, ch = D.model_quality_tables(q)
        got = [s[at + 5:at + 69] for m, at, n in J.markers(s) if m == 0xDB]
        assert got == [bytes(t[D.ZZ[i]] for i in range(64)) for t in (lu, ch)], q
        dqt.append((got[0] + got[1]).hex())
    entries, flags, search = [], set(), 0
    todo = list(CASES)
    while todo:
        c = todo.pop(0)
        e, px, stream = record(c)
        stats = {}
        model = D.model_stream(px, c["cpp"], e["frame"], *D.SAMPLINGS[c["sub"]],
                               c.get("qtables") or D.model_quality_tables(c["quality"]), c["restart"],
                               True, stats)
        assert model == stream, c["name"]
        f, pads = analyse(stream, c["cpp"])
        assert pads == stats["pads"], c["name"]
        for d in stats["dummies"]:
            f.add("dummy_%s_h2v%d" % (d, D.SAMPLINGS[c["sub"]][1]))
        if c.get("search") and "stuffed_ff_in_padding" not in f:
            continue  # (a candidate that does not bring what it was tried for)
        e["flags"] = sorted(f)
        entries.append(e)
        flags |= f
        if not todo and "stuffed_ff_in_padding" not in flags:
            # an FF as the closing byte of an interval is a 1-in-hundreds event: walk seeds
            search += 1
            assert search < 400
            todo.append(dict(name="grey_noise_q100_ri1_padff", kind="noise", seed=1000 + search,
                             dim=(64, 48), cpp=1, sub=0, quality=100, restart=1, search=True))
    missing = [k for k in D.COVERAGE if k not in flags]
    assert not missing, missing
    assert all(max(e["dim_x"], e["frame"][2]) <= 64 and max(e["dim_y"], e["frame"][3]) <= 48
               for e in entries)
    out = dict(pillow=None,
               libjpeg_turbo=features.version("jpg"), coverage=sorted(flags), cases=entries,
               quality_dqt=dqt)
    import PIL
    out["pillow"] = PIL.__version__
    with open(D.GOLDEN, "w") as fh:
        json.dump(out, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print("%d cases, %d bytes, coverage %s" % (len(entries), os.path.getsize(D.GOLDEN), sorted(flags)))


if __name__ == "__main__":
    main()
