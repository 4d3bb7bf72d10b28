"""RawImageData::fixBadPixels (include/rsx.h section 5) as a numpy model, the cases every test of
the stage shares, and the case file the stand-alone programs read.

The model walks one pixel at a time, as the reference does (common/RawImage.cpp:297-323,
common/RawImageDataU16.cpp:399-485, common/RawImageDataFloat.cpp:177-260); binary32 arithmetic
is numpy float32, one operation at a time.  tests/golden/bad_pixels_ref.json holds the
reference's own answers (scripts/record_bad_pixels_ref.cpp wrote them); to rebuild it:

    python tests/bad_pixels_files.py --write-cases /tmp/bp_cases.bin
    /tmp/record_bad_pixels_ref /tmp/bp_cases.bin > /tmp/bp_ref.jsonl
    python tests/bad_pixels_files.py --golden /tmp/bp_ref.jsonl

The last step refuses to write the file unless the model agrees with every recorded answer.
"""
import functools
import hashlib
import json
import os
import struct
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bad_pixels_ref.json")
NAN_X86 = 0xFFC00000


def map_pitch(w):
    return (-(-w // 8) + 15) // 16 * 16


def pos(x, y):
    return (y << 16) | x


def make_map(w, h, positions, map_in=None):
    """the map as transferBadPixelsToMap leaves it: (h, map_pitch) uint8"""
    m = np.zeros((h, map_pitch(w)), np.uint8) if map_in is None else map_in.copy()
    for p in positions:
        x, y = p & 0xFFFF, p >> 16
        assert x < w and y < h
        m[y, x >> 3] |= 1 << (x & 7)
    return m


def map_bits(m, w):
    return np.unpackbits(m, axis=1, bitorder="little")[:, :w].astype(bool)


def bits_map(bad):
    h, w = bad.shape
    full = np.zeros((h, map_pitch(w) * 8), np.uint8)
    full[:, :w] = bad
    return np.packbits(full, axis=1, bitorder="little")


def _walks(bad, x, y, step):
    """the four lists of candidate positions in walk order: [(xx, yy, distance)]"""
    h, w = bad.shape
    return ([(q, y, x - q) for q in range(x - step, -1, -step) if not bad[y, q]],
            [(q, y, q - x) for q in range(x + step, w, step) if not bad[y, q]],
            [(x, q, y - q) for q in range(y - step, -1, -step) if not bad[q, x]],
            [(x, q, q - y) for q in range(y + step, h, step) if not bad[q, x]])


def _fix_u16(img, bad, x, y, step):
    values, dist = [-1] * 4, [0] * 4
    for i, cand in enumerate(_walks(bad, x, y, step)):
        if cand:
            xx, yy, d = cand[0]
            values[i], dist[i] = int(img[yy, xx]), d
    weight, shifts = [0] * 4, 7
    for a in (0, 2):
        t = dist[a] + dist[a + 1]
        if t:
            weight[a] = (t - dist[a]) * 256 // t if dist[a] else 0
            weight[a + 1] = 256 - weight[a]
            shifts += 1
    total = sum(v * wt for v, wt in zip(values, weight) if v >= 0) >> shifts
    return min(max(total, 0), 65535)


def _fix_f32(img, bad, x, y, step):
    """img: float32.  Returns the bit pattern."""
    f = np.float32
    values, dist = [f(-1)] * 4, [f(0)] * 4
    for i, cand in enumerate(_walks(bad, x, y, step)):
        for xx, yy, d in cand:
            if not values[i] < 0:  # (the loop condition: -0.0 and NaN stop the walk)
                break
            values[i], dist[i] = img[yy, xx], f(d)
    weight, div = [f(0)] * 4, f(0.000001)
    for a in (0, 2):
        t = f(dist[a] + dist[a + 1])
        if t > 0:
            weight[a] = f(f(t - dist[a]) / t) if dist[a] > 0 else f(0)
            weight[a + 1] = f(f(1) - weight[a])
            div = f(div + f(1))
    total = f(0)
    for v, wt in zip(values, weight):
        if v >= 0:
            total = f(total + f(v * wt))
    total = f(total / div)
    if np.isnan(total):
        return NAN_X86
    return int(np.array([total], np.float32).view(np.uint32)[0])


def model_fix(img, cfa, positions, map_in=None):
    """img: (h, w) uint16, or uint32 holding binary32 bit patterns.  Returns (image, map or None,
    n_bad, n_fixed): what fixBadPixels leaves; the map is None when the reference makes none."""
    h, w = img.shape
    if not len(positions) and map_in is None:
        return img.copy(), None, 0, 0
    m = make_map(w, h, positions, map_in)
    bad = map_bits(m, w)
    step = 2 if cfa else 1
    out = img.copy()
    fimg = img.view(np.float32) if img.dtype == np.uint32 else None
    end = (w + 15) // 32 * 32
    ys, xs = np.nonzero(bad[:, :end])
    with np.errstate(all="ignore"):
        for y, x in zip(ys.tolist(), xs.tolist()):
            out[y, x] = _fix_u16(img, bad, x, y, step) if fimg is None else \
                _fix_f32(fimg, bad, x, y, step)
    return out, m, int(bad.sum()), len(ys)


# ---------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------
def _image(seed, w, h, f32):
    rng = np.random.default_rng(seed)
    if f32:
        return (rng.random((h, w), np.float32) * np.float32(65535)).astype(np.float32).view(np.uint32)
    return rng.integers(0, 65536, (h, w), dtype=np.uint16)


def _gap(x, y, dl, dr, step, vertical=False):
    """marks (x, y) and its same-lattice neighbours so that the nearest good ones are dl / dr away"""
    out = []
    for q in range(-dl + step, dr, step):
        out.append(pos(x, y + q) if vertical else pos(x + q, y))
    return out


def _random_positions(seed, w, h, density):
    rng = np.random.default_rng(seed)
    ys, xs = np.nonzero(rng.random((h, w)) < density)
    return [pos(int(x), int(y)) for y, x in zip(ys, xs)]


def _bases():
    """(name, w, h, positions(step), map bits(step) or None, patches(step): [(x, y, u16, f32)],
    also as F32)"""
    B = []

    def add(name, w, h, positions, map_fn=None, patches=None, f32=False):
        B.append((name, w, h, positions, map_fn, patches or (lambda s: []), f32))

    W, H = 40, 20
    add("interior", W, H, lambda s: [pos(17, 9)], f32=True)
    for name, (x, y) in (("corner_tl", (0, 0)), ("corner_tr", (W - 1, 0)), ("corner_bl", (0, H - 1)),
                         ("corner_br", (W - 1, H - 1)), ("edge_left", (0, 9)), ("edge_right", (W - 1, 8)),
                         ("edge_top", (17, 0)), ("edge_bottom", (18, H - 1)), ("row1", (17, 1)),
                         ("col1", (1, 9)), ("near_corner_11", (1, 1)), ("near_corner_10", (1, 0)),
                         ("near_corner_01", (0, 1)), ("last_but_one", (W - 2, H - 2))):
        add(name, W, H, lambda s, x=x, y=y: [pos(x, y)], f32=name in ("corner_tl", "edge_left", "edge_right",
                                                                       "edge_bottom", "row1", "col1",
                                                                       "near_corner_11",
                                                                       "near_corner_10"))
    add("two_by_two", 2, 2, lambda s: [pos(0, 0)], f32=True)  # (no neighbour under a CFA: shift 7)
    add("two_rows", 17, 2, lambda s: [pos(8, 0), pos(3, 1)], f32=True)  # (no vertical neighbour under a CFA)

    def pair(a, b, s):
        return (a, b) if s == 1 or (a % 2 == 0 and b % 2 == 0) else (2 * a, 2 * b)

    for a, b in ((2, 4), (1, 2), (3, 5), (2, 62)):
        add("pair_%d_%d" % (a, b), 140, 80,
            lambda s, a=a, b=b: _gap(20, 5, *pair(a, b, s), s) + _gap(131, 12, *pair(a, b, s), s, True) +
            _gap(100, 70, *reversed(pair(a, b, s)), s), f32=True)
    for name, v in (("sides_0", 0), ("sides_65535", 65535)):
        add(name, W, H, lambda s: [pos(20, 10)],
            patches=lambda s, v=v: [(20 + dx, 10 + dy, v, float(v)) for d in (1, 2)
                                    for dx, dy in ((-d, 0), (d, 0), (0, -d), (0, d))], f32=v == 65535)
    add("other_parity_between", W, H,
        lambda s: [pos(20, 10), pos(21, 10), pos(19, 10), pos(20, 11), pos(20, 9)], f32=True)
    add("run_h", 60, 12, lambda s: [pos(x, 5) for x in range(10, 41, s)])
    add("run_v", 20, 60, lambda s: [pos(7, y) for y in range(10, 41, s)], f32=True)
    add("run_h_70", 300, 6, lambda s: [pos(x, 2) for x in range(21, 91)])
    add("run_h_150", 300, 6, lambda s: [pos(x, 3) for x in range(50, 200)], f32=True)
    add("run_v_70_150", 24, 200, lambda s: [pos(5, y) for y in range(33, 103)] +
        [pos(14, y) for y in range(20, 170)], f32=True)
    add("runs_to_the_edges", 100, 40,
        lambda s: [pos(x, 4) for x in range(0, 31)] + [pos(x, 9) for x in range(80, 100)] +
        [pos(50, y) for y in range(0, 12)] + [pos(61, y) for y in range(25, 40)], f32=True)
    add("whole_row", 130, 9, lambda s: [pos(x, 4) for x in range(130)], f32=True)
    add("whole_column", 33, 70, lambda s: [pos(16, y) for y in range(70)], f32=True)
    add("one_lattice", 34, 10, lambda s: [pos(x, y) for y in range(0, 10, 2) for x in range(0, 34, 2)],
        f32=True)
    add("whole_image", 34, 10, lambda s: [pos(x, y) for y in range(10) for x in range(34)], f32=True)
    add("whole_image_but_one", 34, 10,
        lambda s: [pos(x, y) for y in range(10) for x in range(34) if (x, y) != (20, 4)], f32=True)
    for i, w in enumerate((16, 17, 32, 33, 48, 49, 95, 96, 130)):
        add("width_%d" % w, w, 5, lambda s, w=w: _random_positions(100 + w, w, 5, 0.2), f32=i % 2 == 0)
    for i, h in enumerate((2, 3, 66, 130)):
        add("height_%d" % h, 40, h, lambda s, h=h: _random_positions(200 + h, 40, h, 0.1), f32=i % 2 == 1)
    add("duplicates", W, H, lambda s: [pos(17, 9), pos(5, 3), pos(17, 9), pos(17, 9), pos(5, 3)])
    add("map_alone", 49, 20, lambda s: [],
        map_fn=lambda s: _random_positions(301, 49, 20, 0.1), f32=True)
    add("map_and_positions", 49, 20, lambda s: _random_positions(302, 49, 20, 0.05),
        map_fn=lambda s: _random_positions(303, 49, 20, 0.1), f32=True)
    add("empty_map_alone", W, H, lambda s: [], map_fn=lambda s: [])
    for name, d in (("random_0p1", 0.001), ("random_5", 0.05), ("random_50", 0.5)):
        add(name, 520, 130, lambda s, d=d: _random_positions(400 + int(d * 1000), 520, 130, d),
            f32=d != 0.05)
    return B


def _f32_only():
    """(name, w, h, cfa, positions, patches [(x, y, binary32 value)])"""
    neg = [("f32_negative_passed", 60, 30, True, [pos(30, 15)],
            [(28, 15, -3.5), (26, 15, -1.0), (32, 15, -7.0), (30, 13, -2.0), (30, 17, -0.5), (30, 19, -9.0)]),
           ("f32_negative_last_before_edge", 60, 30, True, [pos(4, 15), pos(30, 3)],
            [(2, 15, -3.0), (0, 15, -4.0), (30, 1, -5.0)]),
           ("f32_negative_last_before_edge_plain", 60, 30, False, [pos(2, 15), pos(57, 8)],
            [(1, 15, -3.0), (0, 15, -4.0), (58, 8, -1.0), (59, 8, -2.0)]),
           ("f32_negative_zero", 60, 30, True, [pos(30, 15)], [(28, 15, -0.0), (30, 17, -0.0)]),
           ("f32_nan", 60, 30, False, [pos(30, 15), pos(10, 5)],
            [(29, 15, float("nan")), (30, 16, float("nan")), (10, 4, float("nan")), (10, 6, float("nan")),
             (9, 5, float("nan")), (11, 5, float("nan"))]),
           ("f32_inf", 60, 30, True, [pos(30, 15), pos(0, 4)],
            [(28, 15, float("inf")), (30, 17, float("inf")), (2, 4, float("inf"))]),
           ("f32_inf_left_only", 60, 30, False, [pos(59, 10)], [(58, 10, float("inf"))])]
    return neg


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, cfa, f32, image (h, w) uint16 / uint32 bits, positions, map_in or None)]"""
    out = []
    for name, w, h, positions, map_fn, patches, also_f32 in _bases():
        kinds = [("cfa", True, False), ("plain", False, False)]
        if also_f32:
            kinds.append(("f32_cfa", True, True) if len(out) % 4 < 2 else ("f32_plain", False, True))
        for tag, cfa, f32 in kinds:
            step = 2 if cfa else 1
            seed = int.from_bytes(hashlib.sha256((name + tag).encode()).digest()[:4], "little")
            img = _image(seed, w, h, f32)
            for x, y, v16, v32 in patches(step):
                if f32:
                    img.view(np.float32)[y, x] = v32
                else:
                    img[y, x] = v16
            m = None if map_fn is None else make_map(w, h, map_fn(step))
            out.append(("%s_%s" % (name, tag), cfa, f32, img, tuple(positions(step)), m))
    for name, w, h, cfa, positions, patches in _f32_only():
        seed = int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")
        img = _image(seed, w, h, True)
        for x, y, v in patches:
            img.view(np.float32)[y, x] = v
        out.append((name, cfa, True, img, tuple(positions), None))
    for cfa in (True, False):
        img = _image(77, 50, 24, True)
        f = img.view(np.float32)
        f[:] = -f - np.float32(1)
        out.append(("f32_all_negative_%s" % ("cfa" if cfa else "plain"), cfa, True, img,
                    (pos(20, 10), pos(0, 0), pos(49, 23), pos(21, 10)), None))
    assert len({c[0] for c in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected(name):
    """model_fix of case `name`, computed once"""
    c = {c[0]: c for c in cases()}[name]
    return model_fix(c[3], c[1], c[4], c[5])


def input_hash(case):
    name, cfa, f32, img, positions, m = case
    h, w = img.shape
    d = hashlib.sha256()
    d.update(struct.pack("<6I", w, h, int(cfa), int(f32), len(positions), int(m is not None)))
    d.update(np.asarray(positions, np.uint32).tobytes())
    if m is not None:
        d.update(m.tobytes())
    d.update(np.ascontiguousarray(img).tobytes())
    return d.hexdigest()


def padded(img, pad_samples, fill):
    h, w = img.shape
    buf = np.full((h, w + pad_samples), fill, img.dtype)
    buf[:, :w] = img
    return buf


def write_case_file(path):
    """the file rsx_bad_pixels_host_check and scripts/record_bad_pixels_ref.cpp read: uint32 count,
    then per case a 64-byte name, uint32 w, h, pitch, cfa, f32, n_pos, has_map; the positions; the
    map; the image rows at `pitch`; the model's image; the model's map (zeros where none is made)"""
    cs = cases()
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cs)))
        for i, c in enumerate(cs):
            name, cfa, f32, img, positions, m = c
            h, w = img.shape
            pad = 3 if i % 2 else 0
            want, wmap, _, _ = expected(name)
            f.write(name.encode().ljust(64, b"\0"))
            f.write(struct.pack("<7I", w, h, (w + pad) * img.itemsize, int(cfa), int(f32),
                                len(positions), int(m is not None)))
            f.write(np.asarray(positions, np.uint32).tobytes())
            if m is not None:
                f.write(m.tobytes())
            fill = 0x5A5A if img.dtype == np.uint16 else 0x5A5A5A5A
            f.write(padded(img, pad, fill).tobytes())
            f.write(padded(want, pad, fill).tobytes())
            f.write((np.zeros((h, map_pitch(w)), np.uint8) if wmap is None else wmap).tobytes())


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def model_hashes(name):
    want, wmap, _, _ = expected(name)
    return _sha(want), (None if wmap is None else _sha(wmap))


def _write_golden(recorded_path):
    rec = {}
    for line in open(recorded_path):
        if line.strip():
            r = json.loads(line)
            rec[r["name"]] = r
    out, wrong = {}, []
    for c in cases():
        r = rec[c[0]]
        img_h, map_h = model_hashes(c[0])
        if r["input"] != input_hash(c) or r["image"] != img_h or r["map"] != map_h:
            wrong.append(c[0])
        out[c[0]] = {"input": r["input"], "image": r["image"], "map": r["map"]}
    if wrong:
        sys.exit("the model disagrees with the reference on: %s" % ", ".join(wrong))
    with open(GOLDEN, "w") as f:
        json.dump({"recorder": "scripts/record_bad_pixels_ref.cpp", "cases": out}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases -> %s" % (len(out), GOLDEN))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--write-cases":
        write_case_file(sys.argv[2])
    elif len(sys.argv) == 3 and sys.argv[1] == "--golden":
        _write_golden(sys.argv[2])
    else:
        sys.exit(__doc__)
