"""Records tests/golden/dng_jpeg_ref.json and tests/golden/dng_jpeg_bench_tile.json: JPEG streams
written by Pillow's encoder (libjpeg-turbo) and the SHA-256 of what Pillow's decoder -- libjpeg-
turbo with every default left alone, as JpegDecompressor leaves them -- makes of each.  Damaged and
forged streams carry Pillow's outcome: an exception, or the hash of what it returned.  The long and
wide streams (long_wide_cases, long_damaged_cases) come last in their lists, so that the entries in
front of them stay as they were.

    python scripts/record_dng_jpeg_ref.py

Needs Pillow; the tests do not.  Everything is seeded: a second run writes the same files."""
import base64
import hashlib
import io
import json
import os
import sys
import warnings

import numpy as np
from PIL import Image, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dng_jpeg_files as J  # noqa: E402


def picture(seed, w, h, cpp, noise=12.0, smooth=1.0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 128 + smooth * (70 * np.sin(x / 6.0 + seed) * np.cos(y / 9.0) + 0.8 * (x - y))
    if cpp == 1:
        px = base + rng.normal(0, noise, (h, w))
        return Image.fromarray(np.clip(px, 0, 255).astype(np.uint8), "L")
    px = base[..., None] + rng.normal(0, noise, (h, w, 3)) + np.array([25.0, -10.0, -35.0]) + \
        np.stack([20 * np.cos(y / 5.0), 30 * np.sin(x / 4.0), 0 * x], axis=-1)
    return Image.fromarray(np.clip(px, 0, 255).astype(np.uint8), "RGB")


def encode(img, **kw):
    b = io.BytesIO()
    img.save(b, "JPEG", **kw)
    return b.getvalue()


def outcome(stream):
    """Pillow's: (sha256, width, height, cpp) or None for an exception"""
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            im = Image.open(io.BytesIO(stream))
            im.load()
        a = np.asarray(im)
        if a.dtype != np.uint8 or im.mode not in ("L", "RGB"):
            return None
        return hashlib.sha256(a.tobytes()).hexdigest(), im.width, im.height, 1 if im.mode == "L" else 3
    except Exception:
        return None


def entry(name, stream, cpp, **extra):
    e = dict(name=name, stream=base64.b64encode(stream).decode(), cpp=cpp)
    o = outcome(stream)
    if o is None:
        e.update(sha256=None)
    else:
        assert o[3] == cpp, (name, o)
        e.update(sha256=o[0], width=o[1], height=o[2])
    e.update(extra)
    return e


SUB = {"444": 0, "422": 1, "420": 2}


def base_cases():
    out = []
    seed = [100]

    def add(name, w, h, cpp, noise=5.0, **kw):
        seed[0] += 1
        kw.setdefault("quality", 80)
        s = encode(picture(seed[0], w, h, cpp, noise), **kw)
        e = entry(name, s, cpp)
        assert e["sha256"] is not None and (e["width"], e["height"]) == (w, h), name
        out.append(e)
        return s

    for w, h in ((8, 8), (1, 1), (33, 50)):
        add("grey_%dx%d" % (w, h), w, h, 1)
    for sub, sizes in (("444", ((17, 9), (48, 72))), ("422", ((16, 8), (47, 71))),
                       ("420", ((16, 16), (17, 17), (2, 2), (47, 71)))):
        for w, h in sizes:
            add("%s_%dx%d" % (sub, w, h), w, h, 3, subsampling=SUB[sub])
    s = add("rgb_40x56", 40, 56, 3, subsampling=0, keep_rgb=True)
    assert b"Adobe" in s and b"JFIF" not in s
    add("optimize_420_40x24", 40, 24, 3, subsampling=2, optimize=True)
    add("optimize_grey_24x40", 24, 40, 1, optimize=True)
    s = add("q100_noise_420_32x32", 32, 32, 3, noise=60.0, subsampling=2, quality=100)
    assert b"\xff\x00" in s[J.markers(s)[-1][1]:], "the quality-100 stream holds no stuffed byte"
    add("q100_noise_grey_24x24", 24, 24, 1, noise=60.0, quality=100)
    add("q1_noise_444_32x24", 32, 24, 3, noise=60.0, subsampling=0, quality=1)
    add("q1_noise_grey_40x16", 40, 16, 1, noise=60.0, quality=1)
    for name, blocks in (("restart1_420_64x96", 1), ("restart3_420_64x96", 3), ("restartrow_420_64x96", 4)):
        s = add(name, 64, 96, 3, subsampling=2, restart_marker_blocks=blocks)
        assert b"\xff\xdd" in s, name
        if blocks == 1:
            assert s.count(b"\xff\xd0") >= 2 and b"\xff\xd7" in s, name  # (24 intervals: RSTn wraps)
    s = add("restart1_grey_80x8", 80, 8, 1, restart_marker_blocks=1)
    assert s.count(b"\xff\xd0") >= 2
    # neither JFIF nor Adobe, ids that are neither 1, 2, 3 nor R, G, B: YCbCr
    s = base64.b64decode(next(e for e in out if e["name"] == "444_17x9")["stream"])
    s = J.with_ids(J.without_marker(s, 0xE0), (10, 11, 12))
    assert b"JFIF" not in s
    out.append(entry("forged_ids_444_17x9", s, 3))
    assert out[-1]["sha256"] is not None
    return out


def damaged_cases(cases):
    rng = np.random.default_rng(4242)
    out = []
    by = {e["name"]: base64.b64decode(e["stream"]) for e in cases}
    for base in ("optimize_420_40x24", "restart3_420_64x96", "grey_33x50"):
        s = by[base]
        cpp = 1 if base.startswith("grey") else 3
        sos = J.markers(s)[-1]
        scan = sos[1] + sos[2]

        def add(kind, t):
            out.append(entry("%s/%s" % (base, kind), bytes(t), cpp, base=base))

        add("cut_in_header", s[:int(rng.integers(20, scan - 4))])
        add("cut_mid_scan", s[:int(rng.integers(scan + 8, len(s) - 8))])
        add("cut_before_eoi", s[:-2])
        add("cut_last_data_byte", s[:-3] + s[-2:])
        add("eoi_removed_tail_kept", s[:-2] + b"\0\0")
        if b"\xff\xd2" in s[scan:]:
            at = s.index(b"\xff\xd2", scan)
            add("rst_renumbered", s[:at + 1] + b"\xd5" + s[at + 2:])
            add("rst_removed", s[:at] + s[at + 2:])
        dht = next(a for m, a, _ in J.markers(s) if m == 0xC4)
        t = bytearray(s)
        t[dht + 5 + 2] = 200  # (the count of 3-bit codes: more than can exist)
        add("dht_count", t)
        for k in range(24):
            at = int(rng.integers(scan, len(s) - 2))
            t = bytearray(s)
            t[at] ^= int(rng.integers(1, 256))
            add("byte_%02d_at_%d" % (k, at), t)
    return out


def _segments(s):
    """[(start, end)] of a stream's entropy segments"""
    return [(a, b) for _, _, a, b in J.segments(s, J.parse_header(s))]


def _stuffed(s, a, b):
    """offsets of the FF of every stuffed FF 00 pair in bytes [a, b) of s"""
    return [i for i in range(a, b - 1) if s[i] == 0xFF and s[i + 1] == 0]


def long_wide_cases():
    """Streams past one byte window (8192 bytes in LDS, reloaded every 4096) and tiles past one
    finish workgroup (1024 samples of a row) of rsx_dng_jpeg.hip.  Every property the tests rely on
    is asserted here: a re-recording cannot quietly lose it."""
    out = []

    def add(name, img, cpp, **kw):
        s = encode(img, **kw)
        e = entry(name, s, cpp)
        assert e["sha256"] is not None and (e["width"], e["height"]) == img.size, name
        out.append(e)
        return s

    rng = np.random.default_rng(9601)
    grey = Image.fromarray(rng.integers(0, 256, (96, 96), dtype=np.uint8), "L")
    s = add("long_grey_96x96", grey, 1, quality=100)
    (a, b), = _segments(s)
    assert b - a >= 3 * 4096
    assert _stuffed(s, a, a + 4096) and _stuffed(s, a + 8192, b)
    # (noise in all three components: RGB noise leaves the chroma planes half as loud)
    ycc = Image.fromarray(np.random.default_rng(6401).integers(0, 256, (64, 64, 3), dtype=np.uint8), "YCbCr")
    s = add("long_420_64x64", ycc, 3, quality=100, subsampling=2)
    (a, b), = _segments(s)
    assert b - a > 8192
    s = add("long_restart_grey_96x96", grey, 1, quality=100, restart_marker_blocks=60)
    later = [b - a for a, b in _segments(s)[1:]]
    assert any(n > 4096 for n in later) and any(n < 4096 for n in later), later
    for name, w, h, cpp, kw in (("wide_grey_2064x8", 2064, 8, 1, {}),
                                ("wide_444_704x8", 704, 8, 3, dict(subsampling=0)),
                                ("wide_422_704x8", 704, 8, 3, dict(subsampling=1)),
                                ("wide_420_704x16", 704, 16, 3, dict(subsampling=2))):
        s = add(name, picture(200 + len(out), w, h, cpp), cpp, quality=75, **kw)
        assert w * cpp > 2048 and len(s) < 4096, (name, len(s))
    return out


FILL_RUNS = (1, 4095, 4096, 4097, 8192, 9000)


def long_damaged_cases(cases):
    """long_grey_96x96 cut inside its second and its last window's worth of bytes (with and without
    an EOI behind the cut: only the first gets past the host's marker scan to the kernel), and runs
    of fill bytes in front of a stuffed FF 00 pair, which libjpeg skips: those decode to the base's
    image.  Already as edits of the base (`repeat`: a byte and a count in front of `insert`)."""
    base = "long_grey_96x96"
    c = next(e for e in cases if e["name"] == base)
    s = base64.b64decode(c["stream"])
    (a, b), = _segments(s)
    out = []

    def add(kind, head, insert, tail, **extra):
        rep = extra.get("repeat", (0, 0))
        t = s[:head] + bytes([rep[0]]) * rep[1] + insert + s[len(s) - tail:]
        e = entry("%s/%s" % (base, kind), t, 1, base=base)
        del e["stream"]
        e.update(head=head, insert=insert.hex(), tail=tail, **extra)
        out.append(e)
        return e

    assert a + 4096 < 6000 < a + 8192 and b - 4096 < 12000 < b
    for at in (6000, 12000):
        assert s[at - 1] != 0xFF
        assert add("cut_at_%d" % at, at, b"", 0)["sha256"] is None
        add("cut_at_%d_eoi_kept" % at, at, b"\xff\xd9", 0)
        assert J.model_decode(s[:at] + b"\xff\xd9", 1)[0] == J.OVERFLOW
    add("cut_one_byte_before_eoi", len(s) - 3, b"", 0)
    first = next(i for i in _stuffed(s, a, b) if i - a >= 16)
    beyond = _stuffed(s, a + 8192 + 1, b)[0]
    assert first - a < 4096
    for where, at in (("first_window", first), ("past_8192", beyond)):
        for n in FILL_RUNS:
            e = add("fill_%d_%s" % (n, where), at, b"", len(s) - at, repeat=[255, n])
            assert e["sha256"] == c["sha256"], e["name"]  # (libjpeg skipped the fill bytes)
    return out


def forged_cases():
    """Coefficients no encoder makes from 8-bit pixels, by raising quantisers of a quality-100
    stream (all ones): `moderate` leaves the sample range by more than 512 (where libjpeg's masked
    range-limit table and libjpeg-turbo's saturating SIMD code differ) but stays inside +-16383;
    `extreme` leaves 16 bits."""
    h, w = 8, 16
    x = np.arange(w)[None, :] % 8
    px = np.clip(205 + 40 * np.cos((2 * x + 1) * np.pi / 16) + 0 * np.arange(h)[:, None], 0, 255)
    s = encode(Image.fromarray(px.astype(np.uint8), "L"), quality=100)
    out = []
    for name, q0, q1 in (("moderate", 6, 5), ("extreme", 255, 255)):
        t = J.patched(J.patched(s, 0xDB, 1, q0), 0xDB, 2, q1)
        e = entry("overshoot_" + name, t, 1)
        st, got = J.model_decode(t, 1)
        e["model_status"] = st
        if st == J.OK:
            e["model_matches"] = {lim: J.sha(J.model_decode(t, 1, lim)[1]) == e["sha256"]
                                  for lim in ("saturate", "mask")}
        out.append(e)
    return out


def as_edit(e, by):
    """a damaged stream as an edit of its base: the base's first `head` bytes, `insert` (hex), the
    base's last `tail` bytes -- what tests/dng_jpeg_files.py puts together again (it also knows
    `repeat`, a byte and a count in front of `insert`: long_damaged_cases)"""
    s, b = base64.b64decode(e.pop("stream")), by[e["base"]]
    head = next((i for i in range(min(len(s), len(b))) if s[i] != b[i]), min(len(s), len(b)))
    tail = 0
    while tail < min(len(s), len(b)) - head and s[len(s) - 1 - tail] == b[len(b) - 1 - tail]:
        tail += 1
    e.update(head=head, insert=s[head:len(s) - tail].hex(), tail=tail)
    assert b[:head] + bytes.fromhex(e["insert"]) + b[len(b) - tail:] == s
    return e


def main():
    cases = base_cases()
    import PIL
    by = {e["name"]: base64.b64decode(e["stream"]) for e in cases}
    damaged = [as_edit(e, by) for e in damaged_cases(cases)]
    cases += long_wide_cases()  # (behind everything older: those entries stay as they are)
    damaged += long_damaged_cases(cases)
    doc = dict(pillow=PIL.__version__, libjpeg_turbo=features.version("libjpeg_turbo"),
               cases=cases, damaged=damaged, forged=forged_cases())
    path = os.path.join(ROOT, "tests", "golden", "dng_jpeg_ref.json")
    with open(path, "w") as f:  # (an entry a line)
        f.write("{")
        for key in sorted(doc):
            if isinstance(doc[key], list):
                body = "[\n" + ",\n".join(json.dumps(e, sort_keys=True) for e in doc[key]) + "\n]"
            else:
                body = json.dumps(doc[key])
            f.write("%s\n%s: %s" % ("" if key == sorted(doc)[0] else ",", json.dumps(key), body))
        f.write("\n}\n")
    # (a smooth tile: the benchmark only repeats it where it cannot encode a frame of its own)
    y, x = np.mgrid[0:256, 0:256]
    px = np.stack([128 + 60 * np.sin(x / 37.0) * np.cos(y / 53.0) + d for d in (20, -10, -30)], axis=-1)
    px = px + np.random.default_rng(7).normal(0, 1.0, px.shape)
    s = encode(Image.fromarray(np.clip(px, 0, 255).astype(np.uint8), "RGB"), quality=90, subsampling=2)
    tile = entry("bench_420_256x256", s, 3)
    with open(os.path.join(ROOT, "tests", "golden", "dng_jpeg_bench_tile.json"), "w") as f:
        json.dump(tile, f, sort_keys=True)
        f.write("\n")
    assert os.path.getsize(path) < 160000
    print(path, os.path.getsize(path), "bytes;", len(cases), "cases,", len(doc["damaged"]), "damaged;",
          "bench tile", len(s), "bytes")
    for e in doc["forged"]:
        print(e["name"], "pillow:", e["sha256"] and e["sha256"][:12], "model status", e["model_status"],
              e.get("model_matches"))


if __name__ == "__main__":
    main()
