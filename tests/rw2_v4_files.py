"""Panasonic RW2 V4 test material (include/rsx.h section 3l): a packet writer, stream builders
for both values of section_split_offset, the two kinds of RW2 file Rw2Decoder builds a
PanasonicV4Decompressor for, and a numpy model of the device decode with its zero-pixel list.

A packet is 16 bytes = one 128-bit little-endian number read from bit 128 down, and holds 14
pixels of one row.  In front of the pixels 2, 5, 8 and 11 stands a 2-bit scale; every pixel has
an 8-bit field; every column parity has ONE 4-bit field, behind the parity's first non-zero
8-bit field or, where all were zero, behind its last pixel (12 resp. 13).  That makes 128 bits
whatever the data, and the codec cannot fail, so any bytes are a valid stream.
The input is cut into blocks of 0x4000 bytes = 1024 packets; with split 0x1FF8 a block's bytes
[0x1FF8, 0x4000) are read first (the V5 rotation of rw2_files.py), with split 0 the blocks are
read as they are and the last one may be partial."""
import numpy as np

import rawfiles as R
from rw2_files import BLOCK, SPLIT, PACKETS_PER_BLOCK, rw2_file, v5_rotate, v5_unrotate

N = 14                       # PixelsPerPacket
SPLITS = (0, SPLIT)          # old-style files, PANASONIC_RAWFORMAT 4
OK, INVALID_ARG, IO, UNSUPPORTED = 0, 1, 2, 7
KINDS = ("uniform", "half", "sparse")
STATS = ("sh0", "sh1", "sh2", "sh4", "j0", "neg_mask", "sh4_mask", "lead_zero", "late4")


def consumed(split, w, h):
    """the bytes the constructor's peekStream takes (bufSize)"""
    total = w * h // N * 16
    return total if split == 0 else -(-total // BLOCK) * BLOCK


# ---- packet writer --------------------------------------------------------------------------
def pack_v4(f, scales=(0, 0, 0, 0), g=(0, 0)):
    """One packet from its field values: f = the 14 8-bit fields, scales = the 2-bit fields in
    front of the pixels 2, 5, 8, 11, g = the 4-bit field of the even and of the odd columns.
    The 4-bit fields land where processPixelPacket reads them."""
    assert len(f) == N and len(scales) == 4 and len(g) == 2
    v, pos, done = 0, 128, [False, False]

    def put(x, n):
        nonlocal v, pos
        assert 0 <= int(x) < 1 << n, (x, n)
        pos -= n
        v |= int(x) << pos

    for p in range(N):
        c = p & 1
        if p % 3 == 2:
            put(scales[p // 3], 2)
        put(f[p], 8)
        if not done[c] and (f[p] != 0 or p > 11):
            put(g[c], 4)
            done[c] = True
    assert pos == 0 and done == [True, True]
    return np.frombuffer(v.to_bytes(16, "little"), np.uint8)


# ---- streams --------------------------------------------------------------------------------
def stream_from_packets(split, packets):
    """(k, 16) uint8 packets -> the decompressor's input: split 0 the packets as they are, split
    0x1FF8 padded to whole blocks and rotated"""
    p = np.asarray(packets, np.uint8).reshape(-1, 16)
    if split == 0:
        return p.reshape(-1).copy()
    blocks = -(-len(p) // PACKETS_PER_BLOCK)
    plain = np.zeros(blocks * BLOCK, np.uint8)
    plain[:p.size] = p.reshape(-1)
    return v5_rotate(plain)


def packet_offsets(split, p):
    """the 16 positions in the stream of the bytes of packet p"""
    if split == 0:
        return 16 * p + np.arange(16)
    return (p // PACKETS_PER_BLOCK) * BLOCK + (16 * (p % PACKETS_PER_BLOCK) + SPLIT + np.arange(16)) % BLOCK


def planted_packets():
    """packets for the branches random bytes seldom reach: all fields zero (14 zero pixels), only
    the late 4-bit fields set, a zero lead then values, every scale, and the largest climb"""
    out = [pack_v4([0] * N), pack_v4([0] * N, g=(5, 9)), pack_v4([0] * N, (3, 3, 3, 3), (15, 0))]
    out.append(pack_v4([0, 0, 0, 7, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], g=(3, 12)))
    out.append(pack_v4([0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0], g=(0, 1)))
    for s in range(4):
        out.append(pack_v4([255, 255] + [255] * 12, (s, s, s, s), (15, 15)))
        out.append(pack_v4([1, 1] + [1, 0] * 6, (s, 3 - s, s, 3), (0, 0)))
        out.append(pack_v4([16, 200, 0, 1, 128, 127, 129, 1, 0, 255, 3, 0, 9, 128], (s, 0, 3, s), (7, 8)))
    return out


def random_stream(rng, split, w, h, kind="uniform"):
    """Input bytes of exactly the consumed size.  uniform: any bytes; half: every byte zeroed
    with probability 1/2; sparse: 7 of 8 bytes zero, and the planted packets at random places
    (the late 4-bit field, leading zero fields and whole packets of zero pixels)"""
    n = consumed(split, w, h)
    a = rng.integers(0, 256, size=n, dtype=np.uint8)
    if kind == "half":
        a[rng.integers(0, 2, size=n).astype(bool)] = 0
    elif kind == "sparse":
        a[rng.integers(0, 8, size=n) != 0] = 0
        k = w * h // N
        for pk in planted_packets():
            a[packet_offsets(split, int(rng.integers(0, k)))] = pk
    else:
        assert kind == "uniform", kind
    return a


# ---- files ----------------------------------------------------------------------------------
def new_style_file(w, h, data, gap=0):
    """PANASONIC_RAWFORMAT 4 under PANASONIC_STRIPOFFSET (Rw2Decoder.cpp:121-147): split 0x1FF8"""
    return rw2_file(w, h, 4, None, data, gap)


def old_style_file(w, h, data):
    """Rw2Decoder's old-style file (Rw2Decoder.cpp:79-120): no PANASONIC_STRIPOFFSET, one strip
    under STRIPOFFSETS that ends the file.  With fewer than w h 3 / 2 bytes from the strip's
    offset to the end of the file the decoder takes PanasonicV4Decompressor with split 0."""
    assert len(data) < w * h * 3 // 2
    i = R.Ifd()
    i.add(R.MAKE, R.ASCII, "Panasonic").add(R.MODEL, R.ASCII, "DMC-RSX")
    i.add(2, R.SHORT, w).add(3, R.SHORT, h)
    i.add_blobs(R.STRIPOFFSETS, R.STRIPBYTECOUNTS, [np.asarray(data, np.uint8)])
    return R.tiff_file(i, 0)


def v4_file(split, w, h, data, gap=0):
    return old_style_file(w, h, data) if split == 0 else new_style_file(w, h, data, gap)


# ---- the model ------------------------------------------------------------------------------
def _packets(split, w, h, data):
    """(k, 5) uint64: the four dwords of the image's packets in pixel order, and a zero"""
    k = w * h // N
    d = np.asarray(data, np.uint8)[:consumed(split, w, h)]
    if split:
        d = v5_unrotate(d)
    W = np.zeros((k, 5), np.uint64)
    W[:, :4] = d[:16 * k].reshape(k, 16).view("<u4")
    return W


def _take(W, used, n):
    """the n bits below the `used` (per packet) ones from the packet's top"""
    lo = 128 - used - n
    assert (lo >= 0).all()
    idx = (lo >> 5)[:, None]
    v = np.take_along_axis(W, idx, 1)[:, 0] | (np.take_along_axis(W, idx + 1, 1)[:, 0] << np.uint64(32))
    return ((v >> (lo & 31).astype(np.uint64)) & np.uint64((1 << n) - 1)).astype(np.int64)


def decode_packets(W, stats=None):
    """processPixelPacket (PanasonicV4Decompressor.cpp:173-218) on arrays of packets: the
    (k, 14) int64 values of pred"""
    k = len(W)
    used = np.zeros(k, np.int64)
    sh = np.zeros(k, np.int64)
    pred = [np.zeros(k, np.int64), np.zeros(k, np.int64)]
    nonz = [np.zeros(k, np.int64), np.zeros(k, np.int64)]
    out = np.zeros((k, N), np.int64)
    st = dict.fromkeys(STATS, 0)
    for p in range(N):
        c = p & 1
        if p % 3 == 2:
            sh = 4 >> (3 - _take(W, used, 2))
            used = used + 2
            for s in (0, 1, 2, 4):
                st["sh%d" % s] += int((sh == s).sum())
        f = _take(W, used, 8)
        used = used + 8
        seen = nonz[c] != 0
        # nonz[c]: j = f
        t = pred[c] - (0x80 << sh)
        neg, four = t < 0, sh == 4
        t = np.where(neg | four, t & ((1 << sh) - 1), t) + (f << sh)
        later = np.where(f != 0, t, pred[c])
        # else: the 4-bit field for a non-zero f or behind the parity's last pixel
        take = ~seen & ((f != 0) | (p > 11))
        g = np.where(take, _take(W, np.where(take, used, 0), 4), 0)
        used = used + 4 * take
        first = np.where(take, f << 4 | g, pred[c])
        st["j0"] += int((seen & (f == 0)).sum())
        st["neg_mask"] += int((seen & (f != 0) & neg).sum())
        st["sh4_mask"] += int((seen & (f != 0) & four & ~neg).sum())
        st["lead_zero"] += int((~seen & (f == 0) & (p <= 11)).sum())
        st["late4"] += int((take & (f == 0)).sum())
        pred[c] = np.where(seen, later, first)
        nonz[c] = np.where(seen, nonz[c], f)
        out[:, p] = pred[c]
    assert (used == 128).all()  # a packet always takes exactly its bits
    if stats is not None:
        for key, v in st.items():
            stats[key] = stats.get(key, 0) + v
        stats["pixels"] = stats.get("pixels", 0) + k * N
        stats["max_pred"] = max(stats.get("max_pred", 0), int(out.max(initial=0)))
    return out


def model_decode(split, w, h, data, stats=None):
    """The device's decode: the (h, w) uint16 image and the ascending list of row << 16 | col of
    the pixels with pred == 0 (what zero_is_bad collects)"""
    assert w % N == 0 and split in SPLITS
    pred = decode_packets(_packets(split, w, h, data), stats).reshape(h, w)
    assert pred.min(initial=0) >= 0 and pred.max(initial=0) <= 16287
    rows, cols = np.nonzero(pred == 0)
    return pred.astype(np.uint16), ((rows.astype(np.uint32) << 16) | cols.astype(np.uint32))


def zero_list(img):
    """row << 16 | col of an image's zero pixels, ascending"""
    rows, cols = np.nonzero(np.asarray(img) == 0)
    return (rows.astype(np.uint32) << 16) | cols.astype(np.uint32)
