"""Panasonic RW2 V5 / V6 / V7 test material (include/rsx.h section 3j): packet writers, an RW2
file writer and a numpy model of the device decode.

Every packet is 16 bytes, read as one 128-bit little-endian number (bit 0 = the LSB of byte 0);
packet p holds the pixels [p n, (p + 1) n) in row-major order.
  V7/14 (n 9), V5/14 (n 9), V5/12 (n 10): pixel i = bits [bps i, bps i + bps).
  V5: blocks of 0x4000 bytes = 1024 packets; a block's bytes [0x1FF8, 0x4000) are read first.
  V6/14 (n 11), V6/12 (n 14): from bit 128 down two first pixels of bps bits, then per three
  pixels a 2-bit scale and three fields of 10 (8) bits.
The codecs are fixed rate and cannot fail, so any bytes are a valid stream."""
import numpy as np

import rawfiles as R

LAYOUTS = [(5, 12), (5, 14), (6, 12), (6, 14), (7, 14)]
PIXELS = {(5, 12): 10, (5, 14): 9, (6, 12): 14, (6, 14): 11, (7, 14): 9}
BLOCK, SPLIT, PACKETS_PER_BLOCK = 0x4000, 0x1FF8, 1024
INVALID_ARG, UNSUPPORTED = 1, 7

# tiff/TiffTag.h
PANASONIC_BITSPERSAMPLE, PANASONIC_RAWFORMAT, PANASONIC_STRIPOFFSET = 0x0A, 0x2D, 0x118


def pixels_per_packet(version, bps):
    return PIXELS[(version, bps)]


def consumed(version, bps, w, h):
    """the bytes the constructor's peekStream takes"""
    packets = w * h // PIXELS[(version, bps)]
    return -(-packets // PACKETS_PER_BLOCK) * BLOCK if version == 5 else 16 * packets


# ---- packet writers -------------------------------------------------------------------------
def pack_plain(values, bps):
    """One V5 / V7 packet from its n pixel values"""
    v = 0
    for i, x in enumerate(values):
        v |= (int(x) & ((1 << bps) - 1)) << (bps * i)
    assert v < 1 << 128
    return v.to_bytes(16, "little")


def v6_widths(bps):
    """the widths of pana_cs6_page_decoder's pixelbuffer entries 0, 1, 2, .. (the order
    nextpixel() hands them out: from the packet's top down)"""
    fb, triples = (10, 3) if bps == 14 else (8, 4)
    return [bps, bps] + [2, fb, fb, fb] * triples


def pack_v6(entries, bps):
    """One V6 packet from its pixelbuffer entries: two first pixels, then (scale, f, f, f) per
    triple.  14 bits: 4 unused bits remain at the bottom."""
    widths = v6_widths(bps)
    assert len(entries) == len(widths)
    v, pos = 0, 128
    for e, n in zip(entries, widths):
        pos -= n
        assert 0 <= int(e) < 1 << n, (e, n)
        v |= int(e) << pos
    assert pos == (4 if bps == 14 else 0)
    return v.to_bytes(16, "little")


def v5_rotate(plain):
    """The V5 stream of packets laid out plainly (packet q of block b at 0x4000 b + 16 q,
    whole blocks): every block rotated back so that the decoder's rotation restores it"""
    a = np.asarray(plain, np.uint8).reshape(-1, BLOCK)
    return np.concatenate([a[:, BLOCK - SPLIT:], a[:, :BLOCK - SPLIT]], axis=1).reshape(-1)


def v5_unrotate(data):
    """What ProxyStream::parseBlock builds: [0x1FF8, 0x4000) of each block, then [0, 0x1FF8)"""
    a = np.asarray(data, np.uint8).reshape(-1, BLOCK)
    return np.concatenate([a[:, SPLIT:], a[:, :SPLIT]], axis=1).reshape(-1)


def stream_from_packets(version, packets):
    """(k, 16) uint8 packets -> the decompressor's input (V5: padded to whole blocks, rotated)"""
    p = np.asarray(packets, np.uint8).reshape(-1, 16)
    if version != 5:
        return p.reshape(-1).copy()
    blocks = -(-len(p) // PACKETS_PER_BLOCK)
    plain = np.zeros(blocks * BLOCK, np.uint8)
    plain[:p.size] = p.reshape(-1)
    return v5_rotate(plain)


def random_stream(rng, version, bps, w, h, zero_half=False):
    """Random input bytes of exactly the consumed size; zero_half: every byte zeroed with
    probability 1/2 (V6: reaches the zero-field and the e < 15 branches often)"""
    n = consumed(version, bps, w, h)
    a = rng.integers(0, 256, size=n, dtype=np.uint8)
    if zero_half:
        a[rng.integers(0, 2, size=n).astype(bool)] = 0
    return a


def rw2_file(w, h, version, bps, data, gap=0):
    """Rw2Decoder's new-style file (Rw2Decoder.cpp:65-77, :121-175): one IFD with the sensor
    size in tags 2 and 3, PANASONIC_BITSPERSAMPLE, PANASONIC_RAWFORMAT and the strip under
    PANASONIC_STRIPOFFSET.  The decompressor gets the file from the strip's offset to its end:
    `gap` bytes trail the data.  (The byte counts land in tag 0x117, which nobody reads.)"""
    i = R.Ifd()
    i.add(R.MAKE, R.ASCII, "Panasonic").add(R.MODEL, R.ASCII, "DC-RSX")
    i.add(2, R.SHORT, w).add(3, R.SHORT, h)
    if bps is not None:
        i.add(PANASONIC_BITSPERSAMPLE, R.SHORT, bps)
    i.add(PANASONIC_RAWFORMAT, R.SHORT, version)
    i.add_blobs(PANASONIC_STRIPOFFSET, 0x117, [np.asarray(data, np.uint8)])
    return R.tiff_file(i, gap)


# ---- the model ------------------------------------------------------------------------------
def _packets(version, bps, w, h, data):
    """(k, 4) uint64 dwords of the image's packets, in pixel order"""
    n = PIXELS[(version, bps)]
    k = w * h // n
    d = np.asarray(data, np.uint8)[:consumed(version, bps, w, h)]
    if version == 5:
        d = v5_unrotate(d)
    return d[:16 * k].reshape(k, 16).view("<u4").astype(np.uint64)


def _bits(W, pos, n):
    lo, s = pos >> 5, pos & 31
    v = W[:, lo] >> np.uint64(s)
    if s + n > 32:
        v = v | (W[:, lo + 1] << np.uint64(32 - s))
    return (v & np.uint64((1 << n) - 1)).astype(np.int64)


def v6_entries(W, bps):
    """pixelbuffer entries 0, 1, 2, .. of every packet"""
    out, pos = [], 128
    for n in v6_widths(bps):
        pos -= n
        out.append(_bits(W, pos, n))
    return out


def v6_decode(entries, bps, stats=None):
    """PanasonicV6Decompressor::decompressBlock (:185-219) on arrays of packets, with its
    16-bit truncations and the `else` of its last test kept as they are written"""
    n = PIXELS[(6, bps)]
    zero, cmp_, spixcmp, mask = (0x200, 0x2000, 0xFFFF, 0x3FFF) if bps == 14 else \
        (0x80, 0x800, 0x3FFF, 0xFFF)
    k = len(entries[0])
    oddeven = [np.zeros(k, np.int64), np.zeros(k, np.int64)]
    nonzero = [np.zeros(k, np.int64), np.zeros(k, np.int64)]
    pmul = np.zeros(k, np.int64)
    pixel_base = np.zeros(k, np.int64)
    out = np.zeros((k, n), np.int64)
    nxt = 0
    for pix in range(n):
        if pix % 3 == 2:
            base = entries[nxt].copy()
            nxt += 1
            base[base == 3] = 4
            pixel_base = zero << base
            pmul = 1 << base
        e = entries[nxt].copy()
        nxt += 1
        p = pix % 2
        later = oddeven[p] != 0
        e_l = (e * pmul) & 0xFFFF
        add = (pixel_base < cmp_) & (nonzero[p] > pixel_base)
        e_l = np.where(add, (e_l + nonzero[p] - pixel_base) & 0xFFFF, e_l)
        e_f = np.where(e != 0, e, nonzero[p])
        oddeven[p] = np.where(later, oddeven[p], e)
        enew = np.where(later, e_l, e_f)
        nonzero[p] = np.where(later | (e != 0), enew, nonzero[p])
        spix = (enew - 0xF) & 0xFFFFFFFF
        ok = spix <= spixcmp
        # the else: (int)(epixel + 0x7ffffff1) >> 31, 0 while the sum stays below 2^31
        neg = (enew + 0x7FFFFFF1) >= (1 << 31)
        other = np.where(neg, 0xFFFF, 0) & mask
        out[:, pix] = np.where(ok, spix & spixcmp, other)
        if stats is not None:
            stats["first_zero"] = stats.get("first_zero", 0) + int((~later & (e == 0)).sum())
            stats["below_15"] = stats.get("below_15", 0) + int((~ok & ~neg).sum())
            stats["else_large"] = stats.get("else_large", 0) + int((~ok & neg).sum())
            stats["pixels"] = stats.get("pixels", 0) + k
    return out


def model_decode(version, bps, w, h, data, stats=None):
    """The device's decode: the (h, w) uint16 image"""
    n = PIXELS[(version, bps)]
    assert w % n == 0
    W = _packets(version, bps, w, h, data)
    if version == 6:
        px = v6_decode(v6_entries(W, bps), bps, stats)
    else:
        px = np.stack([_bits(W, bps * i, bps) for i in range(n)], axis=1)
    return px.astype(np.uint16).reshape(h, w)
