"""TEST INFRASTRUCTURE: Samsung SRW files of compression 32770 (SamsungV0Decompressor,
decompressors/SamsungV0Decompressor.cpp:44-204, reached from decoders/SrwDecoder.cpp:85-106).

  BitWriter        BitStreamerMSB32 rows: little-endian 32-bit words filled MSB first
  encode_row       a random valid row: lengths stay in 0..16, dir = 1 only where it is allowed
  random_rows      the rows of a frame (+ statistics of what the encoder drew)
  planned_dirs     the upward blocks of every row from row 2 on, planned instead of drawn
  srw_v0_file      the container: one strip, tag 40976 -> a table of `height` row offsets
  parse_row        one row's headers and adjustments, or the status of its first exception
  model_decode     the whole decode: statuses per row, and the image when every row is fine
  overreads        the closed-form over-read rule of a row's requests

The model is the decomposition the device uses (include/rsx.h section 3k): a parse per row that
depends on nothing but the row's bytes, then a reconstruction down the rows."""
import numpy as np

import rawfiles as R

OK, INVALID_ARG, IO, INPUT_OVERFLOW, UNSUPPORTED, VALUE_RANGE = 0, 1, 2, 5, 7, 10
MIN_W, MAX_W, MAX_H = 16, 5546, 3714
SLICE_OFFSETS = 40976


class BitWriter:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, v, n):
        if n:
            self.acc = (self.acc << n) | (int(v) & ((1 << n) - 1))
            self.n += n

    def bytes(self):
        """whole 32-bit words, each stored little-endian"""
        pad = -self.n % 32
        raw = (self.acc << pad).to_bytes((self.n + pad) // 8, "big")
        return np.frombuffer(raw, ">u4").astype("<u4").tobytes()


def new_stats():
    return {"headers": 0, "ops": [0, 0, 0, 0], "eligible": 0, "up": 0, "lens": set()}


def encode_row(rng, width, row, p_up=0.3, stats=None, plant=False, op_weights=(1, 1, 1, 1), dirs=None):
    """One random valid row.  Every op that keeps its length in 0..16 is drawn with the given
    weights; `plant` forces a length through 15 -> 16 and one to 0 in the first two blocks.
    dirs: a bool per block that says which blocks are upward, instead of the draw with p_up
    (an upward block in row 0 or 1 or in the last block is an error: no valid row has one)."""
    st = stats if stats is not None else new_stats()
    w = BitWriter()
    lens = [7] * 4 if row < 2 else [4] * 4
    nblk = (width + 15) // 16
    if dirs is not None and len(dirs) != nblk:
        raise ValueError("dirs: %d entries for %d blocks" % (len(dirs), nblk))
    for b in range(nblk):
        can_up = row >= 2 and 16 * b + 16 < width
        if dirs is not None:
            up = bool(dirs[b])
            if up and not can_up:
                raise ValueError("block %d of row %d cannot be upward" % (b, row))
        else:
            up = bool(can_up and rng.random() < p_up)
        st["eligible"] += can_up
        st["up"] += up
        ops, vals = [], []
        for i in range(4):
            valid = [0, 3] + ([1] if lens[i] < 16 else []) + ([2] if lens[i] > 0 else [])
            pw = np.array([op_weights[o] for o in valid], float)
            op = int(rng.choice(valid, p=pw / pw.sum()))
            val = int(rng.integers(0, 16))
            if plant and b == 0 and i < 2:
                op, val = 3, (15, 0)[i]
            if plant and b == 1 and i == 0 and nblk > 1:
                op = 1
            if op == 3:
                lens[i] = val
                vals.append(val)
            elif op == 2:
                lens[i] -= 1
            elif op == 1:
                lens[i] += 1
            ops.append(op)
            st["ops"][op] += 1
            st["lens"].add(lens[i])
        st["headers"] += 1
        w.put(up, 1)
        for op in ops:
            w.put(op, 2)
        for v in vals:
            w.put(v, 4)
        fields = rng.integers(0, 1 << 16, size=16)
        for k in range(16):  # 8 even pixels (len 0, 0, 0, 0, 1, 1, 1, 1), then 8 odd ones (2.., 3..)
            w.put(fields[k], lens[k >> 2])
    return w.bytes()


def random_rows(rng, width, height, p_up=0.3, stats=None, plant=False, op_weights=(1, 1, 1, 1),
                dirs=None):
    """dirs: {row: a bool per block} for the rows whose upward blocks are planned, not drawn"""
    return [encode_row(rng, width, y, p_up, stats, plant and y == 0, op_weights,
                       None if dirs is None else dirs.get(y))
            for y in range(height)]


def planned_dirs(width, height, plan):
    """plan {row: upward blocks} -> the `dirs` of random_rows for a frame in which every row from
    row 2 on is planned: the rows the plan does not name have no upward block"""
    nblk = (width + 15) // 16
    return {y: [b in plan.get(y, ()) for b in range(nblk)] for y in range(2, height)}


def tiled_rows(rng, width, height, p_up=0.3, pool=24, op_weights=(1, 1, 1, 1)):
    """A large frame from a small pool of encoded rows (a row's bytes do not depend on its
    number past row 1; the decoded image still does, through the upward blocks)."""
    head = [encode_row(rng, width, y, p_up, op_weights=op_weights) for y in range(min(2, height))]
    body = [encode_row(rng, width, 2, p_up, op_weights=op_weights) for _ in range(pool)]
    pick = rng.integers(0, pool, size=max(0, height - 2))
    return head + [body[int(k)] for k in pick]


def strip_and_offsets(rows):
    offs, pos = [], 0
    for r in rows:
        offs.append(pos)
        pos += len(r)
    return np.frombuffer(b"".join(rows), np.uint8), offs


def srw_v0_file(width, height, strip, offsets, bits=12):
    """rawfiles.srw_v1_file with compression 32770 and tag 40976 (LONG, count 1): the file offset
    of `len(offsets)` little-endian u32 row offsets, appended behind the TIFF structure."""
    def build(table_pos):
        raw = R.Ifd()
        raw.add(R.IMAGEWIDTH, R.LONG, width).add(R.IMAGELENGTH, R.LONG, height)
        raw.add(R.BITSPERSAMPLE, R.SHORT, bits)
        raw.add(R.COMPRESSION, R.LONG, 32770)
        raw.add(SLICE_OFFSETS, R.LONG, table_pos)
        raw.add_blobs(R.STRIPOFFSETS, R.STRIPBYTECOUNTS, [strip])
        root = R.Ifd()
        root.add(R.MAKE, R.ASCII, "SAMSUNG").add(R.MODEL, R.ASCII, "RSX")
        root.add_sub(raw)
        return R.tiff_file(root)

    body = build(len(build(0)))
    table = np.asarray(offsets, dtype="<u4").view(np.uint8)
    return np.concatenate([body, table])


def rows_file(width, height, rows):
    strip, offs = strip_and_offsets(rows)
    return srw_v0_file(width, height, strip, offs)


# ---- the model ------------------------------------------------------------------------------
def overreads(requests, size):
    """requests: (c, n), c the bits consumed before a request of n bits.  The row throws "Buffer
    overflow read in BitStreamer" iff 4 (k - 1) > size + 8, k = max ceil((c + n) / 32)."""
    k = max(-(-(c + n) // 32) for c, n in requests)
    return 4 * (k - 1) > size + 8


def _over(end, size):
    return 4 * ((end + 31) // 32 - 1) > size + 8


def parse_row(data, row, width, requests=None):
    """-> (status, dirs, adj): dirs[nblk] bool, adj[nblk, 16] in stream order turned into column
    order (adj[b, c] belongs to column 16 b + c).  The status is that of the first exception the
    reference would throw, in stream order; dirs and adj are None then."""
    data = bytes(data)
    size = len(data)
    if size < 4:
        return IO, None, None  # "Bit stream size is smaller than MaxProcessBytes"
    nblk = (width + 15) // 16
    total = 32 * ((nblk * 281 + 31) // 32 + 2)
    padded = data + bytes(max(0, total // 8 - size) + (-size % 4))
    big = int.from_bytes(np.frombuffer(padded[:len(padded) // 4 * 4], "<u4").astype(">u4").tobytes(), "big")
    nbits = len(padded) // 4 * 32

    def get(pos, n):
        return (big >> (nbits - pos - n)) & ((1 << n) - 1)

    lens = [7] * 4 if row < 2 else [4] * 4
    dirs = np.zeros(nblk, bool)
    adj = np.zeros((nblk, 16), np.int64)
    pos = 0
    for b in range(nblk):
        if requests is not None:
            requests.append((pos, 32))
        if _over(pos + 32, size):  # fill(32)
            return INPUT_OVERFLOW, None, None
        up = get(pos, 1)
        ops = [get(pos + 1 + 2 * i, 2) for i in range(4)]
        q = pos + 9
        for i in range(4):
            if ops[i] == 3:
                if requests is not None:
                    requests.append((q, 4))
                if _over(q + 4, size):
                    return INPUT_OVERFLOW, None, None
                lens[i] = get(q, 4)
                q += 4
            elif ops[i] == 2:
                lens[i] -= 1
            elif ops[i] == 1:
                lens[i] += 1
            if lens[i] < 0 or lens[i] > 16:
                return VALUE_RANGE, None, None
        if up and (row < 2 or 16 * b + 16 >= width):
            return INVALID_ARG, None, None
        dirs[b] = bool(up)
        for k in range(16):
            n = lens[k >> 2]
            if n == 0:
                continue
            if requests is not None:
                requests.append((q, n))
            if _over(q + n, size):
                return INPUT_OVERFLOW, None, None
            v = get(q, n)
            q += n
            c = 2 * k if k < 8 else 2 * (k - 8) + 1
            adj[b, c] = v - (1 << n) if v >> (n - 1) else v  # signExtend
        pos = q
    return OK, dirs, adj


def reconstruct(width, height, parsed):
    """parsed[y] = (dirs, adj) -> the image before the swap, columns padded to whole blocks"""
    nblk = (width + 15) // 16
    out = np.zeros((height, nblk, 16), np.int64)
    ar = np.arange(nblk)
    zero = np.zeros((nblk, 16), np.int64)
    for y in range(height):
        dirs, adj = parsed[y]
        idx = np.maximum.accumulate(np.where(dirs, ar, -1))
        for p in (0, 1):
            above = out[y - 1 - p] if y - 1 - p >= 0 else zero  # even: one row up, odd: two
            x = adj[:, 14 + p]
            ends_up = above[:, 14 + p] + x  # the last pixel of an upward block
            cs = np.cumsum(x)
            base = np.where(idx >= 0, ends_up[idx] - cs[idx], 128)
            ends = cs + base  # the last pixel of its parity in every block
            pred = np.concatenate([[128], ends[:-1]])  # out(row, col - 2) resp. out(row, col - 1)
            left = pred[:, None] + adj[:, p::2]  # all eight share the one predictor
            up = above[:, p::2] + adj[:, p::2]
            out[y, :, p::2] = np.where(dirs[:, None], up, left) & 0xFFFF
    return out.reshape(height, nblk * 16)


def swap(img):
    """for even row < h - 1 and even col < w - 1: out(row, col + 1) <-> out(row + 1, col)"""
    h, w = img.shape
    img = img.copy()
    a = img[0:h - 1:2, 1::2].copy()
    img[0:h - 1:2, 1::2] = img[1::2, 0:w - 1:2]
    img[1::2, 0:w - 1:2] = a
    return img


def model_decode(width, height, rows, cache=None):
    """rows: the bytes of every row.  -> (status, row statuses, image or None); the status is the
    lowest failing row's.  `cache` (a dict) shares the parse of repeated rows."""
    statuses, parsed = [], []
    for y, r in enumerate(rows):
        key = (bytes(r), y < 2)
        hit = cache.get(key) if cache is not None else None
        if hit is None:
            hit = parse_row(r, y, width)
            if cache is not None:
                cache[key] = hit
        statuses.append(hit[0])
        parsed.append(hit[1:])
    bad = [s for s in statuses if s != OK]
    if bad:
        return bad[0], statuses, None
    pre = reconstruct(width, height, parsed)[:, :width].astype(np.uint16)
    return OK, statuses, swap(pre)
