"""ctypes mirror of include/rsx.h (the C-ABI of the decompression core).

Only plain C types cross the boundary.  These structures are shared by the
product binding (rawspeed_amd/capi.py) and by the test-only bindings of the
oracle (tests/oracle_lib.py), which use the same descriptors.
"""
import ctypes as C

import numpy as np

RSX_ABI_VERSION = 4

# rsx_status
RSX_OK = 0
RSX_ERR_INVALID_ARG = 1
RSX_ERR_IO = 2
RSX_ERR_BAD_HUFFMAN_CODE = 3
RSX_ERR_RESTART_MARKER = 4
RSX_ERR_INPUT_OVERFLOW = 5
RSX_ERR_DEVICE = 6
RSX_ERR_UNSUPPORTED = 7
RSX_ERR_NOMEM = 8
RSX_ERR_TILE_ERRORS = 9
RSX_ERR_VALUE_RANGE = 10
RSX_ERR_VALUE_RANGE = 10

STATUS_NAMES = {
    0: "RSX_OK", 1: "RSX_ERR_INVALID_ARG", 2: "RSX_ERR_IO",
    3: "RSX_ERR_BAD_HUFFMAN_CODE", 4: "RSX_ERR_RESTART_MARKER",
    5: "RSX_ERR_INPUT_OVERFLOW", 6: "RSX_ERR_DEVICE", 7: "RSX_ERR_UNSUPPORTED",
    8: "RSX_ERR_NOMEM", 9: "RSX_ERR_TILE_ERRORS",
    10: "RSX_ERR_VALUE_RANGE",
}

# rsx_bit_order == rawspeed::BitOrder (bitstreams/BitStreams.h:27-35)
ORDER_LSB, ORDER_MSB, ORDER_MSB16, ORDER_MSB32, ORDER_JPEG = range(5)

RSX_MAX_CODE_VALUES = 162
RSX_MAX_COMPONENTS = 4


class Image(C.Structure):
    _fields_ = [("data", C.c_void_p), ("pitch_bytes", C.c_uint32),
                ("dim_x", C.c_int32), ("dim_y", C.c_int32),
                ("cpp", C.c_int32), ("is_cfa", C.c_int32)]


class UnpackDesc(C.Structure):
    _fields_ = [("crop_x", C.c_int32), ("crop_y", C.c_int32),
                ("crop_w", C.c_int32), ("crop_h", C.c_int32),
                ("input_pitch_bytes", C.c_int32),
                ("bits_per_pixel", C.c_int32), ("bit_order", C.c_int32)]


(UNPACK_8BIT_RAW, UNPACK_12BIT_WITH_CONTROL, UNPACK_12BIT_UNPACKED_LEFT_ALIGNED,
 UNPACK_8BIT_LOOKUP) = range(4)


class UnpackVariantDesc(C.Structure):
    _fields_ = [("variant", C.c_int32), ("big_endian", C.c_int32),
                ("w", C.c_int32), ("h", C.c_int32), ("lut", C.c_uint16 * 256)]

    def set_lut(self, lut):
        for i, v in enumerate(lut):
            self.lut[i] = int(v)
        return self


class HuffTable(C.Structure):
    _fields_ = [("n_codes_per_length", C.c_uint8 * 16),
                ("code_values", C.c_uint8 * RSX_MAX_CODE_VALUES),
                ("n_code_values", C.c_uint8), ("fix_dng_bug16", C.c_uint8)]

    @classmethod
    def make(cls, counts, values, fix_dng_bug16=False):
        t = cls()
        assert len(counts) == 16 and len(values) <= RSX_MAX_CODE_VALUES
        for i, c in enumerate(counts):
            t.n_codes_per_length[i] = c
        for i, v in enumerate(values):
            t.code_values[i] = v
        t.n_code_values = len(values)
        t.fix_dng_bug16 = 1 if fix_dng_bug16 else 0
        return t


class LJpegDesc(C.Structure):
    _fields_ = [("tile_x", C.c_int32), ("tile_y", C.c_int32),
                ("tile_w", C.c_int32), ("tile_h", C.c_int32),
                ("mcu_w", C.c_int32), ("mcu_h", C.c_int32),
                ("frame_w", C.c_int32), ("frame_h", C.c_int32),
                ("n_comp", C.c_int32),
                ("rows_per_restart_interval", C.c_int32),
                ("init_pred", C.c_uint16 * RSX_MAX_COMPONENTS),
                ("table_index", C.c_uint8 * RSX_MAX_COMPONENTS),
                ("n_tables", C.c_int32),
                ("tables", HuffTable * RSX_MAX_COMPONENTS)]


class Cr2Desc(C.Structure):
    _fields_ = [("n_comp", C.c_int32), ("x_s_f", C.c_int32),
                ("y_s_f", C.c_int32),
                ("frame_w", C.c_int32), ("frame_h", C.c_int32),
                ("num_slices", C.c_int32), ("slice_width", C.c_int32),
                ("last_slice_width", C.c_int32),
                ("init_pred", C.c_uint16 * RSX_MAX_COMPONENTS),
                ("table_index", C.c_uint8 * RSX_MAX_COMPONENTS),
                ("n_tables", C.c_int32),
                ("tables", HuffTable * RSX_MAX_COMPONENTS)]


class NikonDesc(C.Structure):
    _fields_ = [("bits_ps", C.c_int32), ("split", C.c_int32),
                ("p_up", (C.c_int32 * 2) * 2),
                ("uncorrected_raw_values", C.c_int32), ("curve_size", C.c_int32),
                ("curve", C.c_void_p), ("tables", HuffTable * 2)]

    def set_curve(self, curve):
        """Keeps the numpy array alive on the descriptor."""
        self._curve = np.ascontiguousarray(curve, dtype=np.uint16)
        self.curve = self._curve.ctypes.data
        self.curve_size = self._curve.size


class PentaxDesc(C.Structure):
    _fields_ = [("table", HuffTable)]


class PentaxJob(C.Structure):
    _fields_ = [("desc", PentaxDesc), ("in_offset", C.c_uint64),
                ("in_bytes", C.c_uint64), ("img_offset", C.c_uint64),
                ("img", Image)]


class SamsungV1Desc(C.Structure):
    _fields_ = [("bits", C.c_int32), ("n_entries", C.c_int32),
                ("enc_len", C.c_uint8 * 32), ("diff_len", C.c_uint8 * 32)]

    @classmethod
    def make(cls, tab, bits=12):
        d = cls()
        d.bits, d.n_entries = bits, len(tab)
        for i, (e, l) in enumerate(tab):
            d.enc_len[i], d.diff_len[i] = e, l
        return d


class SamsungV1Job(C.Structure):
    _fields_ = [("desc", SamsungV1Desc), ("in_offset", C.c_uint64),
                ("in_bytes", C.c_uint64), ("img_offset", C.c_uint64),
                ("img", Image)]


class SamsungV2Desc(C.Structure):
    _fields_ = [("bit_depth", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("optflags", C.c_uint32), ("init_val", C.c_uint32)]

    @classmethod
    def from_header(cls, hdr):
        """The fields SamsungV2Decompressor's constructor reads from the 16-byte header
        (SamsungV2Decompressor.cpp:106-132; BitStreamerMSB32: little-endian 32-bit words,
        most significant bit first).  Returns (desc, raw optflags)."""
        w = [int.from_bytes(bytes(hdr[4 * k:4 * k + 4]), "little") for k in range(4)]
        bits = "".join(format(x, "032b") for x in w)
        pos = [0]

        def get(n):
            v = int(bits[pos[0]:pos[0] + n], 2)
            pos[0] += n
            return v
        d = cls()
        get(16), get(4)
        d.bit_depth = get(4) + 1
        get(4), get(4)
        d.width, d.height = get(16), get(16)
        get(16), get(4)
        flags = get(4)
        get(8), get(8), get(8), get(2)
        d.init_val = get(14)
        d.optflags = flags
        return d, flags


class SamsungV2Job(C.Structure):
    _fields_ = [("desc", SamsungV2Desc), ("in_offset", C.c_uint64),
                ("in_bytes", C.c_uint64), ("img_offset", C.c_uint64),
                ("img", Image)]


class SonyArw1Job(C.Structure):
    _fields_ = [("in_offset", C.c_uint64), ("in_bytes", C.c_uint64),
                ("img_offset", C.c_uint64), ("img", Image)]


class PhaseOneStrip(C.Structure):
    _fields_ = [("n", C.c_uint32), ("reserved", C.c_uint32), ("offset", C.c_uint64),
                ("bytes", C.c_uint64)]


class PhaseOneJob(C.Structure):
    _fields_ = [("strips", C.POINTER(PhaseOneStrip)), ("n_strips", C.c_int32),
                ("reserved", C.c_int32), ("in_offset", C.c_uint64), ("in_bytes", C.c_uint64),
                ("img_offset", C.c_uint64), ("img", Image)]


ARW2_TABLE_NONE, ARW2_TABLE_PLAIN, ARW2_TABLE_DITHER = 0, 1, 2


class SonyArw2Desc(C.Structure):
    _fields_ = [("table_mode", C.c_int32), ("reserved", C.c_int32),
                ("table", C.POINTER(C.c_uint16))]


class SonyArw2Job(C.Structure):
    _fields_ = [("desc", SonyArw2Desc), ("in_offset", C.c_uint64), ("in_bytes", C.c_uint64),
                ("img_offset", C.c_uint64), ("img", Image)]


def sony_arw2_desc(mode, table=None):
    """(desc, keep-alive array): `table` as TableLookUp holds it (uint16; None for NONE)"""
    d = SonyArw2Desc()
    d.table_mode = mode
    arr = None
    if table is not None:
        arr = np.ascontiguousarray(table, dtype=np.uint16)
        d.table = arr.ctypes.data_as(C.POINTER(C.c_uint16))
    return d, arr


class NikonSnefDesc(C.Structure):
    _fields_ = [("inv_wb_r", C.c_int32), ("inv_wb_b", C.c_int32),
                ("table", C.POINTER(C.c_uint16))]


class NikonSnefJob(C.Structure):
    _fields_ = [("desc", NikonSnefDesc), ("in_offset", C.c_uint64), ("in_bytes", C.c_uint64),
                ("img_offset", C.c_uint64), ("img", Image)]


def nikon_snef_desc(inv_wb_r, inv_wb_b, table=None):
    """(desc, keep-alive array): `table` as the dithering TableLookUp holds it (uint16, 8192
    entries read; None leaves the pointer NULL)"""
    d = NikonSnefDesc()
    d.inv_wb_r, d.inv_wb_b = inv_wb_r, inv_wb_b
    arr = None
    if table is not None:
        arr = np.ascontiguousarray(table, dtype=np.uint16)
        d.table = arr.ctypes.data_as(C.POINTER(C.c_uint16))
    return d, arr


class Vc5Code(C.Structure):
    _fields_ = [("bits", C.c_uint32), ("size", C.c_uint8), ("count", C.c_uint16),
                ("value", C.c_int16)]


class Vc5Band(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("bytes", C.c_uint32), ("quant", C.c_int16),
                ("precision", C.c_uint16)]


class Vc5Desc(C.Structure):
    _fields_ = [("phase", C.c_int32), ("log_table", C.POINTER(C.c_uint16)),
                ("codes", C.POINTER(Vc5Code)), ("n_codes", C.c_int32),
                ("bands", (Vc5Band * 10) * 4), ("prescale", (C.c_uint8 * 3) * 4)]


class Vc5Job(C.Structure):
    _fields_ = [("desc", Vc5Desc), ("in_offset", C.c_uint64), ("in_bytes", C.c_uint64),
                ("img_offset", C.c_uint64), ("img", Image)]


def vc5_desc(phase, log_table, codes, bands, prescale):
    """(desc, keep-alive objects).  log_table: 4096 uint16 (None leaves the pointer NULL); codes:
    rows (size, bits, count, value) (None: NULL); bands[c][s] = (offset, bytes, quant, precision);
    prescale[c][level - 1]"""
    d = Vc5Desc()
    d.phase = phase
    keep = []
    if log_table is not None:
        t = np.ascontiguousarray(log_table, dtype=np.uint16)
        d.log_table = t.ctypes.data_as(C.POINTER(C.c_uint16))
        keep.append(t)
    if codes is not None:
        arr = (Vc5Code * max(len(codes), 1))()
        for k, (size, bits, count, value) in enumerate(codes):
            arr[k].bits, arr[k].size, arr[k].count, arr[k].value = bits, size, count, value
        d.codes = C.cast(arr, C.POINTER(Vc5Code))
        d.n_codes = len(codes)
        keep.append(arr)
    for c in range(4):
        for s in range(10):
            b = d.bands[c][s]
            b.offset, b.bytes, b.quant, b.precision = bands[c][s]
        for k in range(3):
            d.prescale[c][k] = prescale[c][k]
    return d, keep


RSX_IIQ_MAX_OPS = 16
RSX_IIQ_OP_FLAT_FIELD, RSX_IIQ_OP_QUADRANT_CURVES = 0, 1
RSX_IIQ_OP_SENSOR_DEFECTS = 3  # (2 is not used)


class IiqOp(C.Structure):
    _fields_ = [("kind", C.c_int32), ("chroma", C.c_int32), ("payload", C.c_void_p),
                ("payload_bytes", C.c_uint32), ("black_level", C.c_uint32),
                ("curves", C.c_void_p), ("split_row", C.c_uint32), ("split_col", C.c_uint32)]


class IiqCorr(C.Structure):
    _fields_ = [("n_ops", C.c_int32), ("cfa_w", C.c_int32), ("cfa_h", C.c_int32),
                ("cfa", C.c_uint8 * 64), ("ops", IiqOp * RSX_IIQ_MAX_OPS)]


class IiqCorrectJob(C.Structure):
    _fields_ = [("corr", IiqCorr), ("img_offset", C.c_uint64), ("img", Image)]


def iiq_corr(ops, cfa=None, n_ops=None):
    """(rsx_iiq_corr, keep-alive objects).  ops: ("ff", payload bytes, chroma[, payload_bytes]) or
    ("quad", curves (4, 65536) uint16, split_row, split_col, black_level) or ("defects", payload
    bytes[, payload_bytes]) -- the bytes of entry 0x400 -- or ("kind", k) for an unknown kind; a
    payload or curves of None leaves the pointer NULL.  cfa: (cfa_w, cfa_h,
    colours).  n_ops overrides the count (the list itself holds at most 16)."""
    d = IiqCorr()
    keep = []
    d.n_ops = len(ops) if n_ops is None else n_ops
    if cfa is not None:
        d.cfa_w, d.cfa_h = cfa[0], cfa[1]
        for k, c in enumerate(list(cfa[2])[:64]):
            d.cfa[k] = c
    for k, op in enumerate(ops[:RSX_IIQ_MAX_OPS]):
        o = d.ops[k]
        if op[0] == "ff":
            o.kind, o.chroma = RSX_IIQ_OP_FLAT_FIELD, int(op[2])
            if op[1] is not None:
                a = np.frombuffer(bytes(op[1]), dtype=np.uint8).copy()
                if a.size == 0:
                    a = np.zeros(1, np.uint8)
                o.payload = a.ctypes.data
                o.payload_bytes = len(op[1]) if len(op) < 4 else op[3]
                keep.append(a)
        elif op[0] == "defects":
            o.kind = RSX_IIQ_OP_SENSOR_DEFECTS
            if op[1] is not None:
                a = np.frombuffer(bytes(op[1]), dtype=np.uint8).copy()
                if a.size == 0:
                    a = np.zeros(1, np.uint8)
                o.payload = a.ctypes.data
                o.payload_bytes = len(op[1])
                keep.append(a)
            if len(op) > 2:
                o.payload_bytes = op[2]
        elif op[0] == "quad":
            o.kind = RSX_IIQ_OP_QUADRANT_CURVES
            if op[1] is not None:
                a = np.ascontiguousarray(op[1], dtype=np.uint16).reshape(4 * 65536)
                o.curves = a.ctypes.data
                keep.append(a)
            o.split_row, o.split_col, o.black_level = op[2], op[3], op[4]
        else:
            o.kind = op[1]
    return d, keep


RSX_DNG_POST_MAX_PIXEL_OPS = 16
(DNG_POST_REASON_NONE, DNG_POST_REASON_ROI, DNG_POST_REASON_PLANES, DNG_POST_REASON_PITCH,
 DNG_POST_REASON_DELTA_COUNT, DNG_POST_REASON_DELTA_NOT_FINITE, DNG_POST_REASON_TABLE_SIZE,
 DNG_POST_REASON_POLY_DEGREE, DNG_POST_REASON_UNKNOWN_OPCODE, DNG_POST_REASON_UNSUPPORTED_OPCODE,
 DNG_POST_REASON_INCONSISTENT_LENGTH, DNG_POST_REASON_BAD_POINT, DNG_POST_REASON_SETUP_NOT_U16,
 DNG_POST_REASON_SETUP_CPP, DNG_POST_REASON_SETUP_DELTA_RANGE,
 DNG_POST_REASON_TRIM_EMPTY) = range(16)


class DngPostDesc(C.Structure):
    _fields_ = [("opcodes", C.c_void_p), ("opcodes_bytes", C.c_uint32),
                ("table_count", C.c_uint32), ("table", C.c_void_p), ("is_f32", C.c_int32),
                ("crop_x", C.c_int32), ("crop_y", C.c_int32), ("crop_w", C.c_int32),
                ("crop_h", C.c_int32), ("reserved", C.c_int32)]


class DngPostResult(C.Structure):
    _fields_ = [("list_status", C.c_int32), ("list_reason", C.c_int32),
                ("n_opcodes", C.c_int32), ("n_applied", C.c_int32), ("crop_x", C.c_int32),
                ("crop_y", C.c_int32), ("crop_w", C.c_int32), ("crop_h", C.c_int32),
                ("n_bad", C.c_uint64)]

    def crop(self):
        return (self.crop_x, self.crop_y, self.crop_w, self.crop_h)


class DngPostJob(C.Structure):
    _fields_ = [("desc", DngPostDesc), ("img_offset", C.c_uint64), ("img", Image),
                ("bad_cap", C.c_uint32), ("reserved", C.c_uint32)]


def dng_post_desc(opcodes, table, crop, is_f32=False, opcodes_bytes=None, table_count=None):
    """(rsx_dng_post_desc, keep-alive objects).  opcodes: the OpcodeList1 entry's bytes or None;
    table: the LinearizationTable's values or None; crop: (x, y, w, h) in pixels.  opcodes_bytes /
    table_count override the sizes (a NULL pointer with a size)."""
    d = DngPostDesc()
    keep = []
    if opcodes is not None and len(opcodes):
        a = np.frombuffer(bytes(opcodes), dtype=np.uint8).copy()
        d.opcodes, d.opcodes_bytes = a.ctypes.data, a.size
        keep.append(a)
    if table is not None and len(table):
        t = np.ascontiguousarray(table, dtype=np.uint16)
        d.table, d.table_count = t.ctypes.data, t.size
        keep.append(t)
    if opcodes_bytes is not None:
        d.opcodes_bytes = opcodes_bytes
    if table_count is not None:
        d.table_count = table_count
    d.is_f32 = 1 if is_f32 else 0
    d.crop_x, d.crop_y, d.crop_w, d.crop_h = crop
    return d, keep


class PanasonicDesc(C.Structure):
    _fields_ = [("version", C.c_int32), ("bps", C.c_int32)]


class PanasonicJob(C.Structure):
    _fields_ = [("desc", PanasonicDesc), ("in_offset", C.c_uint64), ("in_bytes", C.c_uint64),
                ("img_offset", C.c_uint64), ("img", Image)]


def panasonic_pixels_per_packet(version, bps):
    """pixels a 16-byte packet holds (include/rsx.h section 3j)"""
    return {(5, 12): 10, (5, 14): 9, (6, 12): 14, (6, 14): 11, (7, 14): 9}[(version, bps)]


def panasonic_consumed(version, bps, dim_x, dim_y):
    """input bytes the decompressor's peekStream takes"""
    packets = dim_x * dim_y // panasonic_pixels_per_packet(version, bps)
    return -(-packets // 1024) * 0x4000 if version == 5 else 16 * packets


class BadPixelsDesc(C.Structure):
    _fields_ = [("positions", C.c_void_p), ("n_positions", C.c_uint32), ("map_pitch", C.c_uint32),
                ("map_in", C.c_void_p), ("map_out", C.c_void_p), ("is_f32", C.c_int32),
                ("reserved", C.c_int32)]


class BadPixelsResult(C.Structure):
    _fields_ = [("n_bad", C.c_uint64), ("n_fixed", C.c_uint64), ("map_made", C.c_int32),
                ("reserved", C.c_int32)]


class BadPixelsJob(C.Structure):
    _fields_ = [("in_offset", C.c_uint64), ("n_positions", C.c_uint32), ("map_pitch", C.c_uint32),
                ("map_in", C.c_void_p), ("is_f32", C.c_int32), ("reserved", C.c_int32),
                ("img_offset", C.c_uint64), ("img", Image)]


def bad_pixels_map_pitch(dim_x):
    """RawImageData::createBadPixelMap's pitch in bytes"""
    return (-(-dim_x // 8) + 15) // 16 * 16


def bad_pixels_desc(positions, dim, map_in=None, is_f32=False, want_map=True, map_pitch=None):
    """(rsx_bad_pixels_desc, keep-alive objects, the map_out array or None).  positions: y << 16 | x
    values; dim: (dim_x, dim_y); map_in: (dim_y, pitch) uint8 or None; map_pitch overrides."""
    d = BadPixelsDesc()
    keep = []
    p = np.ascontiguousarray(positions, dtype=np.uint32)
    if p.size:
        d.positions, d.n_positions = p.ctypes.data, p.size
        keep.append(p)
    d.map_pitch = bad_pixels_map_pitch(dim[0]) if map_pitch is None else map_pitch
    if map_in is not None:
        m = np.ascontiguousarray(map_in, dtype=np.uint8)
        d.map_in = m.ctypes.data
        keep.append(m)
    out = None
    if want_map:
        out = np.full((dim[1], bad_pixels_map_pitch(dim[0])), 0xA5, np.uint8)
        d.map_out = out.ctypes.data
    d.is_f32 = int(is_f32)
    return d, keep, out


class ScaleArea(C.Structure):
    _fields_ = [("offset", C.c_uint32), ("size", C.c_uint32), ("is_vertical", C.c_int32),
                ("reserved", C.c_int32)]


class ScaleDesc(C.Structure):
    _fields_ = [("off_x", C.c_int32), ("off_y", C.c_int32), ("crop_x", C.c_int32),
                ("crop_y", C.c_int32), ("is_f32", C.c_int32), ("black_level", C.c_int32),
                ("has_white", C.c_int32), ("white_point", C.c_int32), ("has_separate", C.c_int32),
                ("black_separate", C.c_int32 * 4), ("n_areas", C.c_uint32), ("areas", C.c_void_p),
                ("dither", C.c_int32), ("host_sse2", C.c_int32)]


class ScaleResult(C.Structure):
    _fields_ = [("black_level", C.c_int32), ("white_point", C.c_int32),
                ("black_separate", C.c_int32 * 4), ("estimated", C.c_int32), ("skipped", C.c_int32),
                ("variant", C.c_int32), ("reserved", C.c_int32), ("n_wrapped", C.c_uint64)]

    def levels(self):
        return (self.black_level, self.white_point, tuple(self.black_separate))


class ScaleJob(C.Structure):
    _fields_ = [("desc", ScaleDesc), ("img_offset", C.c_uint64), ("img", Image)]


def scale_desc(crop, black_level=-1, white_point=None, black_separate=None, areas=(), dither=True,
               host_sse2=True, is_f32=False):
    """(rsx_scale_desc, keep-alive objects).  crop: (off_x, off_y, crop_x, crop_y); white_point and
    black_separate: None when unset; areas: (offset, size, is_vertical) triples."""
    d = ScaleDesc()
    d.off_x, d.off_y, d.crop_x, d.crop_y = crop
    d.is_f32 = int(is_f32)
    d.black_level = black_level
    d.has_white = int(white_point is not None)
    d.white_point = 0 if white_point is None else white_point
    d.has_separate = int(black_separate is not None)
    if black_separate is not None:
        d.black_separate[:] = list(black_separate)
    keep = []
    if len(areas):
        arr = (ScaleArea * len(areas))(*[ScaleArea(o, s, int(v), 0) for o, s, v in areas])
        d.areas, d.n_areas = C.addressof(arr), len(areas)
        keep.append(arr)
    d.dither = int(dither)
    d.host_sse2 = int(host_sse2)
    return d, keep


class DngLossyDesc(C.Structure):
    """the lossy-DNG chain behind the JPEG tiles (include/rsx.h section 4f)"""
    _fields_ = [("stage1", DngPostDesc), ("has_list2", C.c_int32), ("opcodes2_bytes", C.c_uint32),
                ("opcodes2", C.c_void_p), ("scale", ScaleDesc), ("fix", C.c_int32),
                ("reserved", C.c_int32)]


DNG_LOSSY_STAGE1, DNG_LOSSY_SCALED, DNG_LOSSY_LIST2, DNG_LOSSY_FIXED = 1, 2, 4, 8


class DngLossyResult(C.Structure):
    _fields_ = [("list1", DngPostResult), ("list2", DngPostResult), ("scale", ScaleResult),
                ("fixed", BadPixelsResult), ("stages", C.c_uint32), ("reserved", C.c_uint32)]


def dng_lossy_desc(stage1, opcodes2=None, scale=None, fix=False, opcodes2_bytes=None):
    """(rsx_dng_lossy_desc, keep-alive objects).  stage1: (DngPostDesc, keep) of dng_post_desc;
    opcodes2: the OpcodeList2 entry's bytes (b"" is an entry of 0 bytes), None: no list 2;
    scale: (ScaleDesc, keep) of scale_desc, needed with opcodes2."""
    d = DngLossyDesc()
    keep = [stage1[1]]
    d.stage1 = stage1[0]
    if opcodes2 is not None:
        d.has_list2 = 1
        if len(opcodes2):
            a = np.frombuffer(bytes(opcodes2), dtype=np.uint8).copy()
            d.opcodes2, d.opcodes2_bytes = a.ctypes.data, a.size
            keep.append(a)
    if opcodes2_bytes is not None:
        d.opcodes2_bytes = opcodes2_bytes
    if scale is not None:
        d.scale = scale[0]
        keep.append(scale[1])
    d.fix = int(fix)
    return d, keep


class PanasonicV4Desc(C.Structure):
    _fields_ = [("section_split_offset", C.c_uint32), ("zero_is_bad", C.c_int32)]


class PanasonicV4Job(C.Structure):
    _fields_ = [("desc", PanasonicV4Desc), ("in_offset", C.c_uint64), ("in_bytes", C.c_uint64),
                ("img_offset", C.c_uint64), ("img", Image), ("bad_cap", C.c_uint32),
                ("reserved", C.c_uint32)]


def panasonic_v4_consumed(split, dim_x, dim_y):
    """input bytes PanasonicV4Decompressor's peekStream takes (include/rsx.h section 3l)"""
    total = dim_x * dim_y // 14 * 16
    return total if split == 0 else -(-total // 0x4000) * 0x4000


class SamsungV0Job(C.Structure):
    _fields_ = [("row_offsets", C.POINTER(C.c_uint32)), ("n_offsets", C.c_int32),
                ("reserved", C.c_int32), ("in_offset", C.c_uint64), ("in_bytes", C.c_uint64),
                ("img_offset", C.c_uint64), ("img", Image)]


def samsung_v0_offsets(offsets):
    """row offsets -> a ctypes array of uint32 (include/rsx.h section 3k)"""
    arr = (C.c_uint32 * max(1, len(offsets)))()
    for i, o in enumerate(offsets):
        arr[i] = o
    return arr


class DngDeflateDesc(C.Structure):
    _fields_ = [("bps", C.c_int32), ("predictor", C.c_int32)]


class DngDeflateTile(C.Structure):
    """geometry in samples (include/rsx.h section 4b)"""
    _fields_ = [("in_", C.c_void_p), ("in_bytes", C.c_size_t),
                ("tile_w", C.c_uint32), ("tile_h", C.c_uint32),
                ("off_x", C.c_uint32), ("off_y", C.c_uint32),
                ("width", C.c_uint32), ("height", C.c_uint32)]


class DngDeflateJob(C.Structure):
    _fields_ = [("desc", DngDeflateDesc), ("tile_w", C.c_uint32), ("tile_h", C.c_uint32),
                ("off_x", C.c_uint32), ("off_y", C.c_uint32),
                ("width", C.c_uint32), ("height", C.c_uint32),
                ("in_offset", C.c_uint64), ("in_bytes", C.c_uint64),
                ("img_offset", C.c_uint64), ("img", Image)]


class DngJpegTile(C.Structure):
    """one lossy-JPEG tile: its stream and (offX, offY) in pixels (include/rsx.h section 4e)"""
    _fields_ = [("in_", C.c_void_p), ("in_bytes", C.c_size_t),
                ("off_x", C.c_uint32), ("off_y", C.c_uint32)]


JPEG_GREY, JPEG_YCBCR, JPEG_RGB = 0, 1, 2


class DngJpegInfo(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("components", C.c_int32),
                ("h_samp", C.c_int32), ("v_samp", C.c_int32), ("colour_space", C.c_int32),
                ("restart_interval", C.c_uint32), ("n_segments", C.c_uint32)]


class DngJpegJob(C.Structure):
    """the tiles of one image; the host bytes of `tiles` are read while the plan is made"""
    _fields_ = [("n_tiles", C.c_int32), ("tiles", C.POINTER(DngJpegTile)),
                ("in_offsets", C.POINTER(C.c_uint64)), ("img_offset", C.c_uint64), ("img", Image)]


def dng_jpeg_tiles(streams, offsets):
    """streams: bytes-like per tile; offsets: (off_x, off_y) per tile -> (ctypes array, keep-alive)"""
    keep = [np.ascontiguousarray(np.frombuffer(bytes(s), np.uint8)) for s in streams]
    arr = (DngJpegTile * max(1, len(keep)))()
    for i, (a, (ox, oy)) in enumerate(zip(keep, offsets)):
        arr[i].in_, arr[i].in_bytes, arr[i].off_x, arr[i].off_y = a.ctypes.data, a.size, ox, oy
    return arr, keep


def dng_jpeg_job(streams, offsets, img_view, img_offset=0, in_base=0, align=16):
    """One plan job: the streams packed back to back from `in_base` (units of `align` bytes).
    Returns (job, keep-alive, the packed input bytes of this job as a uint8 array)."""
    tiles, keep = dng_jpeg_tiles(streams, offsets)
    offs = (C.c_uint64 * max(1, len(keep)))()
    at = in_base
    for i, a in enumerate(keep):
        offs[i] = at
        at += (a.size + align - 1) // align * align
    packed = np.zeros(at - in_base, np.uint8)
    for i, a in enumerate(keep):
        packed[offs[i] - in_base:offs[i] - in_base + a.size] = a
    j = DngJpegJob()
    j.n_tiles, j.tiles, j.in_offsets, j.img_offset = len(keep), tiles, offs, img_offset
    j.img = img_view
    return j, (tiles, keep, offs), packed


def phase_one_strips(table):
    """[(row, offset, bytes)] -> a ctypes array of rsx_phase_one_strip"""
    arr = (PhaseOneStrip * max(1, len(table)))()
    for i, (n, off, size) in enumerate(table):
        arr[i].n, arr[i].offset, arr[i].bytes = n, off, size
    return arr


class SrawDesc(C.Structure):
    _fields_ = [("version", C.c_int32), ("subsampling_y", C.c_int32),
                ("sraw_coeffs", C.c_int32 * 3), ("hue", C.c_int32)]

    @classmethod
    def make(cls, version, subsampling_y, coeffs, hue):
        d = cls()
        d.version, d.subsampling_y, d.hue = version, subsampling_y, hue
        for i, c in enumerate(coeffs):
            d.sraw_coeffs[i] = c
        return d


class SrawJob(C.Structure):
    _fields_ = [("desc", SrawDesc), ("in_offset", C.c_uint64), ("img_offset", C.c_uint64),
                ("in_", Image), ("img", Image)]


class HasselbladDesc(C.Structure):
    _fields_ = [("table", HuffTable), ("init_pred", C.c_uint16)]

    @classmethod
    def make(cls, table, init_pred):
        d = cls()
        d.table = HuffTable.make(*table)
        d.init_pred = init_pred
        return d


class HasselbladJob(C.Structure):
    _fields_ = [("desc", HasselbladDesc), ("in_offset", C.c_uint64),
                ("in_bytes", C.c_uint64), ("img_offset", C.c_uint64),
                ("img", Image)]


class DngLJpegTile(C.Structure):
    _fields_ = [("desc", LJpegDesc), ("in_", C.c_void_p),
                ("in_bytes", C.c_size_t)]


class DngUnpackTile(C.Structure):
    _fields_ = [("desc", UnpackDesc), ("in_", C.c_void_p),
                ("in_bytes", C.c_size_t)]


class UnpackJob(C.Structure):
    _fields_ = [("desc", UnpackDesc), ("in_offset", C.c_uint64),
                ("in_bytes", C.c_uint64), ("img_offset", C.c_uint64),
                ("img", Image)]


class UnpackVariantJob(C.Structure):
    _fields_ = [("desc", UnpackVariantDesc), ("in_offset", C.c_uint64),
                ("in_bytes", C.c_uint64), ("img_offset", C.c_uint64),
                ("img", Image)]


class LJpegJob(C.Structure):
    _fields_ = [("desc", LJpegDesc), ("in_offset", C.c_uint64),
                ("in_bytes", C.c_uint64), ("img_offset", C.c_uint64),
                ("img", Image)]


class NikonJob(C.Structure):
    _fields_ = [("desc", NikonDesc), ("in_offset", C.c_uint64),
                ("in_bytes", C.c_uint64), ("img_offset", C.c_uint64),
                ("img", Image)]


class Cr2Job(C.Structure):
    _fields_ = [("desc", Cr2Desc), ("in_offset", C.c_uint64),
                ("in_bytes", C.c_uint64), ("img_offset", C.c_uint64),
                ("img", Image)]


def fill_recipe(desc, tables, table_index, init_pred):
    """Fill the PerComponentRecipe part of an LJpegDesc / Cr2Desc."""
    assert 1 <= len(tables) <= RSX_MAX_COMPONENTS
    desc.n_tables = len(tables)
    for i, t in enumerate(tables):
        desc.tables[i] = t
    for c, ti in enumerate(table_index):
        desc.table_index[c] = ti
    for c, p in enumerate(init_pred):
        desc.init_pred[c] = p


FUJI_MAX_STRIPS = 16


class FujiDesc(C.Structure):
    """rsx_fuji_desc (include/rsx.h section 3u)"""
    _fields_ = [("signature", C.c_int32), ("version", C.c_int32), ("raw_type", C.c_int32),
                ("raw_bits", C.c_int32), ("raw_height", C.c_int32),
                ("raw_rounded_width", C.c_int32), ("raw_width", C.c_int32),
                ("block_size", C.c_int32), ("blocks_in_row", C.c_int32),
                ("total_lines", C.c_int32), ("n_strips", C.c_int32), ("reserved", C.c_int32),
                ("strip_offset", C.c_uint64 * FUJI_MAX_STRIPS),
                ("strip_bytes", C.c_uint32 * FUJI_MAX_STRIPS)]


class FujiJob(C.Structure):
    _fields_ = [("desc", FujiDesc), ("in_offset", C.c_uint64), ("in_bytes", C.c_uint64),
                ("img_offset", C.c_uint64), ("img", Image)]


def fuji_desc(header, strips):
    """header: the dict of the ten header fields; strips: [(offset, bytes)]"""
    d = FujiDesc()
    for k, v in header.items():
        setattr(d, k, v)
    d.n_strips = len(strips)
    for i, (off, n) in enumerate(strips):
        d.strip_offset[i], d.strip_bytes[i] = off, n
    return d


class OlympusJob(C.Structure):
    """rsx_olympus_job (include/rsx.h section 3v)"""
    _fields_ = [("in_offset", C.c_uint64), ("in_bytes", C.c_uint64), ("img_offset", C.c_uint64),
                ("img", Image)]


RSX_KODAK_TABLE_NONE, RSX_KODAK_TABLE_PLAIN, RSX_KODAK_TABLE_DITHER = 0, 1, 2


class KodakDesc(C.Structure):
    """rsx_kodak_desc (include/rsx.h section 3w)"""
    _fields_ = [("bps", C.c_int32), ("table_mode", C.c_int32), ("table", C.POINTER(C.c_uint16))]


class KodakJob(C.Structure):
    """rsx_kodak_job"""
    _fields_ = [("desc", KodakDesc), ("in_offset", C.c_uint64), ("in_bytes", C.c_uint64),
                ("img_offset", C.c_uint64), ("img", Image)]


def kodak_table_entries(bps, mode):
    """entries of TableLookUp::tables a mode reads: 1024 / 2048 (bps 10), 4096 / 8192 (bps 12)"""
    return 0 if mode == RSX_KODAK_TABLE_NONE else (2 if mode == RSX_KODAK_TABLE_DITHER else 1) << bps


def kodak_desc(bps, mode, table=None):
    """(desc, keep-alive array): `table` as TableLookUp holds it (uint16; None for NONE)"""
    d = KodakDesc()
    d.bps, d.table_mode = bps, mode
    arr = None
    if table is not None:
        arr = np.ascontiguousarray(table, dtype=np.uint16)
        d.table = arr.ctypes.data_as(C.POINTER(C.c_uint16))
    return d, arr


class CrwDesc(C.Structure):
    """rsx_crw_desc (include/rsx.h section 3x)"""
    _fields_ = [("dec_table", C.c_uint32), ("has_lowbits", C.c_uint32)]


class CrwJob(C.Structure):
    """rsx_crw_job: the scan and the low bits are two ranges of the run's input buffer"""
    _fields_ = [("desc", CrwDesc), ("in_offset", C.c_uint64), ("in_bytes", C.c_uint64),
                ("low_offset", C.c_uint64), ("low_bytes", C.c_uint64),
                ("img_offset", C.c_uint64), ("img", Image)]


def crw_desc(dec_table, has_lowbits):
    d = CrwDesc()
    d.dec_table, d.has_lowbits = dec_table, 1 if has_lowbits else 0
    return d


class FujiRotateDesc(C.Structure):
    """rsx_raf_rotate_desc (include/rsx.h section 3y)"""
    _fields_ = [("crop_x", C.c_int32), ("crop_y", C.c_int32), ("size_x", C.c_int32),
                ("size_y", C.c_int32), ("alt_layout", C.c_int32), ("reserved", C.c_int32)]


class FujiRotateJob(C.Structure):
    """rsx_raf_rotate_job: the source in the run's input buffer, the rotated image in its output"""
    _fields_ = [("desc", FujiRotateDesc), ("in_offset", C.c_uint64), ("img_offset", C.c_uint64),
                ("in_", Image), ("img", Image)]


def fuji_rotate_desc(crop, size, alt_layout):
    d = FujiRotateDesc()
    (d.crop_x, d.crop_y), (d.size_x, d.size_y) = crop, size
    d.alt_layout = 1 if alt_layout else 0
    return d


class SonySrfJob(C.Structure):
    """rsx_sony_srf_job (include/rsx.h section 3z)"""
    _fields_ = [("in_offset", C.c_uint64), ("in_bytes", C.c_uint64), ("img_offset", C.c_uint64),
                ("key", C.c_uint32), ("reserved", C.c_uint32), ("img", Image)]


class ImageHashResult(C.Structure):
    """rsx_image_hash_result (include/rsx.h section 4g)"""
    _fields_ = [("md5", C.c_uint8 * 16), ("byte_sum", C.c_uint64), ("sample_sum", C.c_uint64)]

    def digest(self):
        return bytes(self.md5)


class ImageHashJob(C.Structure):
    """rsx_image_hash_job: the image in the run's input buffer, the line digests and the result in
    its output buffer"""
    _fields_ = [("img_offset", C.c_uint64), ("lines_offset", C.c_uint64),
                ("result_offset", C.c_uint64), ("sample_bytes", C.c_int32),
                ("reserved", C.c_int32), ("img", Image)]


def image_hash_job(img_offset, lines_offset, result_offset, sample_bytes, dim_x, dim_y, cpp,
                   pitch_bytes):
    j = ImageHashJob()
    j.img_offset, j.lines_offset, j.result_offset = img_offset, lines_offset, result_offset
    j.sample_bytes = sample_bytes
    j.img = Image(None, pitch_bytes, dim_x, dim_y, cpp, 0)
    return j


def hex_joined_hash(line_md5):
    """tests/golden_cases.image_hash's form of the image hash, from the 16 dim_y bytes of the line
    digests: the MD5 of the concatenated hex digests"""
    import hashlib
    raw = bytes(line_md5)
    return hashlib.md5(raw.hex().encode()).hexdigest()


# include/rsx.h section 7: the writers
ENCODE_TAIL_JPEG, ENCODE_TAIL_VACUUMER = 0, 1
ENCODE_TABLE_ALL_CATEGORIES = 1
ENCODE_CATEGORIES = 17


class EncodePackResult(C.Structure):
    """rsx_encode_pack_result"""
    _fields_ = [("bytes_written", C.c_uint64), ("stream_bytes", C.c_uint64)]


class EncodeResult(C.Structure):
    """rsx_encode_result"""
    _fields_ = [("status", C.c_int32), ("reserved", C.c_int32), ("bytes", C.c_uint64),
                ("symbol_bits", C.c_uint64)]


class EncodePackJob(C.Structure):
    """rsx_encode_pack_job: the image in the run's input buffer, the stream in its output buffer"""
    _fields_ = [("desc", UnpackDesc), ("reserved", C.c_uint32), ("img_offset", C.c_uint64),
                ("out_offset", C.c_uint64), ("out_cap", C.c_uint64), ("img", Image)]


class EncodeLJpegJob(C.Structure):
    """rsx_encode_ljpeg_job"""
    _fields_ = [("desc", LJpegDesc), ("flags", C.c_uint32), ("reserved", C.c_uint32),
                ("img_offset", C.c_uint64), ("out_offset", C.c_uint64), ("out_cap", C.c_uint64),
                ("img", Image)]


def encode_pack_job(desc, img_offset, out_offset, out_cap, dim_x, dim_y, cpp, pitch_bytes):
    return EncodePackJob(desc, 0, img_offset, out_offset, out_cap,
                         Image(None, pitch_bytes, dim_x, dim_y, cpp, 1))


def encode_ljpeg_job(desc, flags, img_offset, out_offset, out_cap, dim_x, dim_y, cpp, pitch_bytes):
    return EncodeLJpegJob(desc, flags, 0, img_offset, out_offset, out_cap,
                          Image(None, pitch_bytes, dim_x, dim_y, cpp, 1))


# include/rsx.h section 7d: the writers of F32 images
class FpWriteWindow(C.Structure):
    """rsx_fpwrite_window: samples, cpp folded in"""
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32)]


class FpWritePackResult(C.Structure):
    """rsx_fpwrite_pack_result"""
    _fields_ = [("bytes_written", C.c_uint64), ("stream_bytes", C.c_uint64),
                ("inexact", C.c_uint64)]


class FpWritePackJob(C.Structure):
    """rsx_fpwrite_pack_job: the image in the run's input buffer, the stream in its output buffer"""
    _fields_ = [("desc", UnpackDesc), ("reserved", C.c_uint32), ("img_offset", C.c_uint64),
                ("out_offset", C.c_uint64), ("out_cap", C.c_uint64), ("img", Image)]


def fpwrite_pack_job(desc, img_offset, out_offset, out_cap, dim_x, dim_y, cpp, pitch_bytes):
    return FpWritePackJob(desc, 0, img_offset, out_offset, out_cap,
                          Image(None, pitch_bytes, dim_x, dim_y, cpp, 1))


FPWRITE_BLOCK = 16384


class FpWriteDeflateTile(C.Structure):
    """rsx_fpwrite_deflate_tile: geometry in samples, as DngDeflateTile"""
    _fields_ = [("out", C.c_void_p), ("out_cap", C.c_size_t),
                ("tile_w", C.c_uint32), ("tile_h", C.c_uint32),
                ("off_x", C.c_uint32), ("off_y", C.c_uint32),
                ("width", C.c_uint32), ("height", C.c_uint32)]


class FpWriteDeflateResult(C.Structure):
    """rsx_fpwrite_deflate_result"""
    _fields_ = [("status", C.c_int32), ("adler", C.c_uint32), ("bytes", C.c_uint64),
                ("blocks", C.c_uint32), ("stored_blocks", C.c_uint32)]


class FpWriteDeflateJob(C.Structure):
    """rsx_fpwrite_deflate_job"""
    _fields_ = [("desc", DngDeflateDesc), ("tile_w", C.c_uint32), ("tile_h", C.c_uint32),
                ("off_x", C.c_uint32), ("off_y", C.c_uint32),
                ("width", C.c_uint32), ("height", C.c_uint32),
                ("img_offset", C.c_uint64), ("out_offset", C.c_uint64), ("out_cap", C.c_uint64),
                ("img", Image)]


# include/rsx.h section 7e: the baseline-DCT JPEG tile writer
DCTWRITE_JFIF = 1


class DctWriteDesc(C.Structure):
    """rsx_dctwrite_desc: the frame in pixels, luma sampling against chroma, two tables in natural
    order"""
    _fields_ = [("off_x", C.c_uint32), ("off_y", C.c_uint32), ("width", C.c_uint32),
                ("height", C.c_uint32), ("components", C.c_int32), ("h_samp", C.c_int32),
                ("v_samp", C.c_int32), ("restart_interval", C.c_uint32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32), ("qtables", (C.c_uint16 * 64) * 2)]


class DctWriteTile(C.Structure):
    """rsx_dctwrite_tile"""
    _fields_ = [("desc", DctWriteDesc), ("out", C.c_void_p), ("out_cap", C.c_size_t)]


class DctWriteResult(C.Structure):
    """rsx_dctwrite_result"""
    _fields_ = [("status", C.c_int32), ("reserved", C.c_uint32), ("bytes", C.c_uint64),
                ("scan_bytes", C.c_uint64), ("symbol_bits", C.c_uint64)]


class DctWriteJob(C.Structure):
    """rsx_dctwrite_job: the image in the run's input buffer, the stream in its output buffer"""
    _fields_ = [("desc", DctWriteDesc), ("img_offset", C.c_uint64), ("out_offset", C.c_uint64),
                ("out_cap", C.c_uint64), ("img", Image)]


def dctwrite_desc(off_x, off_y, width, height, components, h_samp, v_samp, luma, chroma,
                  restart_interval=0, flags=DCTWRITE_JFIF):
    d = DctWriteDesc(off_x, off_y, width, height, components, h_samp, v_samp, restart_interval,
                     flags, 0)
    for i in range(64):
        d.qtables[0][i] = int(luma[i])
        d.qtables[1][i] = int(chroma[i])
    return d


def dctwrite_job(desc, img_offset, out_offset, out_cap, dim_x, dim_y, cpp, pitch_bytes):
    return DctWriteJob(desc, img_offset, out_offset, out_cap,
                       Image(None, pitch_bytes, dim_x, dim_y, cpp, 0))
