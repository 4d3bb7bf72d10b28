// rsx_rawspeed_shim.h -- the reference-side binding of the C-ABI (include/rsx.h).
//
// This header is what a rawspeed maintainer drops into src/librawspeed/ (see
// INTEGRATION.md): it converts the objects the three hot-path decompressors
// already hold (RawImage, iRectangle2D, PrefixCodeDecoder<> recipes, input
// views) into the plain-C descriptors of include/rsx.h, calls the GPU core and
// turns a non-OK status back into the exception type the reference throws.
// It contains no decoding logic and no copy of reference code; it only reads
// public members of reference types:
//   RawImageData::{dim, pitch, getCpp(), isCFA, getU16DataAsUncroppedArray2DRef()}
//     (common/RawImage.h:104-199, :289-296)
//   AbstractPrefixCodeTranscoder::{code, handleDNGBug16()}
//     (codes/AbstractPrefixCodeTranscoder.h:45,82-84), PrefixCode::nCodesPerLength
//     (codes/PrefixCode.h:45), AbstractPrefixCode::codeValues (codes/AbstractPrefixCode.h:190)
#pragma once

#include "rsx.h"
#include "rsx_pin.h"

#include "adt/Array1DRef.h"
#include "adt/Mutex.h"
#include "adt/Point.h"
#include "codes/PrefixCodeDecoder.h"
#include "common/RawImage.h"
#include "common/TableLookUp.h"
#include "decoders/RawDecoderException.h"
#include "io/Buffer.h"
#include "io/ByteStream.h"
#include "io/IOException.h"
#include "metadata/ColorFilterArray.h"

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>
#include <shared_mutex>
#include <vector>

namespace rawspeed::rsx_shim {

// (the process-wide context() and the optional page-locked pool: rsx_pin.h)

// What became of the units of work (a strip, a scan, a DNG tile) the hunks saw: decoded
// by the device, or left to the method's original body.  Diagnostics only -- the tests
// use it to show that an image was produced by the GPU and not by a silent fall-through.
struct Stats {
  std::atomic<uint64_t> forwarded{0}, fell_through{0};
};
inline Stats& stats() {
  static Stats s;
  return s;
}
// the test every hunk makes on its call's status
inline bool done(int status) {
  ++(status == RSX_OK ? stats().forwarded : stats().fell_through);
  return status == RSX_OK;
}

inline rsx_image view(const RawImage& img) {
  rsx_image v{};
  const auto a = img->getByteDataAsUncroppedArray2DRef(); // UINT16 and F32 images
  v.data = &a(0, 0);
  v.pitch_bytes = implicit_cast<uint32_t>(img->pitch);
  v.dim_x = img->dim.x;
  v.dim_y = img->dim.y;
  v.cpp = implicit_cast<int32_t>(img->getCpp());
  v.is_cfa = img->isCFA ? 1 : 0;
  return v;
}

// SonyArw2Decompressor::decompress(): the table setWithLookUp would use
// (mRaw->table; RawImageData keeps it protected, so the hunk reads it through an accessor)
inline rsx_sony_arw2_desc arw2_desc(const TableLookUp* t) {
  rsx_sony_arw2_desc d{};
  d.table_mode = !t ? RSX_ARW2_TABLE_NONE
                    : (t->dither ? RSX_ARW2_TABLE_DITHER : RSX_ARW2_TABLE_PLAIN);
  d.table = t ? t->tables.data() : nullptr; // (table 0; the call reads its first 4096 / 8192)
  return d;
}

// NefDecoder::DecodeNikonSNef: the descriptor and the call.  `t` is the table
// the curve guard installed (mRaw->table through the accessor of 3i; always the dithering one
// here), inv_wb_r / inv_wb_b what :693-694 computed, `input` the stream the loop would peek.
inline int nikon_snef(const ByteStream& input, const RawImage& img, const TableLookUp* t,
                      int inv_wb_r, int inv_wb_b) {
  rsx_ctx* rsx = context();
  if (!rsx || !t || !t->dither)
    return RSX_ERR_DEVICE;
  rsx_nikon_snef_desc d{};
  d.inv_wb_r = inv_wb_r;
  d.inv_wb_b = inv_wb_b;
  d.table = t->tables.data(); // (table 0; the call reads its first 8192 entries)
  const rsx_image v = view(img);
  const Buffer in = input.peekRemainingBuffer();
  return rsx_nikon_snef_decompress(rsx, &d, in.begin(), in.getSize(), &v);
}

// VC5Decompressor::decode(): what the constructor's tag parse found, handed
// over.  The hunk sits inside the member function, behind initPrefixCodeDecoder() and
// initVC5LogTable(), and feeds this collector from the members it can see: the code book's rows
// with the value decompanded, the 4096 entries of mVC5LogTable, every band's input view with its
// quantisation or precision, every level's prescale.  `tile` is the stream the constructor kept
// (mBs): band offsets count from the first byte of its buffer.  parseVC5() has read that stream
// to its end by now, so its remaining view (peekRemainingBuffer) is empty and lies behind every
// band; Buffer::begin() and Buffer::getSize() are the whole tile whatever the position, and
// every band's input is a view into it (getStream / getSubView never copy).
struct Vc5 {
  rsx_vc5_desc d{};
  std::vector<rsx_vc5_code> codes;
  std::vector<uint16_t> log;
  const uint8_t* base;
  size_t bytes;
  Vc5(const ByteStream& tile, bool gbrg) : base(tile.begin()), bytes(tile.getSize()) {
    d.phase = gbrg ? 1 : 0;
    codes.reserve(264);
    log.reserve(4096);
  }
  void code(uint32_t bits, unsigned size, unsigned count, int value) {
    codes.push_back(rsx_vc5_code{bits, uint8_t(size), uint16_t(count), int16_t(value)});
  }
  // subband 0: the low-pass band of level 3 (its 8-byte-rounded input); 1-3 / 4-6 / 7-9: bands
  // 1..3 of level 3 / 2 / 1
  void band(int channel, int subband, Array1DRef<const uint8_t> input, int quant, int precision) {
    rsx_vc5_band& b = d.bands[channel][subband];
    b.offset = uint64_t(input.begin() - base);
    b.bytes = uint32_t(input.size());
    b.quant = int16_t(quant);
    b.precision = uint16_t(precision);
  }
  void prescale(int channel, int level, int value) { d.prescale[channel][level - 1] = uint8_t(value); }
  int run(const RawImage& img) {
    rsx_ctx* rsx = context();
    if (!rsx || log.size() != 4096)
      return RSX_ERR_DEVICE;
    d.log_table = log.data();
    d.codes = codes.data();
    d.n_codes = int(codes.size());
    const rsx_image v = view(img);
    return rsx_vc5_decompress(rsx, &d, base, bytes, &v);
  }
};

// IiqDecoder::decodeRawInternal(): the correction entries of the 0x110 block as
// an op list, in file order, for rsx_phase_one_decompress_corrected.  The hunk parses the block
// first (what CorrectPhaseOneC's switch does, without touching a pixel) and feeds this collector:
// a flat-field entry and the sensor defects (0x400) are handed over as the bytes of their
// sub-streams -- the bad columns of the defects are corrected on the device, where the entry stands
// in the list; its type-129 records go into mRaw->mBadPixelPositions behind a call that succeeded
// (run), or are fixed on the device in front of the download when the caller interpolates bad
// pixels (fixed: INTEGRATION.md 3r) --; a quadrant entry as the four
// curves the reference's own Spline<>::calculateCurve() gave for the control points of
// :338-373 (its checks have thrown by then, as they would have); the CFA as mRaw->cfa holds it.
// More than RSX_IIQ_MAX_OPS entries, or a CFA of more than 64 positions: `usable` goes false and
// the hunk keeps the host path.
struct IiqCorrections {
  rsx_iiq_corr d{};
  std::vector<std::vector<uint16_t>> curves; // [op]: 4 x 65536, [quadRow][quadCol]
  bool usable = true;
  const rsx_iiq_op* defects_op = nullptr;
  IiqCorrections() { curves.reserve(RSX_IIQ_MAX_OPS); }
  rsx_iiq_op* next(int kind) {
    if (d.n_ops >= RSX_IIQ_MAX_OPS) {
      usable = false;
      return nullptr;
    }
    rsx_iiq_op* op = &d.ops[d.n_ops++];
    op->kind = kind;
    return op;
  }
  void flat_field(const ByteStream& entry, bool chroma) {
    if (rsx_iiq_op* op = next(RSX_IIQ_OP_FLAT_FIELD)) {
      const Buffer b = entry.peekRemainingBuffer();
      op->chroma = chroma ? 1 : 0;
      op->payload = b.begin();
      op->payload_bytes = b.getSize();
    }
  }
  // entry 0x400 (the hunk keeps its "Second sensor defects entry seen" throw)
  void defects(const ByteStream& entry) {
    if (rsx_iiq_op* op = next(RSX_IIQ_OP_SENSOR_DEFECTS)) {
      const Buffer b = entry.peekRemainingBuffer();
      op->payload = b.begin();
      op->payload_bytes = b.getSize();
      defects_op = op;
    }
  }
  // quad[quadRow][quadCol]: 65536 entries each
  void quadrant(const std::vector<uint16_t> (&quad)[2][2], uint32_t split_row, uint32_t split_col,
                uint32_t black_level) {
    if (rsx_iiq_op* op = next(RSX_IIQ_OP_QUADRANT_CURVES)) {
      std::vector<uint16_t>& all = curves.emplace_back();
      all.reserve(4 * 65536);
      for (const auto& row : quad)
        for (const std::vector<uint16_t>& c : row)
          all.insert(all.end(), c.begin(), c.end());
      usable = usable && all.size() == 4 * 65536;
      op->curves = all.data();
      op->split_row = split_row;
      op->split_col = split_col;
      op->black_level = black_level;
    }
  }
  void cfa(const ColorFilterArray& c) {
    const iPoint2D size = c.getSize();
    if (size.area() > 64) {
      usable = false;
      return;
    }
    d.cfa_w = size.x;
    d.cfa_h = size.y;
    for (int y = 0; y < size.y; ++y)
      for (int x = 0; x < size.x; ++x)
        d.cfa[x + y * size.x] = static_cast<uint8_t>(c.getColorAt(x, y));
  }
  // decode + corrections + the one download; `table` and [lo, hi) as in the hunk of 3h
  int run(const uint8_t* lo, size_t bytes, const std::vector<rsx_phase_one_strip>& table,
          const RawImage& img) {
    rsx_ctx* rsx = context();
    if (!rsx || !usable)
      return RSX_ERR_DEVICE;
    const rsx_image v = view(img);
    const int st = rsx_phase_one_decompress_corrected(
        rsx, lo, bytes, implicit_cast<int>(table.size()), table.data(), &d, &v, nullptr);
    if (st == RSX_OK)
      insert_positions(img);
    return st;
  }
  // ... with fixBadPixels() on the device in front of the download (the caller interpolates bad
  // pixels): `map` receives mBadPixelMap when one was made (result->map_made), and the positions
  // stay out of mBadPixelPositions, as transferBadPixelsToMap() leaves them
  int fixed(const uint8_t* lo, size_t bytes, const std::vector<rsx_phase_one_strip>& table,
             const RawImage& img, std::vector<uint8_t>* map, uint32_t map_pitch,
             rsx_bad_pixels_result* result) {
    rsx_ctx* rsx = context();
    if (!rsx || !usable)
      return RSX_ERR_DEVICE;
    const rsx_image v = view(img);
    map->assign(size_t(map_pitch) * size_t(v.dim_y), 0);
    return rsx_phase_one_decompress_fixed(rsx, lo, bytes, implicit_cast<int>(table.size()),
                                           table.data(), &d, &v, nullptr, map->data(), map_pitch,
                                           result);
  }

private:
  // handleBadPixel for every type-129 record inside the image, in file order
  void insert_positions(const RawImage& img) const {
    if (!defects_op)
      return;
    uint32_t n = 0;
    if (rsx_iiq_defect_positions(defects_op->payload, defects_op->payload_bytes, img->dim.x, nullptr,
                                 0, &n) != RSX_OK || n == 0)
      return;
    std::vector<uint32_t> pos(n);
    rsx_iiq_defect_positions(defects_op->payload, defects_op->payload_bytes, img->dim.x, pos.data(),
                             n, &n);
    MutexLocker guard(&img->mBadPixelMutex);
    img->mBadPixelPositions.insert(img->mBadPixelPositions.end(), pos.begin(), pos.end());
  }
};

// PanasonicV5Decompressor / V6 / V7::decompress(): the descriptor and the call;
// `input` is the stream the constructor kept (exactly the bytes peekStream took)
inline int panasonic(int version, uint32_t bps, const ByteStream& input, const RawImage& img) {
  rsx_ctx* rsx = context();
  if (!rsx)
    return RSX_ERR_DEVICE;
  const rsx_panasonic_desc d{version, implicit_cast<int32_t>(bps)};
  const rsx_image v = view(img);
  const Buffer in = input.peekRemainingBuffer();
  return rsx_panasonic_decompress(rsx, &d, in.begin(), in.getSize(), &v);
}

// PanasonicV4Decompressor::decompress(): `input` is the stream the constructor
// kept (exactly the bytes peekStream took).  The zero pixels come back in ascending order and are
// appended to mRaw->mBadPixelPositions under its mutex, as decompressThread does; a list longer
// than the room made for it (RSX_ERR_UNSUPPORTED) leaves the frame to the original code, like any
// status but RSX_OK.
inline int panasonic_v4(const ByteStream& input, const RawImage& img, bool zero_is_bad,
                        uint32_t section_split_offset) {
  rsx_ctx* rsx = context();
  if (!rsx)
    return RSX_ERR_DEVICE;
  constexpr uint32_t MaxBadPixels = 1U << 16; // (real files hold a handful)
  const rsx_panasonic_v4_desc d{section_split_offset, zero_is_bad ? 1 : 0};
  const rsx_image v = view(img);
  const Buffer in = input.peekRemainingBuffer();
  std::vector<uint32_t> bad(zero_is_bad ? MaxBadPixels : 0);
  uint64_t n = 0;
  const int st = rsx_panasonic_v4_decompress(rsx, &d, in.begin(), in.getSize(), &v,
                                             bad.empty() ? nullptr : bad.data(),
                                             implicit_cast<uint32_t>(bad.size()), &n);
  if (st == RSX_OK && n != 0) {
    MutexLocker guard(&img->mBadPixelMutex);
    img->mBadPixelPositions.insert(img->mBadPixelPositions.end(), bad.begin(),
                                   bad.begin() + implicit_cast<std::ptrdiff_t>(n));
  }
  return st;
}

// SamsungV0Decompressor::decompress(): `stripes` are the rows computeStripes cut
// out of the strip, one behind the other; the call takes the strip from the first row up and the
// rows' offsets in it
inline int samsung_v0(const std::vector<ByteStream>& stripes, const RawImage& img) {
  rsx_ctx* rsx = context();
  if (!rsx)
    return RSX_ERR_DEVICE;
  if (stripes.empty())
    return RSX_ERR_INVALID_ARG;
  const uint8_t* lo = stripes.front().peekRemainingBuffer().begin();
  const uint8_t* hi = stripes.back().peekRemainingBuffer().end();
  std::vector<uint32_t> offsets(stripes.size());
  for (size_t i = 0; i < stripes.size(); ++i)
    offsets[i] = implicit_cast<uint32_t>(stripes[i].peekRemainingBuffer().begin() - lo);
  const rsx_image v = view(img);
  return rsx_samsung_v0_decompress(rsx, lo, static_cast<size_t>(hi - lo), offsets.data(),
                                   implicit_cast<int>(offsets.size()), &v, nullptr);
}

// OlympusDecompressor::decompress(): `input` is the stream OrfDecoder hands
// over, the 7 bytes the decompressor skips included
inline int olympus(const ByteStream& input, const RawImage& img) {
  rsx_ctx* rsx = context();
  if (!rsx)
    return RSX_ERR_DEVICE;
  const rsx_image v = view(img);
  const Buffer in = input.peekRemainingBuffer();
  return rsx_olympus_decompress(rsx, in.begin(), in.getSize(), &v);
}

// KodakDecompressor::decompress(): `input` is what DcrDecoder hands over, the
// rest of the file from the strip's offset; `t` the table the curve guard installed (mRaw->table
// through the accessor of 3i; the dithering one, or none with uncorrectedRawValues)
inline int kodak(const ByteStream& input, const RawImage& img, int bps, const TableLookUp* t) {
  rsx_ctx* rsx = context();
  if (!rsx)
    return RSX_ERR_DEVICE;
  rsx_kodak_desc d{};
  d.bps = bps;
  d.table_mode = !t ? RSX_KODAK_TABLE_NONE
                    : (t->dither ? RSX_KODAK_TABLE_DITHER : RSX_KODAK_TABLE_PLAIN);
  d.table = t ? t->tables.data() : nullptr; // (table 0; the call reads its first 2^bps / 2^(bps + 1))
  const rsx_image v = view(img);
  const Buffer in = input.peekRemainingBuffer();
  return rsx_kodak_decompress(rsx, &d, in.begin(), in.getSize(), &v);
}

// CrwDecompressor::decompress(): `input` is the scan behind the 514 bytes
// CrwDecoder skips, `low` the low-bit array the constructor cropped (NULL when the camera has none)
inline int crw(const Array1DRef<const uint8_t>& input, const Array1DRef<const uint8_t>* low,
               const RawImage& img, uint32_t dec_table) {
  rsx_ctx* rsx = context();
  if (!rsx)
    return RSX_ERR_DEVICE;
  rsx_crw_desc d{};
  d.dec_table = dec_table;
  d.has_lowbits = low ? 1u : 0u;
  const rsx_image v = view(img);
  return rsx_crw_decompress(rsx, &d, input.begin(), size_t(input.size()), low ? low->begin() : nullptr,
                            low ? size_t(low->size()) : 0, &v);
}

// RafDecoder::applyCorrections(): the 45 degree rotation of `img` (not yet
// cropped: the crop is the descriptor's) into a new image, which replaces *rotated on RSX_OK with
// fujiRotationPos set; on any other status *rotated is untouched and the hunk falls through
inline int raf_rotate(const RawImage& img, iPoint2D crop_offset, iPoint2D new_size, bool alt_layout,
                      RawImage* rotated) {
  rsx_ctx* rsx = context();
  if (!rsx)
    return RSX_ERR_DEVICE;
  const rsx_raf_rotate_desc d = {crop_offset.x, crop_offset.y, new_size.x,
                                 new_size.y,    alt_layout ? 1 : 0, 0};
  int32_t dim_x = 0, dim_y = 0, pos = 0;
  if (int st = rsx_raf_rotate_geometry(&d, &dim_x, &dim_y, &pos))
    return st;
  RawImage out = RawImage::create(iPoint2D(dim_x, dim_y), RawImageType::UINT16, 1);
  const rsx_image src = view(img), dst = view(out);
  if (int st = rsx_raf_rotate(rsx, &d, &src, &dst))
    return st;
  out->metadata = img->metadata;
  out->metadata.fujiRotationPos = implicit_cast<uint32_t>(pos);
  *rotated = out;
  return RSX_OK;
}

// ArwDecoder::decodeSRF(): `data` is the image buffer at its fixed offset,
// `key` the key behind the reference's derivation; `img` has its dimensions and its data
inline int sony_srf(const Array1DRef<const uint8_t>& data, uint32_t key, const RawImage& img) {
  rsx_ctx* rsx = context();
  if (!rsx)
    return RSX_ERR_DEVICE;
  const rsx_image v = view(img);
  return rsx_sony_srf_decompress(rsx, data.begin(), size_t(data.size()), key, &v);
}

// DngDecoder::decodeRawInternal() / handleMetadata(): what follows the tiles --
// OpcodeList1 and the LinearizationTable look-up -- handed to the tile fan-out so that it runs on
// the device in front of the ONE download.  The hunk fills this BEFORE decodeData (the entries,
// and the crop handleMetadata's ActiveArea / DefaultCrop subFrames will leave), hangs it on the
// DngBatch, and after the decode calls finish(): the logged error, the list's TrimBounds as a
// subFrame, the bad-pixel positions.  `applied` false: the device did not run the stage (a failing
// tile, a list or an image this core refuses) and handleMetadata does what it always did.
struct DngPost {
  static constexpr uint32_t MaxConstantHits = 1U << 16; // (real files hold a handful)
  rsx_dng_post_desc d{};
  std::vector<uint16_t> table;
  rsx_dng_post_result result{};
  std::vector<uint32_t> bad;
  bool applied = false;
  // opcodes: the OPCODELIST1 entry's bytes (nullptr: no entry, or one of count 0, or
  // !applyStage1DngOpcodes); lin: the LINEARIZATIONTABLE (empty: none, or uncorrectedRawValues)
  // `img`: mRaw with dim and cpp set (no pixel is looked at; createData may still be ahead).  Room
  // for positions is made only when the list can produce any: what FixBadPixelsList holds, which
  // rsx_dng_post_validate counts, plus MaxConstantHits when the list is there and the image is
  // one FixBadPixelsConstant runs on.  A list past that room leaves the stage to the host.
  void set(const Buffer* opcodes, std::vector<uint16_t> lin, const iRectangle2D& crop,
           bool is_f32, const RawImage& img) {
    table = std::move(lin);
    d.opcodes = opcodes ? opcodes->begin() : nullptr;
    d.opcodes_bytes = opcodes ? opcodes->getSize() : 0;
    d.table = table.empty() ? nullptr : table.data();
    d.table_count = implicit_cast<uint32_t>(table.size());
    d.is_f32 = is_f32 ? 1 : 0;
    d.crop_x = crop.pos.x;
    d.crop_y = crop.pos.y;
    d.crop_w = crop.dim.x;
    d.crop_h = crop.dim.y;
    bad.clear();
    if (d.opcodes_bytes != 0) {
      rsx_image v{};
      v.dim_x = img->dim.x;
      v.dim_y = img->dim.y;
      v.cpp = implicit_cast<int32_t>(img->getCpp());
      v.pitch_bytes = implicit_cast<uint32_t>(v.dim_x) * implicit_cast<uint32_t>(v.cpp) *
                      (is_f32 ? 4U : 2U);
      rsx_dng_post_result r{};
      (void)rsx_dng_post_validate(&d, &v, &r, nullptr, 0); // (the count; no room yet)
      const uint64_t room = r.n_bad + (!is_f32 && v.cpp == 1 ? MaxConstantHits : 0U);
      bad.resize(implicit_cast<size_t>(std::min<uint64_t>(room, 1U << 26)));
    }
  }
  bool wanted() const { return d.opcodes_bytes != 0 || d.table_count != 0; }
  // behind handleMetadata's own subFrames (the image's crop is the one set() was given)
  void finish(const RawImage& img) const {
    if (result.list_status != RSX_OK)
      img->setError("rsx: DNG opcode list refused as the reference's parser refuses it");
    const iPoint2D off = img->getCropOffset();
    const iRectangle2D trimmed(result.crop_x - off.x, result.crop_y - off.y, result.crop_w,
                               result.crop_h);
    if (!(trimmed.pos == iPoint2D(0, 0)) || !(trimmed.dim == img->dim))
      img->subFrame(trimmed);
    if (result.n_bad != 0) {
      MutexLocker guard(&img->mBadPixelMutex);
      img->mBadPixelPositions.insert(img->mBadPixelPositions.begin(), bad.begin(),
                                     bad.begin() + implicit_cast<std::ptrdiff_t>(result.n_bad));
    }
  }
};

// DngDecoder::decodeRawInternal() / handleMetadata() for compression 0x884c:
// the whole branch for lossy DNGs -- the JPEG tiles, OpcodeList1, the look-up, scaleBlackWhite(),
// OpcodeList2 and, for a caller that interpolates bad pixels, fixBadPixels() -- as ONE call with
// one download (include/rsx.h section 4f).  The hunk fills `stage1` as in 3q, calls setBlack()
// (it reads the IFD alone) and then set(); run() is the tile call; finish() does to mRaw what the
// stages that ran would have done.  What `result.stages` does not name is left to handleMetadata
// as it is: nothing of it after a failing tile, scaleBlackWhite() onwards after a scale stage that
// refused from the image.
struct DngLossy {
  DngPost stage1;
  rsx_dng_lossy_desc d{};
  std::vector<rsx_scale_area> areas;
  rsx_dng_lossy_result result{};
  std::vector<uint32_t> bad;
  std::vector<uint8_t> map;
  // opcodes2: the OPCODELIST2 entry's bytes, an entry of 0 bytes included (nullptr: no entry, or
  // uncorrectedRawValues); `img`: mRaw behind setBlack(), dim and cpp set; fix: the caller
  // interpolates bad pixels.  False: this core refuses the file's lists or levels, or the file
  // fails -- handleMetadata does what it always did, and throws what it always threw.
  bool set(const Buffer* opcodes2, const RawImage& img, bool fix, bool host_sse2) {
    d = rsx_dng_lossy_desc{};
    d.stage1 = stage1.d;
    d.has_list2 = opcodes2 ? 1 : 0;
    d.opcodes2 = opcodes2 ? opcodes2->begin() : nullptr;
    d.opcodes2_bytes = opcodes2 ? opcodes2->getSize() : 0;
    d.fix = fix ? 1 : 0;
    rsx_image v{};
    v.dim_x = img->getUncroppedDim().x;
    v.dim_y = img->getUncroppedDim().y;
    v.cpp = implicit_cast<int32_t>(img->getCpp());
    v.pitch_bytes = implicit_cast<uint32_t>(v.dim_x) * implicit_cast<uint32_t>(v.cpp) * 2U;
    v.is_cfa = img->isCFA ? 1 : 0;
    rsx_dng_post_result r1{};
    const int st1 = rsx_dng_post_validate(&d.stage1, &v, &r1, nullptr, 0);
    if (st1 != RSX_OK && !(st1 == RSX_ERR_UNSUPPORTED && r1.n_bad != 0))
      return false;
    if (d.has_list2) {
      // the scale stage works on the crop list 1 leaves, with what setBlack() left in mRaw
      areas.clear();
      for (const BlackArea& a : img->blackAreas)
        areas.push_back({a.offset, a.size, a.isVertical ? 1 : 0, 0});
      rsx_scale_desc& s = d.scale;
      s.off_x = r1.crop_x;
      s.off_y = r1.crop_y;
      s.crop_x = r1.crop_w;
      s.crop_y = r1.crop_h;
      s.black_level = img->blackLevel;
      s.has_white = img->whitePoint.has_value() ? 1 : 0;
      s.white_point = img->whitePoint.value_or(0);
      s.has_separate = img->blackLevelSeparate.has_value() ? 1 : 0;
      if (img->blackLevelSeparate)
        std::copy_n(img->blackLevelSeparateStorage.begin(), 4, s.black_separate);
      s.n_areas = implicit_cast<uint32_t>(areas.size());
      s.areas = areas.empty() ? nullptr : areas.data();
      s.dither = img->mDitherScale ? 1 : 0;
      s.host_sse2 = host_sse2 ? 1 : 0;
    }
    const int st = rsx_dng_lossy_validate(&d, &v, &result, nullptr, 0);
    if (st != RSX_OK && !(st == RSX_ERR_UNSUPPORTED && result.list1.n_bad + result.list2.n_bad != 0))
      return false;
    const bool any_list = d.stage1.opcodes_bytes != 0 || d.has_list2;
    const uint64_t room = result.list1.n_bad + result.list2.n_bad +
                          (any_list && v.cpp == 1 ? 2U * DngPost::MaxConstantHits : 0U);
    bad.assign(implicit_cast<size_t>(std::min<uint64_t>(room, 1U << 26)), 0);
    // (re-checked against the room: fix with cpp > 1 and positions is refused here)
    return rsx_dng_lossy_validate(&d, &v, &result, bad.data(),
                                  implicit_cast<uint32_t>(bad.size())) == RSX_OK;
  }
  // the tile call; `status` per tile, written only when the image was
  int run(const std::vector<rsx_dng_jpeg_tile>& tiles, const RawImage& img, int32_t* status) {
    rsx_ctx* rsx = context();
    if (!rsx)
      return RSX_ERR_DEVICE;
    const rsx_image v = view(img);
    const uint32_t map_pitch = roundUp((implicit_cast<uint32_t>(v.dim_x) + 7U) / 8U, 16U);
    map.assign(d.fix ? size_t(map_pitch) * size_t(v.dim_y) : 0U, 0);
    return rsx_dng_lossy_decompress(rsx, implicit_cast<int>(tiles.size()), tiles.data(), &d, &v, status,
                                    &result, bad.empty() ? nullptr : bad.data(),
                                    implicit_cast<uint32_t>(bad.size()), map.empty() ? nullptr : map.data());
  }
  // the stages the call ran (RSX_OK, or RSX_ERR_UNSUPPORTED with result.stages != 0), behind
  // handleMetadata's own subFrames: the logged errors, the lists' TrimBounds as a subFrame, the
  // levels scaleBlackWhite() leaves, the positions.  True: the branch of :621-643 is done but for
  // its metadata tail (:635-642), which the hunk keeps.
  bool finish(const RawImage& img) const {
    if (!(result.stages & RSX_DNG_LOSSY_STAGE1))
      return false;
    const bool list2 = (result.stages & RSX_DNG_LOSSY_LIST2) != 0;
    if (result.list1.list_status != RSX_OK || (list2 && result.list2.list_status != RSX_OK))
      img->setError("rsx: DNG opcode list refused as the reference's parser refuses it");
    const rsx_dng_post_result& last = list2 ? result.list2 : result.list1;
    const iPoint2D off = img->getCropOffset();
    const iRectangle2D trimmed(last.crop_x - off.x, last.crop_y - off.y, last.crop_w, last.crop_h);
    if (!(trimmed.pos == iPoint2D(0, 0)) || !(trimmed.dim == img->dim))
      img->subFrame(trimmed);
    if (result.stages & RSX_DNG_LOSSY_SCALED) {
      img->blackLevel = result.scale.black_level;
      if (result.scale.estimated || img->whitePoint)
        img->whitePoint = result.scale.white_point;
    }
    const uint64_t n = result.list1.n_bad + (list2 ? result.list2.n_bad : 0U);
    if (n != 0 && n <= bad.size() && !(result.stages & RSX_DNG_LOSSY_FIXED)) {
      MutexLocker guard(&img->mBadPixelMutex);
      img->mBadPixelPositions.insert(img->mBadPixelPositions.begin(), bad.begin(),
                                     bad.begin() + implicit_cast<std::ptrdiff_t>(n));
    }
    return list2 || !d.has_list2;
  }
};

// status -> the exception the reference would have thrown
[[noreturn]] inline void raise(int st) {
  switch (st) {
  case RSX_ERR_IO:
    ThrowIOE("rsx: %s (out of bounds / truncated input)", rsx_status_string(st));
  case RSX_ERR_INPUT_OVERFLOW:
    ThrowIOE("Buffer overflow read in BitStreamer (rsx)");
  case RSX_ERR_BAD_HUFFMAN_CODE:
    ThrowRDE("bad Huffman code (rsx)");
  default:
    ThrowRDE("rsx: %s: %s", rsx_status_string(st), rsx_ctx_last_error(context()));
  }
}

// ---------------------------------------------------------------------------
// AbstractDngDecompressor::decompress(): ONE batched call for all tiles
// (INTEGRATION.md 4).  The reference's own fan-out (decompressThread<1> / <7>, an
// `omp for` over the tiles) runs unchanged, but while a batch is registered for the
// tiles' input ranges the per-tile hunks of UncompressedDecompressor /
// LJpegDecompressor RECORD their descriptor instead of decoding.  run() then hands
// all recorded tiles to rsx_dng_decompress_* in one call.  Tiles the device path did
// not finish (damaged stream, unsupported shape, no memory) are left to a second
// pass of the same fan-out in which the hunks of the finished tiles return at once
// and the others fall through to the original CPU code -- which decodes them, or
// throws exactly what the reference throws.
// ---------------------------------------------------------------------------
class DngBatch final {
public:
  struct Slot {
    int kind = 0; // 0 = not recorded, 1 = LJPEG scan, 2 = uncompressed strip
    rsx_dng_ljpeg_tile lj{};
    rsx_dng_unpack_tile up{};
    int32_t status = RSX_ERR_UNSUPPORTED;
    uint32_t consumed = 0;
  };
  struct Found {
    DngBatch* batch = nullptr;
    Slot* slot = nullptr;
  };

  DngBatch() = default;
  DngBatch(const DngBatch&) = delete;
  DngBatch& operator=(const DngBatch&) = delete;
  ~DngBatch() {
    std::unique_lock lock(registry().m);
    for (auto it = registry().ranges.begin(); it != registry().ranges.end();)
      it = it->second.batch == this ? registry().ranges.erase(it) : std::next(it);
  }

  // one tile: the bytes the reference hands to its per-tile decompressor
  void add(const uint8_t* begin, size_t size) {
    slots.emplace_back();
    pending.push_back({begin, size});
  }
  void registerTiles() {
    std::unique_lock lock(registry().m);
    for (size_t i = 0; i < pending.size(); ++i)
      registry().ranges[pending[i].first] = {pending[i].first + pending[i].second, this, &slots[i]};
  }
  // the batch (if any) whose tile holds `p`
  static Found find(const uint8_t* p) {
    std::shared_lock lock(registry().m);
    auto& r = registry().ranges;
    auto it = r.upper_bound(p);
    if (it == r.begin())
      return {};
    --it;
    if (p >= it->second.end)
      return {};
    return {it->second.batch, it->second.slot};
  }

  bool replaying = false;
  //  the stage behind the tiles, if DngDecoder hung one here: a batch of one
  // kind of tiles then takes the _post call -- decode, list, look-up, one download
  DngPost* post = nullptr;

  // true: every recorded tile is done; false: a second (CPU) pass is needed
  bool run(const rsx_image& img) {
    std::vector<rsx_dng_ljpeg_tile> lj;
    std::vector<rsx_dng_unpack_tile> up;
    std::vector<Slot*> ljs, ups;
    for (Slot& s : slots) {
      if (s.kind == 1) {
        lj.push_back(s.lj);
        ljs.push_back(&s);
      } else if (s.kind == 2) {
        up.push_back(s.up);
        ups.push_back(&s);
      }
    }
    bool all = true;
    const bool with_post = post && post->wanted() && (lj.empty() != up.empty()) &&
                           lj.size() + up.size() == slots.size();
    if (!lj.empty()) {
      std::vector<int32_t> st(lj.size(), RSX_ERR_DEVICE);
      std::vector<uint32_t> cons(lj.size(), 0);
      int post_rc = RSX_ERR_UNSUPPORTED;
      if (with_post) {
        post_rc = rsx_dng_decompress_ljpeg_post(
            context(), implicit_cast<int>(lj.size()), lj.data(), &post->d, &img, st.data(),
            cons.data(), &post->result, post->bad.empty() ? nullptr : post->bad.data(),
            implicit_cast<uint32_t>(post->bad.size()));
        post->applied = post_rc == RSX_OK;
      }
      // Only RSX_OK and RSX_ERR_TILE_ERRORS wrote the image and the statuses (the _post call was
      // then the whole decode, or the plain call).  Anything else -- a list or tiles the stage
      // refuses, a device failure, a position list past its room -- gets the plain call now, so
      // that no tile is ever marked done without its pixels in the caller's image.
      if (post_rc != RSX_OK && post_rc != RSX_ERR_TILE_ERRORS)
        (void)rsx_dng_decompress_ljpeg(context(), implicit_cast<int>(lj.size()), lj.data(), &img,
                                       st.data(), cons.data());
      for (size_t i = 0; i < ljs.size(); ++i) {
        ljs[i]->status = st[i];
        // LJpegDecoder's marker walk went on from the end of the scan (endOfScan()).  A
        // tile decoded to its full height must have stopped exactly there.  A
        // bottom-overhanging tile stops earlier; that makes no difference to the walk
        // unless there are restart markers left in between, which the reference trips
        // over.  Anything else is redone by the original code.
        const rsx_ljpeg_desc& d = lj[i].desc;
        const bool dri = d.rows_per_restart_interval < d.frame_h;
        const bool full = d.tile_h >= d.frame_h * d.mcu_h;
        if (st[i] == RSX_OK && cons[i] != ljs[i]->consumed && (full || dri))
          ljs[i]->status = RSX_ERR_UNSUPPORTED;
        all = done(ljs[i]->status) && all;
      }
    }
    if (!up.empty()) {
      std::vector<int32_t> st(up.size(), RSX_ERR_DEVICE);
      int post_rc = RSX_ERR_UNSUPPORTED;
      if (with_post) {
        post_rc = rsx_dng_decompress_uncompressed_post(
            context(), implicit_cast<int>(up.size()), up.data(), &post->d, &img, st.data(),
            &post->result, post->bad.empty() ? nullptr : post->bad.data(),
            implicit_cast<uint32_t>(post->bad.size()));
        post->applied = post_rc == RSX_OK;
      }
      if (post_rc != RSX_OK && post_rc != RSX_ERR_TILE_ERRORS) // (as above)
        (void)rsx_dng_decompress_uncompressed(context(), implicit_cast<int>(up.size()), up.data(),
                                              &img, st.data());
      for (size_t i = 0; i < ups.size(); ++i) {
        ups[i]->status = st[i];
        all = done(st[i]) && all;
      }
    }
    return all;
  }

  // Offset of the marker that ends the entropy-coded segment [p, p + n) -- the first
  // FF xx with xx neither 00 (a stuffed FF) nor D0..D7 (RSTn); n if there is none.
  // A tile that is decoded to its full height ends ON that marker, and in a well-formed
  // tile it is the last thing in the buffer: it is looked for from the end (a few bytes)
  // and run() checks the guess against what the decode reports -- a stream with an
  // earlier marker is redone by the original code.  A bottom-overhanging tile stops
  // before the marker, nothing checks the guess then, so it is searched from the front.
  static uint32_t endOfScan(const uint8_t* p, size_t n, bool full_height) {
    auto is_end = [&](size_t i) {
      // (FF FF is fill, not a marker: AbstractLJpegDecoder's peekMarker does not take it)
      return p[i] == 0xFF && p[i + 1] != 0x00 && p[i + 1] != 0xFF &&
             (p[i + 1] < 0xD0 || p[i + 1] > 0xD7);
    };
    if (full_height) {
      for (size_t i = n; i >= 2; --i)
        if (is_end(i - 2))
          return implicit_cast<uint32_t>(i - 2);
      return implicit_cast<uint32_t>(n);
    }
    const uint8_t* q = p;
    const uint8_t* const last = p + (n ? n - 1 : 0);
    while (q < last) {
      q = static_cast<const uint8_t*>(std::memchr(q, 0xFF, size_t(last - q)));
      if (!q)
        break;
      if (is_end(size_t(q - p)))
        return implicit_cast<uint32_t>(q - p);
      ++q;
    }
    return implicit_cast<uint32_t>(n);
  }

private:
  struct Range {
    const uint8_t* end;
    DngBatch* batch;
    Slot* slot;
  };
  struct Registry {
    std::shared_mutex m;
    std::map<const uint8_t*, Range> ranges;
  };
  static Registry& registry() {
    static Registry r;
    return r;
  }
  std::vector<Slot> slots;
  std::vector<std::pair<const uint8_t*, size_t>> pending;
};

// DHT payload of a borrowed decoder -> rsx_huff_table
inline rsx_huff_table table(const PrefixCodeDecoder<>& ht) {
  rsx_huff_table t{};
  const auto& n = ht.code.nCodesPerLength; // index = code length
  for (size_t l = 1; l < n.size() && l <= 16; ++l)
    t.n_codes_per_length[l - 1] = implicit_cast<uint8_t>(n[l]);
  const auto& v = ht.code.codeValues;
  for (size_t i = 0; i < v.size() && i < RSX_MAX_CODE_VALUES; ++i)
    t.code_values[i] = v[i];
  t.n_code_values = implicit_cast<uint8_t>(v.size());
  t.fix_dng_bug16 = ht.handleDNGBug16() ? 1 : 0;
  return t;
}

// recipes -> (tables[], table_index[], init_pred[]), de-duplicating by address
// the way AbstractLJpegDecoder already de-duplicates by content
// (AbstractLJpegDecoder.cpp:258-263)
template <typename Recipe, typename Desc>
inline void recipes(const std::vector<Recipe>& rec, Desc* d) {
  std::vector<const PrefixCodeDecoder<>*> seen;
  d->n_tables = 0;
  for (size_t c = 0; c < rec.size() && c < RSX_MAX_COMPONENTS; ++c) {
    const PrefixCodeDecoder<>* p = &rec[c].ht;
    size_t k = 0;
    while (k < seen.size() && seen[k] != p)
      ++k;
    if (k == seen.size()) {
      seen.push_back(p);
      d->tables[d->n_tables++] = table(*p);
    }
    d->table_index[c] = implicit_cast<uint8_t>(k);
    d->init_pred[c] = rec[c].initPred;
  }
}

} // namespace rawspeed::rsx_shim
