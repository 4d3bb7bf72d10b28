// KodakDecompressor (include/rsx.h section 3w), shared by the kernels of rsx_kodak.hip and by a
// host build (rsx_kodak_host.cpp): the constructor's checks (decompressors/KodakDecompressor.cpp:
// 46-65), the closed forms of a segment's size, one pixel's field and its extension (:67-118), the
// range check and the table (:120-150, common/RawImage.h:335-353).
//
// The codec is cut the way the device runs it.  A segment's size is a closed form of the sum of
// its lengths, so "where does the segment behind this one start" is a function of the offset
// alone -- a map over the stream's even offsets -- and the only serial part of the format, the
// segments' starts, comes out of composing such maps.  Inside a segment every field is addressed
// from a prefix sum of the lengths, and the two predictors are two running sums.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "rsx.h"

#if defined(__HIPCC__)
#define RSX_KD_FN __host__ __device__ __forceinline__
#else
#define RSX_KD_FN inline
#endif

namespace rsx_kodak {

constexpr int32_t MAX_X = 4516, MAX_Y = 3012;
constexpr int32_t SEGMENT = 256; // segment_size

// The descriptor's own checks, then the constructor's in its order, then the pitch and
// input.check(area / 2).
inline int validate(const rsx_kodak_desc* desc, const rsx_image* img, uint64_t in_bytes) {
  if (!desc || !img)
    return RSX_ERR_INVALID_ARG;
  if (desc->table_mode != RSX_KODAK_TABLE_NONE && desc->table_mode != RSX_KODAK_TABLE_PLAIN &&
      desc->table_mode != RSX_KODAK_TABLE_DITHER)
    return RSX_ERR_INVALID_ARG;
  if (desc->table_mode != RSX_KODAK_TABLE_NONE && !desc->table)
    return RSX_ERR_INVALID_ARG;
  if (img->cpp != 1) // "Unexpected component count / data type" (an rsx_image is UINT16)
    return RSX_ERR_INVALID_ARG;
  if (img->dim_x <= 0 || img->dim_y <= 0 || img->dim_x % 4 != 0 || img->dim_x > MAX_X ||
      img->dim_y > MAX_Y) // "Unexpected image dimensions found"
    return RSX_ERR_INVALID_ARG;
  if (desc->bps != 10 && desc->bps != 12) // "Unexpected bits per sample"
    return RSX_ERR_INVALID_ARG;
  if (img->pitch_bytes < uint32_t(img->dim_x) * 2u)
    return RSX_ERR_INVALID_ARG;
  if (in_bytes < uint64_t(img->dim_x) * uint64_t(img->dim_y) / 2u)
    return RSX_ERR_IO;
  return RSX_OK;
}

// entries of TableLookUp::tables a mode reads
RSX_KD_FN uint32_t table_entries(int32_t bps, int32_t mode) {
  return mode == RSX_KODAK_TABLE_NONE ? 0u : (mode == RSX_KODAK_TABLE_DITHER ? 2u : 1u) << bps;
}

// ---------------------------------------------------------------------------------------------
// A segment of `len` pixels (a multiple of 4, at most 256) whose lengths sum to `sum`: the reader
// holds init bits up front and takes 32 more only when it holds fewer than the next length, so it
// never holds 32 spare ones: r = ceil(max(0, sum - init) / 32) reads of 4 bytes.
// ---------------------------------------------------------------------------------------------
RSX_KD_FN uint32_t init_bits(uint32_t len) { return (len & 7u) == 4u ? 16u : 0u; }

RSX_KD_FN uint32_t segment_bytes(uint32_t len, uint32_t sum) {
  const uint32_t init = init_bits(len);
  const uint32_t over = sum > init ? sum - init : 0u;
  return len / 2u + init / 8u + 4u * ((over + 31u) / 32u);
}

// the most a segment of `len` pixels takes (every length 15, the up-front unit counted whether it
// is there or not)
RSX_KD_FN uint32_t segment_bound(uint32_t len) { return len / 2u + 2u + 4u * ((15u * len + 31u) / 32u); }

// the most an image takes
RSX_KD_FN uint64_t image_bound(int32_t dim_x, int32_t dim_y) {
  const uint32_t n = uint32_t(dim_x) / uint32_t(SEGMENT), t = uint32_t(dim_x) % uint32_t(SEGMENT);
  const uint64_t row = uint64_t(n) * segment_bound(uint32_t(SEGMENT)) + (t ? segment_bound(t) : 0u);
  return row * uint64_t(dim_y);
}

// sum of the two lengths a byte holds
RSX_KD_FN uint32_t nibble_sum(uint32_t byte) { return (byte & 15u) + (byte >> 4); }

// Pixel i's field: `cum` bits lie in front of it, `n` is its length (0..15), `area` the bit area
// (behind the lengths).  Bit p of the concatenation is bit p % 16 of the big-endian unit at byte
// 2 (p / 16); a field straddles at most two units.
RSX_KD_FN uint32_t unit_at(const uint8_t* area, uint32_t u) {
  return uint32_t(area[2u * u]) << 8 | uint32_t(area[2u * u + 1u]);
}

RSX_KD_FN uint32_t field_at(const uint8_t* area, uint32_t cum, uint32_t n) {
  if (n == 0)
    return 0;
  const uint32_t u = cum >> 4, sh = cum & 15u;
  uint32_t bits = unit_at(area, u);
  if (sh + n > 16u)
    bits |= unit_at(area, u + 1u) << 16;
  return (bits >> sh) & ((1u << n) - 1u);
}

// PrefixCodeDecoder<>::extend (JPEG figure F.12); 0 for a length of 0
RSX_KD_FN int32_t extend(uint32_t field, uint32_t n) {
  if (n == 0)
    return 0;
  return (field & (1u << (n - 1u))) ? int32_t(field) : int32_t(field) - int32_t((1u << n) - 1u);
}

// !isIntN(value, bps): "Value out of bounds"
RSX_KD_FN bool out_of_range(int32_t value, int32_t bps) { return (uint32_t(value) >> bps) != 0u; }

// setWithLookUp with the generator at 0: `table` as TableLookUp holds it
RSX_KD_FN uint16_t store_value(int32_t value, int32_t mode, const uint16_t* table) {
  if (mode == RSX_KODAK_TABLE_NONE)
    return uint16_t(value);
  return table[mode == RSX_KODAK_TABLE_DITHER ? 2 * value : value];
}

} // namespace rsx_kodak
