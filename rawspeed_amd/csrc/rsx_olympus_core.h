// OlympusDecompressor (include/rsx.h section 3v), shared by the kernels of rsx_olympus.hip and by
// a host build (rsx_olympus_host.cpp): the constructor's checks
// (decompressors/OlympusDecompressor.cpp:218-227), the MSB reader as this codec drives it with its
// over-read rule, one symbol of getDiff (:61-97) and getPred (:130-164).
//
// The codec is cut the way the device runs it.  The walk through the bits needs no pixel: its
// state is the bit position and, per column parity, carry[0] and carry[2]; carry[1] feeds only
// the difference.  A pixel is uint16(pred + diff), so the difference is kept mod 2^16, in the
// place of the pixel it becomes; the reconstruction turns differences into pixels in place.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "rsx.h"

#if defined(__HIPCC__)
#define RSX_OL_FN __host__ __device__ __forceinline__
#else
#define RSX_OL_FN inline
#endif

namespace rsx_olympus {

constexpr int32_t MAX_X = 10400, MAX_Y = 7792;
constexpr uint32_t SKIP = 7; // skipBytes(7) in front of the bit stream (:209)

// The constructor's checks in its order, then the pitch.
inline int validate_image(const rsx_image* img) {
  if (!img)
    return RSX_ERR_INVALID_ARG;
  if (img->cpp != 1) // "Unexpected component count / data type" (an rsx_image is UINT16)
    return RSX_ERR_INVALID_ARG;
  if (img->dim_x <= 0 || img->dim_y <= 0 || img->dim_x % 2 != 0 || img->dim_y % 2 != 0 ||
      img->dim_x > MAX_X || img->dim_y > MAX_Y) // "Unexpected image dimensions found"
    return RSX_ERR_INVALID_ARG;
  if (img->pitch_bytes < uint32_t(img->dim_x) * 2u)
    return RSX_ERR_INVALID_ARG;
  return RSX_OK;
}

// What the reader refuses before the first bit: skipBytes(7), and BitStreamerMSB over less than
// MaxProcessBytes (BitStreamer.h:58-59).
inline int check_input(uint64_t in_bytes) {
  if (in_bytes < SKIP)
    return RSX_ERR_IO;
  if (in_bytes - SKIP < 4)
    return RSX_ERR_IO;
  return RSX_OK;
}

inline int validate(uint64_t in_bytes, const rsx_image* img) {
  if (int st = validate_image(img))
    return st;
  return check_input(in_bytes);
}

// ---------------------------------------------------------------------------------------------
// BitStreamerMSB as this codec drives it: one fill(32) in front of every symbol, and a symbol
// takes at most 31 bits.  With c bits consumed and k words loaded the cache holds level =
// 32 k - c bits; a fill loads word k iff level < 32.  Behind a fill level is 32..63 and behind the
// symbol at least 1, so the word a fill loads is k = ceil(c / 32), and it loads iff c == 0 or c
// is no multiple of 32.  The load throws iff 4 k > size + 8 (BitStreamer.h:125-127).  Where no
// load happens, word c / 32 went through the same test at an earlier fill, and the test is
// monotone, so: a fill at c fails iff 4 ceil(c / 32) > size + 8, i.e. iff c > fill_limit(size).
// Bytes behind the stream read as zero.
// ---------------------------------------------------------------------------------------------
RSX_OL_FN uint64_t fill_limit(uint64_t size) { return 32ull * ((size + 8u) / 4u); }

// The reader with the reference's bookkeeping (the host build and the model's cross-check run it;
// the kernel walks by bit position and fill_limit alone).  Src::word(k): bytes 4 k .. 4 k + 3 of
// the stream as a big-endian word, zero behind its end.
template <class Src>
struct Bits {
  const Src* src;
  uint64_t size;
  uint64_t buf; // the cache, left-aligned
  int32_t level;
  uint64_t k; // words loaded
  RSX_OL_FN void init(const Src* s, uint64_t bytes) {
    src = s;
    size = bytes;
    buf = 0;
    level = 0;
    k = 0;
  }
  RSX_OL_FN uint64_t consumed() const { return 32ull * k - uint64_t(level); }
  // false: the refill lies more than 8 bytes behind the stream
  RSX_OL_FN bool fill() {
    if (level >= 32)
      return true;
    if (4ull * k > size + 8u)
      return false;
    buf |= uint64_t(src->word(k)) << (32 - level);
    level += 32;
    ++k;
    return true;
  }
  RSX_OL_FN uint32_t peek32() const { return uint32_t(buf >> 32); }
  RSX_OL_FN void skip(int32_t n) {
    buf <<= n;
    level -= n;
  }
};

// One column parity's OlympusDifferenceDecoder: carry[0..2]
struct Carry {
  int32_t c0, c1, c2;
};

RSX_OL_FN int32_t active_bits16(uint32_t v) { // numActiveBits(uint16_t), without a branch
  return 31 - __builtin_clz((v & 0xFFFFu) << 1 | 1u);
}

RSX_OL_FN int32_t num_low_bits(const Carry& s) {
  const int32_t bias = s.c2 < 3 ? 2 : 0;
  const int32_t n = active_bits16(uint32_t(s.c0)) - bias; // (implicit_cast<uint16_t>: truncation)
  return n > 2 + bias ? n : 2 + bias;
}

// One symbol (getDiff behind its fill): `window` holds the next 32 bits of the stream, the first
// one in bit 31.  Returns the bits taken (at most 31), updates the carries, *diff = the value
// getDiff returns.  Both forms are computed and one is selected: on the device the walk is a chain
// of scalar instructions, and a select costs it less than a branch.
RSX_OL_FN int32_t symbol(Carry& s, uint32_t window, int32_t* diff) {
  const int32_t nlow = num_low_bits(s);
  const uint32_t b = window >> 17; // peek(15)
  const int32_t sign = -int32_t(b >> 14);
  const int32_t low = int32_t(b >> 12) & 3;
  // leading zeros of the low 12 bits; 12 for none set (the bit behind them stands in)
  const int32_t nlz = __builtin_clz((b & 4095u) << 20 | 1u << 19);
  const bool escape = nlz == 12;
  // escape form: 15 bits, 15 - nlow bits of high (1..13), one bit skipped
  const int32_t high_e = int32_t((window >> (2 + nlow)) & ((1u << (15 - nlow)) - 1u));
  const int32_t high = escape ? high_e : nlz;
  const int32_t used = (escape ? 31 - nlow : nlz + 4) + nlow; // (at most 31)
  const int32_t field = int32_t((window >> (32 - used)) & ((1u << nlow) - 1u));
  s.c0 = (high << nlow) | field;
  const int32_t d = (s.c0 ^ sign) + s.c1;
  s.c1 = (d * 3 + s.c1) >> 5; // (arithmetic)
  s.c2 = s.c0 > 16 ? 0 : s.c2 + 1;
  *diff = int32_t(uint32_t(d) * 4u) | low;
  return used;
}

// getPred for a pixel that has all three neighbours (row >= 2 and col >= 2)
RSX_OL_FN int32_t pred_inner(int32_t left, int32_t up, int32_t nw) {
  const int32_t a = left - nw, b = up - nw;
  const int32_t aa = a < 0 ? -a : a, ab = b < 0 ? -b : b;
  if (((a < 0) != (b < 0)) && a != 0 && b != 0)
    return (aa > 32 || ab > 32) ? left + b : (left + up) >> 1;
  return aa > ab ? left : up;
}

// getPred in plane coordinates: cell (i, j) of one of the four Bayer planes
RSX_OL_FN int32_t pred(int32_t i, int32_t j, int32_t left, int32_t up, int32_t nw) {
  if (i == 0)
    return j == 0 ? 0 : left;
  if (j == 0)
    return up;
  return pred_inner(left, up, nw);
}

} // namespace rsx_olympus
