// CrwDecompressor (include/rsx.h section 3x), shared by the kernels of rsx_crw.hip and by a host
// build (rsx_crw_host.cpp): the six tables of the format (rsx_crw_tables.h), the constructor's checks
// (decompressors/CrwDecompressor.cpp:46-72), the reader's rules as closed forms of positions
// (bitstreams/BitStreamerJPEG.h:106-183, BitStreamer.h:100-132,216-229), one symbol of decodeBlock
// (:167-207) and the per-pixel arithmetic of decompress() (:210-286).
//
// The codec is cut the way the device runs it.  The scan is taken as its un-stuffed form: the data
// bytes in front of the first marker, zeros behind them for ever.  A parser's state is only (bit
// position, coefficient index), so a symbol is a function of the next 32 bits and the index, and
// the reader's two failures are thresholds on the bit position a symbol starts at:
//
//  * fill(32) in front of a symbol that starts at consumed bit c has fetched 4 (ceil(c / 32) + 1)
//    data bytes, in fills of 4; fill k (from 0) happens at the first symbol start c > 32 (k - 1).
//  * no marker: with `size` raw bytes that hold N data bytes and end at raw position R (size, or
//    size + 1 when the last byte is an FF, which the zero padding turns into FF 00), fill k starts
//    at raw position R + 4 k - N once 4 k >= N and throws when that is above size + 16: the first
//    symbol start c > 32 floor((size + 16 + N - R) / 4) is "Buffer overflow read".
//  * a marker behind M data bytes is met by fill km = floor(M / 4), at the first symbol start
//    cm > 32 (km - 1).  That fill leaves 64 bits in the cache (the data in front of the marker,
//    then zeros) and the position at size + 1..4, so four more fills of zeros pass and the fifth,
//    at the first symbol start c > cm + 160, throws.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "rsx.h"
#include "rsx_crw_tables.h"

#if defined(__HIPCC__)
#define RSX_CRW_FN __host__ __device__ __forceinline__
#else
#define RSX_CRW_FN inline
#endif

namespace rsx_crw {

constexpr int32_t MAX_X = 4104, MAX_Y = 3048;
constexpr uint32_t MIN_INPUT = 8;     // BitStreamerJPEG's MaxProcessBytes
constexpr uint32_t N_FIRST = RSX_CRW_N_FIRST, N_SECOND = RSX_CRW_N_SECOND;
constexpr uint32_t NO_THRESHOLD = 0xFFFFFFFFu;

// The constructor's checks in its order, then the pitch; `in_bytes` last (the reader's own
// requirement, which the reference meets when decompress() opens the stream).
inline int validate(const rsx_crw_desc* desc, const rsx_image* img, uint64_t in_bytes,
                    uint64_t low_bytes) {
  if (!desc || !img)
    return RSX_ERR_INVALID_ARG;
  if (img->cpp != 1) // "Unexpected component count / data type" (an rsx_image is UINT16)
    return RSX_ERR_INVALID_ARG;
  if (img->dim_x <= 0 || img->dim_y <= 0 || img->dim_x % 4 != 0 || img->dim_x > MAX_X ||
      img->dim_y > MAX_Y || (uint32_t(img->dim_x) * uint32_t(img->dim_y)) % 64u != 0)
    return RSX_ERR_INVALID_ARG; // "Unexpected image dimensions found"
  if (desc->dec_table > 2u) // "Wrong table number" (initHuffTables runs in the member initialisers,
    return RSX_ERR_INVALID_ARG; // in front of the body; every one of these is INVALID_ARG)
  if (desc->has_lowbits != 0 && low_bytes < uint64_t(img->dim_x) * uint64_t(img->dim_y) / 4u)
    return RSX_ERR_INVALID_ARG; // "Unsufficient number of low bit blocks"
  if (img->pitch_bytes < uint32_t(img->dim_x) * 2u)
    return RSX_ERR_INVALID_ARG;
  if (in_bytes < MIN_INPUT)
    return RSX_ERR_IO;
  return RSX_OK;
}

// the most a frame's scan takes: 64 symbols a block, 31 bits a symbol, every byte stuffed, and
// the marker's two bytes
RSX_CRW_FN uint64_t image_bound(int32_t dim_x, int32_t dim_y) {
  return uint64_t(dim_x) * uint64_t(dim_y) / 64u * 496u + 2u;
}

// ---------------------------------------------------------------------------------------------
// The two canonical codes of a table number, as the decoder uses them: per length the first
// code, the number of codes and the index of the first one's value.
// ---------------------------------------------------------------------------------------------
struct Tables {
  uint16_t first[2][17];
  uint16_t count[2][17];
  uint16_t base[2][17];
  uint8_t values[2][N_SECOND];
};

inline void build_tables(uint32_t table, Tables* t) {
  for (int tree = 0; tree < 2; ++tree) {
    const uint8_t* ncpl = tree ? RSX_CRW_SECOND_NCPL[table] : RSX_CRW_FIRST_NCPL[table];
    const uint8_t* values = tree ? RSX_CRW_SECOND_VALUES[table] : RSX_CRW_FIRST_VALUES[table];
    const uint32_t n = tree ? N_SECOND : N_FIRST;
    uint32_t code = 0, at = 0;
    t->first[tree][0] = t->count[tree][0] = t->base[tree][0] = 0;
    for (int len = 1; len <= 16; ++len) {
      t->first[tree][len] = uint16_t(code);
      t->count[tree][len] = ncpl[len - 1];
      t->base[tree][len] = uint16_t(at);
      code = (code + ncpl[len - 1]) << 1;
      at += ncpl[len - 1];
    }
    for (uint32_t k = 0; k < N_SECOND; ++k)
      t->values[tree][k] = k < n ? values[k] : 0;
  }
}

// ---------------------------------------------------------------------------------------------
// One symbol.  `w` holds the next 32 bits, the first one in bit 31; i is the coefficient index,
// 0 at a block's start.  used == 0: no code of the tree is a prefix of the bits ("bad Huffman
// code"; the second trees are not complete).  Otherwise `used` bits are consumed (at most 31),
// the index becomes `next` (0: the block has ended), and if at >= 0 coefficient `at` is `diff`.
// ---------------------------------------------------------------------------------------------
struct Symbol {
  uint32_t used;
  int32_t next;
  int32_t at;
  int32_t diff;
};

// PrefixCodeDecoder<>::extend (JPEG figure F.12)
RSX_CRW_FN int32_t extend(uint32_t field, uint32_t n) {
  return (field & (1u << (n - 1u))) ? int32_t(field) : int32_t(field) - int32_t((1u << n) - 1u);
}

RSX_CRW_FN Symbol symbol(const Tables* t, uint32_t w, int32_t i) {
  const int tree = i > 0;
  const uint32_t top = w >> 16;
  Symbol s;
  s.used = 0;
  s.next = 0;
  s.at = -1;
  s.diff = 0;
  uint32_t cv = 0, clen = 0;
#pragma unroll 1
  for (uint32_t len = 1; len <= 16; ++len) {
    const uint32_t k = (top >> (16u - len)) - t->first[tree][len];
    if (k < t->count[tree][len]) {
      cv = t->values[tree][t->base[tree][len] + k];
      clen = len;
      break;
    }
  }
  if (clen == 0)
    return s;
  const uint32_t len = cv & 15u;
  s.used = clen;
  if (cv == 0 && i > 0)
    return s; // end of block
  if (cv == 0xffu) {
    ++i;
  } else {
    i += int32_t(cv >> 4);
    if (len != 0) {
      // (getBitsNoFill(len) is consumed whether or not the run has passed coefficient 63)
      const uint32_t field = (w << clen) >> (32u - len);
      s.used = clen + len;
      if (i < 64) {
        s.at = i;
        s.diff = extend(field, len);
      }
    }
    ++i;
  }
  s.next = i >= 64 ? 0 : i;
  return s;
}

// ---------------------------------------------------------------------------------------------
// The reader's overflow as thresholds (the closed forms at the top): a symbol that starts at a
// consumed bit above the threshold fails with "Buffer overflow read in BitStreamer".
// ---------------------------------------------------------------------------------------------
// no marker in `size` raw bytes that hold n_data data bytes; ends_ff: the last raw byte is an FF
RSX_CRW_FN uint32_t overflow_threshold(uint32_t size, uint32_t n_data, bool ends_ff) {
  return 32u * ((size + 16u + n_data - (size + (ends_ff ? 1u : 0u))) / 4u);
}
// a marker behind m data bytes: the fill that meets it is taken at the first symbol start above
// this (below 0: at the stream's first symbol) ...
RSX_CRW_FN int64_t marker_fill_threshold(uint32_t m) { return 32 * (int64_t(m / 4u) - 1); }
// ... and with that symbol start cm the overflow is the first symbol start above this
RSX_CRW_FN uint32_t marker_overflow_threshold(uint32_t cm) { return cm + 160u; }

// ---------------------------------------------------------------------------------------------
// Pixels
// ---------------------------------------------------------------------------------------------
// !isIntN(value, 10): "Error decompressing"
RSX_CRW_FN bool out_of_range(int32_t value) { return (uint32_t(value) >> 10) != 0u; }

// pixel << 2 | the pixel's two low bits (byte `c` holds four pixels, the first in bits 0..1)
RSX_CRW_FN uint16_t merge_low(uint32_t value, uint32_t c, uint32_t p, int32_t dim_x) {
  uint32_t v = (value << 2) | ((c >> (2u * p)) & 3u);
  if (dim_x == 2672 && v < 512u)
    v += 2u; // ("No idea why this is needed")
  return uint16_t(v);
}

} // namespace rsx_crw
