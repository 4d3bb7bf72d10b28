// RawImageData::fixBadPixels (include/rsx.h section 5), shared by the kernels of
// rsx_bad_pixels.hip and by a host build (rsx_bad_pixels_host.cpp): the geometry of the bad-pixel
// map, the validation of a call, the search for the nearest good pixel and the two interpolations
// (common/RawImage.cpp:201-239, 297-323, common/RawImageDataU16.cpp:399-485,
// common/RawImageDataFloat.cpp:177-260).
//
// The map.  createBadPixelMap makes rows of roundUp(ceil(w / 8), 16) bytes, bit x & 7 of byte
// x >> 3.  A row therefore is a whole number of little-endian 64-bit words, bit x & 63 of word
// x >> 6: the ROW MAP here is the reference's map, byte for byte.  The COLUMN MAP holds the same
// bits the other way round -- column x is ceil(h / 64) words, bit y & 63 of word y >> 6 -- so that
// a walk up or down a column reads words as a walk along a row does.
//
// The search.  fixBadPixel steps one pixel (two under a CFA) at a time until it stands on a pixel
// that is inside the image and not marked.  Here the unmarked bits of a word, masked to the
// pixel's parity under a CFA (64 is even: one mask serves every word of a line) and to the side
// of the pixel, answer with one count of leading or trailing zeros; a run of marked pixels costs
// its length / 64 words.
//
// The interpolation is the reference's, quirks included: a direction without a good pixel has the
// distance 0, and an axis on which only ONE side was found gives that side the weight 0 (its
// distance is the whole total) and the missing side all of it -- the axis then contributes
// nothing but still raises the shift (uint16) or the divisor (F32).  In binary32 every operation
// is rounded on its own: this header turns contraction off for the translation unit that includes
// it (hipcc fuses a multiply and an add by default, through the round-to-nearest intrinsics as
// well once they are inlined), the host build is compiled with -ffp-contract=off; division is the
// correctly rounded one on both.  The one value that differs between processors is the NaN an
// invalid operation makes (+inf times the weight 0): the reference's result on x86-64, where the
// recorded answers come from, is the default NaN with the sign bit set; a NaN result is stored as
// that pattern.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "rsx.h"

#if defined(__HIPCC__)
#define RSX_BP_FN __host__ __device__ __forceinline__
#else
#define RSX_BP_FN inline
#endif

namespace rsx_bp {

#if defined(__HIPCC__)
#pragma clang fp contract(off)
#endif
RSX_BP_FN float f_add(float a, float b) { return a + b; }
RSX_BP_FN float f_sub(float a, float b) { return a - b; }
RSX_BP_FN float f_mul(float a, float b) { return a * b; }
RSX_BP_FN float f_div(float a, float b) { return a / b; }
#if defined(__HIP_DEVICE_COMPILE__)
RSX_BP_FN int clz64(uint64_t v) { return __clzll(static_cast<long long>(v)); }
RSX_BP_FN int ctz64(uint64_t v) { return __ffsll(static_cast<unsigned long long>(v)) - 1; }
RSX_BP_FN int popc64(uint64_t v) { return __popcll(v); }
#else
RSX_BP_FN int clz64(uint64_t v) { return __builtin_clzll(v); }
RSX_BP_FN int ctz64(uint64_t v) { return __builtin_ctzll(v); }
RSX_BP_FN int popc64(uint64_t v) { return __builtin_popcountll(v); }
#endif

constexpr uint32_t NAN_X86 = 0xFFC00000u;
constexpr int32_t MAX_DIM = 65536; // a position holds 16 bits of x and of y

// createBadPixelMap's pitch in bytes
RSX_BP_FN uint32_t map_pitch(uint32_t w) { return ((w + 7u) / 8u + 15u) / 16u * 16u; }

// The geometry of one image as the lanes see it.
struct Geo {
  uint32_t w, h;
  uint32_t pitch;   // image bytes a row
  uint32_t wpr;     // words a row of the row map: map_pitch / 8
  uint32_t wpc;     // words a column of the column map: ceil(h / 64)
  uint32_t step;    // 2 under a CFA, else 1
  uint32_t is_f32;
  uint32_t fix_end; // fixBadPixelsThread scans (w + 15) / 32 blocks of 32: pixels below this x
};

RSX_BP_FN Geo make_geo(uint32_t w, uint32_t h, uint32_t pitch, bool cfa, bool f32) {
  Geo g;
  g.w = w;
  g.h = h;
  g.pitch = pitch;
  g.wpr = map_pitch(w) / 8u;
  g.wpc = (h + 63u) / 64u;
  g.step = cfa ? 2u : 1u;
  g.is_f32 = f32 ? 1u : 0u;
  g.fix_end = (w + 15u) / 32u * 32u;
  return g;
}

// the checks of a call on its image alone (rsx_bad_pixels_validate's first three groups)
inline int validate_image(const rsx_image* img, bool is_f32) {
  if (!img)
    return RSX_ERR_INVALID_ARG;
  const uint32_t ss = is_f32 ? 4u : 2u;
  if (img->cpp < 1 || img->dim_x <= 0 || img->dim_y <= 0)
    return RSX_ERR_INVALID_ARG;
  if (uint64_t(img->pitch_bytes) < uint64_t(img->dim_x) * uint64_t(img->cpp) * ss ||
      img->pitch_bytes % ss != 0)
    return RSX_ERR_INVALID_ARG;
  if (img->cpp > 1)
    return RSX_ERR_UNSUPPORTED; // (the reference's own cpp > 1 path races with itself: rsx.h)
  if (img->dim_x > MAX_DIM || img->dim_y > MAX_DIM)
    return RSX_ERR_UNSUPPORTED;
  return RSX_OK;
}

// a map handed in: its pitch, and no bit outside the image (the padding of a row included)
inline int validate_map(const uint8_t* map, uint32_t pitch, uint32_t w, uint32_t h) {
  if (pitch != map_pitch(w))
    return RSX_ERR_INVALID_ARG;
  for (uint32_t y = 0; y < h; ++y) {
    const uint8_t* row = map + size_t(y) * pitch;
    for (uint32_t b = w / 8u; b < pitch; ++b) {
      const uint32_t keep = b == w / 8u ? (1u << (w & 7u)) - 1u : 0u;
      if (row[b] & ~keep)
        return RSX_ERR_INVALID_ARG;
    }
  }
  return RSX_OK;
}

inline int validate(const rsx_bad_pixels_desc* desc, const rsx_image* img) {
  if (!desc || !img)
    return RSX_ERR_INVALID_ARG;
  if (!desc->positions && desc->n_positions != 0)
    return RSX_ERR_INVALID_ARG;
  if (int st = validate_image(img, desc->is_f32 != 0))
    return st;
  const uint32_t w = uint32_t(img->dim_x), h = uint32_t(img->dim_y);
  if (desc->map_in || desc->map_out || desc->map_pitch != 0)
    if (desc->map_pitch != map_pitch(w))
      return RSX_ERR_INVALID_ARG;
  for (uint32_t i = 0; i < desc->n_positions; ++i) {
    const uint32_t p = desc->positions[i];
    if ((p & 0xFFFFu) >= w || (p >> 16) >= h)
      return RSX_ERR_INVALID_ARG;
  }
  if (desc->map_in)
    if (int st = validate_map(desc->map_in, desc->map_pitch, w, h))
      return st;
  return RSX_OK;
}

// the parity mask of a walk from position p: every bit, or the bits of p's parity
RSX_BP_FN uint64_t parity_mask(uint32_t p, uint32_t step) {
  return step == 1u ? ~0ull : 0x5555555555555555ull << (p & 1u);
}

// The nearest unmarked position below p on a line of n bits (its words at `line`) among those
// `par` admits; -1 if there is none.
RSX_BP_FN int find_below(const uint64_t* line, uint32_t p, uint64_t par) {
  uint32_t wi = p >> 6;
  uint64_t m = ~line[wi] & par & ((1ull << (p & 63u)) - 1ull);
  for (;;) {
    if (m)
      return int(wi * 64u) + 63 - clz64(m);
    if (wi == 0u)
      return -1;
    --wi;
    m = ~line[wi] & par;
  }
}

// ... above p (positions n and up do not exist; their bits are not marked)
RSX_BP_FN int find_above(const uint64_t* line, uint32_t n, uint32_t p, uint64_t par) {
  const uint32_t last = (n - 1u) >> 6;
  const uint64_t last_mask = (n & 63u) ? (1ull << (n & 63u)) - 1ull : ~0ull;
  uint32_t wi = p >> 6;
  uint64_t m = ~line[wi] & par & ((p & 63u) == 63u ? 0ull : ~0ull << ((p & 63u) + 1u));
  for (;;) {
    if (wi == last)
      m &= last_mask;
    if (m)
      return int(wi * 64u) + ctz64(m);
    if (wi == last)
      return -1;
    ++wi;
    m = ~line[wi] & par;
  }
}

RSX_BP_FN const uint8_t* px_at(const uint8_t* img, const Geo& g, uint32_t x, uint32_t y) {
  return img + size_t(y) * g.pitch + size_t(x) * (g.is_f32 ? 4u : 2u);
}

// RawImageDataU16::fixBadPixel for the marked pixel (x, y): the value it gets
RSX_BP_FN uint16_t fix_u16(const Geo& g, const uint64_t* rowmap, const uint64_t* colmap,
                           const uint8_t* img, uint32_t x, uint32_t y) {
  const uint64_t* row = rowmap + size_t(y) * g.wpr;
  const uint64_t* col = colmap + size_t(x) * g.wpc;
  const uint64_t px = parity_mask(x, g.step), py = parity_mask(y, g.step);
  int values[4] = {-1, -1, -1, -1}, dist[4] = {0, 0, 0, 0}, weight[4] = {0, 0, 0, 0};
  int q = find_below(row, x, px);
  if (q >= 0) {
    values[0] = *reinterpret_cast<const uint16_t*>(px_at(img, g, uint32_t(q), y));
    dist[0] = int(x) - q;
  }
  q = find_above(row, g.w, x, px);
  if (q >= 0) {
    values[1] = *reinterpret_cast<const uint16_t*>(px_at(img, g, uint32_t(q), y));
    dist[1] = q - int(x);
  }
  q = find_below(col, y, py);
  if (q >= 0) {
    values[2] = *reinterpret_cast<const uint16_t*>(px_at(img, g, x, uint32_t(q)));
    dist[2] = int(y) - q;
  }
  q = find_above(col, g.h, y, py);
  if (q >= 0) {
    values[3] = *reinterpret_cast<const uint16_t*>(px_at(img, g, x, uint32_t(q)));
    dist[3] = q - int(y);
  }
  int shifts = 7;
  if (const int t = dist[0] + dist[1]; t) {
    weight[0] = dist[0] ? (t - dist[0]) * 256 / t : 0;
    weight[1] = 256 - weight[0];
    ++shifts;
  }
  if (const int t = dist[2] + dist[3]; t) {
    weight[2] = dist[2] ? (t - dist[2]) * 256 / t : 0;
    weight[3] = 256 - weight[2];
    ++shifts;
  }
  int total = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (values[i] >= 0)
      total += values[i] * weight[i];
  total >>= shifts;
  return uint16_t(total < 0 ? 0 : total > 65535 ? 65535 : total);
}

RSX_BP_FN float load_f32(const uint8_t* p) { return *reinterpret_cast<const float*>(p); }

// One direction of RawImageDataFloat::fixBadPixel: the loop runs while values[curr] < 0, so a good
// pixel with a negative value is recorded, distance and all, and the walk goes on behind it.
// below: towards 0.  `horizontal`: along row `fixed`, else along column `fixed`.
RSX_BP_FN void walk_f32(const Geo& g, const uint64_t* line, uint32_t n, uint32_t p, uint64_t par,
                        bool below, bool horizontal, uint32_t fixed, const uint8_t* img,
                        float* value, float* dist) {
  float v = -1.0F, d = 0.0F;
  uint32_t at = p;
  while (v < 0.0F) {
    const int q = below ? find_below(line, at, par) : find_above(line, n, at, par);
    if (q < 0)
      break;
    at = uint32_t(q);
    v = load_f32(horizontal ? px_at(img, g, at, fixed) : px_at(img, g, fixed, at));
    d = float(below ? int(p) - q : q - int(p));
  }
  *value = v;
  *dist = d;
}

// RawImageDataFloat::fixBadPixel for the marked pixel (x, y): the bits it gets
RSX_BP_FN uint32_t fix_f32(const Geo& g, const uint64_t* rowmap, const uint64_t* colmap,
                           const uint8_t* img, uint32_t x, uint32_t y) {
  const uint64_t* row = rowmap + size_t(y) * g.wpr;
  const uint64_t* col = colmap + size_t(x) * g.wpc;
  const uint64_t px = parity_mask(x, g.step), py = parity_mask(y, g.step);
  float values[4], dist[4], weight[4] = {0.0F, 0.0F, 0.0F, 0.0F};
  walk_f32(g, row, g.w, x, px, true, true, y, img, &values[0], &dist[0]);
  walk_f32(g, row, g.w, x, px, false, true, y, img, &values[1], &dist[1]);
  walk_f32(g, col, g.h, y, py, true, false, x, img, &values[2], &dist[2]);
  walk_f32(g, col, g.h, y, py, false, false, x, img, &values[3], &dist[3]);
  float total_div = 0.000001F;
  if (const float t = f_add(dist[0], dist[1]); t > 0.0F) {
    weight[0] = dist[0] > 0.0F ? f_div(f_sub(t, dist[0]), t) : 0.0F;
    weight[1] = f_sub(1.0F, weight[0]);
    total_div = f_add(total_div, 1.0F);
  }
  if (const float t = f_add(dist[2], dist[3]); t > 0.0F) {
    weight[2] = dist[2] > 0.0F ? f_div(f_sub(t, dist[2]), t) : 0.0F;
    weight[3] = f_sub(1.0F, weight[2]);
    total_div = f_add(total_div, 1.0F);
  }
  float total = 0.0F;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (values[i] >= 0.0F)
      total = f_add(total, f_mul(values[i], weight[i]));
  total = f_div(total, total_div);
  if (total != total)
    return NAN_X86;
  union {
    float f;
    uint32_t u;
  } b;
  b.f = total;
  return b.u;
}

// bit `t` of the 64 words rowmap[(64 yw + r) wpr + xw], r = 0 .. 63, as word yw of column
// 64 xw + t of the column map
RSX_BP_FN uint64_t column_word(const Geo& g, const uint64_t* rowmap, uint32_t xw, uint32_t t,
                               uint32_t yw) {
  uint64_t out = 0;
  const uint32_t y0 = yw * 64u, rows = g.h - y0 < 64u ? g.h - y0 : 64u;
  for (uint32_t r = 0; r < rows; ++r)
    out |= ((rowmap[size_t(y0 + r) * g.wpr + xw] >> t) & 1ull) << r;
  return out;
}

} // namespace rsx_bp
