// Lossy-JPEG DNG tiles (compression 0x884c; include/rsx.h section 4e), shared by the kernels of
// rsx_dng_jpeg.hip and by a host build (rsx_jpeg_host.cpp): what JpegDecompressor::decode
// (decompressors/JpegDecompressor.cpp:128-170) gets from libjpeg-turbo's default decoder --
// jpeg_read_header, the Huffman decode of jdhuff.c, jpeg_idct_islow, the triangle-filter
// upsampling of jdsample.c and the YCbCr conversion of jdcolor.c -- and the window it copies.
//
// The header parse and the segment table are the host's.  The entropy decode of a segment, the
// transform of a block and the value of an output sample are written once, for both sides.
//
// Where libjpeg would warn and go on, the tile is refused (a status, nothing written).  Beyond
// what an encoder makes from 8-bit pixels the SIMD code that every x86-64 libjpeg-turbo runs and
// its C code part ways (16-bit products and sums, a saturating against a masked range limit): a
// tile with a dequantised coefficient or a value behind the column pass outside +-OVERSHOOT is
// refused, and inside that range the range limit saturates, as the SIMD code does.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "rsx.h"

#if defined(__HIPCC__)
#define RSX_JP_FN __host__ __device__ __forceinline__
#else
#define RSX_JP_FN inline
#endif

namespace rsx_jpeg {

constexpr int CS_GREY = 0, CS_YCC = 1, CS_RGB = 2;
constexpr int LOOK_BITS = 9;
constexpr int32_t OVERSHOOT = 16383; // twice what fits 16-bit sums; an encoder's data stays below 8200
constexpr uint32_t BATCH = 8;        // blocks the walking lane hands to the wavefront at a time

// One derived Huffman table as the walking lane reads it.
struct Huff {
  uint16_t look[1 << LOOK_BITS]; // (length << 8) | symbol for codes of up to LOOK_BITS bits, else 0
  int32_t maxcode[18];           // the largest code of a length, -1: none
  int32_t valoff[18];            // index of a length's first symbol minus its first code
  uint8_t vals[256];
};
// The tables of a tile, per component: what a segment's wavefront copies into LDS.
struct Tables {
  Huff dc[3], ac[3];
  uint16_t q[3][64]; // natural order
};

// A tile as both kernels see it.
struct Tile {
  uint64_t in_off;       // the tile's bytes in the plan's input
  uint64_t img_off;      // the image in the plan's output
  uint64_t plane_off[3]; // the component planes in the scratch, whole MCUs
  uint32_t plane_w[3];   // bytes a plane row
  uint32_t comp_w[3], comp_h[3]; // the component's own (downsampled) size
  uint32_t pitch;
  uint32_t off_x, off_y, copy_w, copy_h; // the window, pixels
  uint32_t mcus_x;
  uint32_t tables;       // index of its Tables
  uint8_t ncomp, hs, vs, colour;
  uint32_t in_bytes;
};
// An entropy segment: a whole scan, or one restart interval.
struct Segment {
  uint32_t tile;
  uint32_t first_mcu, n_mcus;
  uint32_t start, end; // bytes of the tile; no marker inside
};

RSX_JP_FN uint32_t natural_order(uint32_t k) {
  static constexpr uint8_t ZZ[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                     12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                     58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return ZZ[k & 63u];
}

// ---------------------------------------------------------------------------------------------
// The bit walk of jdhuff.c over one segment.  Src::at(i) is byte i of the tile.
// ---------------------------------------------------------------------------------------------
template <class Src>
struct Bits {
  const Src* src;
  uint32_t pos, end;
  uint64_t acc; // the low n bits are the bits not yet taken
  int n;
  RSX_JP_FN void init(const Src* s, uint32_t start, uint32_t stop) {
    src = s;
    pos = start;
    end = stop;
    acc = 0;
    n = 0;
  }
  // fill_bit_buffer: FF 00 is the byte FF, further FFs in front of the 00 are fill bytes
  RSX_JP_FN void refill() {
    // four bytes at a time while none of them is FF (their reads do not wait for each other)
    while (n <= 32 && pos + 4u <= end) {
      const uint32_t b0 = src->at(pos), b1 = src->at(pos + 1u), b2 = src->at(pos + 2u),
                     b3 = src->at(pos + 3u);
      if (b0 == 0xFFu || b1 == 0xFFu || b2 == 0xFFu || b3 == 0xFFu)
        break;
      acc = (acc << 32) | ((b0 << 24) | (b1 << 16) | (b2 << 8) | b3);
      n += 32;
      pos += 4u;
    }
    while (n < 32 && pos < end) {
      const uint32_t b = src->at(pos);
      if (b == 0xFFu) {
        uint32_t j = pos + 1u;
        while (j < end && src->at(j) == 0xFFu)
          ++j;
        if (j < end && src->at(j) == 0u) {
          pos = j + 1u;
        } else {
          pos = end; // (nothing but fill bytes in front of the segment's end)
          break;
        }
      } else {
        ++pos;
      }
      acc = (acc << 8) | b;
      n += 8;
    }
  }
  // the next 16 bits, zeros behind the last one
  RSX_JP_FN uint32_t peek16() const {
    return uint32_t(n >= 16 ? acc >> (n - 16) : acc << (16 - n)) & 0xFFFFu;
  }
};

// a symbol of `T`: >= 0, or -RSX_ERR_BAD_HUFFMAN_CODE / -RSX_ERR_INPUT_OVERFLOW
template <class Src>
RSX_JP_FN int huff_symbol(Bits<Src>& B, const Huff& T) {
  if (B.n < 16)
    B.refill();
  const uint32_t v = B.peek16();
  const uint32_t e = T.look[v >> (16 - LOOK_BITS)];
  int l, sym;
  if (e) {
    l = int(e >> 8);
    sym = int(e & 255u);
  } else {
    int32_t c = 0;
    for (l = LOOK_BITS + 1; l <= 16; ++l) {
      c = int32_t(v >> (16 - l));
      if (c <= T.maxcode[l])
        break;
    }
    if (l > 16)
      return -RSX_ERR_BAD_HUFFMAN_CODE;
    sym = T.vals[uint32_t(c + T.valoff[l]) & 255u];
  }
  if (l > B.n)
    return -RSX_ERR_INPUT_OVERFLOW; // (the data ends inside the code)
  B.n -= l;
  return sym;
}

// `s` bits and HUFF_EXTEND, 1 <= s <= 15; *ok false where the data ends first
template <class Src>
RSX_JP_FN int32_t extend_bits(Bits<Src>& B, int s, bool* ok) {
  if (B.n < s)
    B.refill();
  if (B.n < s) {
    *ok = false;
    return 0;
  }
  const int32_t r = int32_t((B.acc >> (B.n - s)) & ((1u << s) - 1u));
  B.n -= s;
  return r < (1 << (s - 1)) ? r - (1 << s) + 1 : r;
}

// One block (decode_mcu_slow's loop body) into coef[64], natural order, zeroed by the caller;
// order[k] = natural_order(k), wherever the caller keeps it close.  RSX_OK or the refusal.
template <class Src, class Coef>
RSX_JP_FN int decode_block(Bits<Src>& B, const Huff& dc, const Huff& ac, const uint8_t* order,
                           int32_t* pred, Coef* coef) {
  int s = huff_symbol(B, dc);
  if (s < 0)
    return -s;
  bool ok = true;
  if (s) {
    const int32_t d = extend_bits(B, s, &ok);
    if (!ok)
      return RSX_ERR_INPUT_OVERFLOW;
    *pred += d;
    if (*pred < -32768 || *pred > 32767)
      return RSX_ERR_UNSUPPORTED; // (libjpeg keeps 16 bits of it)
  }
  coef[0] = Coef(*pred);
  for (uint32_t k = 1; k < 64u; ++k) {
    s = huff_symbol(B, ac);
    if (s < 0)
      return -s;
    const uint32_t r = uint32_t(s) >> 4;
    s &= 15;
    if (s) {
      k += r;
      if (k > 63u)
        return RSX_ERR_BAD_HUFFMAN_CODE; // a coefficient index past 63
      const int32_t v = extend_bits(B, s, &ok);
      if (!ok)
        return RSX_ERR_INPUT_OVERFLOW;
      coef[order[k]] = Coef(v);
    } else {
      if (r != 15u)
        break; // EOB
      k += 15u;
      if (k > 63u)
        return RSX_ERR_BAD_HUFFMAN_CODE;
    }
  }
  return RSX_OK;
}

// ---------------------------------------------------------------------------------------------
// jpeg_idct_islow (jidctint.c, CONST_BITS 13, PASS1_BITS 2): one pass over eight values.  The
// sums wrap as two's complement does; with every input inside +-OVERSHOOT the results never do.
// ---------------------------------------------------------------------------------------------
RSX_JP_FN int32_t descale(uint32_t x, int nbits) {
  return int32_t(x + (1u << (nbits - 1))) >> nbits;
}

RSX_JP_FN void idct_pass(const int32_t in[8], int32_t out[8], int shift) {
  typedef uint32_t U;
  const U i0 = U(in[0]), i1 = U(in[1]), i2 = U(in[2]), i3 = U(in[3]);
  const U i4 = U(in[4]), i5 = U(in[5]), i6 = U(in[6]), i7 = U(in[7]);
  U z1 = (i2 + i6) * 4433u;
  U tmp2 = z1 - i6 * 15137u;
  U tmp3 = z1 + i2 * 6270u;
  U tmp0 = (i0 + i4) << 13;
  U tmp1 = (i0 - i4) << 13;
  const U tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = i7;
  tmp1 = i5;
  tmp2 = i3;
  tmp3 = i1;
  z1 = tmp0 + tmp3;
  U z2 = tmp1 + tmp2, z3 = tmp0 + tmp2, z4 = tmp1 + tmp3;
  const U z5 = (z3 + z4) * 9633u;
  tmp0 *= 2446u;
  tmp1 *= 16819u;
  tmp2 *= 25172u;
  tmp3 *= 12299u;
  z1 *= U(-7373);
  z2 *= U(-20995);
  z3 *= U(-16069);
  z4 *= U(-3196);
  z3 += z5;
  z4 += z5;
  tmp0 += z1 + z3;
  tmp1 += z2 + z4;
  tmp2 += z2 + z3;
  tmp3 += z1 + z4;
  out[0] = descale(tmp10 + tmp3, shift);
  out[7] = descale(tmp10 - tmp3, shift);
  out[1] = descale(tmp11 + tmp2, shift);
  out[6] = descale(tmp11 - tmp2, shift);
  out[2] = descale(tmp12 + tmp1, shift);
  out[5] = descale(tmp12 - tmp1, shift);
  out[3] = descale(tmp13 + tmp0, shift);
  out[4] = descale(tmp13 - tmp0, shift);
}

// The column pass of column `col` of a block: coefficients times quantisers, into ws[r * 8 + col].
// false: a value leaves +-OVERSHOOT.
template <class Coef>
RSX_JP_FN bool idct_column(const Coef* coef, const uint16_t* q, uint32_t col, int32_t* ws) {
  int32_t in[8], out[8];
  bool ok = true;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    in[r] = int32_t(coef[r * 8 + col]) * int32_t(q[r * 8 + col]);
    ok = ok && in[r] >= -OVERSHOOT && in[r] <= OVERSHOOT;
    if (!ok)
      in[r] = 0;
  }
  idct_pass(in, out, 13 - 2);
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    ok = ok && out[r] >= -OVERSHOOT && out[r] <= OVERSHOOT;
    ws[r * 8 + col] = ok ? out[r] : 0;
  }
  return ok;
}

// The row pass of row `row`: eight samples, range-limited (saturating) around 128.
RSX_JP_FN void idct_row(const int32_t* ws, uint32_t row, uint8_t out[8]) {
  int32_t in[8], o[8];
#pragma unroll
  for (int c = 0; c < 8; ++c)
    in[c] = ws[row * 8 + c];
  idct_pass(in, o, 13 + 2 + 3);
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int32_t v = o[c] + 128;
    out[c] = uint8_t(v < 0 ? 0 : v > 255 ? 255 : v);
  }
}

// Block b of a segment: its component, and where its 8 x 8 samples go in that plane.
RSX_JP_FN void block_place(const Tile& T, const Segment& S, uint32_t b, uint32_t* comp, uint64_t* at) {
  const uint32_t luma = T.ncomp == 1 ? 1u : uint32_t(T.hs) * T.vs;
  const uint32_t per_mcu = T.ncomp == 1 ? 1u : luma + 2u;
  const uint32_t mcu = S.first_mcu + b / per_mcu, k = b % per_mcu;
  const uint32_t mx = mcu % T.mcus_x, my = mcu / T.mcus_x;
  uint32_t c = 0, bx = mx, by = my;
  if (T.ncomp != 1) {
    if (k < luma) {
      bx = mx * T.hs + k % T.hs;
      by = my * T.vs + k / T.hs;
    } else {
      c = 1u + (k - luma);
    }
  }
  *comp = c;
  // (selects, not indexing: the tile stays in registers)
  const uint64_t off = c == 0 ? T.plane_off[0] : c == 1 ? T.plane_off[1] : T.plane_off[2];
  const uint32_t pw = c == 0 ? T.plane_w[0] : c == 1 ? T.plane_w[1] : T.plane_w[2];
  *at = off + uint64_t(by) * 8u * pw + uint64_t(bx) * 8u;
}

// the component of block b of a segment alone
RSX_JP_FN uint32_t block_comp(const Tile& T, uint32_t b) {
  if (T.ncomp == 1)
    return 0u;
  const uint32_t luma = uint32_t(T.hs) * T.vs, k = b % (luma + 2u);
  return k < luma ? 0u : 1u + (k - luma);
}

// ---------------------------------------------------------------------------------------------
// An output pixel: the planes upsampled (jdsample.c: the triangle filters where the component is
// more than two samples wide, replication otherwise) and converted (jdcolor.c).
// ---------------------------------------------------------------------------------------------
RSX_JP_FN uint32_t plane_at(const uint8_t* planes, const Tile& T, int c, uint32_t x, uint32_t y) {
  return planes[T.plane_off[c] + uint64_t(y) * T.plane_w[c] + x];
}

RSX_JP_FN uint32_t chroma_at(const uint8_t* planes, const Tile& T, int c, uint32_t x, uint32_t y) {
  if (T.hs == 1)
    return plane_at(planes, T, c, x, y);
  const uint32_t dw = T.comp_w[c], dh = T.comp_h[c];
  const uint32_t i = x >> 1;
  if (T.vs == 1) { // h2v1
    const uint32_t cur = plane_at(planes, T, c, i, y);
    if (dw <= 2u)
      return cur;
    if (x & 1u)
      return i + 1u == dw ? cur : (3u * cur + plane_at(planes, T, c, i + 1u, y) + 2u) >> 2;
    return i == 0u ? cur : (3u * cur + plane_at(planes, T, c, i - 1u, y) + 1u) >> 2;
  }
  const uint32_t r = y >> 1; // h2v2
  if (dw <= 2u)
    return plane_at(planes, T, c, i, r);
  // the row above the first and below the last real row are those rows again
  const uint32_t far = (y & 1u) ? (r + 1u < dh ? r + 1u : r) : (r ? r - 1u : 0u);
  const uint32_t cur = 3u * plane_at(planes, T, c, i, r) + plane_at(planes, T, c, i, far);
  if (x & 1u) {
    if (i + 1u == dw)
      return (4u * cur + 7u) >> 4;
    return (3u * cur + 3u * plane_at(planes, T, c, i + 1u, r) + plane_at(planes, T, c, i + 1u, far) + 7u) >> 4;
  }
  if (i == 0u)
    return (4u * cur + 8u) >> 4;
  return (3u * cur + 3u * plane_at(planes, T, c, i - 1u, r) + plane_at(planes, T, c, i - 1u, far) + 8u) >> 4;
}

RSX_JP_FN uint32_t clamp255(int32_t v) { return uint32_t(v < 0 ? 0 : v > 255 ? 255 : v); }

// pixel (x, y) of the tile: out[0 .. ncomp)
RSX_JP_FN void pixel_at(const uint8_t* planes, const Tile& T, uint32_t x, uint32_t y, uint32_t out[3]) {
  const uint32_t a = plane_at(planes, T, 0, x, y);
  if (T.ncomp == 1) {
    out[0] = a;
    return;
  }
  const uint32_t b = chroma_at(planes, T, 1, x, y), c = chroma_at(planes, T, 2, x, y);
  if (T.colour == CS_RGB) {
    out[0] = a;
    out[1] = b;
    out[2] = c;
    return;
  }
  // build_ycc_rgb_table: FIX(1.40200), FIX(1.77200), FIX(0.71414), FIX(0.34414), ONE_HALF
  const int32_t cb = int32_t(b) - 128, cr = int32_t(c) - 128, y0 = int32_t(a);
  out[0] = clamp255(y0 + ((91881 * cr + 32768) >> 16));
  out[1] = clamp255(y0 + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
  out[2] = clamp255(y0 + ((116130 * cb + 32768) >> 16));
}

// ---------------------------------------------------------------------------------------------
// The host's part: jpeg_read_header and what jpeg_start_decompress derives.
// ---------------------------------------------------------------------------------------------
struct Header {
  uint32_t width, height;
  int ncomp;
  int id[4], h[4], v[4], tq[4], td[4], ta[4];
  int hs, vs; // the luma factors (1 for a single component)
  int colour;
  uint32_t dri;
  size_t scan; // the first entropy-coded byte
  uint32_t mcus_x, mcus_y;
  uint32_t comp_w[3], comp_h[3];
  bool jfif, adobe;
  int adobe_transform;
  uint16_t q[4][64];
  bool has_q[4];
  uint8_t bits[8][17], vals[8][256]; // 0 .. 3 DC, 4 .. 7 AC
  bool has_h[8];
};

// jpeg_make_d_derived_tbl; false: the counts are no prefix code, or a DC symbol above 15
inline bool derive_table(const uint8_t bits[17], const uint8_t vals[256], bool is_dc, Huff* T) {
  uint8_t size[257];
  uint32_t code_of[257];
  int p = 0;
  for (int l = 1; l <= 16; ++l)
    for (int i = 0; i < bits[l]; ++i) {
      if (p >= 256)
        return false;
      size[p++] = uint8_t(l);
    }
  size[p] = 0;
  const int n = p;
  uint32_t code = 0;
  int si = size[0];
  p = 0;
  while (size[p]) {
    while (size[p] == si)
      code_of[p++] = code++;
    if (code >= (1u << si))
      return false;
    code <<= 1;
    ++si;
  }
  for (int i = 0; i < (1 << LOOK_BITS); ++i)
    T->look[i] = 0;
  for (int i = 0; i < 256; ++i)
    T->vals[i] = i < n ? vals[i] : 0;
  p = 0;
  for (int l = 1; l <= 16; ++l) {
    if (bits[l]) {
      T->valoff[l] = p - int32_t(code_of[p]);
      p += bits[l];
      T->maxcode[l] = int32_t(code_of[p - 1]);
    } else {
      T->valoff[l] = 0;
      T->maxcode[l] = -1;
    }
  }
  T->maxcode[0] = -1;
  T->valoff[0] = 0;
  T->maxcode[17] = 0xFFFFF;
  T->valoff[17] = 0;
  for (int i = 0; i < n; ++i) {
    if (is_dc && vals[i] > 15)
      return false;
    const int l = size[i];
    if (l > LOOK_BITS)
      continue;
    const uint32_t first = code_of[i] << (LOOK_BITS - l);
    for (uint32_t k = 0; k < (1u << (LOOK_BITS - l)); ++k)
      T->look[first + k] = uint16_t((l << 8) | vals[i]);
  }
  return true;
}

inline uint32_t be16(const uint8_t* p) { return (uint32_t(p[0]) << 8) | p[1]; }

// The markers up to SOS.  RSX_OK, or RSX_ERR_IO for a broken header, RSX_ERR_UNSUPPORTED for what
// this decoder leaves to the CPU.
inline int parse_header(const uint8_t* p, size_t n, Header* H) {
  *H = Header();
  if (n >= (uint64_t(1) << 32))
    return RSX_ERR_UNSUPPORTED;
  if (n < 4 || p[0] != 0xFF || p[1] != 0xD8)
    return RSX_ERR_IO;
  size_t at = 2;
  bool sof = false;
  for (;;) {
    if (at + 2 > n || p[at] != 0xFF)
      return RSX_ERR_IO;
    while (at < n && p[at] == 0xFF)
      ++at; // (fill bytes in front of a marker)
    if (at >= n)
      return RSX_ERR_IO;
    const uint32_t m = p[at++];
    if (m == 0x00 || m == 0x01 || m == 0xD8 || m == 0xD9 || (m >= 0xD0 && m <= 0xD7))
      return RSX_ERR_IO;
    if (at + 2 > n)
      return RSX_ERR_IO;
    const size_t len = be16(p + at);
    if (len < 2 || at + len > n)
      return RSX_ERR_IO; // a segment past the end
    const uint8_t* d = p + at + 2;
    const size_t dl = len - 2;
    at += len;
    if (m == 0xE0) {
      if (dl >= 14 && d[0] == 'J' && d[1] == 'F' && d[2] == 'I' && d[3] == 'F' && d[4] == 0)
        H->jfif = true;
    } else if (m == 0xEE) {
      if (dl >= 12 && d[0] == 'A' && d[1] == 'd' && d[2] == 'o' && d[3] == 'b' && d[4] == 'e') {
        H->adobe = true;
        H->adobe_transform = d[11];
      }
    } else if (m == 0xDB) {
      size_t i = 0;
      while (i < dl) {
        const int prec = d[i] >> 4, idx = d[i] & 15;
        ++i;
        if (idx > 3 || prec > 1 || i + (prec ? 128u : 64u) > dl)
          return RSX_ERR_IO;
        for (uint32_t k = 0; k < 64u; ++k) {
          H->q[idx][natural_order(k)] = uint16_t(prec ? be16(d + i + 2 * k) : d[i + k]);
        }
        i += prec ? 128 : 64;
        H->has_q[idx] = true;
      }
    } else if (m == 0xC4) {
      size_t i = 0;
      while (i < dl) {
        if (i + 17 > dl)
          return RSX_ERR_IO;
        const int tc = d[i] >> 4, th = d[i] & 15;
        if (tc > 1 || th > 3)
          return RSX_ERR_IO; // a table index out of range
        const int slot = tc * 4 + th;
        uint32_t count = 0;
        H->bits[slot][0] = 0;
        for (int l = 1; l <= 16; ++l) {
          H->bits[slot][l] = d[i + l];
          count += d[i + l];
        }
        i += 17;
        if (count > 256 || i + count > dl)
          return RSX_ERR_IO;
        for (uint32_t k = 0; k < 256u; ++k)
          H->vals[slot][k] = k < count ? d[i + k] : 0;
        i += count;
        H->has_h[slot] = true;
      }
    } else if (m == 0xC0 || m == 0xC1) {
      if (sof || dl < 6)
        return RSX_ERR_IO;
      sof = true;
      const int prec = d[0];
      H->height = be16(d + 1);
      H->width = be16(d + 3);
      H->ncomp = d[5];
      if (prec == 12)
        return RSX_ERR_UNSUPPORTED;
      if (prec != 8 || H->width == 0 || H->height == 0 || H->ncomp == 0 || dl != 6u + 3u * H->ncomp)
        return RSX_ERR_IO;
      if (H->ncomp != 1 && H->ncomp != 3)
        return RSX_ERR_UNSUPPORTED; // four components: CMYK / YCCK
      for (int c = 0; c < H->ncomp; ++c) {
        H->id[c] = d[6 + 3 * c];
        H->h[c] = d[7 + 3 * c] >> 4;
        H->v[c] = d[7 + 3 * c] & 15;
        H->tq[c] = d[8 + 3 * c];
        if (H->h[c] < 1 || H->h[c] > 4 || H->v[c] < 1 || H->v[c] > 4 || H->tq[c] > 3)
          return RSX_ERR_IO;
      }
    } else if (m >= 0xC2 && m <= 0xCF && m != 0xC8 && m != 0xCC) {
      return RSX_ERR_UNSUPPORTED; // progressive, lossless, differential, arithmetic
    } else if (m == 0xDD) {
      if (dl != 2)
        return RSX_ERR_IO;
      H->dri = be16(d);
    } else if (m == 0xDA) {
      if (!sof || dl < 1)
        return RSX_ERR_IO;
      const int ns = d[0];
      if (ns < 1 || ns > 4 || dl != 4u + 2u * ns)
        return RSX_ERR_IO;
      for (int i = 0; i < ns; ++i) {
        int c = -1;
        for (int k = 0; k < H->ncomp; ++k)
          if (H->id[k] == d[1 + 2 * i]) {
            c = k;
            break;
          }
        if (c < 0)
          return RSX_ERR_IO;
      }
      if (ns != H->ncomp)
        return RSX_ERR_UNSUPPORTED; // several scans, or a scan that is not interleaved
      for (int i = 0; i < ns; ++i) {
        if (H->id[i] != d[1 + 2 * i])
          return RSX_ERR_UNSUPPORTED; // (the scan's order is not the frame's)
        H->td[i] = d[2 + 2 * i] >> 4;
        H->ta[i] = d[2 + 2 * i] & 15;
        if (H->td[i] > 3 || H->ta[i] > 3 || !H->has_h[H->td[i]] || !H->has_h[4 + H->ta[i]] ||
            !H->has_q[H->tq[i]])
          return RSX_ERR_IO; // the scan names a table that is not there
      }
      const uint8_t* e = d + 1 + 2 * ns;
      if (e[0] != 0 || e[1] != 63 || e[2] != 0)
        return RSX_ERR_UNSUPPORTED;
      H->scan = at;
      break;
    }
    // (everything else -- APPn, COM, DAC, DNL, ... -- is skipped by its length)
  }
  // default_decompress_parms
  if (H->ncomp == 1) {
    H->colour = CS_GREY;
    H->hs = H->vs = 1; // (one component alone: its factors do not matter)
  } else {
    if (H->jfif)
      H->colour = CS_YCC;
    else if (H->adobe)
      H->colour = H->adobe_transform == 0 ? CS_RGB : CS_YCC;
    else if (H->id[0] == 'R' && H->id[1] == 'G' && H->id[2] == 'B')
      H->colour = CS_RGB;
    else
      H->colour = CS_YCC;
    H->hs = H->h[0];
    H->vs = H->v[0];
    const bool chroma_1x1 = H->h[1] == 1 && H->v[1] == 1 && H->h[2] == 1 && H->v[2] == 1;
    if (!chroma_1x1 || H->hs > 2 || H->vs > 2 || (H->hs == 1 && H->vs == 2))
      return RSX_ERR_UNSUPPORTED; // (4:4:0 among them)
    if (H->colour == CS_RGB && (H->hs != 1 || H->vs != 1))
      return RSX_ERR_UNSUPPORTED;
  }
  H->mcus_x = (H->width + 8u * H->hs - 1u) / (8u * H->hs);
  H->mcus_y = (H->height + 8u * H->vs - 1u) / (8u * H->vs);
  for (int c = 0; c < H->ncomp; ++c) {
    H->comp_w[c] = c == 0 ? H->width : (H->width + H->hs - 1u) / H->hs;
    H->comp_h[c] = c == 0 ? H->height : (H->height + H->vs - 1u) / H->vs;
  }
  return RSX_OK;
}

// The markers of the entropy-coded data: RST0, RST1, ... modulo 8 between the restart intervals
// and nothing else in front of EOI.  seg_end[i] is where segment i stops, seg_start[i] where it
// begins; n_segments of them are expected.  RSX_OK or the refusal.
template <class Emit>
inline int scan_segments(const uint8_t* p, size_t n, const Header& H, Emit emit) {
  const uint64_t mcus = uint64_t(H.mcus_x) * H.mcus_y;
  const uint64_t per = H.dri ? H.dri : mcus;
  const uint64_t n_seg = (mcus + per - 1) / per;
  uint64_t seg = 0;
  size_t start = H.scan, at = H.scan;
  for (;;) {
    while (at < n && p[at] != 0xFF)
      ++at;
    if (at >= n)
      return RSX_ERR_INPUT_OVERFLOW; // no EOI
    size_t j = at + 1;
    while (j < n && p[j] == 0xFF)
      ++j;
    if (j >= n)
      return RSX_ERR_INPUT_OVERFLOW;
    const uint32_t m = p[j];
    if (m == 0) {
      at = j + 1;
      continue;
    }
    // a marker: segment `seg` stops at `at`
    const bool last = seg + 1 == n_seg;
    if (m == 0xD9) {
      if (!last)
        return RSX_ERR_INPUT_OVERFLOW; // the data ends before the last MCU
    } else if (m >= 0xD0 && m <= 0xD7) {
      if (last || !H.dri || m != 0xD0u + uint32_t(seg & 7u))
        return RSX_ERR_RESTART_MARKER;
    } else {
      return RSX_ERR_RESTART_MARKER; // a marker where none belongs
    }
    emit(uint32_t(seg), uint32_t(seg * per), uint32_t(last ? mcus - seg * per : per), uint32_t(start),
         uint32_t(at));
    if (last)
      return RSX_OK;
    ++seg;
    start = at = j + 1;
  }
}

// rsx_dng_jpeg_validate: the header, then the image and the window
inline int validate_tile(const uint8_t* in, size_t in_bytes, uint32_t off_x, uint32_t off_y,
                         const rsx_image& img, Header* H) {
  if (!in || img.dim_x <= 0 || img.dim_y <= 0 || img.cpp < 1 || img.pitch_bytes % 2u != 0 ||
      uint64_t(img.pitch_bytes) < uint64_t(img.dim_x) * uint32_t(img.cpp) * 2u)
    return RSX_ERR_INVALID_ARG;
  if (off_x >= uint32_t(img.dim_x) || off_y >= uint32_t(img.dim_y))
    return RSX_ERR_INVALID_ARG;
  if (int st = parse_header(in, in_bytes, H))
    return st;
  if (H->ncomp != img.cpp)
    return RSX_ERR_INVALID_ARG; // JpegDecompressor.cpp: output_components != cpp
  for (int c = 0; c < H->ncomp; ++c) {
    Huff t;
    if (!derive_table(H->bits[H->td[c]], H->vals[H->td[c]], true, &t) ||
        !derive_table(H->bits[4 + H->ta[c]], H->vals[4 + H->ta[c]], false, &t))
      return RSX_ERR_IO;
  }
  return RSX_OK;
}

// rsx_dng_jpeg_validate itself
inline int validate_call(const rsx_dng_jpeg_tile* tile, const rsx_image* img, rsx_dng_jpeg_info* info) {
  if (!tile || !img)
    return RSX_ERR_INVALID_ARG;
  Header H;
  if (int st = validate_tile(tile->in, tile->in_bytes, tile->off_x, tile->off_y, *img, &H))
    return st;
  if (info) {
    const uint64_t mcus = uint64_t(H.mcus_x) * H.mcus_y;
    info->width = H.width;
    info->height = H.height;
    info->components = H.ncomp;
    info->h_samp = H.hs;
    info->v_samp = H.vs;
    info->colour_space = H.colour;
    info->restart_interval = H.dri;
    info->n_segments = uint32_t(H.dri ? (mcus + H.dri - 1) / H.dri : 1);
  }
  return RSX_OK;
}

inline void fill_tables(const Header& H, Tables* T) {
  for (int c = 0; c < 3; ++c) {
    const int k = c < H.ncomp ? c : 0;
    derive_table(H.bits[H.td[k]], H.vals[H.td[k]], true, &T->dc[c]);
    derive_table(H.bits[4 + H.ta[k]], H.vals[4 + H.ta[k]], false, &T->ac[c]);
    for (int i = 0; i < 64; ++i)
      T->q[c][i] = H.q[H.tq[k]][i];
  }
}

// the tile's geometry but the offsets (the planes back to back from plane_off[0] = base)
inline uint64_t fill_tile(const Header& H, uint32_t off_x, uint32_t off_y, const rsx_image& img,
                          uint64_t base, Tile* T) {
  *T = Tile();
  T->ncomp = uint8_t(H.ncomp);
  T->hs = uint8_t(H.hs);
  T->vs = uint8_t(H.vs);
  T->colour = uint8_t(H.colour);
  T->mcus_x = H.mcus_x;
  T->pitch = img.pitch_bytes;
  T->off_x = off_x;
  T->off_y = off_y;
  T->copy_w = uint32_t(img.dim_x) - off_x < H.width ? uint32_t(img.dim_x) - off_x : H.width;
  T->copy_h = uint32_t(img.dim_y) - off_y < H.height ? uint32_t(img.dim_y) - off_y : H.height;
  for (int c = 0; c < H.ncomp; ++c) {
    const uint32_t hc = c == 0 ? H.hs : 1u, vc = c == 0 ? H.vs : 1u;
    T->plane_off[c] = base;
    T->plane_w[c] = H.mcus_x * hc * 8u;
    T->comp_w[c] = H.comp_w[c];
    T->comp_h[c] = H.comp_h[c];
    base += (uint64_t(T->plane_w[c]) * (uint64_t(H.mcus_y) * vc * 8u) + 15u) & ~uint64_t(15);
  }
  return base;
}

} // namespace rsx_jpeg
