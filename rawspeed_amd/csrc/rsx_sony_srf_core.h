// ArwDecoder::SonyDecrypt and ArwDecoder::decodeSRF (include/rsx.h section 3z), shared by the kernel
// of rsx_sony_srf.hip and by a host build (rsx_sony_srf_host.cpp): the pad from the key
// (decoders/ArwDecoder.cpp:533-542), the stream (:544-559), the checks of decodeSRF (:76-79) and the
// jump that lets a chunk of the stream start without the words in front of it.
//
// With w[0..126] the byte-swapped pad, the loop is w[n] = w[n - 127] ^ w[n - 63] for n >= 127 and
// output word i = input word i ^ w[127 + i].  Every bit lane is a linear recurrence over GF(2) with
// the characteristic polynomial P = x^127 + x^64 + 1, so
//   w[n + m] = sum over the set bits j of (x^n mod P) of w[j + m]                       (the jump)
//   w[n] = w[n - 127 2^k] ^ w[n - 63 2^k] for n >= 127 2^k            (P^(2^k), the doubling identity)
// The device takes the stream in chunks of CHUNK words.  A chunk computes x^(its first word) mod P
// by square-and-multiply (about 22 squarings of a 127-bit polynomial), its first 127 words from the
// table w[0..252], and the rest with the doubling identity: with K words known and 127 2^k <= K the
// next 63 2^k are independent of each other.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "rsx.h"

#if defined(__HIPCC__)
#define RSX_SRF_FN __host__ __device__ __forceinline__
#define RSX_SRF_UNROLL8 _Pragma("unroll 8")
#else
#define RSX_SRF_FN inline
#define RSX_SRF_UNROLL8
#endif

namespace rsx_sony_srf {

constexpr int32_t MAX_X = 3360, MAX_Y = 2460; // decodeSRF :76
constexpr int PAD = 127;                      // words of state
constexpr int TABLE = 2 * PAD - 1;            // w[0..252]: what the jump of 127 words reads
constexpr int CHUNK = 2048;                   // words of the stream a workgroup makes

// decodeSRF's checks, then the pitch, getSubView(off, len), and the size SonyDecrypt's invariants
// do not hold for (len / 4 drops two bytes when width height is odd).
inline int validate(uint64_t in_bytes, const rsx_image* img) {
  if (!img)
    return RSX_ERR_INVALID_ARG;
  if (img->cpp != 1)
    return RSX_ERR_INVALID_ARG;
  if (img->dim_x < 1 || img->dim_y < 1 || img->dim_x > MAX_X || img->dim_y > MAX_Y)
    return RSX_ERR_INVALID_ARG; // "Unexpected image dimensions found"
  if (img->pitch_bytes < uint32_t(img->dim_x) * 2u || img->pitch_bytes % 2u != 0)
    return RSX_ERR_INVALID_ARG;
  if (in_bytes < 2ull * uint64_t(img->dim_x) * uint64_t(img->dim_y))
    return RSX_ERR_IO;
  if ((uint64_t(img->dim_x) * uint64_t(img->dim_y)) % 2u != 0)
    return RSX_ERR_UNSUPPORTED;
  return RSX_OK;
}

RSX_SRF_FN uint32_t bswap32(uint32_t v) {
  return v << 24 | (v & 0xFF00u) << 8 | (v >> 8 & 0xFF00u) | v >> 24;
}

// the two pixels of a decrypted word (read as the host's little-endian uint32): 16-bit big-endian
// each, returned as pix(2j) | pix(2j + 1) << 16
RSX_SRF_FN uint32_t widen_be16(uint32_t v) { return (v & 0x00FF00FFu) << 8 | (v >> 8 & 0x00FF00FFu); }

// w[0 .. n) for n >= 127: the pad as SonyDecrypt leaves it in front of its loop (:536-542), walked on
inline void table_from_key(uint32_t key, uint32_t* w, int n) {
  for (int p = 0; p < 4; ++p)
    w[p] = key = uint32_t(key * 48828125u + 1u);
  w[3] = w[3] << 1 | (w[0] ^ w[2]) >> 31;
  for (int p = 4; p < PAD; ++p)
    w[p] = (w[p - 4] ^ w[p - 2]) << 1 | (w[p - 3] ^ w[p - 1]) >> 31;
  for (int p = 0; p < PAD; ++p)
    w[p] = bswap32(w[p]);
  for (int p = PAD; p < n; ++p)
    w[p] = w[p - 127] ^ w[p - 63];
}

// A polynomial over GF(2) of degree <= 126: bit j of lo is x^j, bit j of hi is x^(64 + j).
struct Poly {
  uint64_t lo, hi;
};

// zeros between the bits of v: bit i -> bit 2 i
RSX_SRF_FN uint64_t spread32(uint32_t v) {
  uint64_t x = v;
  x = (x | x << 16) & 0x0000FFFF0000FFFFull;
  x = (x | x << 8) & 0x00FF00FF00FF00FFull;
  x = (x | x << 4) & 0x0F0F0F0F0F0F0F0Full;
  x = (x | x << 2) & 0x3333333333333333ull;
  x = (x | x << 1) & 0x5555555555555555ull;
  return x;
}

// a^2 mod P: squaring spreads the bits (degree <= 252); x^127 = x^64 + 1 folds the upper 126 bits
// down, and the at most 63 bits that leaves above x^126 once more
RSX_SRF_FN Poly square(Poly a) {
  const uint64_t s0 = spread32(uint32_t(a.lo)), s1 = spread32(uint32_t(a.lo >> 32));
  const uint64_t s2 = spread32(uint32_t(a.hi)), s3 = spread32(uint32_t(a.hi >> 32));
  const uint64_t h0 = s1 >> 63 | s2 << 1, h1 = s2 >> 63 | s3 << 1; // bits 127 .. 252
  uint64_t r0 = s0 ^ h0;
  uint64_t r1 = (s1 & 0x7FFFFFFFFFFFFFFFull) ^ h1 ^ h0;
  const uint64_t r2 = h1;                   // (h1 has 62 bits)
  const uint64_t g = r1 >> 63 | r2 << 1;    // bits 127 .. 190 of (r0, r1, r2): at most 63 of them
  r1 &= 0x7FFFFFFFFFFFFFFFull;
  return Poly{r0 ^ g, r1 ^ g};
}

RSX_SRF_FN Poly times_x(Poly a) {
  const uint64_t top = a.hi >> 62 & 1u; // x^126 becomes x^127 = x^64 + 1
  Poly r{a.lo << 1, (a.hi << 1 | a.lo >> 63) & 0x7FFFFFFFFFFFFFFFull};
  r.lo ^= top;
  r.hi ^= top;
  return r;
}

// x^n mod P, from the top bit of n down
RSX_SRF_FN Poly x_pow(uint64_t n) {
  Poly r{1u, 0u};
  for (int b = 63; b >= 0; --b) {
    if (n >> b == 0)
      continue;
    r = square(r);
    if (n >> b & 1u)
      r = times_x(r);
  }
  return r;
}

// w[n + m] from the table w[0 .. 252] and c = x^n mod P, m in 0 .. 126
RSX_SRF_FN uint32_t jump_word(Poly c, const uint32_t* table, int m) {
  uint32_t acc = 0;
  RSX_SRF_UNROLL8
  for (int j = 0; j < 64; ++j)
    acc ^= table[j + m] & (0u - uint32_t(c.lo >> j & 1u));
  RSX_SRF_UNROLL8
  for (int j = 0; j < 63; ++j)
    acc ^= table[64 + j + m] & (0u - uint32_t(c.hi >> j & 1u));
  return acc;
}

// How far the doubling identity reaches with K >= 127 words known: the shift k with
// 127 2^k <= K < 127 2^(k + 1); words [K, K + 63 2^k) then read only words below K.
RSX_SRF_FN int doubling_shift(uint32_t known) {
  int k = 0;
  while ((uint32_t(2 * PAD) << k) <= known)
    ++k;
  return k;
}

} // namespace rsx_sony_srf
