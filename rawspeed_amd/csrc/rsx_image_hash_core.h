// The image hash of include/rsx.h section 4g, shared by the kernels of rsx_image_hash.hip and by a
// host build (rsx_image_hash_host.cpp): MD5 as RFC 1321 states it (the block compression, the
// padding, a streaming hasher for any length and alignment), the checks of a job and the two exact
// sums of rawspeed-identify.
//
// The constants are floor(2^32 |sin(i + 1)|), i = 0 .. 63, the shifts are the RFC's four rows of
// four.  A digest is the state words A, B, C, D in little-endian order (what hashlib's digest()
// returns).  rstest's hash of an image is the MD5 of the 16 dim_y bytes of its rows' digests, each
// row hashed over dim_x cpp samples as stored, padding of the pitch excluded.
//
// A lane of the row kernel keeps the state and the sixteen words of a block in registers: the
// loops below are unrolled there, so every index is a constant and no array reaches memory.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "rsx.h"

#if defined(__HIPCC__)
#define RSX_IH_FN __host__ __device__ __forceinline__
#define RSX_IH_UNROLL _Pragma("unroll")
#elif defined(__GNUC__)
#define RSX_IH_FN inline
#define RSX_IH_UNROLL _Pragma("GCC unroll 64")
#else
#define RSX_IH_FN inline
#define RSX_IH_UNROLL
#endif

namespace rsx_imghash {

// The limits behind RSX_ERR_UNSUPPORTED: a row of fewer than 2^28 bytes and fewer than 2^24 rows
// keep every chain (a row; the 16 dim_y bytes of the digests) far below the upper word of MD5's
// bit count.  The count is written as 64 bits all the same.
constexpr uint64_t MAX_ROW_BYTES = uint64_t(1) << 28;
constexpr int32_t MAX_ROWS = int32_t(1) << 24;
constexpr int ROWS_PER_WAVE = 64;

// the checks of section 4g, in its order
inline int validate(const rsx_image* img, int32_t sample_bytes) {
  if (!img)
    return RSX_ERR_INVALID_ARG;
  if (sample_bytes != 2 && sample_bytes != 4)
    return RSX_ERR_INVALID_ARG;
  if (img->cpp < 1 || img->dim_x < 1 || img->dim_y < 1)
    return RSX_ERR_INVALID_ARG;
  const uint64_t row_bytes = uint64_t(img->dim_x) * uint64_t(img->cpp) * uint64_t(sample_bytes);
  if (uint64_t(img->pitch_bytes) < row_bytes || img->pitch_bytes % uint32_t(sample_bytes) != 0)
    return RSX_ERR_INVALID_ARG;
  if (row_bytes >= MAX_ROW_BYTES || img->dim_y >= MAX_ROWS)
    return RSX_ERR_UNSUPPORTED;
  return RSX_OK;
}

// T[i] = floor(2^32 |sin(i + 1)|)
RSX_IH_FN constexpr uint32_t sine_constant(int i) {
  constexpr uint32_t T[64] = {
      0xD76AA478u, 0xE8C7B756u, 0x242070DBu, 0xC1BDCEEEu, 0xF57C0FAFu, 0x4787C62Au, 0xA8304613u,
      0xFD469501u, 0x698098D8u, 0x8B44F7AFu, 0xFFFF5BB1u, 0x895CD7BEu, 0x6B901122u, 0xFD987193u,
      0xA679438Eu, 0x49B40821u, 0xF61E2562u, 0xC040B340u, 0x265E5A51u, 0xE9B6C7AAu, 0xD62F105Du,
      0x02441453u, 0xD8A1E681u, 0xE7D3FBC8u, 0x21E1CDE6u, 0xC33707D6u, 0xF4D50D87u, 0x455A14EDu,
      0xA9E3E905u, 0xFCEFA3F8u, 0x676F02D9u, 0x8D2A4C8Au, 0xFFFA3942u, 0x8771F681u, 0x6D9D6122u,
      0xFDE5380Cu, 0xA4BEEA44u, 0x4BDECFA9u, 0xF6BB4B60u, 0xBEBFBC70u, 0x289B7EC6u, 0xEAA127FAu,
      0xD4EF3085u, 0x04881D05u, 0xD9D4D039u, 0xE6DB99E5u, 0x1FA27CF8u, 0xC4AC5665u, 0xF4292244u,
      0x432AFF97u, 0xAB9423A7u, 0xFC93A039u, 0x655B59C3u, 0x8F0CCC92u, 0xFFEFF47Du, 0x85845DD1u,
      0x6FA87E4Fu, 0xFE2CE6E0u, 0xA3014314u, 0x4E0811A1u, 0xF7537E82u, 0xBD3AF235u, 0x2AD7D2BBu,
      0xEB86D391u};
  return T[i];
}

// the rotation of step i: RFC 1321's S11 .. S44
RSX_IH_FN constexpr int step_shift(int i) {
  constexpr int S[16] = {7, 12, 17, 22, 5, 9, 14, 20, 4, 11, 16, 23, 6, 10, 15, 21};
  return S[4 * (i / 16) + i % 4];
}

// the word of the block step i reads
RSX_IH_FN constexpr int step_word(int i) {
  return i < 16 ? i : i < 32 ? (5 * i + 1) % 16 : i < 48 ? (3 * i + 5) % 16 : (7 * i) % 16;
}

// (the builtin keeps the rotation one instruction on the device: written with shifts, the compiler
// folds the two halves into the addition behind it, three instructions for two)
RSX_IH_FN uint32_t rotl(uint32_t v, int n) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_rotateleft32(v, uint32_t(n));
#else
  return v << n | v >> (32 - n);
#endif
}

RSX_IH_FN void init_state(uint32_t s[4]) {
  s[0] = 0x67452301u;
  s[1] = 0xEFCDAB89u;
  s[2] = 0x98BADCFEu;
  s[3] = 0x10325476u;
}

// one 64-byte block w (little-endian words) into the state
RSX_IH_FN void compress(uint32_t s[4], const uint32_t w[16]) {
  uint32_t a = s[0], b = s[1], c = s[2], d = s[3];
  RSX_IH_UNROLL
  for (int i = 0; i < 64; ++i) {
    uint32_t f;
    if (i < 16)
      f = d ^ (b & (c ^ d)); // F = (b & c) | (~b & d)
    else if (i < 32)
      f = c ^ (d & (b ^ c)); // G = (b & d) | (c & ~d)
    else if (i < 48)
      f = b ^ c ^ d;         // H
    else
      f = c ^ (b | ~d);      // I
    const uint32_t t = a + f + sine_constant(i) + w[step_word(i)];
    a = d;
    d = c;
    c = b;
    b += rotl(t, step_shift(i));
  }
  s[0] += a;
  s[1] += b;
  s[2] += c;
  s[3] += d;
}

// The end of a message of `total_bytes` bytes whose last r = total_bytes % 64 bytes are the low
// bytes of w: 0x80, zeros and the 64-bit bit count, one block for r < 56 and two otherwise.  What
// w holds above byte r does not matter.  w is used up.
RSX_IH_FN void finish(uint32_t s[4], uint32_t w[16], uint64_t total_bytes) {
  const uint32_t r = uint32_t(total_bytes & 63u);
  RSX_IH_UNROLL
  for (int i = 0; i < 16; ++i) {
    const uint32_t lo = 4u * uint32_t(i);
    if (r >= lo + 4u)
      continue;
    if (r <= lo) {
      w[i] = r == lo ? 0x80u : 0u;
    } else {
      const uint32_t k = 8u * (r - lo); // 8, 16 or 24 bits of the word belong to the message
      w[i] = (w[i] & ((1u << k) - 1u)) | 0x80u << k;
    }
  }
  if (r >= 56u) {
    compress(s, w);
    RSX_IH_UNROLL
    for (int i = 0; i < 14; ++i)
      w[i] = 0u;
  }
  const uint64_t bits = total_bytes << 3;
  w[14] = uint32_t(bits);
  w[15] = uint32_t(bits >> 32);
  compress(s, w);
}

// the sums of the four bytes and of the two 16-bit halves of a word
RSX_IH_FN uint32_t add_bytes(uint32_t acc, uint32_t w) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_sad_u8(w, 0u, acc);
#else
  return acc + (w & 0xFFu) + (w >> 8 & 0xFFu) + (w >> 16 & 0xFFu) + (w >> 24);
#endif
}
RSX_IH_FN uint32_t add_halves(uint32_t acc, uint32_t w) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_sad_u16(w, 0u, acc);
#else
  return acc + (w & 0xFFFFu) + (w >> 16);
#endif
}

// the digest of a state: A, B, C, D, little-endian
inline void store_digest(const uint32_t s[4], uint8_t out[16]) {
  for (int i = 0; i < 4; ++i)
    for (int k = 0; k < 4; ++k)
      out[4 * i + k] = uint8_t(s[i] >> (8 * k));
}

// A row the way a lane of the row kernel takes it: whole blocks, then the rest and the padding
// made in the sixteen words; the two sums while the words pass.  The host reads with memcpy (any
// alignment, never a byte past row_bytes).
inline void hash_row(const uint8_t* row, uint32_t row_bytes, uint32_t s[4], uint64_t* byte_sum,
                     uint64_t* half_sum) {
  uint32_t w[16];
  init_state(s);
  uint64_t bytes = 0, halves = 0;
  const uint32_t blocks = row_bytes / 64u, rest = row_bytes % 64u;
  for (uint32_t b = 0; b <= blocks; ++b) {
    const uint8_t* p = row + size_t(64) * b;
    uint8_t last[64] = {0};
    if (b == blocks) {
      memcpy(last, p, rest);
      p = last;
    }
    RSX_IH_UNROLL
    for (int i = 0; i < 16; ++i)
      w[i] = uint32_t(p[4 * i]) | uint32_t(p[4 * i + 1]) << 8 | uint32_t(p[4 * i + 2]) << 16 |
             uint32_t(p[4 * i + 3]) << 24;
    uint32_t bs = 0, hs = 0;
    RSX_IH_UNROLL
    for (int i = 0; i < 16; ++i) {
      bs = add_bytes(bs, w[i]);
      hs = add_halves(hs, w[i]);
    }
    bytes += bs;
    halves += hs;
    if (b < blocks)
      compress(s, w);
  }
  finish(s, w, row_bytes);
  *byte_sum = bytes;
  *half_sum = halves;
}

// RFC 1321's MD5Init / MD5Update / MD5Final: any length, any alignment, in any pieces
struct Md5 {
  uint32_t s[4];
  uint64_t total;
  uint8_t pending[64]; // the total % 64 bytes no block has taken yet

  Md5() : total(0) {
    init_state(s);
    memset(pending, 0, sizeof pending);
  }
  void block(const uint8_t* p) {
    uint32_t w[16];
    for (int i = 0; i < 16; ++i)
      w[i] = uint32_t(p[4 * i]) | uint32_t(p[4 * i + 1]) << 8 | uint32_t(p[4 * i + 2]) << 16 |
             uint32_t(p[4 * i + 3]) << 24;
    compress(s, w);
  }
  void update(const uint8_t* p, size_t n) {
    size_t have = size_t(total & 63u);
    total += n;
    if (have) {
      const size_t take = n < 64 - have ? n : 64 - have;
      memcpy(pending + have, p, take);
      p += take;
      n -= take;
      have += take;
      if (have < 64)
        return;
      block(pending);
    }
    for (; n >= 64; p += 64, n -= 64)
      block(p);
    if (n)
      memcpy(pending, p, n);
  }
  void final(uint8_t out[16]) {
    const size_t have = size_t(total & 63u);
    uint32_t w[16];
    memset(pending + have, 0, 64 - have);
    for (int i = 0; i < 16; ++i)
      w[i] = uint32_t(pending[4 * i]) | uint32_t(pending[4 * i + 1]) << 8 |
             uint32_t(pending[4 * i + 2]) << 16 | uint32_t(pending[4 * i + 3]) << 24;
    finish(s, w, total);
    store_digest(s, out);
  }
};

} // namespace rsx_imghash
