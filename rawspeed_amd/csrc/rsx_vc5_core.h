// The arithmetic of VC5Decompressor (include/rsx.h section 4c), shared by the kernels of
// rsx_vc5.hip and by a host build (rsx_vc5_host.cpp): the code book's look-up table, the parse
// of one bit segment of a high-pass band, the inverse wavelet filters and the Bayer merge.
// Everything here compiles as host C++, so the loops that meet damaged streams run on the CPU,
// under sanitizers, before they run on a card.
//
// A band stream (decompressors/VC5Decompressor.cpp:683-742, :948-960) is a sequence of symbols: a
// code word of the book, then one sign bit when the word's value is not zero; a symbol stands
// for `count` coefficients of value * quant.  The decoder carries nothing from one symbol to the
// next but the bit position and the number of coefficients so far, which is what lets a stream
// be parsed from many positions at once: parse_count() walks the symbols that START in one
// segment from a given entry offset and says where it leaves the segment and how many
// coefficients it met; parse_write() repeats the walk once entry and coefficient base are the
// true ones, writes, and gives the band's verdict when it meets the band's end.
//
// The bit reader's rule (BitStreamerMSB, bitstreams/BitStreamer.h:100-132): the decoder refills
// four bytes at a time in front of a symbol, bytes behind the chunk read as zeros, and a refill
// that starts more than eight bytes behind the chunk throws.  In terms of the bit offset c at
// which a symbol starts that is: c > 32 * floor((bytes + 8) / 4) fails.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RSX_VC5_FN __host__ __device__ __forceinline__
#else
#define RSX_VC5_FN inline
#endif

namespace rsx_vc5 {

constexpr uint32_t MAX_CODES = 264;  // CodeTraits<VC5CodeTag>::MaxNumCodeValues
constexpr uint32_t MAX_SIZE = 26;    // ... ::MaxCodeLenghtBits
constexpr uint32_t MAX_COUNT = 511;  // RLVRunLengthBitWidth = 9
constexpr int32_t MAX_VALUE = 1023;  // the 10 bits above the count in a 19-bit code value
constexpr uint32_t L1_BITS = 12, L1_SIZE = 1u << L1_BITS;
#ifndef RSX_VC5_SEG_BITS
#define RSX_VC5_SEG_BITS 128         // (other lengths were measured: DESIGN.md 4.13)
#endif
constexpr uint32_t SEG_BITS = RSX_VC5_SEG_BITS; // bits of a segment: one lane's share of a window
static_assert(SEG_BITS % 32 == 0 && SEG_BITS >= 64, "a segment is whole words and holds a symbol");

// A band's verdict, numbered like the library's statuses (include/rsx.h)
enum : uint32_t {
  B_OK = 0,
  B_MARKER = 1,   // RSX_ERR_INVALID_ARG: a count-0 symbol in front of the last coefficient, a run
                  // past it, or no end marker behind it (the ThrowRDEs of :703-726)
  B_CODE = 3,     // RSX_ERR_BAD_HUFFMAN_CODE: 26 bits that start no code word
  B_OVERREAD = 5, // RSX_ERR_INPUT_OVERFLOW: a symbol that starts behind the reader's limit
  B_RANGE = 10,   // RSX_ERR_VALUE_RANGE: value * quant outside int16_t
  B_NONE = 0xFFFFFFFFu
};

// The look-up table of a code book.  Rows are sorted by their code word left-aligned in 26 bits
// (`start`); prefix-free words own disjoint intervals [start, start + 2^(26 - size)).  l1 is
// indexed by the first 12 bits: bit 31 set -> a word of at most 12 bits owns the whole entry and
// the low bits are its info; else rows [lo, lo + n) (lo = bits 0-8, n = bits 16-24) start inside
// the entry and are searched; n = 0 -> no word starts with these bits.
//   info = size | count << 5 | (value & 0x7FF) << 14
struct Table {
  uint32_t l1[L1_SIZE];
  uint32_t start[MAX_CODES];
  uint32_t info[MAX_CODES];
};
struct TableRef {
  const uint32_t* l1;
  const uint32_t* start;
  const uint32_t* info;
};
constexpr uint32_t L1_DIRECT = 0x80000000u;

RSX_VC5_FN uint32_t i_size(uint32_t info) { return info & 31u; }
RSX_VC5_FN uint32_t i_count(uint32_t info) { return (info >> 5) & 511u; }
RSX_VC5_FN int32_t i_value(uint32_t info) { return int32_t(info << 7) >> 21; } // 11 bits, signed

struct Code {
  uint32_t bits;
  uint8_t size;
  uint16_t count;
  int16_t value;
};

// Builds `t` from n code words; false when the set is not one the decoder can take: no or more
// than 264 words, a size outside 1..26, bits that do not fit the size, a count above 511, a
// |value| above 1023, or two words of which one is a prefix of the other (or equal).
inline bool build_table(const Code* codes, int n, Table* t) {
  if (!codes || n < 1 || n > int(MAX_CODES))
    return false;
  uint32_t order[MAX_CODES];
  for (int i = 0; i < n; ++i) {
    const Code& c = codes[i];
    if (c.size < 1 || c.size > MAX_SIZE || (uint64_t(c.bits) >> c.size) != 0 ||
        c.count > MAX_COUNT || c.value > MAX_VALUE || c.value < -MAX_VALUE)
      return false;
    order[i] = uint32_t(i);
  }
  auto start_of = [&](uint32_t i) { return codes[i].bits << (MAX_SIZE - codes[i].size); };
  for (int i = 1; i < n; ++i) // (insertion sort: 264 rows at most)
    for (int j = i; j > 0 && start_of(order[j - 1]) > start_of(order[j]); --j) {
      const uint32_t x = order[j];
      order[j] = order[j - 1];
      order[j - 1] = x;
    }
  for (uint32_t p = 0; p < L1_SIZE; ++p)
    t->l1[p] = 0;
  for (uint32_t i = 0; i < MAX_CODES; ++i)
    t->start[i] = t->info[i] = 0;
  uint64_t prev_end = 0;
  for (int r = 0; r < n; ++r) {
    const Code& c = codes[order[r]];
    const uint32_t s = start_of(order[r]);
    const uint64_t end = uint64_t(s) + (uint64_t(1) << (MAX_SIZE - c.size));
    if (s < prev_end)
      return false; // overlaps the row before: not prefix-free
    prev_end = end;
    const uint32_t info =
        uint32_t(c.size) | (uint32_t(c.count) << 5) | ((uint32_t(int32_t(c.value)) & 0x7FFu) << 14);
    t->start[r] = s;
    t->info[r] = info;
    const uint32_t p0 = s >> (MAX_SIZE - L1_BITS);
    if (c.size <= L1_BITS) {
      for (uint32_t p = p0; p < uint32_t(end >> (MAX_SIZE - L1_BITS)); ++p)
        t->l1[p] = L1_DIRECT | info;
    } else {
      uint32_t e = t->l1[p0];
      if ((e >> 16) == 0)
        e = uint32_t(r);
      t->l1[p0] = e + (1u << 16); // (rows are sorted: those of one entry are neighbours)
    }
  }
  return true;
}

// the info of the word that the 26 bits x start with, or B_NONE
RSX_VC5_FN uint32_t lookup(const TableRef& t, uint32_t x) {
  const uint32_t e = t.l1[x >> (MAX_SIZE - L1_BITS)];
  if (e & L1_DIRECT)
    return e & 0x01FFFFFFu;
  uint32_t lo = e & 0x1FFu, n = (e >> 16) & 0x1FFu;
  if (n == 0)
    return B_NONE;
  uint32_t hi = lo + n;
  while (hi - lo > 1) { // the last row of [lo, hi) that starts at or in front of x
    const uint32_t mid = (lo + hi) >> 1;
    if (t.start[mid] <= x)
      lo = mid;
    else
      hi = mid;
  }
  if (lo >= MAX_CODES)
    return B_NONE;
  const uint32_t s = t.start[lo], info = t.info[lo];
  if (s > x || x - s >= (1u << (MAX_SIZE - i_size(info))))
    return B_NONE;
  return info;
}

// One symbol from the 27 bits x (the stream's next bits, left-aligned in 27).
struct Symbol {
  uint32_t len;   // bits of the symbol: the word and its sign bit; 0: no word
  uint32_t count;
  int32_t value;  // signed, not yet dequantised
};
RSX_VC5_FN Symbol symbol(const TableRef& t, uint32_t x27) {
  Symbol s;
  const uint32_t info = lookup(t, x27 >> 1);
  if (info == B_NONE) {
    s.len = 0, s.count = 0, s.value = 0;
    return s;
  }
  const uint32_t size = i_size(info);
  int32_t v = i_value(info);
  s.len = size;
  if (v != 0) {
    if ((x27 >> (MAX_SIZE - size)) & 1u)
      v = -v;
    s.len = size + 1;
  }
  s.count = i_count(info);
  s.value = v;
  return s;
}

RSX_VC5_FN bool fits_i16(int32_t v) { return v >= -32768 && v <= 32767; }

// the last bit offset at which a symbol of a chunk of `bytes` bytes may start
RSX_VC5_FN uint64_t start_limit(uint32_t bytes) { return 32ull * ((uint64_t(bytes) + 8u) / 4u); }

// What a lane learns from a segment.
struct SegCount {
  uint32_t exit;  // bits by which the last symbol reaches into the next segment
  uint32_t ncoef; // coefficients of the symbols walked
  uint32_t term;  // 1: the walk stopped at a symbol that ends or fails the band wherever it lies:
                  // behind the limit, no word, a count of 0, a product outside int16_t
};

// R: peek27(pos) = the 27 bits at bit `pos` of the window, zeros behind the chunk.  The walk
// covers the symbols that start in [pos, seg_end); `lim` = start_limit - the window's first bit,
// clamped to [-1, 2^30].
template <class R>
RSX_VC5_FN SegCount parse_count(const R& rd, const TableRef& t, int32_t quant, uint32_t pos,
                                uint32_t seg_end, int32_t lim) {
  SegCount c;
  c.ncoef = 0, c.term = 0;
  while (pos < seg_end) {
    if (int32_t(pos) > lim) {
      c.term = 1;
      break;
    }
    const Symbol s = symbol(t, rd.peek27(pos));
    if (s.len == 0 || s.count == 0 || !fits_i16(s.value * quant)) {
      c.term = 1;
      break;
    }
    c.ncoef += s.count;
    pos += s.len;
  }
  c.exit = c.term ? 0u : pos - seg_end;
  return c;
}

// The same walk with the true entry and the true number `p` of coefficients in front of it;
// writes the non-zero runs to out[0, n) and returns B_NONE, or the band's verdict when the walk
// meets the band's end: the symbol behind coefficient n - 1 (wherever it starts) must be the end
// marker -- value +1, count 0, not dequantised (verifyIsAtEnd, :703-711) -- and every symbol in
// front of it goes through decode() (:713-730): dequantised, then a count of 0 is an error.
template <class R>
RSX_VC5_FN uint32_t parse_write(const R& rd, const TableRef& t, int32_t quant, uint32_t pos,
                                uint32_t seg_end, int32_t lim, uint32_t p, uint32_t n,
                                int16_t* out) {
  while (pos < seg_end || p == n) {
    if (int32_t(pos) > lim)
      return B_OVERREAD;
    const Symbol s = symbol(t, rd.peek27(pos));
    if (s.len == 0)
      return B_CODE;
    if (p == n)
      return s.value == 1 && s.count == 0 ? B_OK : B_MARKER;
    const int32_t v = s.value * quant;
    if (!fits_i16(v))
      return B_RANGE;
    if (s.count == 0)
      return B_MARKER;
    const uint32_t room = n - p, run = s.count < room ? s.count : room;
    if (v != 0)
      for (uint32_t k = 0; k < run; ++k)
        out[p + k] = int16_t(v);
    if (s.count > room)
      return B_MARKER; // "Not all pixels consumed"
    p += s.count;
    pos += s.len;
  }
  return B_NONE;
}

// ---------------------------------------------------------------------------------------------
// Inverse wavelet (:137-287).  kind: 0 the first row / column, 1 a middle one, 2 the last; the
// three lows are rows / columns r, r + 1, r + 2 with r = 0, x - 1, x - 2 for the three kinds.
// ---------------------------------------------------------------------------------------------
RSX_VC5_FN int32_t convolute(int32_t m0, int32_t m1, int32_t m2, int32_t m3, int32_t high,
                             int32_t l0, int32_t l1, int32_t l2, int32_t shift) {
  const int32_t lows = (m1 * l0 + m2 * l1 + m3 * l2 + 4) >> 3;
  int32_t total = m0 * high + lows;
  total *= 1 << shift;
  return total >> 1;
}
RSX_VC5_FN void filter_pair(int kind, int32_t high, int32_t l0, int32_t l1, int32_t l2,
                            int32_t shift, int32_t* even, int32_t* odd) {
  if (kind == 0) {
    *even = convolute(1, 11, -4, 1, high, l0, l1, l2, shift);
    *odd = convolute(-1, 5, 4, -1, high, l0, l1, l2, shift);
  } else if (kind == 1) {
    *even = convolute(1, 1, 8, -1, high, l0, l1, l2, shift);
    *odd = convolute(-1, -1, 8, 1, high, l0, l1, l2, shift);
  } else {
    *even = convolute(1, -1, 4, 5, high, l0, l1, l2, shift);
    *odd = convolute(-1, 1, -4, 11, high, l0, l1, l2, shift);
  }
}
RSX_VC5_FN int edge_kind(uint32_t x, uint32_t n) { return x == 0 ? 0 : (x + 1 < n ? 1 : 2); }
RSX_VC5_FN uint32_t edge_first(uint32_t x, int kind) { return kind == 0 ? 0u : x - uint32_t(kind); }
RSX_VC5_FN int32_t trunc16(int32_t v) { return int32_t(int16_t(uint16_t(uint32_t(v)))); }
RSX_VC5_FN int32_t clamp14(int32_t v) { return v < 0 ? 0 : (v > 16383 ? 16383 : v); }

// One level of one channel: bands 0..3 of w x h coefficients (band 0 with its own pitch), the
// result 2w x 2h with pitch 2w.  cell (r, c) -> out rows 2r, 2r + 1, columns 2c, 2c + 1.
struct LevelView {
  const int16_t* b0;
  const int16_t* b1;
  const int16_t* b2;
  const int16_t* b3;
  uint32_t pitch0, w, h;
  int32_t shift; // descaleShift: 2 when the level's prescale is 2
  int32_t clamp; // the last level: clampBits(., 14)
};
// the vertical pass at column `col` for row pair r: the two rows of one intermediate
RSX_VC5_FN void vertical(const int16_t* high, uint32_t hpitch, const int16_t* low, uint32_t lpitch,
                         uint32_t r, uint32_t h, uint32_t col, int32_t* even, int32_t* odd) {
  const int kind = edge_kind(r, h);
  const uint32_t r0 = edge_first(r, kind);
  const int16_t* l = low + uint64_t(r0) * lpitch + col;
  int32_t e, o;
  filter_pair(kind, high[uint64_t(r) * hpitch + col], l[0], l[lpitch], l[2 * uint64_t(lpitch)], 0,
              &e, &o);
  *even = trunc16(e);
  *odd = trunc16(o);
}
// out[0..1] = row 2r, out[2..3] = row 2r + 1 (columns 2c, 2c + 1), as stored
RSX_VC5_FN void level_cell(const LevelView& L, uint32_t r, uint32_t c, int16_t out[4]) {
  const int kind = edge_kind(c, L.w);
  const uint32_t c0 = edge_first(c, kind);
  int32_t le[3], lo[3], he, ho;
#pragma unroll
  for (uint32_t k = 0; k < 3; ++k) // the low-pass intermediate: high = band 2, low = band 0
    vertical(L.b2, L.w, L.b0, L.pitch0, r, L.h, c0 + k, &le[k], &lo[k]);
  vertical(L.b3, L.w, L.b1, L.w, r, L.h, c, &he, &ho); // the high-pass one: band 3, band 1
  int32_t v[4];
  filter_pair(kind, he, le[0], le[1], le[2], L.shift, &v[0], &v[1]);
  filter_pair(kind, ho, lo[0], lo[1], lo[2], L.shift, &v[2], &v[3]);
#pragma unroll
  for (int k = 0; k < 4; ++k)
    out[k] = int16_t(uint16_t(uint32_t(L.clamp ? clamp14(v[k]) : v[k])));
}

// ---------------------------------------------------------------------------------------------
// The merge of a 2x2 cell (:900-928): px[0..1] the upper row, px[2..3] the lower one.
// ---------------------------------------------------------------------------------------------
RSX_VC5_FN uint16_t log_lookup(const uint16_t* table, int32_t v) {
  return table[v < 0 ? 0 : (v > 4095 ? 4095 : v)];
}
RSX_VC5_FN void merge_cell(int32_t gs, int32_t rg, int32_t bg, int32_t gd, int phase,
                           const uint16_t* table, uint16_t px[4]) {
  rg -= 2048, bg -= 2048, gd -= 2048;
  const uint16_t r = log_lookup(table, gs + 2 * rg), b = log_lookup(table, gs + 2 * bg);
  const uint16_t g1 = log_lookup(table, gs + gd), g2 = log_lookup(table, gs - gd);
  if (phase == 0) // RGGB
    px[0] = r, px[1] = g1, px[2] = g2, px[3] = b;
  else // GBRG: the rows change places, the greens keep their order (applyStablePhaseShift)
    px[0] = g1, px[1] = b, px[2] = r, px[3] = g2;
}

// the size of wavelet `k` (0: the channel plane, 1..3: the levels) of an image dimension
RSX_VC5_FN uint32_t level_dim(uint32_t image_dim, int k) {
  uint32_t d = image_dim;
  for (int i = 0; i <= k; ++i)
    d = (d + 1) / 2;
  return d;
}

} // namespace rsx_vc5
