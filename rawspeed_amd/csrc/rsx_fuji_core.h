// FujiDecompressor (include/rsx.h section 3u), shared by the kernel of rsx_fuji.hip and by a host
// build (rsx_fuji_host.cpp): the container parse and the validation of a call, the bit reader with
// its over-read rule, and the arithmetic of one strip as the reference writes it
// (decompressors/FujiDecompressor.cpp): bitDiff (:432-442), the sample decode (:444-502), the
// gradient quantiser (:168-187, four compares instead of the 2 << raw_bits table), both
// interpolations (:511-563), the X-Trans bit/no-bit pattern (:706-722), the pass order and the
// helper columns (:586-704), the line rotation (:760-777) and the copy-out index maps (:337-405).
//
// A pass is cut the way the device runs it: what depends on the lines above only becomes records
// (even_record: the prediction and the gradient of an even position, final at once where the
// position takes no bits; odd_record: Rb, Rc, whether Rb lies outside [min, max](Rc, Rd), and
// 9 q(Rb - Rc)), and walk() is the serial chain over those records.  The host build runs the same
// cut on one thread a strip.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "rsx.h"

#if defined(__HIPCC__)
#define RSX_FJ_FN __host__ __device__ __forceinline__
#else
#define RSX_FJ_FN inline
#endif

namespace rsx_fuji {

enum Line : int32_t { R0 = 0, R1, R2, R3, R4, G0, G1, G2, G3, G4, G5, G6, G7, B0, B1, B2, B3, B4, LTOTAL };
constexpr int32_t BLOCK = 768;         // block_size: the header check allows no other
constexpr int32_t MAX_LW = 512;        // line_width of X-Trans; Bayer has 384
constexpr int32_t STRIDE = MAX_LW + 2; // samples of a line buffer, helper columns included
constexpr int32_t GRADS = 41;
constexpr int32_t TABLE_INTS = 3 * GRADS * 2; // grad_even resp. grad_odd as {value1, value2} ints
constexpr int32_t ZEROS_CAP = 1 << 20;        // the zero count saturates here (only its size class matters)

struct Params {
  int32_t raw_bits, total, q4, max_diff, escape_at; // escape_at = max_bits - raw_bits - 1
  int32_t lw;                                       // line_width
  int32_t xtrans;
};

// fuji_compressed_params (:189-237) for the depths validate() lets through (14 and 16)
RSX_FJ_FN void params_init(Params* P, int32_t raw_type, int32_t raw_bits) {
  P->raw_bits = raw_bits;
  P->total = 1 << raw_bits;
  P->q4 = P->total - 1;
  P->max_diff = 1 << (raw_bits - 6);
  P->escape_at = raw_bits * (64 / raw_bits) - raw_bits - 1;
  P->xtrans = raw_type == 16;
  P->lw = P->xtrans ? (BLOCK * 2) / 3 : BLOCK >> 1;
}

// ---------------------------------------------------------------------------------------------
// The container (FujiDecompressor's constructor, :850-899) and the checks
// ---------------------------------------------------------------------------------------------
RSX_FJ_FN bool header_ok(const rsx_fuji_desc& d) {
  // FujiHeader::operator bool, :919-937
  const int32_t lh = 6;
  const bool invalid =
      d.signature != 0x4953 || d.version != 1 || d.raw_height > 0x3000 || d.raw_height < lh ||
      d.raw_height % lh || d.raw_width > 0x3000 || d.raw_width < 0x300 || d.raw_width % 24 ||
      d.raw_rounded_width > 0x3000 || d.block_size != 0x300 || d.raw_rounded_width < d.block_size ||
      d.raw_rounded_width % d.block_size || d.raw_rounded_width - d.raw_width >= d.block_size ||
      d.blocks_in_row > 0x10 || d.blocks_in_row == 0 ||
      d.blocks_in_row != d.raw_rounded_width / d.block_size ||
      d.blocks_in_row != (d.raw_width + d.block_size - 1) / d.block_size || d.total_lines > 0x800 ||
      d.total_lines == 0 || d.total_lines != d.raw_height / lh ||
      (d.raw_bits != 12 && d.raw_bits != 14 && d.raw_bits != 16) ||
      (d.raw_type != 16 && d.raw_type != 0);
  return !invalid;
}

inline int parse(const uint8_t* in, size_t in_bytes, rsx_fuji_desc* d) {
  if (!in || !d)
    return RSX_ERR_INVALID_ARG;
  rsx_fuji_desc z = {};
  *d = z;
  if (in_bytes < 16)
    return RSX_ERR_IO;
  auto be16 = [&](size_t at) { return int32_t(in[at]) << 8 | int32_t(in[at + 1]); };
  d->signature = be16(0);
  d->version = in[2];
  d->raw_type = in[3];
  d->raw_bits = in[4];
  d->raw_height = be16(5);
  d->raw_rounded_width = be16(7);
  d->raw_width = be16(9);
  d->block_size = be16(11);
  d->blocks_in_row = in[13];
  d->total_lines = be16(14);
  if (!header_ok(*d))
    return RSX_OK; // (validate refuses it; no strip is read)
  const uint64_t n = uint64_t(d->blocks_in_row);
  uint64_t pos = 16;
  if (in_bytes - pos < 4 * n)
    return RSX_ERR_IO;
  for (uint64_t i = 0; i < n; ++i) {
    const uint8_t* p = in + pos + 4 * i;
    d->strip_bytes[i] = uint32_t(p[0]) << 24 | uint32_t(p[1]) << 16 | uint32_t(p[2]) << 8 | p[3];
  }
  pos += 4 * n;
  if (const uint64_t raw_offset = 4 * n; raw_offset & 0xC) {
    const uint64_t padding = 0x10 - (raw_offset & 0xC);
    if (in_bytes - pos < padding)
      return RSX_ERR_IO;
    pos += padding;
  }
  for (uint64_t i = 0; i < n; ++i) {
    if (in_bytes - pos < d->strip_bytes[i])
      return RSX_ERR_IO;
    d->strip_offset[i] = pos;
    pos += d->strip_bytes[i];
  }
  d->n_strips = int32_t(n);
  return RSX_OK;
}

inline int validate(const rsx_fuji_desc* d, const rsx_image* img) {
  if (!d || !img)
    return RSX_ERR_INVALID_ARG;
  if (img->cpp != 1) // "Unexpected component count / data type" (an rsx_image is UINT16)
    return RSX_ERR_INVALID_ARG;
  if (!header_ok(*d)) // "compressed RAF header check"
    return RSX_ERR_INVALID_ARG;
  if (img->dim_x != d->raw_width || img->dim_y != d->raw_height)
    return RSX_ERR_INVALID_ARG; // "RAF header specifies different dimensions!"
  if (img->pitch_bytes < uint32_t(img->dim_x) * 2u)
    return RSX_ERR_INVALID_ARG;
  if (d->raw_bits == 12)
    return RSX_ERR_UNSUPPORTED; // "Aha, finally, a 12-bit compressed RAF!"
  if ((d->block_size % 3 && d->raw_type == 16) || ((d->block_size & 1) && d->raw_type == 0))
    return RSX_ERR_INVALID_ARG; // "fuji_block_checks"
  if (d->n_strips != d->blocks_in_row) // (a desc that parse() did not complete)
    return RSX_ERR_INVALID_ARG;
  return RSX_OK;
}

// getStream per strip against the bytes the call was given
inline int check_strips(const rsx_fuji_desc& d, uint64_t in_bytes) {
  for (int32_t i = 0; i < d.n_strips; ++i)
    if (d.strip_offset[i] > in_bytes || in_bytes - d.strip_offset[i] < d.strip_bytes[i])
      return RSX_ERR_IO;
  return RSX_OK;
}

// how many columns of strip n go to the image (FujiStrip::width)
RSX_FJ_FN int32_t strip_width(int32_t raw_width, int32_t n) {
  const int32_t left = raw_width - BLOCK * n;
  return left < BLOCK ? left : BLOCK;
}

// What the chain reads from memory.  On the device every lane of the wave runs the chain alike
// (same addresses, same values); telling the compiler so keeps the chain's arithmetic and its
// branches on the scalar unit (1537 ms a frame against 2100 ms with the chain on lane 0's vector
// registers, same run).
RSX_FJ_FN uint32_t uni(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return uint32_t(__builtin_amdgcn_readfirstlane(int32_t(v)));
#else
  return v;
#endif
}

// ---------------------------------------------------------------------------------------------
// BitStreamerMSB as this codec drives it: every request is fill(32).  With c bits consumed and k
// words loaded the cache holds 32 k - c bits; a fill loads word k iff that is below 32, and after
// it k = ceil(c / 32) + 1.  The load of the word at byte 4 k throws iff 4 k > size + 8
// (BitStreamer.h:125-127), so a fill at c fails iff 4 ceil(c / 32) > size + 8.  Bytes behind the
// strip read as zero.  Src::word(k): bytes 4 k .. 4 k + 3 as a big-endian word.
// ---------------------------------------------------------------------------------------------
template <class Src>
struct Bits {
  const Src* src;
  uint32_t size;
  uint64_t buf; // the cache, left-aligned
  int32_t level;
  uint32_t k;
  RSX_FJ_FN void init(const Src* s, uint32_t bytes) {
    src = s;
    size = bytes;
    buf = 0;
    level = 0;
    k = 0;
  }
  RSX_FJ_FN uint64_t consumed() const { return 32ull * k - uint64_t(level); }
  // false: the refill lies more than 8 bytes behind the strip
  RSX_FJ_FN bool fill() {
    if (level >= 32)
      return true;
    if (4ull * k > uint64_t(size) + 8u)
      return false;
    buf |= uint64_t(uni(src->word(k))) << (32 - level);
    level += 32;
    ++k;
    return true;
  }
  RSX_FJ_FN uint32_t peek32() const { return uint32_t(buf >> 32); }
  RSX_FJ_FN void skip(int32_t n) {
    buf = n >= 64 ? 0 : buf << n;
    level -= n;
  }
};

RSX_FJ_FN int32_t clz32(uint32_t v) { return v ? __builtin_clz(v) : 32; }
RSX_FJ_FN int32_t iabs(int32_t v) { return v < 0 ? -v : v; }
RSX_FJ_FN int32_t imax(int32_t a, int32_t b) { return a > b ? a : b; }
RSX_FJ_FN int32_t imin(int32_t a, int32_t b) { return a < b ? a : b; }

RSX_FJ_FN int32_t bit_diff(int32_t value1, int32_t value2) {
  int32_t dec = imax(clz32(uint32_t(value2)) - clz32(uint32_t(value1)), 0);
  if ((value2 << dec) < value1)
    ++dec;
  return imin(dec, 15);
}

// GetGradient (:168-187) of cur_val - q_point[4] = v
RSX_FJ_FN int32_t quant1(int32_t v) {
  const int32_t a = iabs(v);
  const int32_t g = int32_t(a > 0) + int32_t(a >= 0x12) + int32_t(a >= 0x43) + int32_t(a >= 0x114);
  return v < 0 ? -g : g;
}

// fuji_decode_sample: the value, or -1 with *st set.  `tbl`: the 41 {value1, value2} pairs.
template <class Src>
RSX_FJ_FN int32_t decode_sample(Bits<Src>& B, const Params& P, int32_t grad, int32_t interp,
                                int32_t* tbl, int32_t* st) {
  int32_t zeros = 0;
  for (;;) { // (bounded by the strip's bytes: every all-zero batch moves the next fill a word on)
    if (!B.fill()) {
      *st = RSX_ERR_INPUT_OVERFLOW;
      return -1;
    }
    const int32_t n = clz32(B.peek32());
    zeros = imin(zeros + n, ZEROS_CAP);
    B.skip(n == 32 ? 32 : n + 1);
    if (n != 32)
      break;
  }
  int32_t* e = tbl + 2 * iabs(grad);
  int32_t v1 = int32_t(uni(uint32_t(e[0]))), v2 = int32_t(uni(uint32_t(e[1])));
  int32_t bits, delta;
  if (zeros < P.escape_at) {
    bits = bit_diff(v1, v2);
    delta = zeros << bits;
  } else {
    bits = P.raw_bits;
    delta = 1;
  }
  if (!B.fill()) {
    *st = RSX_ERR_INPUT_OVERFLOW;
    return -1;
  }
  int32_t code = 0;
  if (bits) {
    code = int32_t(B.peek32() >> (32 - bits));
    B.skip(bits);
  }
  code += delta;
  if (code < 0 || code >= P.total) {
    *st = RSX_ERR_VALUE_RANGE;
    return -1;
  }
  code = (code & 1) ? -1 - code / 2 : code / 2;
  v1 += iabs(code);
  if (v2 == 0x40) {
    v1 >>= 1;
    v2 >>= 1;
  }
  e[0] = v1;
  e[1] = v2 + 1;
  interp += grad < 0 ? -code : code;
  if (interp < 0)
    interp += P.total;
  else if (interp > P.q4)
    interp -= P.total;
  if (interp < 0)
    return 0;
  return imin(interp, P.q4);
}

// ---------------------------------------------------------------------------------------------
// Records: what a position takes from the lines above
// ---------------------------------------------------------------------------------------------
// whether even position i of component comp of pass `row` is pure interpolation (:710-713)
RSX_FJ_FN bool xtrans_no_bits(int32_t row, int32_t i, int32_t comp) {
  const bool even = (i & 1) == 0;
  if (comp == 0)
    return row == 0 || (row == 2 && even) || (row == 4 && !even) || row == 5;
  return row == 1 || row == 2 || (row == 3 && !even) || (row == 5 && even);
}

// the two lines of pass `row` (fuji_decode_block's colour counters over RGGB, :643-703)
RSX_FJ_FN void pass_lines(int32_t row, int32_t* c0, int32_t* c1) {
  const int32_t h = row >> 1;
  if (row & 1) {
    *c0 = G2 + row;
    *c1 = B2 + h;
  } else {
    *c0 = R2 + h;
    *c1 = G2 + row;
  }
}

// even position col of line c: interp | (grad + 40) << 16 | no_bits << 24.  above1 = line c - 1,
// above2 = line c - 2.
RSX_FJ_FN uint32_t even_record(const uint16_t* above1, const uint16_t* above2, int32_t col,
                               bool no_bits) {
  const int32_t Rb = above1[1 + 2 * col], Rc = above1[2 * col], Rd = above1[2 + 2 * col];
  const int32_t Rf = above2[1 + 2 * col];
  const int32_t dcb = iabs(Rc - Rb), dfb = iabs(Rf - Rb), ddb = iabs(Rd - Rb);
  int32_t t1, t2;
  if (dcb > imax(dfb, ddb)) {
    t1 = Rf;
    t2 = Rd;
  } else {
    t1 = ddb > imax(dcb, dfb) ? Rf : Rd;
    t2 = Rc;
  }
  const int32_t interp = (2 * Rb + t1 + t2) >> 2;
  const int32_t grad = 9 * quant1(Rb - Rf) + quant1(Rc - Rb);
  return uint32_t(interp) | uint32_t(grad + 40) << 16 | uint32_t(no_bits) << 24;
}

// odd position col of line c: {Rb | Rc << 16, (9 q(Rb - Rc) + 36) | outside << 8}
RSX_FJ_FN void odd_record(const uint16_t* above1, int32_t col, uint32_t* r0, uint32_t* r1) {
  const int32_t Rb = above1[2 + 2 * col], Rc = above1[1 + 2 * col], Rd = above1[3 + 2 * col];
  const bool outside = Rb < imin(Rc, Rd) || Rb > imax(Rc, Rd);
  *r0 = uint32_t(Rb) | uint32_t(Rc) << 16;
  *r1 = uint32_t(9 * quant1(Rb - Rc) + 36) | uint32_t(outside) << 8;
}

// Iterations [i0, i1) of a pass's chain (:622-640): the even phase of both lines, and four
// iterations behind it the odd one.  ev: [2][MAX_LW / 2] even records; od: [2][MAX_LW / 2][2] odd
// records; ge, go: grad_even[row % 3], grad_odd[row % 3].  RSX_OK, or the first failure.
template <class Src>
RSX_FJ_FN int32_t walk(Bits<Src>& B, const Params& P, uint16_t* l0, uint16_t* l1, int32_t i0,
                       int32_t i1, const uint32_t* ev, const uint32_t* od, int32_t* ge,
                       int32_t* go) {
  const int32_t half = P.lw / 2;
  int32_t st = RSX_OK;
  for (int32_t i = i0; i < i1; ++i) {
    if (i < half) {
      for (int32_t comp = 0; comp < 2; ++comp) {
        const uint32_t rec = uni(ev[comp * (MAX_LW / 2) + i]);
        if (rec >> 24)
          continue; // (final since the records were made)
        const int32_t v = decode_sample(B, P, int32_t((rec >> 16) & 0xFFu) - 40,
                                        int32_t(rec & 0xFFFFu), ge, &st);
        if (st != RSX_OK)
          return st;
        (comp ? l1 : l0)[1 + 2 * i] = uint16_t(v);
      }
    }
    if (i >= 4) {
      const int32_t col = i - 4;
      for (int32_t comp = 0; comp < 2; ++comp) {
        uint16_t* l = comp ? l1 : l0;
        const uint32_t r0 = uni(od[(comp * (MAX_LW / 2) + col) * 2]);
        const uint32_t r1 = uni(od[(comp * (MAX_LW / 2) + col) * 2 + 1]);
        const int32_t Ra = int32_t(uni(l[1 + 2 * col])), Rg = int32_t(uni(l[3 + 2 * col]));
        const int32_t Rb = int32_t(r0 & 0xFFFFu), Rc = int32_t(r0 >> 16);
        int32_t interp = Ra + Rg;
        if (r1 >> 8)
          interp = (interp + 2 * Rb) >> 1;
        interp >>= 1;
        const int32_t grad = int32_t(r1 & 0xFFu) - 36 + quant1(Rc - Ra);
        const int32_t v = decode_sample(B, P, grad, interp, go, &st);
        if (st != RSX_OK)
          return st;
        l[2 + 2 * col] = uint16_t(v);
      }
    }
  }
  return RSX_OK;
}

// fuji_extend_generic over the colours of a pass (:586-603): `lines` = 18 lines of STRIDE samples
RSX_FJ_FN void extend_one(uint16_t* lines, int32_t i, int32_t lw) {
  lines[i * STRIDE] = lines[(i - 1) * STRIDE + 1];
  lines[i * STRIDE + lw + 1] = lines[(i - 1) * STRIDE + lw];
}

// the rotation behind a line of the strip (:760-777): colour k's first line, its line count
RSX_FJ_FN int32_t colour_first(int32_t k) { return k == 0 ? R0 : k == 1 ? G0 : B0; }
RSX_FJ_FN int32_t colour_count(int32_t k) { return k == 1 ? 8 : 5; }

// copy_line (:337-405): the sample of image row r (0..5) of a line and column x of the strip
RSX_FJ_FN int32_t out_index(bool xtrans, int32_t r, int32_t x) {
  int32_t colour, idx; // 0 red, 1 green, 2 blue
  if (xtrans) {
    // getAsCFAColors(XTransPhase(0, 0)), common/XTransPhase.h:61-71; two bits a cell
    const uint32_t pat[6] = {0x945u, 0x165u, 0x612u, 0x165u, 0x945u, 0x498u};
    const int32_t m = x % 6;
    colour = int32_t(pat[r] >> (2 * m)) & 3;
    const int32_t t = x % 3;
    idx = (((x * 2 / 3) & 0x7FFFFFFE) | (t & 1)) + (t >> 1);
  } else {
    colour = (r & 1) + (x & 1);
    idx = x >> 1;
  }
  const int32_t line = colour == 0 ? R2 + (r >> 1) : colour == 1 ? G2 + r : B2 + (r >> 1);
  return line * STRIDE + 1 + idx;
}

} // namespace rsx_fuji
