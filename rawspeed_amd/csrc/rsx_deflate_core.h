// rsx_deflate_core.h -- the deflate writer of F32 DNG tiles (compression 8; include/rsx.h section
// 7d), for the device (rsx_fpwrite_deflate.hip) and the host
// (rsx_fpwrite_host.cpp): the predicted byte planes, the greedy parse of one block, the
// length-limited tables, the bit emit of a block into a scratch of its own, the scan of a tile's
// blocks (dynamic or stored, bit positions, Adler-32) and the byte of the finished stream at any
// position.  Every step is a function of the tile's bytes alone and runs the same statements on
// both sides, so the device stream is the host stream.
//
// The rules, all deterministic:
//   bytes    tests/dng_deflate_files.py::tile_bytes of the narrow samples, zero outside the window.
//   blocks   RSX_FPWRITE_BLOCK input bytes each, the last one shorter.
//   matches  the candidate of position i is the greatest earlier position, at most 32768 back and
//            not before the tile's first byte, whose bytes i..i+2 hash alike (every position is
//            entered, whatever the parse took); distance 1 is tried as well and wins ties; the
//            longer wins; a match ends with its block; length 3..258; a match of length 3 is
//            dropped beyond distance 4096.
//   tables   Huffman lengths of the block's counts (the two least weights merge, ties by node
//            number), limited to 15 (7 for the code-length code): lengths above the limit are
//            set to it, then the longest shorter code of the least count is lengthened while
//            Kraft's sum is above 1, then codes are shortened (the longest that fits the gap,
//            the greatest count first) until it is exactly 1.
//   choice   a block is stored where the stored form, padding included, is not longer.
#pragma once

#include "rsx.h"
#include "rsx_fp_narrow.h"

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RSX_DFL_HD __host__ __device__ inline
#else
#define RSX_DFL_HD inline
#endif

namespace rsx_deflate {

constexpr uint32_t BLOCK = RSX_FPWRITE_BLOCK;
constexpr int HASH_BITS = 12;
constexpr uint32_t HASH_SIZE = 1u << HASH_BITS;
constexpr uint32_t WINDOW = 32768;
constexpr uint32_t TOO_FAR = 4096; // a match of length 3 is taken only up to this distance
constexpr int NLL = 286, ND = 30, NCL = 19;
constexpr uint32_t ADLER_MOD = 65521;
constexpr uint32_t NO_DYNAMIC = 0xFFFFFFFFu; // a block whose tables could not be made: stored

RSX_DFL_HD uint32_t pred_factor(int32_t predictor, uint32_t cpp) {
  return (predictor == 3 ? 1u : predictor == 34894 ? 2u : 4u) * cpp;
}

// rsx_dng_deflate_validate's verdicts in its order (the stream's size check has nothing to look
// at), then the writer's own: pointers and pitch are the caller's to check.
RSX_DFL_HD int validate_tile(const rsx_dng_deflate_desc& d, uint32_t tile_w, uint32_t tile_h,
                             uint32_t off_x, uint32_t off_y, uint32_t width, uint32_t height,
                             const rsx_image& img) {
  if (d.bps != 16 && d.bps != 24 && d.bps != 32)
    return RSX_ERR_INVALID_ARG;
  if (d.predictor != 3 && d.predictor != 34894 && d.predictor != 34895)
    return RSX_ERR_INVALID_ARG;
  if (img.cpp < 1 || img.cpp > 4 || img.dim_x <= 0 || img.dim_y <= 0 || img.pitch_bytes % 4u != 0)
    return RSX_ERR_INVALID_ARG;
  if (tile_w == 0 || tile_h == 0 || width == 0 || height == 0 || width > tile_w || height > tile_h)
    return RSX_ERR_INVALID_ARG;
  if (uint64_t(off_x) + width > uint64_t(img.dim_x) * uint32_t(img.cpp) ||
      uint64_t(off_y) + height > uint64_t(img.dim_y))
    return RSX_ERR_INVALID_ARG;
  if (uint64_t(img.pitch_bytes) < uint64_t(img.dim_x) * uint32_t(img.cpp) * 4u)
    return RSX_ERR_INVALID_ARG;
  // (the reader's limit is 2^32; the writer's block positions are 32-bit counts of bits)
  if (uint64_t(d.bps / 8) * tile_w * uint64_t(tile_h) >= (uint64_t(1) << 28))
    return RSX_ERR_UNSUPPORTED;
  return RSX_OK;
}

RSX_DFL_HD uint32_t blocks_of(uint64_t n_bytes) { return uint32_t((n_bytes + BLOCK - 1) / BLOCK); }

// The closed form: the tile's bytes, 6 bytes a block (3 header bits, up to 7 bits of padding, LEN
// and NLEN), 2 of wrapper, 4 of trailer.  The emit writes single bytes: no word padding.
RSX_DFL_HD uint64_t bound_of(uint64_t n_bytes) { return n_bytes + 6ull * blocks_of(n_bytes) + 6ull; }

struct TileGeom {
  uint64_t img_off;   // the sample (off_y, off_x), from the images' base
  uint64_t out_off;   // the stream's first byte, from the streams' base
  uint64_t out_cap;
  uint64_t plane_off; // the tile's bytes in the plan's plane scratch
  uint32_t img_pitch;
  uint32_t tile_w, tile_h, width, height;
  uint32_t bytesps, pf;
  uint32_t n_bytes, row_bytes;
  uint32_t first_block, n_blocks; // of the plan's flat list of blocks
  uint32_t first_group;           // of the emit kernel's flat list of workgroups
};

RSX_DFL_HD void tile_geom(const rsx_dng_deflate_desc& d, uint32_t tile_w, uint32_t tile_h,
                          uint32_t off_x, uint32_t off_y, uint32_t width, uint32_t height,
                          const rsx_image& img, uint64_t img_off, uint64_t out_off, uint64_t out_cap,
                          TileGeom* g) {
  g->img_off = img_off + uint64_t(off_y) * img.pitch_bytes + uint64_t(off_x) * 4u;
  g->out_off = out_off;
  g->out_cap = out_cap;
  g->plane_off = 0;
  g->img_pitch = img.pitch_bytes;
  g->tile_w = tile_w, g->tile_h = tile_h, g->width = width, g->height = height;
  g->bytesps = uint32_t(d.bps) / 8u;
  g->pf = pred_factor(d.predictor, uint32_t(img.cpp));
  g->row_bytes = tile_w * g->bytesps;
  g->n_bytes = g->row_bytes * tile_h;
  g->first_block = 0;
  g->n_blocks = blocks_of(g->n_bytes);
  g->first_group = 0;
}

// byte `col` of row `row` before the predictor: plane col / tile_w (most significant first) of
// sample col % tile_w; 0 outside the window
RSX_DFL_HD uint32_t raw_byte(const uint8_t* img, const TileGeom& g, uint32_t row, uint32_t col,
                             bool* inexact) {
  const uint32_t p = col / g.tile_w, x = col - p * g.tile_w;
  uint32_t n = 0;
  if (x < g.width && row < g.height) {
    const uint32_t v =
        reinterpret_cast<const uint32_t*>(img + g.img_off + uint64_t(row) * g.img_pitch)[x];
    if (!narrow_fp_bps(v, 8u * g.bytesps, &n)) {
      n = 0;
      *inexact = true;
    }
  }
  return (n >> (8u * (g.bytesps - 1u - p))) & 0xFFu;
}

// byte i of the tile as deflate sees it
RSX_DFL_HD uint8_t plane_byte(const uint8_t* img, const TileGeom& g, uint32_t i, bool* inexact) {
  const uint32_t row = i / g.row_bytes, col = i - row * g.row_bytes;
  uint32_t b = raw_byte(img, g, row, col, inexact);
  if (g.row_bytes > g.pf && col >= g.pf)
    b -= raw_byte(img, g, row, col - g.pf, inexact);
  return uint8_t(b);
}

// ---------------------------------------------------------------------------------------------
// One block
// ---------------------------------------------------------------------------------------------
struct BlockWork {
  int32_t head[HASH_SIZE];
  uint32_t sym[BLOCK];     // a literal, or 1 << 31 | length << 16 | distance - 1
  uint32_t freq[NLL + ND + NCL + 1];
  uint32_t w[2 * NLL];     // the tree under construction: weights,
  uint16_t par[2 * NLL];   //   parents,
  uint16_t act[NLL];       //   live nodes,
  uint16_t leaf[NLL];      //   and the symbol of a leaf
  uint16_t code[NLL + ND + NCL + 1];
  uint8_t len[NLL + ND + NCL + 1];
  uint8_t cls[NLL + ND + 2]; // the code-length symbols of the two tables
  uint8_t clx[NLL + ND + 2]; //   and their extra values
  uint8_t out[BLOCK + 16];   // the dynamic form, from bit 0
  uint32_t n_sym, n_cls;
  uint32_t bits;             // of the dynamic form (NO_DYNAMIC: none)
  uint32_t matches, distances_used;
  uint64_t sum_a, sum_b;     // Adler-32 partials: sum of b, sum of (len - j) b_j
};
constexpr int OFF_D = NLL, OFF_CL = NLL + ND;

RSX_DFL_HD uint32_t hash3(const uint8_t* p) {
  return ((uint32_t(p[0]) << 16 | uint32_t(p[1]) << 8 | p[2]) * 2654435761u) >> (32 - HASH_BITS);
}

RSX_DFL_HD void length_code(uint32_t len, uint32_t* code, uint32_t* eb, uint32_t* extra) {
  const uint32_t l = len - 3u;
  if (len == 258u) {
    *code = 285, *eb = 0, *extra = 0;
  } else if (l < 8u) {
    *code = 257u + l, *eb = 0, *extra = 0;
  } else {
    const uint32_t e = uint32_t(31 - __builtin_clz(l)) - 2u;
    *code = 257u + (e + 1u) * 4u + ((l >> e) & 3u), *eb = e, *extra = l & ((1u << e) - 1u);
  }
}

RSX_DFL_HD void dist_code(uint32_t dist, uint32_t* code, uint32_t* eb, uint32_t* extra) {
  const uint32_t d = dist - 1u;
  if (d < 4u) {
    *code = d, *eb = 0, *extra = 0;
  } else {
    const uint32_t e = uint32_t(31 - __builtin_clz(d)) - 1u;
    *code = 2u * e + 2u + ((d >> e) & 1u), *eb = e, *extra = d & ((1u << e) - 1u);
  }
}

// Huffman lengths of freq[0..n), limited to maxbits, into len[0..n).  Returns the number of used
// symbols, or -1 where the limiter found no code to shorten (the caller stores the block).
RSX_DFL_HD int build_lengths(const uint32_t* freq, int n, int maxbits, uint8_t* len, BlockWork* W) {
  int m = 0;
  for (int i = 0; i < n; ++i) {
    len[i] = 0;
    if (freq[i]) {
      W->w[m] = freq[i];
      W->leaf[m] = uint16_t(i);
      W->act[m] = uint16_t(m);
      ++m;
    }
  }
  if (m == 0)
    return 0;
  if (m == 1) {
    len[W->leaf[0]] = 1;
    return 1;
  }
  int count = m, next = m;
  while (count > 1) {
    int ia = -1, ib = -1; // the least and the second least: by weight, then by node number
    for (int k = 0; k < count; ++k) {
      const uint32_t wk = W->w[W->act[k]];
      if (ia < 0 || wk < W->w[W->act[ia]] || (wk == W->w[W->act[ia]] && W->act[k] < W->act[ia])) {
        ib = ia;
        ia = k;
      } else if (ib < 0 || wk < W->w[W->act[ib]] ||
                 (wk == W->w[W->act[ib]] && W->act[k] < W->act[ib])) {
        ib = k;
      }
    }
    W->w[next] = W->w[W->act[ia]] + W->w[W->act[ib]];
    W->par[W->act[ia]] = uint16_t(next);
    W->par[W->act[ib]] = uint16_t(next);
    W->act[ia] = uint16_t(next);
    W->act[ib] = W->act[count - 1];
    --count;
    ++next;
  }
  const int root = next - 1;
  bool over = false;
  for (int k = 0; k < m; ++k) {
    int d = 0;
    for (int t = k; t != root; t = W->par[t])
      ++d;
    if (d > maxbits) {
      d = maxbits;
      over = true;
    }
    len[W->leaf[k]] = uint8_t(d);
  }
  if (!over)
    return m;
  // Kraft's sum in units of 2^-maxbits
  const uint32_t cap = 1u << maxbits;
  uint32_t K = 0;
  for (int i = 0; i < n; ++i)
    if (len[i])
      K += 1u << (maxbits - len[i]);
  while (K > cap) {
    int pick = -1;
    for (int l = maxbits - 1; l >= 1 && pick < 0; --l)
      for (int i = 0; i < n; ++i)
        if (len[i] == l && (pick < 0 || freq[i] < freq[pick]))
          pick = i;
    if (pick < 0)
      return -1;
    K -= 1u << (maxbits - len[pick] - 1);
    ++len[pick];
  }
  while (K < cap) {
    const uint32_t gap = cap - K;
    int pick = -1;
    for (int l = maxbits; l >= 2 && pick < 0; --l)
      if ((1u << (maxbits - l)) <= gap)
        for (int i = 0; i < n; ++i)
          if (len[i] == l && (pick < 0 || freq[i] > freq[pick]))
            pick = i;
    if (pick < 0)
      return -1;
    K += 1u << (maxbits - len[pick]);
    --len[pick];
  }
  return m;
}

// canonical codes (RFC 1951 3.2.2), bit-reversed: the writer puts bits least significant first
RSX_DFL_HD void assign_codes(const uint8_t* len, int n, int maxbits, uint16_t* code) {
  uint32_t count[16] = {0};
  uint32_t nextc[16];
  for (int i = 0; i < n; ++i)
    ++count[len[i]];
  count[0] = 0;
  uint32_t c = 0;
  for (int b = 1; b <= maxbits; ++b) {
    c = (c + count[b - 1]) << 1;
    nextc[b] = c;
  }
  for (int i = 0; i < n; ++i) {
    const int l = len[i];
    if (!l) {
      code[i] = 0;
      continue;
    }
    uint32_t v = nextc[l]++, r = 0;
    for (int b = 0; b < l; ++b)
      r |= ((v >> b) & 1u) << (l - 1 - b);
    code[i] = uint16_t(r);
  }
}

struct BitWriter {
  uint8_t* buf;
  uint32_t cap, pos, nacc, bits;
  uint64_t acc;
};

RSX_DFL_HD void put(BitWriter& b, uint32_t v, uint32_t n) {
  b.acc |= uint64_t(v) << b.nacc;
  b.nacc += n;
  b.bits += n;
  while (b.nacc >= 8u) {
    if (b.pos < b.cap) // (a form longer than the stored one is never read)
      b.buf[b.pos] = uint8_t(b.acc);
    ++b.pos;
    b.acc >>= 8;
    b.nacc -= 8u;
  }
}

RSX_DFL_HD uint8_t cl_order(int i) {
  return uint8_t("\x10\x11\x12\x00\x08\x07\x09\x06\x0a\x05\x0b\x04\x0c\x03\x0d\x02\x0e\x01\x0f"[i]);
}

// Block [start, start + n) of the tile's bytes `data` (n_total of them) into W: the parse, the
// tables and the dynamic form from bit 0 of W->out.
RSX_DFL_HD void compress_block(const uint8_t* data, uint32_t n_total, uint32_t start, uint32_t n,
                               bool last, BlockWork* W) {
  const uint32_t end = start + n;
  for (uint32_t i = 0; i < HASH_SIZE; ++i)
    W->head[i] = -1;
  for (int i = 0; i < NLL + ND + NCL + 1; ++i)
    W->freq[i] = 0;
  for (uint32_t p = start > WINDOW ? start - WINDOW : 0u; p < start; ++p)
    if (p + 2u < n_total)
      W->head[hash3(data + p)] = int32_t(p);
  uint32_t ns = 0, matches = 0;
  uint64_t sa = 0, sb = 0;
  for (uint32_t j = 0; j < n; ++j) {
    sa += data[start + j];
    sb += uint64_t(n - j) * data[start + j];
  }
  uint32_t i = start;
  while (i < end) {
    const uint32_t maxl = end - i < 258u ? end - i : 258u;
    uint32_t best = 0, bd = 0;
    if (maxl >= 3u) {
      uint32_t l1 = 0, lh = 0, dh = 0;
      if (i >= 1u)
        while (l1 < maxl && data[i + l1] == data[i + l1 - 1u])
          ++l1;
      const int32_t c = W->head[hash3(data + i)];
      if (c >= 0 && i - uint32_t(c) <= WINDOW) {
        dh = i - uint32_t(c);
        while (lh < maxl && data[i + lh] == data[uint32_t(c) + lh])
          ++lh;
      }
      if (l1 >= lh)
        best = l1, bd = 1u;
      else
        best = lh, bd = dh;
      if (best == 3u && bd > TOO_FAR) // three literals are cheaper than a far distance's extra bits
        best = l1 >= 3u ? l1 : 0u, bd = 1u;
    }
    const uint32_t step = best >= 3u ? best : 1u;
    if (best >= 3u) {
      uint32_t lc, dc, eb, ex;
      length_code(best, &lc, &eb, &ex);
      dist_code(bd, &dc, &eb, &ex);
      ++W->freq[lc];
      ++W->freq[OFF_D + dc];
      W->sym[ns++] = 1u << 31 | best << 16 | (bd - 1u);
      ++matches;
    } else {
      ++W->freq[data[i]];
      W->sym[ns++] = data[i];
    }
    for (uint32_t p = i; p < i + step; ++p)
      if (p + 2u < n_total)
        W->head[hash3(data + p)] = int32_t(p);
    i += step;
  }
  W->freq[256] = 1;
  W->n_sym = ns;
  W->matches = matches;
  W->sum_a = sa;
  W->sum_b = sb;
  W->bits = NO_DYNAMIC;
  W->n_cls = 0;
  uint8_t* lll = W->len;
  uint8_t* ld = W->len + OFF_D;
  uint8_t* lcl = W->len + OFF_CL;
  if (build_lengths(W->freq, NLL, 15, lll, W) < 0)
    return;
  const int used_d = build_lengths(W->freq + OFF_D, ND, 15, ld, W);
  if (used_d < 0)
    return;
  W->distances_used = uint32_t(used_d);
  if (used_d == 0)
    ld[0] = 1; // a block without matches still sends one distance code
  int hlit = NLL, hdist = ND;
  while (hlit > 257 && lll[hlit - 1] == 0)
    --hlit;
  while (hdist > 1 && ld[hdist - 1] == 0)
    --hdist;
  // the lengths of both tables as one sequence, run-length coded (16: repeat 3-6, 17: zeros 3-10,
  // 18: zeros 11-138)
  uint32_t nc = 0;
  const int total = hlit + hdist;
  for (int k = 0; k < total;) {
    const uint8_t v = k < hlit ? lll[k] : ld[k - hlit];
    int run = 1;
    while (k + run < total && (k + run < hlit ? lll[k + run] : ld[k + run - hlit]) == v)
      ++run;
    int left = run;
    if (v == 0) {
      while (left >= 11) {
        const int r = left < 138 ? left : 138;
        W->cls[nc] = 18, W->clx[nc++] = uint8_t(r - 11);
        left -= r;
      }
      if (left >= 3) {
        W->cls[nc] = 17, W->clx[nc++] = uint8_t(left - 3);
        left = 0;
      }
    } else {
      W->cls[nc] = v, W->clx[nc++] = 0;
      --left;
      while (left >= 3) {
        const int r = left < 6 ? left : 6;
        W->cls[nc] = 16, W->clx[nc++] = uint8_t(r - 3);
        left -= r;
      }
    }
    for (; left > 0; --left)
      W->cls[nc] = v, W->clx[nc++] = 0;
    k += run;
  }
  W->n_cls = nc;
  for (uint32_t k = 0; k < nc; ++k)
    ++W->freq[OFF_CL + W->cls[k]];
  const int used_cl = build_lengths(W->freq + OFF_CL, NCL, 7, lcl, W);
  if (used_cl < 0)
    return;
  if (used_cl == 1) // a complete code needs a second word
    lcl[lcl[0] ? 1 : 0] = 1;
  assign_codes(lll, NLL, 15, W->code);
  assign_codes(ld, ND, 15, W->code + OFF_D);
  assign_codes(lcl, NCL, 7, W->code + OFF_CL);
  int hclen = NCL;
  while (hclen > 4 && lcl[cl_order(hclen - 1)] == 0)
    --hclen;
  BitWriter b{W->out, uint32_t(sizeof W->out), 0, 0, 0, 0};
  put(b, last ? 1u : 0u, 1);
  put(b, 2u, 2);
  put(b, uint32_t(hlit - 257), 5);
  put(b, uint32_t(hdist - 1), 5);
  put(b, uint32_t(hclen - 4), 4);
  for (int k = 0; k < hclen; ++k)
    put(b, lcl[cl_order(k)], 3);
  for (uint32_t k = 0; k < nc; ++k) {
    const uint32_t s = W->cls[k];
    put(b, W->code[OFF_CL + s], lcl[s]);
    if (s == 16u)
      put(b, W->clx[k], 2);
    else if (s == 17u)
      put(b, W->clx[k], 3);
    else if (s == 18u)
      put(b, W->clx[k], 7);
  }
  for (uint32_t k = 0; k < ns; ++k) {
    const uint32_t s = W->sym[k];
    if (s >> 31) {
      uint32_t lc, dc, eb, ex;
      length_code((s >> 16) & 0x1FFu, &lc, &eb, &ex);
      put(b, W->code[lc], lll[lc]);
      if (eb)
        put(b, ex, eb);
      dist_code((s & 0xFFFFu) + 1u, &dc, &eb, &ex);
      put(b, W->code[OFF_D + dc], ld[dc]);
      if (eb)
        put(b, ex, eb);
    } else {
      put(b, W->code[s], lll[s]);
    }
  }
  put(b, W->code[256], lll[256]);
  W->bits = b.bits;
  if (b.nacc)
    put(b, 0u, 8u - b.nacc);
}

// ---------------------------------------------------------------------------------------------
// A tile's blocks in order
// ---------------------------------------------------------------------------------------------
struct BlockInfo {
  uint32_t pos;    // the block's first bit in the stream
  uint32_t stored; // 1: stored; the padding behind the 3 header bits in bits 8..
};

struct TileInfo {
  int32_t status;
  uint32_t adler;
  uint64_t bytes; // of the stream (0 unless status is RSX_OK)
  uint64_t total_bits;
  uint32_t blocks, stored_blocks;
};

// positions, choices, Adler-32 and the verdict of a tile whose blocks are compressed
RSX_DFL_HD void scan_tile(const TileGeom& g, const BlockWork* works, bool inexact, BlockInfo* info,
                          TileInfo* t) {
  uint64_t pos = 16;
  uint64_t A = 1, B = 0;
  uint32_t n_stored = 0;
  for (uint32_t k = 0; k < g.n_blocks; ++k) {
    const BlockWork& W = works[g.first_block + k];
    const uint32_t n = k + 1u < g.n_blocks ? BLOCK : g.n_bytes - k * BLOCK;
    const uint32_t pad = (8u - uint32_t((pos + 3u) & 7u)) & 7u;
    const uint64_t stored = 3u + pad + 32u + 8ull * n;
    const bool st = W.bits == NO_DYNAMIC || stored <= W.bits;
    info[g.first_block + k].pos = uint32_t(pos);
    info[g.first_block + k].stored = (st ? 1u : 0u) | pad << 8;
    pos += st ? stored : W.bits;
    n_stored += st ? 1u : 0u;
    B = (B + uint64_t(n % ADLER_MOD) * A + W.sum_b) % ADLER_MOD;
    A = (A + W.sum_a) % ADLER_MOD;
  }
  t->adler = uint32_t(B << 16 | A);
  t->total_bits = pos;
  t->blocks = g.n_blocks;
  t->stored_blocks = n_stored;
  const uint64_t bytes = (pos + 7u) / 8u + 4u;
  t->status = inexact ? RSX_ERR_VALUE_RANGE : bytes > g.out_cap ? RSX_ERR_INPUT_OVERFLOW : RSX_OK;
  t->bytes = t->status == RSX_OK ? bytes : 0;
}

// bit `rel` of block k of the tile
RSX_DFL_HD uint32_t block_bit(const TileGeom& g, const BlockWork* works, const BlockInfo* info,
                              const uint8_t* data, uint32_t k, uint32_t rel) {
  const BlockInfo& I = info[g.first_block + k];
  if (!(I.stored & 1u))
    return (works[g.first_block + k].out[rel >> 3] >> (rel & 7u)) & 1u;
  const uint32_t pad = I.stored >> 8;
  if (rel < 3u + pad)
    return rel == 0u && k + 1u == g.n_blocks ? 1u : 0u;
  const uint32_t n = k + 1u < g.n_blocks ? BLOCK : g.n_bytes - k * BLOCK;
  const uint32_t q = rel - 3u - pad, at = q >> 3;
  const uint32_t byte = at == 0u   ? n & 0xFFu
                        : at == 1u ? n >> 8
                        : at == 2u ? ~n & 0xFFu
                        : at == 3u ? (~n >> 8) & 0xFFu
                                   : data[k * BLOCK + at - 4u];
  return (byte >> (q & 7u)) & 1u;
}

// byte j of the tile's stream (j < t.bytes)
RSX_DFL_HD uint8_t stream_byte(const TileGeom& g, const TileInfo& t, const BlockWork* works,
                               const BlockInfo* info, const uint8_t* data, uint64_t j) {
  if (j < 2u)
    return j == 0u ? 0x78 : 0x01; // CMF 0x78, FLG: no FDICT, FCHECK makes 0x7801 a multiple of 31
  if (j + 4u >= t.bytes)
    return uint8_t(t.adler >> (8u * uint32_t(t.bytes - 1u - j)));
  const uint64_t first = 8u * j;
  uint32_t lo = 0, hi = g.n_blocks - 1u;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1u) >> 1;
    if (info[g.first_block + mid].pos <= first)
      lo = mid;
    else
      hi = mid - 1u;
  }
  uint32_t v = 0;
  for (uint32_t b = 0; b < 8u; ++b) {
    const uint64_t bit = first + b;
    if (bit >= t.total_bits)
      break;
    while (lo + 1u < g.n_blocks && info[g.first_block + lo + 1u].pos <= bit)
      ++lo;
    v |= block_bit(g, works, info, data, lo, uint32_t(bit - info[g.first_block + lo].pos)) << b;
  }
  return uint8_t(v);
}

} // namespace rsx_deflate
