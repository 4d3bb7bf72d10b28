// rsx_dctwrite_core.h -- the baseline-DCT JPEG tile writer (include/rsx.h section 7e, DESIGN.md
// 4.29) stated once for host and device: the checks, the container, the quality scaling, the
// per-sample arithmetic (jccolor, jcsample), the per-block arithmetic (jfdctint, the quantiser),
// the block order of a scan with its dummy blocks, and the symbol step of T.81 F.1.2.  The kernels
// of rsx_dctwrite.hip and the host walk of rsx_dctwrite_host.cpp are both made of these.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "rsx.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RSX_DCT_HD __host__ __device__ __forceinline__
#define RSX_DCT_UNROLL _Pragma("unroll")
#else
#define RSX_DCT_HD inline
#define RSX_DCT_UNROLL
#endif

namespace rsx_dctw {

constexpr uint32_t BLOCK_BITS_MAX = 1658; // 9 + 11 of DC, 63 (16 + 10) of AC
constexpr uint32_t BLOCK_BYTES_BOUND = 416;

// ------------------------------------------------------------------------------------ tables
// zig-zag position -> natural index
#define RSX_DCT_ZIGZAG                                                                            \
  {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,        \
   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,        \
   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}
static const uint8_t ZIGZAG[64] = RSX_DCT_ZIGZAG;

// T.81 Annex K.1
static const uint8_t STD_LUMA_Q[64] = {
    16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
    14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
    18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
static const uint8_t STD_CHROMA_Q[64] = {
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
    99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// T.81 Annex K.3: counts of the code lengths 1..16, then the values
static const uint8_t DC_LUMA_BITS[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
static const uint8_t DC_CHROMA_BITS[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
static const uint8_t DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const uint8_t AC_LUMA_BITS[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
static const uint8_t AC_LUMA_VALS[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
    0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0,
    0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
    0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5,
    0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa};
static const uint8_t AC_CHROMA_BITS[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
static const uint8_t AC_CHROMA_VALS[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
    0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
    0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa};

// The encoder's view of the four tables: code and length by symbol; entry [t] is for table t
// (0 luma, 1 chroma).  A length of 0 never occurs for a symbol the walk makes.
struct HuffEnc {
  uint16_t dc_code[2][12];
  uint8_t dc_len[2][12];
  uint16_t ac_code[2][256];
  uint8_t ac_len[2][256];
};

inline void canonical(const uint8_t* bits, const uint8_t* vals, uint16_t* code, uint8_t* len) {
  uint32_t c = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    for (int i = 0; i < bits[l - 1]; ++i, ++k, ++c) {
      code[vals[k]] = uint16_t(c);
      len[vals[k]] = uint8_t(l);
    }
    c <<= 1;
  }
}

inline void build_huff(HuffEnc* h) {
  std::memset(h, 0, sizeof *h);
  canonical(DC_LUMA_BITS, DC_VALS, h->dc_code[0], h->dc_len[0]);
  canonical(DC_CHROMA_BITS, DC_VALS, h->dc_code[1], h->dc_len[1]);
  canonical(AC_LUMA_BITS, AC_LUMA_VALS, h->ac_code[0], h->ac_len[0]);
  canonical(AC_CHROMA_BITS, AC_CHROMA_VALS, h->ac_code[1], h->ac_len[1]);
}

// jpeg_quality_scaling and jpeg_add_quant_table with force_baseline
inline int quality_tables(int quality, uint16_t* luma, uint16_t* chroma) {
  if (quality < 1 || quality > 100 || !luma || !chroma)
    return RSX_ERR_INVALID_ARG;
  const long scale = quality < 50 ? 5000 / quality : 200 - quality * 2;
  for (int i = 0; i < 64; ++i) {
    long a = (long(STD_LUMA_Q[i]) * scale + 50) / 100, b = (long(STD_CHROMA_Q[i]) * scale + 50) / 100;
    luma[i] = uint16_t(a < 1 ? 1 : a > 255 ? 255 : a);
    chroma[i] = uint16_t(b < 1 ? 1 : b > 255 ? 255 : b);
  }
  return RSX_OK;
}

// ---------------------------------------------------------------------------------- geometry
struct Geom {
  uint64_t img_off, out_off, out_cap;
  uint32_t pitch, dim_x, dim_y, n_comp;
  uint32_t off_x, off_y, width, height;
  uint32_t hs, vs;         // luma against chroma
  uint32_t cw, ch;         // chroma plane: ceil(width / hs) x ceil(height / vs)
  uint32_t wib, hib;       // luma plane in blocks
  uint32_t mcus_x, n_mcu;  // MCUs a row, MCUs
  uint32_t bpm;            // blocks an MCU: hs vs (+ 2)
  uint32_t ri, n_int;      // MCUs an interval (n_mcu if there is one interval), intervals
  uint32_t n_blocks;       // n_mcu bpm
  uint32_t hdr_bytes;
  // the plan's (rsx_dctwrite.hip)
  uint32_t first_block, first_bwg, first_int, first_wwg, hdr_off, q_index;
  uint64_t first_word, words_bound;
};

inline int validate(const rsx_dctwrite_desc* d, const rsx_image* img) {
  if (!d || !img)
    return RSX_ERR_INVALID_ARG;
  if (img->dim_x < 1 || img->dim_y < 1 || img->cpp < 1 || img->pitch_bytes % 2u != 0 ||
      uint64_t(img->pitch_bytes) < 2ull * uint64_t(img->cpp) * uint64_t(img->dim_x))
    return RSX_ERR_INVALID_ARG;
  if (d->components != img->cpp)
    return RSX_ERR_INVALID_ARG;
  if (d->off_x >= uint32_t(img->dim_x) || d->off_y >= uint32_t(img->dim_y))
    return RSX_ERR_INVALID_ARG;
  if (d->width < 1 || d->width > 65535u || d->height < 1 || d->height > 65535u)
    return RSX_ERR_INVALID_ARG;
  if (d->restart_interval > 65535u)
    return RSX_ERR_INVALID_ARG;
  if ((d->flags & ~RSX_DCTWRITE_JFIF) != 0 || d->reserved != 0)
    return RSX_ERR_INVALID_ARG;
  for (int t = 0; t < (d->components > 1 ? 2 : 1); ++t)
    for (int i = 0; i < 64; ++i)
      if (d->qtables[t][i] < 1 || d->qtables[t][i] > 255)
        return RSX_ERR_INVALID_ARG;
  if (d->components != 1 && d->components != 3)
    return RSX_ERR_UNSUPPORTED;
  const bool listed = (d->h_samp == 1 && d->v_samp == 1) || (d->h_samp == 2 && d->v_samp == 1) ||
                      (d->h_samp == 2 && d->v_samp == 2);
  if (!listed || (d->components == 1 && d->h_samp * d->v_samp != 1))
    return RSX_ERR_UNSUPPORTED;
  return RSX_OK;
}

inline uint32_t header_bytes(const rsx_dctwrite_desc& d) {
  const uint32_t n = uint32_t(d.components), t = n > 1 ? 2u : 1u;
  return 2u + ((d.flags & RSX_DCTWRITE_JFIF) ? 18u : 0u) + t * 69u + (10u + 3u * n) +
         t * (33u + 183u) + (d.restart_interval ? 6u : 0u) + (8u + 2u * n);
}

// of a descriptor validate() accepts
inline void geom_of(const rsx_dctwrite_desc& d, const rsx_image& img, uint64_t img_off,
                    uint64_t out_off, uint64_t out_cap, Geom* g) {
  std::memset(g, 0, sizeof *g);
  g->img_off = img_off, g->out_off = out_off, g->out_cap = out_cap;
  g->pitch = img.pitch_bytes, g->dim_x = uint32_t(img.dim_x), g->dim_y = uint32_t(img.dim_y);
  g->n_comp = uint32_t(d.components);
  g->off_x = d.off_x, g->off_y = d.off_y, g->width = d.width, g->height = d.height;
  g->hs = uint32_t(d.h_samp), g->vs = uint32_t(d.v_samp);
  g->cw = (d.width + g->hs - 1u) / g->hs, g->ch = (d.height + g->vs - 1u) / g->vs;
  g->wib = (d.width + 7u) / 8u, g->hib = (d.height + 7u) / 8u;
  g->mcus_x = (d.width + 8u * g->hs - 1u) / (8u * g->hs);
  g->n_mcu = g->mcus_x * ((d.height + 8u * g->vs - 1u) / (8u * g->vs));
  g->bpm = g->n_comp == 1 ? 1u : g->hs * g->vs + 2u;
  g->ri = d.restart_interval ? d.restart_interval : g->n_mcu;
  g->n_int = (g->n_mcu + g->ri - 1u) / g->ri;
  g->n_blocks = g->n_mcu * g->bpm; // (at most 8192 x 8192 x 3)
  g->hdr_bytes = header_bytes(d);
}

inline uint64_t bound_of(const Geom& g) {
  return uint64_t(g.hdr_bytes) + uint64_t(g.n_blocks) * BLOCK_BYTES_BOUND + 4ull * g.n_int + 2u;
}

// the bytes SOI .. SOS segment
inline void write_header(const rsx_dctwrite_desc& d, std::vector<uint8_t>* out) {
  std::vector<uint8_t>& o = *out;
  const uint32_t n = uint32_t(d.components);
  auto put = [&](std::initializer_list<int> l) {
    for (int v : l)
      o.push_back(uint8_t(v));
  };
  put({0xFF, 0xD8});
  if (d.flags & RSX_DCTWRITE_JFIF)
    put({0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
  for (uint32_t t = 0; t < (n > 1 ? 2u : 1u); ++t) {
    put({0xFF, 0xDB, 0, 67, int(t)});
    for (int i = 0; i < 64; ++i)
      o.push_back(uint8_t(d.qtables[t][ZIGZAG[i]]));
  }
  put({0xFF, 0xC0, 0, int(8 + 3 * n), 8, int(d.height >> 8), int(d.height & 255), int(d.width >> 8),
       int(d.width & 255), int(n)});
  for (uint32_t c = 0; c < n; ++c)
    put({int(c + 1), c == 0 ? (d.h_samp << 4) | d.v_samp : 0x11, c == 0 ? 0 : 1});
  for (uint32_t t = 0; t < (n > 1 ? 2u : 1u); ++t) {
    const uint8_t* dcb = t ? DC_CHROMA_BITS : DC_LUMA_BITS;
    put({0xFF, 0xC4, 0, 31, int(t)});
    o.insert(o.end(), dcb, dcb + 16);
    o.insert(o.end(), DC_VALS, DC_VALS + 12);
    put({0xFF, 0xC4, 0, 181, int(0x10 | t)});
    o.insert(o.end(), t ? AC_CHROMA_BITS : AC_LUMA_BITS, (t ? AC_CHROMA_BITS : AC_LUMA_BITS) + 16);
    o.insert(o.end(), t ? AC_CHROMA_VALS : AC_LUMA_VALS, (t ? AC_CHROMA_VALS : AC_LUMA_VALS) + 162);
  }
  if (d.restart_interval)
    put({0xFF, 0xDD, 0, 4, int(d.restart_interval >> 8), int(d.restart_interval & 255)});
  put({0xFF, 0xDA, 0, int(6 + 2 * n), int(n)});
  for (uint32_t c = 0; c < n; ++c)
    put({int(c + 1), c == 0 ? 0x00 : 0x11});
  put({0, 63, 0});
}

// ------------------------------------------------------------------------- the order of a scan
// block `lb` of the job in scan order: its component (0 luma, 1 Cb, 2 Cr), its place in the
// component's block grid, and whether it is a dummy
struct Where {
  uint32_t comp, bx, by;
  bool dummy;
};

RSX_DCT_HD Where where_of(const Geom& g, uint32_t lb) {
  Where w;
  const uint32_t m = lb / g.bpm, k = lb - m * g.bpm;
  const uint32_t my = m / g.mcus_x, mx = m - my * g.mcus_x;
  const uint32_t ny = g.hs * g.vs;
  if (g.n_comp == 1 || k < ny) {
    const uint32_t ky = k / g.hs, kx = k - ky * g.hs;
    w.comp = 0;
    w.bx = mx * g.hs + kx;
    w.by = my * g.vs + ky;
    w.dummy = w.bx >= g.wib || w.by >= g.hib;
  } else {
    w.comp = 1u + (k - ny);
    w.bx = mx, w.by = my;
    w.dummy = false; // (ceil(ceil(w / hs) / 8) = ceil(w / (8 hs)))
  }
  return w;
}

// the block whose DC is block lb's predictor: the last real block of lb's component before it in
// the interval; false where there is none (the predictor is 0)
RSX_DCT_HD bool predictor_block(const Geom& g, uint32_t lb, uint32_t* prev) {
  const uint32_t m = lb / g.bpm, k = lb - m * g.bpm;
  const uint32_t ny = g.hs * g.vs;
  const uint32_t first = (m / g.ri) * g.ri * g.bpm; // the interval's first block
  if (g.n_comp != 1 && k >= ny) {
    if (lb < first + g.bpm)
      return false;
    *prev = lb - g.bpm;
    return true;
  }
  // luma: back over the luma blocks, dummies skipped (block 0 of an MCU never is one)
  uint32_t b = lb;
  for (;;) {
    const uint32_t kb = b % g.bpm;
    if (kb != 0)
      b -= 1u;
    else if (b >= first + g.bpm)
      b = b - g.bpm + ny - 1u;
    else
      return false;
    if (!where_of(g, b).dummy)
      break;
  }
  *prev = b;
  return true;
}

// ---------------------------------------------------------------------- per-sample arithmetic
RSX_DCT_HD int ycc_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
RSX_DCT_HD int ycc_cb(int r, int g, int b) {
  return (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16;
}
RSX_DCT_HD int ycc_cr(int r, int g, int b) {
  return (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16;
}

// component `comp` of frame pixel (x, y), x < width and y < height; *over: a sample above 255
RSX_DCT_HD int frame_sample(const Geom& g, const uint8_t* base, uint32_t comp, uint32_t x, uint32_t y,
                            bool* over) {
  const uint32_t ix = g.off_x + x < g.dim_x ? g.off_x + x : g.dim_x - 1u;
  const uint32_t iy = g.off_y + y < g.dim_y ? g.off_y + y : g.dim_y - 1u;
  const uint16_t* p = reinterpret_cast<const uint16_t*>(base + g.img_off + uint64_t(iy) * g.pitch) +
                      uint64_t(ix) * g.n_comp;
  if (g.n_comp == 1) {
    *over |= p[0] > 255u;
    return p[0];
  }
  const int r = p[0], gr = p[1], b = p[2];
  *over |= (r | gr | b) > 255;
  return comp == 0 ? ycc_y(r, gr, b) : comp == 1 ? ycc_cb(r, gr, b) : ycc_cr(r, gr, b);
}

// row r of real block (bx, by) of component `comp`, minus 128
RSX_DCT_HD void block_row(const Geom& g, const uint8_t* base, const Where& w, uint32_t r, int* d,
                          bool* over) {
  const bool sub = w.comp != 0 && g.hs * g.vs != 1;
  if (!sub) {
    uint32_t y = w.by * 8u + r;
    y = y < g.height ? y : g.height - 1u;
    RSX_DCT_UNROLL
    for (uint32_t i = 0; i < 8; ++i) {
      const uint32_t x = w.bx * 8u + i;
      d[i] = frame_sample(g, base, w.comp, x < g.width ? x : g.width - 1u, y, over) - 128;
    }
    return;
  }
  uint32_t cy = w.by * 8u + r;
  cy = cy < g.ch ? cy : g.ch - 1u;
  const uint32_t y0 = g.vs * cy;
  const uint32_t y1 = y0 + 1u < g.height ? y0 + 1u : g.height - 1u;
  RSX_DCT_UNROLL
  for (uint32_t i = 0; i < 8; ++i) {
    const uint32_t cx = w.bx * 8u + i;
    const uint32_t x0 = 2u * cx < g.width ? 2u * cx : g.width - 1u;
    const uint32_t x1 = 2u * cx + 1u < g.width ? 2u * cx + 1u : g.width - 1u;
    int s = frame_sample(g, base, w.comp, x0, y0, over) + frame_sample(g, base, w.comp, x1, y0, over);
    if (g.vs == 2) {
      s += frame_sample(g, base, w.comp, x0, y1, over) + frame_sample(g, base, w.comp, x1, y1, over);
      d[i] = ((s + 1 + int(i & 1u)) >> 2) - 128;
    } else {
      d[i] = ((s + int(i & 1u)) >> 1) - 128;
    }
  }
}

// ----------------------------------------------------------------------- per-block arithmetic
// one pass of jfdctint over 8 values: FIRST is the row pass (results scaled up by 4), the other
// the column pass (that factor removed; the 8 of the transform stays for the quantiser)
RSX_DCT_HD int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

template <bool FIRST>
RSX_DCT_HD void fdct_pass(int* d) {
  constexpr int CB = 13, P1 = 2;
  const int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
  const int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  constexpr int SH = FIRST ? CB - P1 : CB + P1;
  if (FIRST) {
    d[0] = (tmp10 + tmp11) * (1 << P1);
    d[4] = (tmp10 - tmp11) * (1 << P1);
  } else {
    d[0] = descale(tmp10 + tmp11, P1);
    d[4] = descale(tmp10 - tmp11, P1);
  }
  int z1 = (tmp12 + tmp13) * 4433;
  d[2] = descale(z1 + tmp13 * 6270, SH);
  d[6] = descale(z1 + tmp12 * -15137, SH);
  z1 = tmp4 + tmp7;
  int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
  const int z5 = (z3 + z4) * 9633;
  const int t4 = tmp4 * 2446, t5 = tmp5 * 16819, t6 = tmp6 * 25172, t7 = tmp7 * 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  d[7] = descale(t4 + z1 + z3, SH);
  d[5] = descale(t5 + z2 + z4, SH);
  d[3] = descale(t6 + z2 + z3, SH);
  d[1] = descale(t7 + z1 + z4, SH);
}

// sign(x) ((|x| + 4 q) / (8 q)) by the reciprocal of 8 q: recip = floor(2^32 / (8 q)) + 1, exact
// for |x| <= 32767 and q <= 255 (the check program walks all 32768 x 255 pairs)
RSX_DCT_HD uint32_t recip_of(uint32_t q) { return uint32_t((1ull << 32) / (8u * q)) + 1u; }
RSX_DCT_HD int quantise(int x, uint32_t q, uint32_t recip) {
  const uint32_t a = uint32_t(x < 0 ? -x : x) + 4u * q;
  const int v = int((uint64_t(a) * recip) >> 32);
  return x < 0 ? -v : v;
}

// ------------------------------------------------------------------------------ the symbol step
RSX_DCT_HD uint32_t bit_length(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return 32u - uint32_t(__clz(int(v)));
#endif
  uint32_t n = 0;
  while (v) {
    ++n;
    v >>= 1;
  }
  return n;
}

// the bits of a value of category n: the value, or value - 1 in n bits if negative
RSX_DCT_HD uint32_t value_bits(int v, uint32_t n) {
  return uint32_t(v < 0 ? v - 1 : v) & ((1u << n) - 1u);
}

// The symbols of one block to `sink.put(bits, n)` (n <= 16 per call): the DC difference, then the
// ACs of `zz` (64 coefficients in zig-zag order; NULL for a dummy block: none).  COEF(k) reads
// coefficient k; the device reads them as 16-byte words, the host from an array.
template <class Sink, class Coef>
RSX_DCT_HD void walk_block(const HuffEnc& h, uint32_t t, int diff, bool dummy, Coef coef, Sink& sink) {
  const uint32_t nd = bit_length(uint32_t(diff < 0 ? -diff : diff));
  sink.put(h.dc_code[t][nd], h.dc_len[t][nd]);
  if (nd)
    sink.put(value_bits(diff, nd), nd);
  uint32_t run = 0;
  if (!dummy) {
    for (uint32_t k = 1; k < 64; ++k) {
      const int v = coef(k);
      if (v == 0) {
        ++run;
        continue;
      }
      while (run > 15) {
        sink.put(h.ac_code[t][0xF0], h.ac_len[t][0xF0]);
        run -= 16;
      }
      const uint32_t n = bit_length(uint32_t(v < 0 ? -v : v));
      const uint32_t s = (run << 4) | n;
      sink.put(h.ac_code[t][s], h.ac_len[t][s]);
      sink.put(value_bits(v, n), n);
      run = 0;
    }
  } else {
    run = 63;
  }
  if (run)
    sink.put(h.ac_code[t][0], h.ac_len[t][0]);
}

// the bytes of a closed interval of T bits, and the 1-bits that close it
RSX_DCT_HD uint64_t interval_bytes(uint64_t T, uint32_t* ones) {
  const uint64_t b = (T + 7u) >> 3;
  *ones = uint32_t(b * 8u - T);
  return b;
}

} // namespace rsx_dctw
