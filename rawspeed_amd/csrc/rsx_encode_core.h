// rsx_encode_core.h -- the arithmetic of the writers (include/rsx.h section 7):
// the inverse of UncompressedDecompressor::decodePackedInt (what bitstreams/BitVacuumer{LSB,MSB,
// MSB16,MSB32}.h write) and the inverse of LJpegDecompressor::decode (codes/
// PrefixCodeVectorEncoder.h + bitstreams/BitVacuumerJPEG.h).  Plain C++ that builds for the host
// (rsx_encode_host.cpp, one thread) and for the device (rsx_encode_pack.hip, rsx_encode_ljpeg.hip):
// the checks, the canonical code, the per-sample step, the tail rules, and a single-threaded walk
// of whole jobs that the device is held against.
#pragma once

#include "rsx.h"

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RSX_ENC_HD __host__ __device__ __forceinline__
#else
#define RSX_ENC_HD inline
#endif

namespace rsx_encode {

// ---------------------------------------------------------------------------------------------
// Packed integers
// ---------------------------------------------------------------------------------------------
constexpr int PACK_LANE_BYTES = 16;                             // a lane's piece of the output
constexpr int PACK_THREADS = 256;                               // lanes of a workgroup
constexpr int PACK_BLOCK_BYTES = PACK_LANE_BYTES * PACK_THREADS; // a workgroup's piece

RSX_ENC_HD uint64_t round_up4(uint64_t v) { return (v + 3u) & ~uint64_t(3); }

// rsx_unpack_validate's checks on the geometry in its order (UncompressedDecompressor.cpp:106-169;
// the reader's input is the stream this writes, so the size check is the 32-bit one alone), then
// what a writer needs beyond a reader: the rows it reads exist, and the output has room.
// One deliberate difference from handing BitVacuumer::put() an oversized value: a sample's bits
// above bits_per_pixel are dropped here (BitStreamCache::push does not mask; rsx_synth_pack_rows
// does), so any image is accepted.
RSX_ENC_HD int validate_pack(const rsx_unpack_desc* d, const rsx_image* img, uint64_t out_cap) {
  if (!d || !img)
    return RSX_ERR_INVALID_ARG;
  const uint64_t need = uint64_t(uint32_t(d->crop_h)) * uint64_t(uint32_t(d->input_pitch_bytes));
  if (need > 0xFFFFFFFFull)
    return RSX_ERR_IO;
  if (d->crop_w <= 0 || d->crop_h <= 0)
    return RSX_ERR_INVALID_ARG;
  if (d->input_pitch_bytes < 1)
    return RSX_ERR_INVALID_ARG;
  if (d->bit_order < RSX_ORDER_LSB || d->bit_order > RSX_ORDER_MSB32)
    return RSX_ERR_INVALID_ARG;
  if (img->cpp < 1 || img->cpp > 3)
    return RSX_ERR_INVALID_ARG;
  if (d->bits_per_pixel > 16 && d->bits_per_pixel <= 32)
    return RSX_ERR_UNSUPPORTED; // the widths of F32 images: integer images only
  if (d->bits_per_pixel < 1 || d->bits_per_pixel > 16)
    return RSX_ERR_INVALID_ARG;
  const uint64_t bits = uint64_t(d->crop_w) * uint64_t(img->cpp) * uint64_t(d->bits_per_pixel);
  if (bits % 8 != 0)
    return RSX_ERR_INVALID_ARG;
  if (uint64_t(d->input_pitch_bytes) < bits / 8)
    return RSX_ERR_INVALID_ARG;
  if (d->crop_x < 0 || d->crop_y < 0)
    return RSX_ERR_INVALID_ARG;
  if (uint64_t(d->crop_y) > uint64_t(img->dim_y))
    return RSX_ERR_INVALID_ARG;
  if (uint64_t(d->crop_x) + uint64_t(d->crop_w) > uint64_t(img->dim_x))
    return RSX_ERR_INVALID_ARG;
  const bool copy_path = d->bit_order == RSX_ORDER_LSB && d->bits_per_pixel == 16;
  if (!copy_path && need < 4)
    return RSX_ERR_IO;
  // the writer's own: every row read lies in the image, rows hold their samples
  if (uint64_t(d->crop_y) + uint64_t(d->crop_h) > uint64_t(img->dim_y))
    return RSX_ERR_INVALID_ARG;
  if (img->pitch_bytes % 2 != 0 ||
      uint64_t(img->pitch_bytes) < uint64_t(d->crop_w) * uint64_t(img->cpp) * 2u)
    return RSX_ERR_INVALID_ARG;
  if (out_cap < round_up4(need))
    return RSX_ERR_INVALID_ARG;
  return RSX_OK;
}

struct PackGeom {
  uint64_t img_off;      // first row read, from the images' base
  uint64_t out_off;      // first byte written, from the streams' base
  uint64_t stream_bytes; // crop_h * pitch
  uint64_t out_bytes;    // round_up4(stream_bytes): BitVacuumer::flush pads to a 32-bit chunk
  uint32_t img_pitch;
  uint32_t pitch;        // of the stream
  uint32_t row_bytes;    // of a stream row that hold samples
  uint32_t bps;
  uint32_t order;
  uint32_t first_block;  // of the plan's flat list of workgroups
};

RSX_ENC_HD void pack_geom(const rsx_unpack_desc& d, const rsx_image& img, uint64_t img_off,
                          uint64_t out_off, PackGeom* g) {
  g->img_off = img_off + uint64_t(d.crop_y) * img.pitch_bytes;
  g->out_off = out_off;
  g->stream_bytes = uint64_t(d.crop_h) * uint64_t(d.input_pitch_bytes);
  g->out_bytes = round_up4(g->stream_bytes);
  g->img_pitch = img.pitch_bytes;
  g->pitch = uint32_t(d.input_pitch_bytes);
  g->row_bytes = uint32_t(uint64_t(d.crop_w) * uint64_t(img.cpp) * uint64_t(d.bits_per_pixel) / 8);
  g->bps = uint32_t(d.bits_per_pixel);
  g->order = uint32_t(d.bit_order);
  g->first_block = 0;
}

RSX_ENC_HD void or_word(uint32_t (&w)[4], int i, uint32_t v) {
  // (no indexing by a variable: the four words stay in registers)
  w[0] |= i == 0 ? v : 0u;
  w[1] |= i == 1 ? v : 0u;
  w[2] |= i == 2 ? v : 0u;
  w[3] |= i == 3 ? v : 0u;
}

RSX_ENC_HD uint32_t bswap32(uint32_t v) {
  return v >> 24 | (v >> 8 & 0xFF00u) | (v << 8 & 0xFF0000u) | v << 24;
}

// The 16 bytes [16 k, 16 k + 16) of the output of job g, as four little-endian words: the samples
// that cover them, gathered.  Stream byte s lies in memory at s (LSB, MSB), s ^ 1 (MSB16) or s ^ 3
// (MSB32), and 16 k is a multiple of every chunk size, so the 16 memory bytes are
// the 16 stream bytes of the same range, permuted.  Bytes of the pitch beyond row_bytes and bytes
// beyond stream_bytes are zero.  `img` is the images' base.
// I: the type the byte and bit positions are computed in.  uint32_t serves every stream the
// validation accepts (crop_h * pitch <= 0xFFFFFFFF) whose rows are shorter than 2^28 bytes (the bit
// position of a sample in its row then fits); uint64_t serves the rest.
template <class I>
RSX_ENC_HD void pack_chunk_t(const uint8_t* img, const PackGeom& g, I k, uint32_t (&out)[4]) {
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  const I begin = k * I(16), stream = I(g.stream_bytes), pitch = I(g.pitch);
  // (begin + 16 may pass 2^32: the comparison is made on what is left)
  const I end = stream - begin < I(16) ? stream : begin + I(16);
  const uint32_t bps = g.bps, mask = (1u << bps) - 1u;
  const bool lsb = g.order == RSX_ORDER_LSB;
  I pos = begin;
  while (pos < end) {
    const I r = pos / pitch, row0 = r * pitch;
    // (row0 + pitch may pass 2^32 too)
    const I seg_end = end - row0 < pitch ? end : row0 + pitch;
    const I b = pos - row0;
    I b_end = seg_end - row0;
    if (b_end > I(g.row_bytes))
      b_end = I(g.row_bytes);
    if (b < b_end) {
      const uint16_t* src =
          reinterpret_cast<const uint16_t*>(img + g.img_off + uint64_t(r) * g.img_pitch);
      const I x0 = I(8) * b / I(bps), x1 = (I(8) * b_end - I(1)) / I(bps);
      // bit of sample x in the 128 of this piece: from -15 up
      const int lead = int(pos - begin) * 8;
      for (I x = x0; x <= x1; ++x) {
        int rel = lead + int(x * I(bps) - I(8) * b);
        uint64_t t = src[x] & mask;
        if (lsb) {
          if (rel < 0) {
            t >>= -rel;
            rel = 0;
          }
          t <<= rel & 31;
          or_word(w, rel >> 5, uint32_t(t));
          or_word(w, (rel >> 5) + 1, uint32_t(t >> 32));
        } else {
          // w[i] holds stream bytes 4 i .. 4 i + 3, the first one on top
          t <<= 64u - bps;
          if (rel < 0) {
            t <<= -rel;
            rel = 0;
          }
          t >>= rel & 31;
          or_word(w, rel >> 5, uint32_t(t >> 32));
          or_word(w, (rel >> 5) + 1, uint32_t(t));
        }
      }
    }
    pos = seg_end;
  }
  for (int i = 0; i < 4; ++i)
    out[i] = g.order == RSX_ORDER_MSB     ? bswap32(w[i])
             : g.order == RSX_ORDER_MSB16 ? (w[i] << 16 | w[i] >> 16)
                                          : w[i];
}

RSX_ENC_HD bool pack_fits_32_bits(const PackGeom& g) {
  return g.stream_bytes <= 0xFFFFFFFFull && g.row_bytes < (1u << 28);
}

RSX_ENC_HD void pack_chunk(const uint8_t* img, const PackGeom& g, uint64_t k, uint32_t (&out)[4]) {
  if (pack_fits_32_bits(g))
    pack_chunk_t<uint32_t>(img, g, uint32_t(k), out);
  else
    pack_chunk_t<uint64_t>(img, g, k, out);
}

// The reference walk of one job: a chunk after the other.
inline void pack_walk(const uint8_t* img, const PackGeom& g, uint8_t* out) {
  for (uint64_t k = 0; k * 16u < g.out_bytes; ++k) {
    uint32_t w[4];
    pack_chunk(img, g, k, w);
    for (uint64_t i = 0; i < 16u && k * 16u + i < g.out_bytes; ++i)
      out[g.out_off + k * 16u + i] = uint8_t(w[i >> 2] >> (8u * (i & 3u)));
  }
}

// ---------------------------------------------------------------------------------------------
// Lossless JPEG, predictor 1
// ---------------------------------------------------------------------------------------------
constexpr int LJPEG_THREADS = 256; // lanes of a workgroup: a lane a sample
constexpr int LJPEG_RUN = 256;     // samples of one job a workgroup owns
constexpr int N_CATEGORIES = 17;   // SSSS 0..16

// A symbol word is a code of at most 16 bits followed by at most 16 difference bits.
constexpr int MAX_CODE_BITS = 16, MAX_DIFF_BITS = 16;
static_assert(MAX_CODE_BITS + MAX_DIFF_BITS <= 32, "a symbol word fits one 32-bit word");
// ... so a workgroup's samples fill at most LJPEG_RUN words of the un-stuffed stream
constexpr int LJPEG_RUN_BYTES = LJPEG_RUN * 4;

// The canonical code of a DHT (HuffmanCode.h:66-92, the derivation validate_huff_table accepts),
// by category.  A category listed twice keeps its first code: PrefixCodeVectorEncoder::
// getCodeIndexOfCodeValue returns the first match.
struct EncTable {
  uint16_t code[N_CATEGORIES];
  uint8_t len[N_CATEGORIES]; // 0: the table lacks the category
  uint8_t fix16;
};

inline void build_enc_table(const rsx_huff_table& t, EncTable* e) {
  for (int i = 0; i < N_CATEGORIES; ++i)
    e->code[i] = 0, e->len[i] = 0;
  e->fix16 = t.fix_dng_bug16 ? 1 : 0;
  uint32_t code = 0;
  unsigned k = 0;
  for (int l = 1; l <= 16; ++l) {
    for (unsigned i = 0; i < t.n_codes_per_length[l - 1] && k < t.n_code_values; ++i, ++k) {
      const unsigned v = t.code_values[k];
      if (v < unsigned(N_CATEGORIES) && e->len[v] == 0) {
        e->code[v] = uint16_t(code);
        e->len[v] = uint8_t(l);
      }
      ++code;
    }
    code <<= 1;
  }
}

// AbstractPrefixCodeEncoder::reduce (AbstractPrefixCodeEncoder.h:48-58) of a 16-bit difference:
// the category and the bits that follow the code.  -32768 has category 16.
RSX_ENC_HD void reduce(int32_t d, uint32_t* diff, uint32_t* ssss) {
  uint32_t a = uint32_t(d < 0 ? -d : d), n = 0;
  while (a) {
    ++n;
    a >>= 1;
  }
  *ssss = n;
  *diff = (d >= 0 ? uint32_t(d) : uint32_t(d - 1)) & ((1u << n) - 1u);
}

RSX_ENC_HD uint32_t category(int32_t d) {
  uint32_t diff, ssss;
  reduce(d, &diff, &ssss);
  return ssss;
}

// The symbol word of difference d under table e, right-aligned, and its length in bits: the code,
// then the ssss low bits; for ssss 16 the code alone, or with fix_dng_bug16 the code and 16 zero
// bits (what the reader skips: PrefixCodeVectorEncoder.h:80-90).  Length 0: e lacks the category.
RSX_ENC_HD uint32_t symbol(const uint16_t* code, const uint8_t* len, uint32_t fix16, int32_t d,
                           uint32_t* n_bits) {
  uint32_t diff, ssss;
  reduce(d, &diff, &ssss);
  const uint32_t l = len[ssss];
  if (l == 0) {
    *n_bits = 0;
    return 0;
  }
  uint32_t extra = ssss;
  if (ssss == 16) {
    extra = fix16 ? 16u : 0u;
    diff = 0;
  }
  *n_bits = l + extra;
  return extra == 0 ? uint32_t(code[ssss]) : (uint32_t(code[ssss]) << extra | diff);
}

// the subset of rsx_ljpeg_desc whose every decoded pixel exists in the image (after
// rsx_ljpeg_validate has accepted the descriptor)
RSX_ENC_HD int validate_ljpeg_subset(const rsx_ljpeg_desc& d, const rsx_image& img) {
  if (d.mcu_h != 1 || d.mcu_w != d.n_comp || d.n_comp < 1 || d.n_comp > 4)
    return RSX_ERR_UNSUPPORTED; // MCU 2x2
  if (int64_t(d.frame_w) * d.mcu_w != int64_t(img.cpp) * d.tile_w)
    return RSX_ERR_UNSUPPORTED; // a wider frame or a trailing partial MCU
  if (d.frame_h != d.tile_h)
    return RSX_ERR_UNSUPPORTED;
  if (img.pitch_bytes % 2 != 0 || uint64_t(img.pitch_bytes) < uint64_t(img.dim_x) * img.cpp * 2u)
    return RSX_ERR_INVALID_ARG;
  return RSX_OK;
}

struct LJpegGeom {
  uint64_t img_off;      // sample (row 0, 0) of the tile, from the images' base
  uint64_t out_off, out_cap;
  uint32_t img_pitch;
  uint32_t rows, row_samples, n_comp;
  uint32_t rpi;          // rows of an interval (>= rows: one interval)
  uint32_t n_int;        // intervals
  uint32_t int_blocks;   // workgroups of a whole interval
  uint32_t first_block;  // of the plan's flat list of workgroups
  uint32_t n_blocks;
  uint32_t first_int;    // of the plan's flat list of intervals
  uint32_t tail;         // RSX_ENCODE_TAIL_*
  uint16_t init_pred[4];
  uint8_t table[4];      // the plan's table of component c, from table_base
  uint32_t table_base;
};

RSX_ENC_HD void ljpeg_geom(const rsx_ljpeg_desc& d, const rsx_image& img, uint64_t img_off,
                           uint64_t out_off, uint64_t out_cap, uint32_t tail, LJpegGeom* g) {
  g->img_off = img_off + uint64_t(d.tile_y) * img.pitch_bytes +
               uint64_t(d.tile_x) * uint64_t(img.cpp) * 2u;
  g->out_off = out_off;
  g->out_cap = out_cap;
  g->img_pitch = img.pitch_bytes;
  g->rows = uint32_t(d.tile_h);
  g->row_samples = uint32_t(d.frame_w) * uint32_t(d.n_comp);
  g->n_comp = uint32_t(d.n_comp);
  g->rpi = uint32_t(d.rows_per_restart_interval) < g->rows ? uint32_t(d.rows_per_restart_interval)
                                                           : g->rows;
  g->n_int = (g->rows + g->rpi - 1u) / g->rpi;
  g->int_blocks = uint32_t((uint64_t(g->rpi) * g->row_samples + LJPEG_RUN - 1u) / LJPEG_RUN);
  g->first_block = g->first_int = 0;
  g->n_blocks = 0;
  g->tail = tail;
  for (int c = 0; c < 4; ++c) {
    g->init_pred[c] = d.init_pred[c];
    g->table[c] = c < d.n_comp ? d.table_index[c] : 0;
  }
  g->table_base = 0;
}

// workgroups of job g: every interval but the last has int_blocks of them
RSX_ENC_HD uint64_t ljpeg_blocks(const LJpegGeom& g) {
  const uint64_t last_rows = g.rows - uint64_t(g.n_int - 1u) * g.rpi;
  return uint64_t(g.n_int - 1u) * g.int_blocks +
         (last_rows * g.row_samples + LJPEG_RUN - 1u) / LJPEG_RUN;
}

// rsx_encode_ljpeg_bound: 4 bytes a sample, doubled for stuffing, 2 a marker, 8
RSX_ENC_HD uint64_t ljpeg_bound(const LJpegGeom& g) {
  return uint64_t(g.rows) * g.row_samples * 8u + uint64_t(g.n_int - 1u) * 2u + 8u;
}

// The difference of sample s of tile row r: predictor 1 as LJpegDecompressor reconstructs it --
// the left sample of the component; for the first MCU of a row the first MCU of the row above;
// in the first row of the tile or of a restart interval init_pred[c].  d = int16(uint16(x - pred)).
RSX_ENC_HD int32_t ljpeg_difference(const uint8_t* img, const LJpegGeom& g, uint32_t r, uint32_t s) {
  const uint16_t* row = reinterpret_cast<const uint16_t*>(img + g.img_off + uint64_t(r) * g.img_pitch);
  uint32_t pred;
  if (s >= g.n_comp)
    pred = row[s - g.n_comp];
  else if (r % g.rpi == 0)
    pred = g.init_pred[s];
  else
    pred = reinterpret_cast<const uint16_t*>(reinterpret_cast<const uint8_t*>(row) - g.img_pitch)[s];
  return int32_t(int16_t(uint16_t(uint32_t(row[s]) - pred)));
}

// How interval `i` of a job ends, given its T symbol bits; returns its un-stuffed byte count and
// sets *ones to the 1-bits OR-ed into the low end of its last byte.
//   RSX_ENCODE_TAIL_JPEG      1-bits up to a byte boundary (T.81 F.1.2.3), a final FF stuffed like
//                             any other; every interval in front of a marker ends like this in
//                             either mode, because the reference's reader needs the marker at the
//                             next byte;
//   RSX_ENCODE_TAIL_VACUUMER  the last interval ends as BitVacuumerJPEG::flush ends it: zero bits
//                             up to a whole 32-bit chunk, its bytes stuffed like the others.
RSX_ENC_HD uint64_t interval_bytes(uint64_t T, bool last, uint32_t tail, uint32_t* ones) {
  if (last && tail == RSX_ENCODE_TAIL_VACUUMER) {
    *ones = 0;
    return (T + 31u) / 32u * 4u;
  }
  *ones = uint32_t((8u - T % 8u) % 8u);
  return (T + 7u) / 8u;
}

struct LJpegWalkResult {
  int32_t status;
  uint64_t bytes, symbol_bits;
  uint64_t hist[4 * N_CATEGORIES];
};

// The reference walk of one job on one thread: `tabs` are the job's EncTables by table index, `out`
// the streams' base (nullptr: count only).  Data-dependent statuses: a category the component's
// table lacks -> RSX_ERR_BAD_HUFFMAN_CODE; a stream longer than out_cap -> RSX_ERR_INPUT_OVERFLOW;
// both with 0 bytes reported and nothing written past out_cap.
inline void ljpeg_walk(const uint8_t* img, const LJpegGeom& g, const EncTable* tabs, uint8_t* out,
                       LJpegWalkResult* res) {
  res->status = RSX_OK;
  res->bytes = res->symbol_bits = 0;
  for (int i = 0; i < 4 * N_CATEGORIES; ++i)
    res->hist[i] = 0;
  uint64_t n = 0; // bytes so far
  bool overflow = false, missing = false;
  auto put = [&](uint8_t b) {
    if (n < g.out_cap) {
      if (out)
        out[g.out_off + n] = b;
    } else
      overflow = true;
    ++n;
  };
  auto data = [&](uint8_t b) {
    put(b);
    if (b == 0xFF)
      put(0x00);
  };
  for (uint32_t i = 0; i < g.n_int && !missing; ++i) {
    if (i > 0) {
      put(0xFF);
      put(uint8_t(0xD0 + (i - 1u) % 8u));
    }
    uint64_t acc = 0, T = 0;
    uint32_t nacc = 0;
    const uint32_t r1 = (i + 1u) * uint64_t(g.rpi) < g.rows ? (i + 1u) * g.rpi : g.rows;
    for (uint32_t r = i * g.rpi; r < r1 && !missing; ++r)
      for (uint32_t s = 0; s < g.row_samples; ++s) {
        const int32_t d = ljpeg_difference(img, g, r, s);
        const uint32_t c = s % g.n_comp;
        ++res->hist[c * N_CATEGORIES + category(d)];
        if (!tabs)
          continue;
        const EncTable& e = tabs[g.table[c]];
        uint32_t nb;
        const uint32_t w = symbol(e.code, e.len, e.fix16, d, &nb);
        if (nb == 0) {
          missing = true;
          break;
        }
        acc = acc << nb | w;
        nacc += nb;
        T += nb;
        for (; nacc >= 8; nacc -= 8)
          data(uint8_t(acc >> (nacc - 8)));
      }
    if (!tabs || missing)
      continue;
    res->symbol_bits += T;
    uint32_t ones;
    const uint64_t total = interval_bytes(T, i + 1u == g.n_int, g.tail, &ones);
    uint64_t done = T / 8u;
    if (nacc) {
      data(uint8_t(acc << (8u - nacc)) | uint8_t((1u << ones) - 1u));
      ++done;
    }
    for (; done < total; ++done)
      data(0);
  }
  if (missing)
    res->status = RSX_ERR_BAD_HUFFMAN_CODE;
  else if (overflow)
    res->status = RSX_ERR_INPUT_OVERFLOW;
  res->bytes = res->status == RSX_OK && tabs ? n : 0;
  if (res->status != RSX_OK)
    res->symbol_bits = 0;
}

// ---------------------------------------------------------------------------------------------
// The table of a histogram: T.81 Annex K.2 (Figures K.1 - K.4), written from the standard.
// counts[17] by category; a category with count 0 is left out; with `all_categories` every absent
// category gets a count of 1 first.  The all-ones code point is reserved (the extra symbol of
// frequency 1) and no code is longer than 16 bits.  Returns RSX_ERR_INVALID_ARG for an empty
// histogram.
// ---------------------------------------------------------------------------------------------
inline int huff_from_histogram(const uint64_t* counts, bool all_categories, rsx_huff_table* t) {
  constexpr int N = N_CATEGORIES + 1; // the reserved symbol is the last one
  uint64_t freq[N];
  int codesize[N], others[N];
  bool any = false;
  for (int i = 0; i < N_CATEGORIES; ++i) {
    freq[i] = counts[i] == 0 && all_categories ? 1 : counts[i];
    any = any || freq[i] != 0;
  }
  if (!any)
    return RSX_ERR_INVALID_ARG;
  freq[N - 1] = 1;
  for (int i = 0; i < N; ++i)
    codesize[i] = 0, others[i] = -1;
  // Figure K.1: merge the two least frequent trees (v1: the largest index among equals)
  for (;;) {
    int v1 = -1, v2 = -1;
    for (int i = 0; i < N; ++i)
      if (freq[i] && (v1 < 0 || freq[i] <= freq[v1]))
        v1 = i;
    for (int i = 0; i < N; ++i)
      if (freq[i] && i != v1 && (v2 < 0 || freq[i] <= freq[v2]))
        v2 = i;
    if (v2 < 0)
      break;
    freq[v1] += freq[v2];
    freq[v2] = 0;
    for (++codesize[v1]; others[v1] >= 0; ++codesize[v1])
      v1 = others[v1];
    others[v1] = v2;
    for (++codesize[v2]; others[v2] >= 0; ++codesize[v2])
      v2 = others[v2];
  }
  // Figure K.2: codes of each size
  int bits[33];
  for (int i = 0; i <= 32; ++i)
    bits[i] = 0;
  for (int i = 0; i < N; ++i)
    if (codesize[i])
      ++bits[codesize[i] > 32 ? 32 : codesize[i]];
  // Figure K.3: no code longer than 16 bits, then the reserved code point goes
  for (int i = 32; i > 16;) {
    if (bits[i] > 0) {
      int j = i - 2;
      while (bits[j] == 0)
        --j;
      bits[i] -= 2;
      ++bits[i - 1];
      bits[j + 1] += 2;
      --bits[j];
    } else
      --i;
  }
  int top = 16;
  while (bits[top] == 0)
    --top;
  --bits[top];
  // Figure K.4: the values in order of code size
  for (size_t i = 0; i < sizeof *t; ++i)
    reinterpret_cast<uint8_t*>(t)[i] = 0;
  unsigned k = 0;
  for (int size = 1; size <= 32; ++size)
    for (int v = 0; v < N_CATEGORIES; ++v)
      if (codesize[v] == size)
        t->code_values[k++] = uint8_t(v);
  for (int l = 1; l <= 16; ++l)
    t->n_codes_per_length[l - 1] = uint8_t(bits[l]);
  t->n_code_values = uint8_t(k);
  return RSX_OK;
}

// ---------------------------------------------------------------------------------------------
// The container around a scan: SOI, SOF3, DHT(s), optional DRI, SOS; EOI
// goes behind the entropy bytes.  `hdr` gets the bytes in front of the scan; the two bytes of EOI
// are returned in eoi.  Returns the header's length, or 0 when hdr_cap is too small.
// ---------------------------------------------------------------------------------------------
inline size_t ljpeg_container(const rsx_ljpeg_desc& d, int precision, uint8_t* hdr, size_t hdr_cap) {
  // SOI, SOF3 of four components, four DHTs of 162 values, DRI, SOS of four components
  constexpr size_t MAX = 2 + (10 + 3 * RSX_MAX_COMPONENTS) +
                         RSX_MAX_COMPONENTS * (2 + 2 + 1 + 16 + RSX_MAX_CODE_VALUES) + 6 +
                         (2 + 6 + 2 * RSX_MAX_COMPONENTS);
  uint8_t buf[MAX];
  size_t n = 0;
  if (d.n_comp < 1 || d.n_comp > RSX_MAX_COMPONENTS || d.n_tables < 1 ||
      d.n_tables > RSX_MAX_COMPONENTS)
    return 0;
  // (a descriptor the validation has not seen writes no byte past the buffer either)
  auto b = [&](unsigned v) {
    if (n < MAX)
      buf[n] = uint8_t(v);
    ++n;
  };
  auto be16 = [&](unsigned v) { b(v >> 8), b(v & 0xFFu); };
  be16(0xFFD8);
  be16(0xFFC3);
  be16(8 + 3 * d.n_comp);
  b(precision);
  be16(unsigned(d.frame_h));
  be16(unsigned(d.frame_w));
  b(d.n_comp);
  for (int c = 0; c < d.n_comp; ++c)
    b(c + 1), b(0x11), b(0);
  for (int i = 0; i < d.n_tables; ++i) {
    const rsx_huff_table& t = d.tables[i];
    be16(0xFFC4);
    be16(2 + 1 + 16 + t.n_code_values);
    b(i);
    for (int l = 0; l < 16; ++l)
      b(t.n_codes_per_length[l]);
    for (unsigned v = 0; v < t.n_code_values; ++v)
      b(t.code_values[v]);
  }
  if (d.rows_per_restart_interval < d.tile_h) {
    be16(0xFFDD);
    be16(4);
    be16(unsigned(int64_t(d.rows_per_restart_interval) * d.frame_w));
  }
  be16(0xFFDA);
  be16(6 + 2 * d.n_comp);
  b(d.n_comp);
  for (int c = 0; c < d.n_comp; ++c)
    b(c + 1), b(d.table_index[c] << 4);
  b(1); // predictor
  b(0);
  b(0); // point transform
  if (n > hdr_cap || n > MAX)
    return 0;
  for (size_t i = 0; i < n; ++i)
    hdr[i] = buf[i];
  return n;
}

} // namespace rsx_encode
