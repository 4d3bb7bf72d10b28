/*
 * rsx_synth.c -- host-side stream writers used to synthesise inputs.
 *
 * The reference ships writers for every bit order and a Huffman encoder that
 * only its tests / fuzzers / benchmarks use (bitstreams/BitVacuumer*.h,
 * codes/PrefixCodeVectorEncoder.h:80-90).  This file is our own equivalent:
 * a packed-integer row writer for the four UncompressedDecompressor bit
 * orders, a lossless-JPEG (predictor 1) scan + container writer that emits
 * exactly the layout AbstractLJpegDecoder accepts, and
 * a deterministic "sensor-like" image model.  Plain C, no GPU, no reference
 * code.  Built into rawspeed_amd/librsx_synth.so.
 */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* ------------------------------------------------------------------------ */
/* Packed-integer rows (the inverse of decodePackedInt,                      */
/* UncompressedDecompressor.cpp:188-200; stream addressing SURVEY.md A.1).   */
/* ------------------------------------------------------------------------ */

/* Writes rows x cols samples of `bps` bits each, every row followed by zero
 * padding up to `pitch_bytes`, as ONE continuous bit stream in the given
 * order (0 LSB, 1 MSB, 2 MSB16, 3 MSB32).  Returns bytes written
 * (rows*pitch_bytes) or 0 on a bad argument (pitch too small, bits not a
 * multiple of 8, or total size not a multiple of the order's word size). */
size_t rsx_synth_pack_rows(int order, int bps, const uint16_t* samples,
                           size_t sample_stride, int cols, int rows,
                           int pitch_bytes, uint8_t* out) {
  const uint64_t row_bits = (uint64_t)cols * (uint64_t)bps;
  if (bps < 1 || bps > 16 || row_bits % 8 != 0 ||
      (uint64_t)pitch_bytes < row_bits / 8 || order < 0 || order > 3)
    return 0;
  const size_t total = (size_t)rows * (size_t)pitch_bytes;
  const size_t word = order == 2 ? 2 : (order == 3 ? 4 : 1);
  if (total % word != 0)
    return 0;
  memset(out, 0, total);
  const uint32_t mask = (1u << bps) - 1u;
  for (int r = 0; r < rows; ++r) {
    uint8_t* row = out + (size_t)r * pitch_bytes;
    const uint16_t* src = samples + (size_t)r * sample_stride;
    uint64_t acc = 0;
    int nacc = 0;
    size_t o = 0;
    if (order == 0) { /* LSB first */
      for (int x = 0; x < cols; ++x) {
        acc |= (uint64_t)(src[x] & mask) << nacc;
        nacc += bps;
        while (nacc >= 8) {
          row[o++] = (uint8_t)acc;
          acc >>= 8;
          nacc -= 8;
        }
      }
    } else { /* MSB first byte stream; word swizzle applied afterwards */
      for (int x = 0; x < cols; ++x) {
        acc = (acc << bps) | (src[x] & mask);
        nacc += bps;
        while (nacc >= 8) {
          row[o++] = (uint8_t)(acc >> (nacc - 8));
          nacc -= 8;
        }
      }
    }
  }
  if (order == 2) { /* MSB16: stream byte 2i <-> memory byte 2i+1 */
    for (size_t i = 0; i + 1 < total; i += 2) {
      uint8_t t = out[i];
      out[i] = out[i + 1];
      out[i + 1] = t;
    }
  } else if (order == 3) { /* MSB32: reverse within LE u32 words */
    for (size_t i = 0; i + 3 < total; i += 4) {
      uint8_t a = out[i], b = out[i + 1];
      out[i] = out[i + 3];
      out[i + 1] = out[i + 2];
      out[i + 2] = b;
      out[i + 3] = a;
    }
  }
  return total;
}

/* ------------------------------------------------------------------------ */
/* Deterministic pixel sources                                               */
/* ------------------------------------------------------------------------ */

static uint64_t splitmix64(uint64_t* s) {
  uint64_t z = (*s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

/* Uniform random `bits`-bit samples. */
void rsx_synth_uniform(uint16_t* out, size_t n, int bits, uint64_t seed) {
  uint64_t s = seed * 0x2545F4914F6CDD1Dull + 1;
  const uint16_t mask = (uint16_t)((1u << bits) - 1u);
  size_t i = 0;
  for (; i + 4 <= n; i += 4) {
    uint64_t r = splitmix64(&s);
    out[i] = (uint16_t)r & mask;
    out[i + 1] = (uint16_t)(r >> 16) & mask;
    out[i + 2] = (uint16_t)(r >> 32) & mask;
    out[i + 3] = (uint16_t)(r >> 48) & mask;
  }
  if (i < n) {
    uint64_t r = splitmix64(&s);
    for (; i < n; ++i, r >>= 16)
      out[i] = (uint16_t)r & mask;
  }
}

/* "Sensor-like" w x h image (SURVEY.md 8(d) cfg 3): smooth ramp + 2x2 CFA
 * offset + approximately Gaussian noise (sum of four uniforms, sigma ~= 24),
 * clamped to [0, 2^prec - 1]. */
void rsx_synth_sensor_image(uint16_t* out, int w, int h, size_t stride,
                            int prec, uint64_t seed) {
  uint64_t s = seed * 0x9E3779B97F4A7C15ull + 12345;
  const int maxv = (1 << prec) - 1;
  /* sum of 4 U[0,65536): mean 131070, sigma = 65536*sqrt(4/12) = 37837.2 */
  const double k = 24.0 / 37837.2;
  for (int y = 0; y < h; ++y) {
    uint16_t* row = out + (size_t)y * stride;
    for (int x = 0; x < w; ++x) {
      uint64_t r = splitmix64(&s);
      int sum = (int)(r & 0xFFFF) + (int)((r >> 16) & 0xFFFF) +
                (int)((r >> 32) & 0xFFFF) + (int)(r >> 48);
      double base = 2000.0 + 6000.0 * x / w + 3000.0 * y / h +
                    500.0 * ((x ^ y) & 1);
      int v = (int)(base + (sum - 131070) * k + 0.5);
      if (v < 0)
        v = 0;
      if (v > maxv)
        v = maxv;
      row[x] = (uint16_t)v;
    }
  }
}

/* ------------------------------------------------------------------------ */
/* Lossless JPEG writer                                                      */
/* ------------------------------------------------------------------------ */

typedef struct jpeg_writer {
  uint8_t* out;
  size_t cap, n;
  uint64_t acc;
  int nacc;
  int overflow;
  int raw; /* 1: plain MSB bit stream, no FF00 stuffing (BitStreamerMSB input) */
} jpeg_writer;

static void jw_byte_raw(jpeg_writer* w, uint8_t b) {
  if (w->n < w->cap)
    w->out[w->n] = b;
  else
    w->overflow = 1;
  w->n++;
}
static void jw_data_byte(jpeg_writer* w, uint8_t b) {
  jw_byte_raw(w, b);
  if (b == 0xFF && !w->raw)
    jw_byte_raw(w, 0x00); /* byte stuffing */
}
static void jw_bits(jpeg_writer* w, uint32_t v, int n) {
  if (n == 0)
    return;
  w->acc = (w->acc << n) | (v & ((n >= 32) ? 0xFFFFFFFFu : ((1u << n) - 1u)));
  w->nacc += n;
  while (w->nacc >= 8) {
    jw_data_byte(w, (uint8_t)(w->acc >> (w->nacc - 8)));
    w->nacc -= 8;
  }
}
/* pad with 1-bits to a byte boundary */
static void jw_flush(jpeg_writer* w) {
  if (w->nacc > 0)
    jw_bits(w, 0xFFu, 8 - w->nacc);
  w->acc = 0;
}

typedef struct enc_table {
  uint16_t code[17];
  uint8_t len[17]; /* 0 = category absent from the table */
} enc_table;

/* canonical code from DHT counts + values (JPEG Annex C) */
static int enc_table_build(enc_table* t, const uint8_t counts[16],
                           const uint8_t* values, int n_values) {
  memset(t, 0, sizeof *t);
  uint32_t code = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    for (int i = 0; i < counts[l - 1]; ++i, ++k) {
      if (k >= n_values || values[k] > 16)
        return -1;
      t->code[values[k]] = (uint16_t)code;
      t->len[values[k]] = (uint8_t)l;
      code++;
    }
    code <<= 1;
  }
  return k == n_values ? 0 : -1;
}

/* Encodes `rows` stream-order rows of `row_samples` samples (component of
 * sample s = s % n_comp; row_samples = frame_w * n_comp) with predictor 1 as
 * LJpegDecompressor / Cr2Decompressor reconstruct it:
 *   pred(r, s) = s >= n_comp ? X[r][s - n_comp]
 *              : (r is the first row of a restart interval ? init_pred[s]
 *                                                          : X[r-1][s]).
 * tables: n_comp pointers to {16 counts, values} pairs (may alias).
 * rows_per_ri: 0 = no restart markers; else RSTn (n = (i-1)%8) is written
 * between intervals.  fix16: emit 16 extra (zero) bits after an SSSS=16 code.
 * Returns the number of entropy bytes, or 0 on overflow / missing category. */
size_t rsx_synth_ljpeg_encode_pattern(const uint16_t* samples, size_t row_stride,
                                      int row_samples, int rows, int n_comp,
                                      int period, const uint8_t* comp_of_phase,
                                      const uint16_t* init_pred,
                                      const uint8_t* const* counts,
                                      const uint8_t* const* values,
                                      const int* n_values, int rows_per_ri,
                                      int fix16, uint8_t* out, size_t cap,
                                      uint64_t* n_symbol_bits);

size_t rsx_synth_ljpeg_encode_scan(const uint16_t* samples, size_t row_stride,
                                   int row_samples, int rows, int n_comp,
                                   const uint16_t* init_pred,
                                   const uint8_t* const* counts,
                                   const uint8_t* const* values,
                                   const int* n_values, int rows_per_ri,
                                   int fix16, uint8_t* out, size_t cap,
                                   uint64_t* n_symbol_bits) {
  static const uint8_t identity[4] = {0, 1, 2, 3};
  return rsx_synth_ljpeg_encode_pattern(samples, row_stride, row_samples, rows, n_comp,
                                        n_comp, identity, init_pred, counts, values,
                                        n_values, rows_per_ri, fix16, out, cap,
                                        n_symbol_bits);
}

/* General form: sample s of a row belongs to component comp_of_phase[s % period]
 * (period <= 8).  Its predictor is the previous sample of the same component in
 * the row; for the first one of a row it is init_pred[c] (first row / first row
 * of a restart interval) or the first sample of that component in the row above.
 * period == n_comp with the identity map is plain LJPEG predictor 1; period 4
 * (0,0,1,2) / 6 (0,0,0,0,1,2) are Canon sRaw <3,2,1> / <3,2,2>
 * (the layout Cr2DecompressorImpl.h:431-465 decodes). */
size_t rsx_synth_ljpeg_encode_pattern(const uint16_t* samples, size_t row_stride,
                                      int row_samples, int rows, int n_comp,
                                      int period, const uint8_t* comp_of_phase,
                                      const uint16_t* init_pred,
                                      const uint8_t* const* counts,
                                      const uint8_t* const* values,
                                      const int* n_values, int rows_per_ri,
                                      int fix16, uint8_t* out, size_t cap,
                                      uint64_t* n_symbol_bits) {
  enc_table tabs[4];
  if (n_comp < 1 || n_comp > 4 || period < 1 || period > 8)
    return 0;
  for (int c = 0; c < n_comp; ++c)
    if (enc_table_build(&tabs[c], counts[c], values[c], n_values[c]))
      return 0;
  int first_pos[4] = {-1, -1, -1, -1};
  for (int p = period - 1; p >= 0; --p) {
    if (comp_of_phase[p] >= n_comp)
      return 0;
    first_pos[comp_of_phase[p]] = p;
  }
  jpeg_writer w = {out, cap, 0, 0, 0, 0, 0};
  uint64_t bits = 0;
  for (int r = 0; r < rows; ++r) {
    const uint16_t* cur = samples + (size_t)r * row_stride;
    const uint16_t* up = r > 0 ? samples + (size_t)(r - 1) * row_stride : NULL;
    int ri_first = rows_per_ri > 0 ? (r % rows_per_ri == 0) : (r == 0);
    if (rows_per_ri > 0 && r > 0 && ri_first) {
      jw_flush(&w);
      jw_byte_raw(&w, 0xFF);
      jw_byte_raw(&w, (uint8_t)(0xD0 + ((r / rows_per_ri - 1) % 8)));
    }
    int last[4] = {-1, -1, -1, -1};
    for (int s = 0; s < row_samples; ++s) {
      const int c = comp_of_phase[s % period];
      uint16_t pred;
      if (last[c] >= 0)
        pred = cur[last[c]];
      else
        pred = ri_first ? init_pred[c] : up[first_pos[c]];
      last[c] = s;
      const int d = (int16_t)(uint16_t)(cur[s] - pred);
      int ssss = 0;
      if (d == -32768) {
        ssss = 16;
      } else {
        int a = d < 0 ? -d : d;
        while (a) {
          ++ssss;
          a >>= 1;
        }
      }
      const enc_table* t = &tabs[c];
      if (t->len[ssss] == 0)
        return 0; /* category not in table */
      jw_bits(&w, t->code[ssss], t->len[ssss]);
      bits += t->len[ssss];
      if (ssss == 16) {
        if (fix16) {
          jw_bits(&w, 0, 16);
          bits += 16;
        }
      } else if (ssss) {
        const uint32_t v = d >= 0 ? (uint32_t)d : (uint32_t)(d + (1 << ssss) - 1);
        jw_bits(&w, v, ssss);
        bits += ssss;
      }
    }
  }
  jw_flush(&w);
  if (n_symbol_bits)
    *n_symbol_bits = bits;
  return w.overflow ? 0 : w.n;
}

/* NikonDecompressor stream (NikonDecompressor.cpp:515-539) for an image of
 * 15-bit values: plain MSB bit stream, one Huffman table, the sample at
 * (row, col) is predicted from (row, col - 2), the first two of a row from
 * (row - 2, col) and those of rows 0 / 1 from p_up[2 * row + col].  Differences
 * are plain ints here (the decoder does not wrap), so |diff| must fit the
 * table's categories.  Returns the byte count (padded with zero bits), 0 on
 * overflow / missing category. */
static size_t nikon_encode_tab(const uint16_t* samples, size_t row_stride, int w, int h,
                               const int32_t* p_up, const enc_table* tab, uint8_t* out,
                               size_t cap, uint64_t* n_symbol_bits) {
  jpeg_writer wr = {out, cap, 0, 0, 0, 0, 1};
  uint64_t bits = 0;
  for (int r = 0; r < h; ++r) {
    const uint16_t* cur = samples + (size_t)r * row_stride;
    for (int x = 0; x < w; ++x) {
      int pred;
      if (x >= 2)
        pred = cur[x - 2];
      else if (r >= 2)
        pred = samples[(size_t)(r - 2) * row_stride + x];
      else
        pred = p_up[2 * r + x];
      const int d = (int)cur[x] - pred;
      int ssss = 0;
      for (int a = d < 0 ? -d : d; a; a >>= 1)
        ++ssss;
      if (ssss > 15 || tab->len[ssss] == 0)
        return 0;
      jw_bits(&wr, tab->code[ssss], tab->len[ssss]);
      bits += tab->len[ssss] + ssss;
      if (ssss)
        jw_bits(&wr, d >= 0 ? (uint32_t)d : (uint32_t)(d + (1 << ssss) - 1), ssss);
    }
  }
  if (wr.nacc > 0)
    jw_bits(&wr, 0, 8 - wr.nacc);
  if (n_symbol_bits)
    *n_symbol_bits = bits;
  return wr.overflow ? 0 : wr.n;
}

size_t rsx_synth_nikon_encode(const uint16_t* samples, size_t row_stride, int w,
                              int h, const int32_t* p_up, const uint8_t* counts,
                              const uint8_t* values, int n_values, uint8_t* out,
                              size_t cap, uint64_t* n_symbol_bits) {
  enc_table tab;
  if (enc_table_build(&tab, counts, values, n_values))
    return 0;
  return nikon_encode_tab(samples, row_stride, w, h, p_up, &tab, out, cap, n_symbol_bits);
}

/* Same stream layout with a prefix code that is not a canonical JPEG one
 * (SamsungV1Decompressor.cpp:88-117): entry i = (enc_len[i], diff_len[i]) owns
 * the next 1024 >> enc_len[i] slots of a 10-bit table, so its code is the first
 * slot's index >> (10 - enc_len[i]). */
size_t rsx_synth_prefix_encode(const uint16_t* samples, size_t row_stride, int w, int h,
                               const int32_t* p_up, const uint8_t* enc_len,
                               const uint8_t* diff_len, int n_entries, uint8_t* out,
                               size_t cap, uint64_t* n_symbol_bits) {
  enc_table tab;
  memset(&tab, 0, sizeof tab);
  unsigned pos = 0;
  for (int i = 0; i < n_entries; ++i) {
    if (enc_len[i] < 1 || enc_len[i] > 10 || diff_len[i] > 16)
      return 0;
    tab.code[diff_len[i]] = (uint16_t)(pos >> (10 - enc_len[i]));
    tab.len[diff_len[i]] = enc_len[i];
    pos += 1024u >> enc_len[i];
  }
  if (pos != 1024)
    return 0;
  return nikon_encode_tab(samples, row_stride, w, h, p_up, &tab, out, cap, n_symbol_bits);
}

/* SonyArw1Decompressor stream (SonyArw1Decompressor.cpp:59-93): plain MSB-first
 * bits; per pixel the length code -- "11" 1, "10" 2, "010" 3, "011" 0, "00" +
 * k zeros + "1" = 4 + k (the final "1" is absent for 17) -- then the difference
 * bits with JPEG sign extension.  One predictor (start 0) runs over the whole
 * image in decode order: columns right to left, in a column the even rows and
 * then the odd rows.  `samples` may hold any int16-representable value stored as
 * uint16 (the decoder rejects values outside 0..4095). */
size_t rsx_synth_sony_arw1_encode(const uint16_t* samples, size_t row_stride, int w, int h,
                                  uint8_t* out, size_t cap, uint64_t* n_symbol_bits) {
  jpeg_writer wr = {out, cap, 0, 0, 0, 0, 1};
  uint64_t bits = 0;
  int pred = 0;
  if (h & 1)
    return 0;
  for (int col = w - 1; col >= 0; --col) {
    for (int i = 0; i < h; ++i) {
      const int row = i < h / 2 ? 2 * i : 2 * (i - h / 2) + 1;
      const int cur = (int16_t)samples[(size_t)row * row_stride + col];
      const int d = cur - pred;
      pred = cur;
      int len = 0;
      for (int a = d < 0 ? -d : d; a; a >>= 1)
        ++len;
      if (len > 17)
        return 0;
      int nb;
      if (len == 0) {
        jw_bits(&wr, 3, 3); /* 011 */
        nb = 3;
      } else if (len <= 3) {
        static const uint8_t code[4] = {0, 3, 2, 2}, clen[4] = {0, 2, 2, 3};
        jw_bits(&wr, code[len], clen[len]); /* 11, 10, 010 */
        nb = clen[len];
      } else {
        const int k = len - 4;
        jw_bits(&wr, 0, 2);
        if (k)
          jw_bits(&wr, 0, k);
        nb = 2 + k;
        if (len < 17) {
          jw_bits(&wr, 1, 1);
          ++nb;
        }
      }
      bits += (uint64_t)(nb + len);
      if (len)
        jw_bits(&wr, d >= 0 ? (uint32_t)d : (uint32_t)(d + (1 << len) - 1), len);
    }
  }
  if (wr.nacc > 0)
    jw_bits(&wr, 0, 8 - wr.nacc);
  if (n_symbol_bits)
    *n_symbol_bits = bits;
  return wr.overflow ? 0 : wr.n;
}

/* HasselbladDecompressor stream (HasselbladDecompressor.cpp:71-100): pixels two at
 * a time as [len1 code][len2 code][len1 bits][len2 bits], both predictors restart
 * from init_pred on every row, arithmetic mod 2^16; BitStreamerMSB32 input, i.e.
 * the MSB-first bit stream is stored as little-endian 32-bit words.  Returns the
 * byte count (a multiple of 4), 0 on overflow / missing category. */
size_t rsx_synth_hasselblad_encode(const uint16_t* samples, size_t row_stride, int w,
                                   int h, unsigned init_pred, const uint8_t* counts,
                                   const uint8_t* values, int n_values, uint8_t* out,
                                   size_t cap, uint64_t* n_symbol_bits) {
  enc_table tab;
  if (enc_table_build(&tab, counts, values, n_values) || (w & 1))
    return 0;
  jpeg_writer wr = {out, cap, 0, 0, 0, 0, 1};
  uint64_t bits = 0;
  for (int r = 0; r < h; ++r) {
    const uint16_t* cur = samples + (size_t)r * row_stride;
    uint16_t p[2] = {(uint16_t)init_pred, (uint16_t)init_pred};
    for (int x = 0; x < w; x += 2) {
      int d[2], ssss[2];
      for (int k = 0; k < 2; ++k) {
        d[k] = (int16_t)(uint16_t)(cur[x + k] - p[k]); /* -32768 .. 32767 */
        p[k] = cur[x + k];
        ssss[k] = 0;
        if (d[k] == -32768) {
          ssss[k] = 16; /* the all-ones field */
        } else {
          for (int a = d[k] < 0 ? -d[k] : d[k]; a; a >>= 1)
            ++ssss[k];
        }
        if (tab.len[ssss[k]] == 0)
          return 0;
      }
      for (int k = 0; k < 2; ++k) {
        jw_bits(&wr, tab.code[ssss[k]], tab.len[ssss[k]]);
        bits += tab.len[ssss[k]] + ssss[k];
      }
      for (int k = 0; k < 2; ++k) {
        if (ssss[k] == 16)
          jw_bits(&wr, 0xFFFFu, 16);
        else if (ssss[k])
          jw_bits(&wr, d[k] >= 0 ? (uint32_t)d[k] : (uint32_t)(d[k] + (1 << ssss[k]) - 1),
                  ssss[k]);
      }
    }
  }
  if (wr.nacc > 0)
    jw_bits(&wr, 0, 8 - wr.nacc);
  while (wr.n % 4)
    jw_byte_raw(&wr, 0);
  if (wr.overflow)
    return 0;
  for (size_t i = 0; i + 4 <= wr.n; i += 4) { /* MSB-first words -> little-endian */
    uint8_t t = out[i];
    out[i] = out[i + 3];
    out[i + 3] = t;
    t = out[i + 1];
    out[i + 1] = out[i + 2];
    out[i + 2] = t;
  }
  if (n_symbol_bits)
    *n_symbol_bits = bits;
  return wr.n;
}

static void put16(uint8_t** p, unsigned v) {
  *(*p)++ = (uint8_t)(v >> 8);
  *(*p)++ = (uint8_t)v;
}

/* Writes SOI, SOF3, one DHT per distinct table, [DRI], SOS into `out`
 * (all fields big-endian,
 * AbstractLJpegDecoder.cpp:127-228).  comp_table[c] = DHT slot (0..3) of
 * component c; slot_counts/slot_values/slot_n describe slot i for i <
 * n_slots.  h_samp/v_samp give the SOF HiVi nibbles (1/1 for raw data).
 * Returns header size. */
size_t rsx_synth_ljpeg_header(uint8_t* out, int prec, int frame_w, int frame_h,
                              int n_comp, const int* comp_table, int n_slots,
                              const uint8_t* const* slot_counts,
                              const uint8_t* const* slot_values,
                              const int* slot_n, int restart_interval_mcus,
                              const int* h_samp, const int* v_samp) {
  uint8_t* p = out;
  *p++ = 0xFF;
  *p++ = 0xD8; /* SOI */
  *p++ = 0xFF;
  *p++ = 0xC3; /* SOF3 */
  put16(&p, 8 + 3 * n_comp);
  *p++ = (uint8_t)prec;
  put16(&p, frame_h);
  put16(&p, frame_w);
  *p++ = (uint8_t)n_comp;
  for (int c = 0; c < n_comp; ++c) {
    *p++ = (uint8_t)(c + 1);
    *p++ = (uint8_t)(((h_samp ? h_samp[c] : 1) << 4) | (v_samp ? v_samp[c] : 1));
    *p++ = 0;
  }
  for (int s = 0; s < n_slots; ++s) {
    *p++ = 0xFF;
    *p++ = 0xC4; /* DHT */
    put16(&p, 2 + 1 + 16 + slot_n[s]);
    *p++ = (uint8_t)s; /* class 0, destination s */
    memcpy(p, slot_counts[s], 16);
    p += 16;
    memcpy(p, slot_values[s], slot_n[s]);
    p += slot_n[s];
  }
  if (restart_interval_mcus > 0) {
    *p++ = 0xFF;
    *p++ = 0xDD; /* DRI */
    put16(&p, 4);
    put16(&p, restart_interval_mcus);
  }
  *p++ = 0xFF;
  *p++ = 0xDA; /* SOS */
  put16(&p, 6 + 2 * n_comp);
  *p++ = (uint8_t)n_comp;
  for (int c = 0; c < n_comp; ++c) {
    *p++ = (uint8_t)(c + 1);
    *p++ = (uint8_t)(comp_table[c] << 4);
  }
  *p++ = 1; /* Ss = predictor 1 */
  *p++ = 0; /* Se */
  *p++ = 0; /* Ah/Al: Pt = 0 */
  return (size_t)(p - out);
}

/* PhaseOneDecompressor rows (PhaseOneDecompressor.cpp:85-136): one BitStreamerMSB32
 * stream per row (MSB-first bits stored as little-endian 32-bit words, each row
 * padded with zeros to a whole word).  A group of 8 pixels (col < w & ~7) starts
 * with a length header for the even and one for the odd columns: j zeros, a 1 if
 * j < 5, then bit b selects {8,7,6,9,11,10,5,12,14,13}[2 (j - 1) + b]; a single 1
 * keeps the length (never at col 0, where any 1 in the prefix is the decoder's
 * "Can not initialize lengths").  Length 14 stores the 16-bit value; any other L
 * stores d - 1 + 2^(L-1) in L bits, d = value - previous value of the parity
 * (mod 2^16).  The last w % 8 pixels are raw 16-bit values.  Per header, drawn
 * with the seeded generator: keep the length (p_keep / 65536, if it still fits),
 * 14 (p_raw / 65536), a random fitting length (p_wide / 65536), else the shortest
 * that fits.  Rows go back to back into `out`; row_off[r] .. row_off[r + 1] is row
 * r.  Returns the bytes written, 0 on overflow. */
static const uint8_t p1_lengths[10] = {8, 7, 6, 9, 11, 10, 5, 12, 14, 13};

static int p1_fits(int len, int d) {
  return len == 14 || (d >= 1 - (1 << (len - 1)) && d <= (1 << (len - 1)));
}

size_t rsx_synth_phase_one_encode(const uint16_t* samples, size_t row_stride, int w, int h,
                                  uint32_t p_keep, uint32_t p_raw, uint32_t p_wide,
                                  uint64_t seed, uint8_t* out, size_t cap, uint64_t* row_off) {
  uint64_t rs = seed * 0x2545F4914F6CDD1Dull + 7;
  size_t n = 0;
  const int gw = w & ~7;
  for (int row = 0; row < h; ++row) {
    const uint16_t* v = samples + (size_t)row * row_stride;
    uint32_t acc = 0;
    int nacc = 0;
    row_off[row] = n;
#define P1_PUT(val, nb)                                                        \
  do {                                                                         \
    for (int _i = (nb)-1; _i >= 0; --_i) {                                     \
      acc = (acc << 1) | (((uint32_t)(val) >> _i) & 1u);                       \
      if (++nacc == 32) {                                                      \
        if (n + 4 > cap)                                                       \
          return 0;                                                            \
        out[n] = (uint8_t)acc;                                                 \
        out[n + 1] = (uint8_t)(acc >> 8);                                      \
        out[n + 2] = (uint8_t)(acc >> 16);                                     \
        out[n + 3] = (uint8_t)(acc >> 24);                                     \
        n += 4;                                                                \
        acc = 0;                                                               \
        nacc = 0;                                                              \
      }                                                                        \
    }                                                                          \
  } while (0)
    int pred[2] = {0, 0}, len[2] = {0, 0};
    for (int col = 0; col < w; ++col) {
      if (col < gw && (col & 7) == 0) {
        for (int p = 0; p < 2; ++p) {
          /* the shortest length that holds the group's four differences of parity p */
          int need = 5, prev = pred[p];
          for (int k = p; k < 8; k += 2) {
            const int d = (int16_t)(uint16_t)(v[col + k] - prev);
            prev = v[col + k];
            while (!p1_fits(need, d))
              ++need;
          }
          const uint64_t r = splitmix64(&rs);
          const uint32_t rk = r & 0xFFFFu, rr = (r >> 16) & 0xFFFFu, rw = (r >> 32) & 0xFFFFu;
          int L;
          if (col == 0) {
            L = need <= 13 && rr >= p_raw ? 13 : 14;
          } else if (len[p] >= need && rk < p_keep) {
            P1_PUT(1, 1);
            continue;
          } else if (rr < p_raw) {
            L = 14;
          } else if (rw < p_wide) {
            L = need + (int)((r >> 48) % (uint32_t)(15 - need));
          } else {
            L = need;
          }
          int idx = 0;
          while (p1_lengths[idx] != L)
            ++idx;
          const int j = idx / 2 + 1;
          P1_PUT(0, j);
          if (j < 5)
            P1_PUT(1, 1);
          P1_PUT(idx & 1, 1);
          len[p] = L;
        }
      }
      const int L = col >= gw ? 14 : len[col & 1];
      const int cur = v[col];
      if (L == 14) {
        P1_PUT(cur, 16);
      } else {
        const int d = (int16_t)(uint16_t)(cur - pred[col & 1]);
        P1_PUT((uint32_t)(d - 1 + (1 << (L - 1))), L);
      }
      pred[col & 1] = cur;
    }
    if (nacc)
      P1_PUT(0, 32 - nacc);
#undef P1_PUT
  }
  row_off[h] = n;
  return n;
}

/* ------------------------------------------------------------------------ */
/* FujiDecompressor (compressed RAF) strip writer.  The reference has no     */
/* encoder: this runs the decoder's state (decompressors/FujiDecompressor.   */
/* cpp:444-779: 18 line buffers, the two sets of gradient tables, the pass   */
/* order, the helper columns, the rotation) forward over `target`, 6         */
/* total_lines rows of 768 pixels, and emits per coded sample the smallest   */
/* code -- direct or over either wrap by total_values -- that makes the      */
/* decoder reach the target: zeros, a 1 and bitDiff bits, or the escape      */
/* (max_bits - raw_bits - 1 zeros, a 1, raw_bits bits of code - 1) where the */
/* zero count of the regular form would reach the escape's.  X-Trans         */
/* positions that take no bits get their interpolation whatever the target   */
/* says: `reached` (same shape) gets the pixels a decoder will return.       */
/* plant_kind 1 (regular form) / 2 (escape form): the first coded sample at  */
/* or behind index plant_at that can carry an out-of-range code in that form */
/* gets one, and the writer stops there (*planted = 1; the rows of the lines */
/* before it are in `reached`).  plant_kind 3 (a long escape): the first      */
/* coded sample at or behind plant_at whose code is at least 1 is written as */
/* plant_zeros zeros, a 1 and raw_bits bits of code - 1 -- a decoder takes   */
/* any zero count of at least the escape's for the escape --, *planted = 1,  */
/* and the writer goes on: the pixels are those of the strip without it.     */
/* The bits are padded with zeros to a byte.                                 */
/* Returns the bytes written, 0 on overflow of `cap`.                        */
/* ------------------------------------------------------------------------ */
enum { FJ_STRIDE = 514, FJ_LINES = 18, FJ_R2 = 2, FJ_G2 = 7, FJ_B2 = 15 };

typedef struct fj_enc {
  int raw_bits, total, q4, escape_at, lw, xtrans;
  uint16_t lines[FJ_LINES][FJ_STRIDE];
  int want[FJ_LINES][FJ_STRIDE];
  int ge[3][41][2], go[3][41][2];
  uint8_t* out;
  size_t n, cap;
  uint64_t acc;
  int nacc, overflow;
  int plant_kind, planted;
  uint32_t plant_at, plant_zeros, n_coded;
} fj_enc;

static void fj_put(fj_enc* e, uint32_t v, int nbits) {
  /* nbits <= 48: the zeros and the 1 of a sample, or its code bits */
  e->acc = (e->acc << nbits) | v;
  e->nacc += nbits;
  while (e->nacc >= 8) {
    e->nacc -= 8;
    if (e->n >= e->cap) {
      e->overflow = 1;
      return;
    }
    e->out[e->n++] = (uint8_t)(e->acc >> e->nacc);
  }
  e->acc &= ((uint64_t)1 << e->nacc) - 1;
}

static int fj_quant(int v) {
  const int a = v < 0 ? -v : v;
  const int g = a >= 0x114 ? 4 : a >= 0x43 ? 3 : a >= 0x12 ? 2 : a > 0 ? 1 : 0;
  return v < 0 ? -g : g;
}

static int fj_width(unsigned v) {
  int n = 0;
  while (v) {
    ++n;
    v >>= 1;
  }
  return n;
}

static int fj_bit_diff(int v1, int v2) {
  int dec = fj_width((unsigned)v1) - fj_width((unsigned)v2);
  if (dec < 0)
    dec = 0;
  if ((v2 << dec) < v1)
    ++dec;
  return dec > 15 ? 15 : dec;
}

/* one coded sample: returns the value the decoder reaches, -1 behind a planted code */
static int fj_sample(fj_enc* e, int grad, int interp, int (*tbl)[2], int want) {
  int* t = tbl[grad < 0 ? -grad : grad];
  const int bits = fj_bit_diff(t[0], t[1]);
  const int s = grad < 0 ? -1 : 1;
  long best = -1;
  for (int k = 0; k < 3; ++k) {
    const long d = (long)s * (want - interp + (k == 1 ? e->total : k == 2 ? -e->total : 0));
    const long code = d >= 0 ? 2 * d : -2 * d - 1;
    if (code < e->total && (best < 0 || code < best))
      best = code;
  }
  long code = best;
  int bad = 0, long_run = 0;
  if (e->plant_kind && !e->planted && e->n_coded >= e->plant_at) {
    if (e->plant_kind == 3) {
      long_run = code >= 1;
    } else if (e->plant_kind == 2) {
      bad = 2;
      code = e->total;
    } else if (((long)(e->escape_at - 1) << bits) >= e->total) {
      bad = 1;
      code = (long)(e->escape_at - 1) << bits;
    }
  }
  if (bad || long_run)
    e->planted = 1;
  if (long_run) {
    for (uint32_t left = e->plant_zeros; left;) {
      const int m = left > 32 ? 32 : (int)left;
      fj_put(e, 0, m);
      left -= (uint32_t)m;
    }
    fj_put(e, 1, 1);
    fj_put(e, (uint32_t)(code - 1), e->raw_bits);
  } else if ((code >> bits) < e->escape_at && bad != 2) {
    const int zeros = (int)(code >> bits);
    fj_put(e, 1, zeros + 1);
    if (bits)
      fj_put(e, (uint32_t)(code & ((1L << bits) - 1)), bits);
  } else {
    fj_put(e, 1, e->escape_at + 1);
    fj_put(e, (uint32_t)(code - 1), e->raw_bits);
  }
  if (bad)
    return -1;
  ++e->n_coded;
  code = (code & 1) ? -1 - code / 2 : code / 2;
  t[0] += (int)(code < 0 ? -code : code);
  if (t[1] == 0x40) {
    t[0] >>= 1;
    t[1] >>= 1;
  }
  t[1]++;
  int v = grad < 0 ? interp - (int)code : interp + (int)code;
  if (v < 0)
    v += e->total;
  else if (v > e->q4)
    v -= e->total;
  if (v < 0)
    return 0;
  return v > e->q4 ? e->q4 : v;
}

static void fj_even(const fj_enc* e, int c, int col, int* grad, int* interp) {
  const uint16_t* a = e->lines[c - 1];
  const int Rb = a[1 + 2 * col], Rc = a[2 * col], Rd = a[2 + 2 * col];
  const int Rf = e->lines[c - 2][1 + 2 * col];
  const int dcb = abs(Rc - Rb), dfb = abs(Rf - Rb), ddb = abs(Rd - Rb);
  int t1, t2;
  if (dcb > (dfb > ddb ? dfb : ddb)) {
    t1 = Rf;
    t2 = Rd;
  } else {
    t1 = ddb > (dcb > dfb ? dcb : dfb) ? Rf : Rd;
    t2 = Rc;
  }
  *interp = (2 * Rb + t1 + t2) >> 2;
  *grad = 9 * fj_quant(Rb - Rf) + fj_quant(Rc - Rb);
}

static void fj_odd(const fj_enc* e, int c, int col, int* grad, int* interp) {
  const uint16_t* a = e->lines[c - 1];
  const int Ra = e->lines[c][1 + 2 * col], Rg = e->lines[c][3 + 2 * col];
  const int Rb = a[2 + 2 * col], Rc = a[1 + 2 * col], Rd = a[3 + 2 * col];
  const int mn = Rc < Rd ? Rc : Rd, mx = Rc < Rd ? Rd : Rc;
  int v = Ra + Rg;
  if (Rb < mn || Rb > mx)
    v = (v + 2 * Rb) >> 1;
  *interp = v >> 1;
  *grad = 9 * fj_quant(Rb - Rc) + fj_quant(Rc - Ra);
}

static int fj_no_bits(int row, int i, int comp) {
  const int even = (i & 1) == 0;
  if (comp == 0)
    return row == 0 || (row == 2 && even) || (row == 4 && !even) || row == 5;
  return row == 1 || row == 2 || (row == 3 && !even) || (row == 5 && even);
}

/* (line, position) of image row r of a strip line and strip column x */
static void fj_out_index(int xtrans, int r, int x, int* line, int* pos) {
  static const char xt[6][7] = {"GGRGGB", "GGBGGR", "BRGRBG", "GGBGGR", "GGRGGB", "RBGBRG"};
  char colour;
  int idx;
  if (xtrans) {
    colour = xt[r][x % 6];
    idx = (((x * 2 / 3) & 0x7FFFFFFE) | ((x % 3) & 1)) + ((x % 3) >> 1);
  } else {
    colour = (r & 1) == (x & 1) ? ((r & 1) ? 'B' : 'R') : 'G';
    idx = x >> 1;
  }
  *line = colour == 'R' ? FJ_R2 + (r >> 1) : colour == 'G' ? FJ_G2 + r : FJ_B2 + (r >> 1);
  *pos = 1 + idx;
}

/* the six passes of a line of the strip; 0, or -1 behind a planted code */
static int fj_block(fj_enc* e) {
  const int half = e->lw / 2;
  int counter[3] = {0, 0, 0}; /* red, green, blue lines used */
  static const int first[3] = {FJ_R2, FJ_G2, FJ_B2}, last[3] = {4, 12, 17};
  for (int row = 0; row < 6; ++row) {
    const int k[2] = {(row & 1) ? 1 : 0, (row & 1) ? 2 : 1};
    int c[2];
    for (int comp = 0; comp < 2; ++comp)
      c[comp] = first[k[comp]] + counter[k[comp]]++;
    for (int i = 0; i < half + 4; ++i) {
      if (i < half)
        for (int comp = 0; comp < 2; ++comp) {
          int grad, interp, v;
          fj_even(e, c[comp], i, &grad, &interp);
          if (e->xtrans && fj_no_bits(row, i, comp))
            v = interp;
          else if ((v = fj_sample(e, grad, interp, e->ge[row % 3],
                                  e->want[c[comp]][1 + 2 * i])) < 0)
            return -1;
          e->lines[c[comp]][1 + 2 * i] = (uint16_t)v;
        }
      if (i >= 4)
        for (int comp = 0; comp < 2; ++comp) {
          int grad, interp, v;
          const int col = i - 4;
          fj_odd(e, c[comp], col, &grad, &interp);
          if ((v = fj_sample(e, grad, interp, e->go[row % 3], e->want[c[comp]][2 + 2 * col])) < 0)
            return -1;
          e->lines[c[comp]][2 + 2 * col] = (uint16_t)v;
        }
    }
    for (int comp = 0; comp < 2; ++comp)
      for (int i = first[k[comp]]; i <= last[k[comp]]; ++i) {
        e->lines[i][0] = e->lines[i - 1][1];
        e->lines[i][e->lw + 1] = e->lines[i - 1][e->lw];
      }
  }
  return 0;
}

size_t rsx_synth_fuji_encode_strip(int raw_type, int raw_bits, int total_lines,
                                   const uint16_t* target, int plant_kind, uint32_t plant_at,
                                   uint32_t plant_zeros, uint8_t* out, size_t cap, uint16_t* reached, int* planted) {
  fj_enc* e = (fj_enc*)calloc(1, sizeof(fj_enc));
  if (!e)
    return 0;
  e->raw_bits = raw_bits;
  e->total = 1 << raw_bits;
  e->q4 = e->total - 1;
  e->escape_at = raw_bits * (64 / raw_bits) - raw_bits - 1;
  e->xtrans = raw_type == 16;
  e->lw = e->xtrans ? 512 : 384;
  e->out = out;
  e->cap = cap;
  e->plant_kind = plant_kind;
  e->plant_at = plant_at;
  e->plant_zeros = plant_zeros;
  for (int j = 0; j < 3; ++j)
    for (int i = 0; i < 41; ++i) {
      e->ge[j][i][0] = e->go[j][i][0] = 1 << (raw_bits - 6);
      e->ge[j][i][1] = e->go[j][i][1] = 1;
    }
  memset(reached, 0, (size_t)total_lines * 6 * 768 * sizeof(uint16_t));
  for (int cur = 0; cur < total_lines; ++cur) {
    for (int r = 0; r < 6; ++r)
      for (int x = 0; x < 768; ++x) {
        int line, pos;
        fj_out_index(e->xtrans, r, x, &line, &pos);
        e->want[line][pos] = target[((size_t)cur * 6 + r) * 768 + x];
      }
    if (fj_block(e) < 0)
      break;
    for (int r = 0; r < 6; ++r)
      for (int x = 0; x < 768; ++x) {
        int line, pos;
        fj_out_index(e->xtrans, r, x, &line, &pos);
        reached[((size_t)cur * 6 + r) * 768 + x] = e->lines[line][pos];
      }
    if (cur + 1 == total_lines)
      break;
    static const int a[3] = {0, 5, 13}, b[3] = {5, 8, 5};
    for (int k = 0; k < 3; ++k) {
      memcpy(e->lines[a[k]], e->lines[a[k] + b[k] - 2], 2 * sizeof e->lines[0]);
      e->lines[a[k] + 2][e->lw + 1] = e->lines[a[k] + 1][e->lw];
    }
  }
  if (e->nacc)
    fj_put(e, 0, 8 - e->nacc);
  if (planted)
    *planted = e->planted;
  const size_t n = e->overflow ? 0 : e->n;
  free(e);
  return n;
}

/* ------------------------------------------------------------------------ */
/* Compressed ORF (OlympusDecompressor.cpp): the 7 bytes the decoder skips,  */
/* then one MSB-first bit string over all rows.  A symbol is a sign bit, the */
/* two low bits of the difference, then either `high` zeros and a one        */
/* (high <= 11) or twelve zeros, 15 - n bits of high and one bit the decoder */
/* skips, and then n = numLowBits bits; n follows from the carries of the    */
/* symbol's column parity, which start at zero in every row.                 */
/* ------------------------------------------------------------------------ */
typedef struct {
  uint8_t* out;
  size_t cap, n;
  uint32_t acc;
  int fill; /* bits in acc */
  int overflow;
} OlyBits;

static void oly_put(OlyBits* w, uint32_t v, int bits) {
  for (int i = bits - 1; i >= 0; --i) {
    w->acc = w->acc << 1 | ((v >> i) & 1u);
    if (++w->fill == 8) {
      if (w->n < w->cap)
        w->out[w->n++] = (uint8_t)w->acc;
      else
        w->overflow = 1;
      w->acc = 0;
      w->fill = 0;
    }
  }
}

static size_t oly_finish(OlyBits* w) {
  if (w->fill)
    oly_put(w, 0, 8 - w->fill);
  return w->overflow ? 0 : w->n;
}

typedef struct {
  int32_t c0, c1, c2;
} OlyCarry;

static int oly_low_bits(const OlyCarry* c) {
  const int bias = c->c2 < 3 ? 2 : 0;
  uint32_t v = (uint32_t)c->c0 & 0xFFFFu;
  int active = 0;
  while (v) {
    ++active;
    v >>= 1;
  }
  const int n = active - bias;
  return n > 2 + bias ? n : 2 + bias;
}

/* one symbol as given; returns the carry[0] it makes */
static int32_t oly_emit(OlyBits* w, int n, int sign, int low, int escape, uint32_t high,
                        uint32_t field, int skipped_bit) {
  oly_put(w, (uint32_t)sign & 1u, 1);
  oly_put(w, (uint32_t)low & 3u, 2);
  if (!escape) {
    oly_put(w, 0, (int)high);
    oly_put(w, 1, 1);
  } else {
    oly_put(w, 0, 12);
    oly_put(w, high, 15 - n);
    oly_put(w, (uint32_t)skipped_bit & 1u, 1);
  }
  oly_put(w, field, n);
  return (int32_t)(high << n | field);
}

static void oly_after(OlyCarry* c, int32_t c0, int sign) {
  c->c0 = c0;
  const int32_t d = (c0 ^ -sign) + c->c1;
  c->c1 = (3 * d + c->c1) >> 5;
  c->c2 = c0 > 16 ? 0 : c->c2 + 1;
}

static int32_t oly_pred(const uint16_t* img, int w, int row, int col) {
  if (row < 2 && col < 2)
    return 0;
  const int32_t left = col >= 2 ? img[(size_t)row * w + col - 2] : 0;
  if (row < 2)
    return left;
  const int32_t up = img[(size_t)(row - 2) * w + col];
  if (col < 2)
    return up;
  const int32_t nw = img[(size_t)(row - 2) * w + col - 2];
  const int32_t a = left - nw, b = up - nw;
  const int32_t aa = a < 0 ? -a : a, ab = b < 0 ? -b : b;
  if ((a < 0) != (b < 0) && a != 0 && b != 0)
    return (aa > 32 || ab > 32) ? left + b : (left + up) >> 1;
  return aa > ab ? left : up;
}

/* The stream that decodes to `target` (h rows of w pixels, no padding).  Returns its size, 7
 * leading bytes included, or 0: the image cannot be reached, or `cap` is too small. */
size_t rsx_synth_olympus_encode(int w, int h, const uint16_t* target, uint8_t* out, size_t cap) {
  if (w <= 0 || h <= 0 || (w & 1) || cap < 7)
    return 0;
  memset(out, 0, 7);
  OlyBits bw = {out + 7, cap - 7, 0, 0, 0, 0};
  for (int row = 0; row < h; ++row) {
    OlyCarry c[2] = {{0, 0, 0}, {0, 0, 0}};
    for (int col = 0; col < w; ++col) {
      OlyCarry* s = &c[col & 1];
      const int32_t p = oly_pred(target, w, row, col);
      /* the difference mod 2^16, as the representative next to zero */
      const int32_t diff = (int32_t)(((uint32_t)(target[(size_t)row * w + col] - p) + 32768u) & 0xFFFFu) - 32768;
      const int low = diff & 3;
      const int32_t x = (diff >> 2) - s->c1;
      const int sign = x < 0;
      const int32_t c0 = sign ? ~x : x;
      const int n = oly_low_bits(s);
      const uint32_t high = (uint32_t)c0 >> n, field = (uint32_t)c0 & ((1u << n) - 1u);
      if (high <= 11)
        oly_emit(&bw, n, sign, low, 0, high, field, 0);
      else if (c0 < (1 << 15))
        oly_emit(&bw, n, sign, low, 1, high, field, 1);
      else
        return 0;
      oly_after(s, c0, sign);
    }
  }
  const size_t n = oly_finish(&bw);
  return bw.overflow ? 0 : n + 7;
}

/* The stream of planted symbols: `syms` holds n_syms symbols in stream order, six ints each
 * (sign, low, escape form, high, low field, the bit the escape form skips); the low field is
 * masked to the symbol's numLowBits, high to 15 - numLowBits in the escape form.  The symbols
 * behind them, up to w h, are (0, 0, regular, 0, 0).  Returns the size, or 0. */
size_t rsx_synth_olympus_plant(int w, int h, const int32_t* syms, int n_syms, uint8_t* out,
                               size_t cap) {
  if (w <= 0 || h <= 0 || (w & 1) || cap < 7)
    return 0;
  memset(out, 0, 7);
  OlyBits bw = {out + 7, cap - 7, 0, 0, 0, 0};
  int k = 0;
  for (int row = 0; row < h; ++row) {
    OlyCarry c[2] = {{0, 0, 0}, {0, 0, 0}};
    for (int col = 0; col < w; ++col, ++k) {
      OlyCarry* s = &c[col & 1];
      static const int32_t none[6] = {0, 0, 0, 0, 0, 0};
      const int32_t* y = k < n_syms ? syms + 6 * (size_t)k : none;
      const int n = oly_low_bits(s);
      const int escape = y[2] != 0;
      if (!escape && (y[3] < 0 || y[3] > 11))
        return 0;
      const uint32_t high = escape ? (uint32_t)y[3] & ((1u << (15 - n)) - 1u) : (uint32_t)y[3];
      const uint32_t field = (uint32_t)y[4] & ((1u << n) - 1u);
      const int32_t c0 = oly_emit(&bw, n, y[0] & 1, y[1], escape, high, field, y[5]);
      oly_after(s, c0, y[0] & 1);
    }
  }
  const size_t n = oly_finish(&bw);
  return bw.overflow ? 0 : n + 7;
}

/* ------------------------------------------------------------------------ */
/* Kodak DCR (KodakDecompressor.cpp:67-150): rows of segments of at most 256 */
/* pixels; a segment is one 4-bit length a pixel, then the fields as         */
/* big-endian 16-bit units filled from the least significant bit: one unit   */
/* up front if (len & 7) == 4, then 4 bytes whenever the reader runs dry.    */
/* Every pixel gets the shortest length that holds its difference from the   */
/* pixel two to its left (0 at a segment's start).                           */
/* ------------------------------------------------------------------------ */
size_t rsx_synth_kodak_encode(int w, int h, const uint16_t* target, uint8_t* out, size_t cap) {
  if (w <= 0 || h <= 0 || (w & 3))
    return 0;
  size_t pos = 0;
  for (int row = 0; row < h; ++row) {
    for (int col = 0; col < w; col += 256) {
      const int len = w - col < 256 ? w - col : 256;
      const uint16_t* px = target + (size_t)row * (size_t)w + col;
      uint8_t n[256];
      uint32_t field[256];
      uint32_t total = 0;
      int32_t pred[2] = {0, 0};
      for (int i = 0; i < len; ++i) {
        const int32_t d = (int32_t)px[i] - pred[i & 1];
        pred[i & 1] = px[i];
        const uint32_t a = (uint32_t)(d < 0 ? -d : d);
        int bits = 0;
        while (bits < 16 && (a >> bits))
          ++bits;
        if (bits > 15)
          return 0;
        n[i] = (uint8_t)bits;
        field[i] = (uint32_t)(d >= 0 ? d : d + (1 << bits) - 1);
        total += (uint32_t)bits;
      }
      const uint32_t init = (len & 7) == 4 ? 16u : 0u;
      const uint32_t over = total > init ? total - init : 0u;
      const size_t area = init / 8u + 4u * ((over + 31u) / 32u);
      if (pos + (size_t)len / 2 + area > cap)
        return 0;
      for (int k = 0; k < len / 2; ++k)
        out[pos++] = (uint8_t)(n[2 * k] | n[2 * k + 1] << 4);
      memset(out + pos, 0, area);
      uint32_t cum = 0;
      for (int i = 0; i < len; ++i) {
        for (int b = 0; b < n[i]; ++b, ++cum)
          if ((field[i] >> b) & 1u)
            out[pos + 2 * (cum >> 4) + ((cum & 15u) < 8u ? 1 : 0)] |= (uint8_t)(1u << (cum & 7u));
      }
      pos += area;
    }
  }
  return pos;
}

/* ------------------------------------------------------------------------ */
/* Canon CRW (CrwDecompressor.cpp:167-286): blocks of 64 differences, the    */
/* first tree for coefficient 0 (a running sum over the frame's blocks), the */
/* second for run << 4 | len behind it, f0 for sixteen zeros, 00 behind the  */
/* last coefficient that is not zero; JPEG-stuffed.  `target` holds the      */
/* 10-bit values (0..1023); every difference gets the shortest length.       */
/* ------------------------------------------------------------------------ */
#include "../rsx_crw_tables.h"

typedef struct {
  uint8_t* out;
  size_t cap, pos;
  uint32_t acc;
  int held;
  int overflow;
} crw_bits;

static void crw_put(crw_bits* b, uint32_t v, int n) {
  for (int k = n - 1; k >= 0; --k) {
    b->acc = (b->acc << 1) | ((v >> k) & 1u);
    if (++b->held == 8) {
      const uint8_t byte = (uint8_t)b->acc;
      if (b->pos + 2 > b->cap) {
        b->overflow = 1;
      } else {
        b->out[b->pos++] = byte;
        if (byte == 0xFF)
          b->out[b->pos++] = 0;
      }
      b->acc = 0;
      b->held = 0;
    }
  }
}

/* the first code of the tree whose value is cv */
static int crw_code(const uint8_t* ncpl, const uint8_t* values, uint32_t cv, uint32_t* code) {
  uint32_t c = 0, at = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int k = 0; k < ncpl[len - 1]; ++k, ++c, ++at)
      if (values[at] == cv) {
        *code = c;
        return len;
      }
    c <<= 1;
  }
  return 0;
}

size_t rsx_synth_crw_encode(int w, int h, int table, const uint16_t* target, uint8_t* out,
                            size_t cap) {
  if (w <= 0 || h <= 0 || (w & 3) || ((size_t)w * (size_t)h) % 64 || table < 0 || table > 2)
    return 0;
  uint32_t code[2][256];
  uint8_t len[2][256];
  for (int cv = 0; cv < 256; ++cv) {
    len[0][cv] = (uint8_t)crw_code(RSX_CRW_FIRST_NCPL[table], RSX_CRW_FIRST_VALUES[table], (uint32_t)cv,
                                   &code[0][cv]);
    len[1][cv] = (uint8_t)crw_code(RSX_CRW_SECOND_NCPL[table], RSX_CRW_SECOND_VALUES[table], (uint32_t)cv,
                                   &code[1][cv]);
  }
  crw_bits bw = {out, cap, 0, 0, 0, 0};
  const size_t n_blocks = (size_t)w * (size_t)h / 64;
  int32_t carry = 0;
  for (size_t b = 0; b < n_blocks; ++b) {
    int32_t d[64];
    for (int k = 0; k < 64; ++k) {
      const size_t p = 64 * b + (size_t)k, col = p % (size_t)w;
      const int32_t pred = col < 2 ? 512 : (int32_t)target[p - 2];
      d[k] = (int32_t)target[p] - pred;
    }
    const int32_t first = d[0];
    d[0] -= carry;
    carry = first;
    int last = 0;
    for (int k = 1; k < 64; ++k)
      if (d[k])
        last = k;
    for (int i = 0; i <= last;) {
      int run = 0;
      if (i > 0) {
        while (d[i + run] == 0)
          ++run;
        while (run >= 16) {
          crw_put(&bw, code[1][0xF0], len[1][0xF0]);
          run -= 16;
          i += 16;
        }
      }
      const int32_t v = d[i + run];
      const uint32_t a = (uint32_t)(v < 0 ? -v : v);
      int n = 0;
      while (a >> n)
        ++n;
      const uint32_t cv = (uint32_t)(run << 4 | n);
      const int tree = i > 0;
      if (n > (tree ? 10 : 11) || len[tree][cv] == 0)
        return 0;
      crw_put(&bw, code[tree][cv], len[tree][cv]);
      crw_put(&bw, (uint32_t)(v >= 0 ? v : v + (1 << n) - 1), n);
      i += run + 1;
    }
    if (last < 63)
      crw_put(&bw, code[1][0x00], len[1][0x00]);
  }
  if (bw.held)
    crw_put(&bw, 0, 8 - bw.held);
  return bw.overflow ? 0 : bw.pos;
}
