// rsx_fpwrite_core.h -- the arithmetic of the floating-point writers (include/rsx.h section 7d,
// DESIGN.md 4.28): the inverse of UncompressedDecompressor's F32 branches (copyPixels and
// decodePackedFP<Pump, Binary16 | Binary24>, .cpp:171-186, :212-245) with the exact narrowing of
// rsx_fp_narrow.h, and the width class of a window of samples.  Plain C++ that builds for the host
// (rsx_fpwrite_host.cpp, one thread) and for the device (rsx_fpwrite_pack.hip): the checks, the
// gather of a lane's 16 output bytes, and a single-threaded walk of whole jobs that the device is
// held against.
#pragma once

#include "rsx.h"
#include "rsx_fp_narrow.h"

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RSX_FPW_HD __host__ __device__ __forceinline__
#else
#define RSX_FPW_HD inline
#endif

namespace rsx_fpwrite {

constexpr int PACK_LANE_BYTES = 16;                              // a lane's piece of the output
constexpr int PACK_THREADS = 256;                                // lanes of a workgroup
constexpr int PACK_BLOCK_BYTES = PACK_LANE_BYTES * PACK_THREADS; // a workgroup's piece
constexpr int FIT_THREADS = 256;
constexpr int FIT_LANE_SAMPLES = 16;                             // samples a lane of the fit kernel reads
constexpr int FIT_BLOCK_SAMPLES = FIT_THREADS * FIT_LANE_SAMPLES;
constexpr uint32_t FIT_MAX_BLOCKS = 1024;                        // workgroups of one window

RSX_FPW_HD uint64_t round_up4(uint64_t v) { return (v + 3u) & ~uint64_t(3); }

// The first sample of a row that the reader writes: copyPixels starts at out(y, offset.x * cpp)
// (.cpp:216-217), decodePackedFP at out(row, offset.x + col) (.cpp:181).
RSX_FPW_HD uint64_t first_sample(const rsx_unpack_desc& d, const rsx_image& img) {
  return d.bits_per_pixel == 32 ? uint64_t(d.crop_x) * uint64_t(img.cpp) : uint64_t(d.crop_x);
}

// rsx_unpack_f32_validate's verdicts in its order (the reader's input is the stream this writes,
// so of its size checks the 32-bit one alone applies), then what a writer needs beyond a reader:
// the rows it reads exist, rows of 4-byte samples hold what is read, and the output has room.
RSX_FPW_HD int validate_pack(const rsx_unpack_desc* d, const rsx_image* img, uint64_t out_cap) {
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
  if (d->bits_per_pixel < 1 || d->bits_per_pixel > 32)
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
  if (d->bits_per_pixel != 32) {
    const bool byte_order = d->bit_order == RSX_ORDER_MSB || d->bit_order == RSX_ORDER_LSB;
    if (!byte_order || (d->bits_per_pixel != 16 && d->bits_per_pixel != 24))
      return RSX_ERR_INVALID_ARG; // "Unsupported floating-point input bitwidth/bit packing"
    if (need < 4)
      return RSX_ERR_IO;
  }
  // the writer's own: it reads the image, so the image has a size (a negative one would pass the
  // reader's unsigned comparisons above), every row read lies in it, rows hold their samples
  if (img->dim_x < 1 || img->dim_y < 1)
    return RSX_ERR_INVALID_ARG;
  if (uint64_t(d->crop_y) + uint64_t(d->crop_h) > uint64_t(img->dim_y))
    return RSX_ERR_INVALID_ARG;
  if (img->pitch_bytes % 4 != 0 ||
      uint64_t(img->pitch_bytes) <
          (first_sample(*d, *img) + uint64_t(d->crop_w) * uint64_t(img->cpp)) * 4u)
    return RSX_ERR_INVALID_ARG;
  if (out_cap < round_up4(need))
    return RSX_ERR_INVALID_ARG;
  return RSX_OK;
}

struct PackGeom {
  uint64_t img_off;      // first sample read, from the images' base
  uint64_t out_off;      // first byte written, from the streams' base
  uint64_t stream_bytes; // crop_h * pitch
  uint64_t out_bytes;    // round_up4(stream_bytes): BitVacuumer::flush pads to a 32-bit chunk
  uint32_t img_pitch;
  uint32_t pitch;        // of the stream
  uint32_t row_bytes;    // of a stream row that hold samples
  uint32_t bytesps;      // 2, 3 or 4
  uint32_t big_endian;   // MSB order of a 16- or 24-bit stream; a 32-bit stream is copied
  uint32_t first_block;  // of the plan's flat list of workgroups
  uint32_t job;          // whose count of inexact samples this job adds to
  uint32_t reserved;
};

RSX_FPW_HD void pack_geom(const rsx_unpack_desc& d, const rsx_image& img, uint64_t img_off,
                          uint64_t out_off, PackGeom* g) {
  g->img_off = img_off + uint64_t(d.crop_y) * img.pitch_bytes + first_sample(d, img) * 4u;
  g->out_off = out_off;
  g->stream_bytes = uint64_t(d.crop_h) * uint64_t(d.input_pitch_bytes);
  g->out_bytes = round_up4(g->stream_bytes);
  g->img_pitch = img.pitch_bytes;
  g->pitch = uint32_t(d.input_pitch_bytes);
  g->row_bytes = uint32_t(uint64_t(d.crop_w) * uint64_t(img.cpp) * uint64_t(d.bits_per_pixel) / 8);
  g->bytesps = uint32_t(d.bits_per_pixel) / 8u;
  g->big_endian = d.bits_per_pixel != 32 && d.bit_order == RSX_ORDER_MSB ? 1u : 0u;
  g->first_block = 0;
  g->job = 0;
  g->reserved = 0;
}

RSX_FPW_HD void or_byte(uint32_t (&w)[4], uint32_t i, uint32_t byte) {
  // (no indexing by a variable: the four words stay in registers)
  const uint32_t v = byte << (8u * (i & 3u));
  w[0] |= (i >> 2) == 0u ? v : 0u;
  w[1] |= (i >> 2) == 1u ? v : 0u;
  w[2] |= (i >> 2) == 2u ? v : 0u;
  w[3] |= (i >> 2) == 3u ? v : 0u;
}

// The 16 bytes [16 k, 16 k + 16) of the output of job g as four little-endian words: the samples
// that cover them, narrowed and gathered.  Bytes of the pitch beyond row_bytes and bytes beyond
// stream_bytes are zero.  Returns how many samples whose FIRST stream byte lies in the piece have
// no narrow pattern (every sample is counted by exactly one piece); such a sample's bytes are
// zero.  `img` is the images' base.  The stream is at most 2^32 - 1 bytes (validate_pack).
RSX_FPW_HD uint32_t pack_chunk(const uint8_t* img, const PackGeom& g, uint64_t k, uint32_t (&out)[4]) {
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  uint32_t inexact = 0;
  const uint64_t begin = k * 16u;
  const uint64_t end = g.stream_bytes - begin < 16u ? g.stream_bytes : begin + 16u;
  const uint32_t bps = 8u * g.bytesps;
  if (g.bytesps == 4u && g.pitch % 4u == 0u) {
    // copyPixels with rows on the word grid: a word of the stream is a sample or padding, whole
    for (uint32_t i = 0; i < 4u; ++i) {
      const uint64_t pos = begin + 4u * i;
      uint32_t v = 0;
      if (pos < g.stream_bytes) {
        const uint32_t r = uint32_t(pos) / g.pitch, b = uint32_t(pos) - r * g.pitch;
        if (b < g.row_bytes)
          v = reinterpret_cast<const uint32_t*>(img + g.img_off + uint64_t(r) * g.img_pitch)[b >> 2];
      }
      out[i] = v;
    }
    return 0;
  }
  uint64_t pos = begin;
  while (pos < end) {
    const uint64_t r = uint32_t(pos) / g.pitch, row0 = r * g.pitch; // (pos < 2^32)
    const uint64_t seg_end = end - row0 < g.pitch ? end : row0 + g.pitch;
    const uint32_t b = uint32_t(pos - row0);
    uint32_t b_end = uint32_t(seg_end - row0);
    if (b_end > g.row_bytes)
      b_end = g.row_bytes;
    if (b < b_end) {
      const uint32_t* src = reinterpret_cast<const uint32_t*>(img + g.img_off + r * g.img_pitch);
      const uint32_t x0 = b / g.bytesps, x1 = (b_end - 1u) / g.bytesps;
      const uint32_t lead = uint32_t(pos - begin);
      for (uint32_t x = x0; x <= x1; ++x) {
        uint32_t n;
        const bool exact = narrow_fp_bps(src[x], bps, &n);
        const uint32_t first = x * g.bytesps; // the sample's first byte in the row
        if (!exact) {
          n = 0;
          inexact += first >= b ? 1u : 0u;
        }
        for (uint32_t j = 0; j < g.bytesps; ++j) {
          const uint32_t at = first + j; // byte of the row
          if (at >= b && at < b_end) {
            const uint32_t shift = g.big_endian ? 8u * (g.bytesps - 1u - j) : 8u * j;
            or_byte(w, lead + (at - b), (n >> shift) & 0xFFu);
          }
        }
      }
    }
    pos = seg_end;
  }
  for (int i = 0; i < 4; ++i)
    out[i] = w[i];
  return inexact;
}

// The reference walk of one job: a chunk after the other.  Returns the count of inexact samples.
inline uint64_t pack_walk(const uint8_t* img, const PackGeom& g, uint8_t* out) {
  uint64_t inexact = 0;
  for (uint64_t k = 0; k * 16u < g.out_bytes; ++k) {
    uint32_t w[4];
    inexact += pack_chunk(img, g, k, w);
    for (uint64_t i = 0; i < 16u && k * 16u + i < g.out_bytes; ++i)
      out[g.out_off + k * 16u + i] = uint8_t(w[i >> 2] >> (8u * (i & 3u)));
  }
  return inexact;
}

// ---------------------------------------------------------------------------------------------
// The width class of windows
// ---------------------------------------------------------------------------------------------
// A window of samples (x and w count samples, cpp folded in) inside the image
RSX_FPW_HD int validate_fit(const rsx_image* img, int n_windows, const rsx_fpwrite_window* win) {
  if (!img || !win || n_windows < 1)
    return RSX_ERR_INVALID_ARG;
  if (img->cpp < 1 || img->cpp > 4 || img->dim_x < 1 || img->dim_y < 1 || img->pitch_bytes % 4 != 0 ||
      uint64_t(img->pitch_bytes) < uint64_t(img->dim_x) * uint64_t(img->cpp) * 4u)
    return RSX_ERR_INVALID_ARG;
  const uint64_t row = uint64_t(img->dim_x) * uint64_t(img->cpp);
  for (int i = 0; i < n_windows; ++i) {
    const rsx_fpwrite_window& q = win[i];
    if (q.x < 0 || q.y < 0 || q.w < 1 || q.h < 1 || uint64_t(q.x) + uint64_t(q.w) > row ||
        uint64_t(q.y) + uint64_t(q.h) > uint64_t(img->dim_y))
      return RSX_ERR_INVALID_ARG;
  }
  return RSX_OK;
}

struct FitGeom {
  uint64_t img_off;     // the window's first sample, from the image's base
  uint64_t samples;     // w * h
  uint32_t w;
  uint32_t img_pitch;
  uint32_t first_block; // of the launch's flat list of workgroups
  uint32_t n_blocks;    // workgroups of this window: each takes every n_blocks-th piece
};

RSX_FPW_HD void fit_geom(const rsx_image& img, const rsx_fpwrite_window& q, FitGeom* g) {
  g->img_off = uint64_t(q.y) * img.pitch_bytes + uint64_t(q.x) * 4u;
  g->samples = uint64_t(q.w) * uint64_t(q.h);
  g->w = uint32_t(q.w);
  g->img_pitch = img.pitch_bytes;
  // rows that follow each other without a gap are one row (no division per sample)
  if (uint64_t(q.w) * 4u == img.pitch_bytes && g->samples <= 0xFFFFFFFFull)
    g->w = uint32_t(g->samples);
  const uint64_t pieces = (g->samples + FIT_BLOCK_SAMPLES - 1u) / FIT_BLOCK_SAMPLES;
  g->n_blocks = uint32_t(pieces < FIT_MAX_BLOCKS ? pieces : FIT_MAX_BLOCKS);
  g->first_block = 0;
}

// the class of sample i of the window (row-major)
RSX_FPW_HD uint32_t fit_sample_class(const uint8_t* img, const FitGeom& g, uint64_t i) {
  uint64_t r = 0;
  if (i >= g.w)
    r = i <= 0xFFFFFFFFull ? uint64_t(uint32_t(i) / g.w) : i / g.w;
  const uint64_t c = i - r * g.w;
  return fp_fit_class(reinterpret_cast<const uint32_t*>(img + g.img_off + r * g.img_pitch)[c]);
}

RSX_FPW_HD int32_t fit_bps_of_class(uint32_t cls) { return cls == 0u ? 16 : cls == 1u ? 24 : 32; }

inline int32_t fit_walk(const uint8_t* img, const FitGeom& g) {
  uint32_t cls = 0;
  for (uint64_t i = 0; i < g.samples; ++i) {
    const uint32_t c = fit_sample_class(img, g, i);
    cls = c > cls ? c : cls;
  }
  return fit_bps_of_class(cls);
}

} // namespace rsx_fpwrite
