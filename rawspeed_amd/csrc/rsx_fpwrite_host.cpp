// rsx_fpwrite_host.cpp -- rsx_fpwrite_core.h and rsx_fp_narrow.h as host C++: the single-threaded
// reference walk that the device kernels (rsx_fpwrite_pack.hip) are held against, built into
// rawspeed_amd/librsx_fpwrite_host.so.  With -DRSX_FPWRITE_HOST_MAIN the same source is a program
// (AddressSanitizer + UBSan where the runtimes exist) that checks the narrowing over every
// binary16 and binary24 pattern and their binary32 neighbours, and walks small pack geometries
// and windows.
#include "rsx_fpwrite_core.h"
#include "rsx_deflate_core.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace rsx_fpwrite;

extern "C" {

int rsx_fpwrite_host_pack_block_bytes(void) { return PACK_BLOCK_BYTES; }
int rsx_fpwrite_host_fit_block_samples(void) { return FIT_BLOCK_SAMPLES; }
int rsx_fpwrite_host_fit_max_blocks(void) { return int(FIT_MAX_BLOCKS); }

// 1 and *out = the narrow pattern iff x has one under bps (16, 24, 32)
int rsx_fpwrite_host_narrow(uint32_t x, int bps, uint32_t* out) {
  return narrow_fp_bps(x, uint32_t(bps), out) ? 1 : 0;
}

uint32_t rsx_fpwrite_host_widen(uint32_t n, int bps) {
  return bps == 16 ? widen_fp_plain<10, 5>(n) : bps == 24 ? widen_fp_plain<16, 7>(n) : n;
}

// patterns [first, first + n) of the narrow format widened at once
void rsx_fpwrite_host_widen_range(uint32_t first, size_t n, int bps, uint32_t* out) {
  for (size_t i = 0; i < n; ++i)
    out[i] = rsx_fpwrite_host_widen(first + uint32_t(i), bps);
}

// the width class (0, 1, 2 for 16, 24, 32 bits) of n samples at once
void rsx_fpwrite_host_fit_class_many(const uint32_t* x, size_t n, uint8_t* out) {
  for (size_t i = 0; i < n; ++i)
    out[i] = uint8_t(fp_fit_class(x[i]));
}

// n samples at once: out[i] the narrow pattern, exact[i] 1 or 0
void rsx_fpwrite_host_narrow_many(const uint32_t* x, size_t n, int bps, uint32_t* out,
                                  uint8_t* exact) {
  for (size_t i = 0; i < n; ++i)
    exact[i] = narrow_fp_bps(x[i], uint32_t(bps), &out[i]) ? 1 : 0;
}

int rsx_fpwrite_host_pack_validate(const rsx_unpack_desc* d, const rsx_image* img, size_t out_cap) {
  return validate_pack(d, img, out_cap);
}

// img->data: the image in host memory.  The bytes are written whatever the status.
int rsx_fpwrite_host_pack(const rsx_unpack_desc* d, const rsx_image* img, uint8_t* out,
                          size_t out_cap, rsx_fpwrite_pack_result* res) {
  if (!d || !img || !img->data || !out || !res)
    return RSX_ERR_INVALID_ARG;
  std::memset(res, 0, sizeof *res);
  if (int st = validate_pack(d, img, out_cap))
    return st;
  PackGeom g;
  pack_geom(*d, *img, 0, 0, &g);
  res->inexact = pack_walk(static_cast<const uint8_t*>(img->data), g, out);
  res->stream_bytes = g.stream_bytes;
  res->bytes_written = res->inexact ? 0 : g.out_bytes;
  return res->inexact ? RSX_ERR_VALUE_RANGE : RSX_OK;
}

int rsx_fpwrite_host_fit(const rsx_image* img, int n_windows, const rsx_fpwrite_window* win,
                         int32_t* min_bps_out) {
  if (!img || !img->data || !min_bps_out)
    return RSX_ERR_INVALID_ARG;
  if (int st = validate_fit(img, n_windows, win))
    return st;
  for (int i = 0; i < n_windows; ++i) {
    FitGeom g;
    fit_geom(*img, win[i], &g);
    min_bps_out[i] = fit_walk(static_cast<const uint8_t*>(img->data), g);
  }
  return RSX_OK;
}

// One tile through rsx_deflate_core.h on one thread: what the device must write byte for byte.
// img->data: the image in host memory.  Returns the tile's status.
int rsx_fpwrite_host_deflate(const rsx_dng_deflate_desc* d, const rsx_fpwrite_deflate_tile* t,
                             const rsx_image* img, rsx_fpwrite_deflate_result* res) {
  using namespace rsx_deflate;
  if (!d || !t || !img || !img->data || !res)
    return RSX_ERR_INVALID_ARG;
  std::memset(res, 0, sizeof *res);
  if (int st = validate_tile(*d, t->tile_w, t->tile_h, t->off_x, t->off_y, t->width, t->height, *img))
    return res->status = st;
  TileGeom g;
  tile_geom(*d, t->tile_w, t->tile_h, t->off_x, t->off_y, t->width, t->height, *img, 0, 0, t->out_cap,
            &g);
  std::vector<uint8_t> data(g.n_bytes);
  bool inexact = false;
  for (uint32_t i = 0; i < g.n_bytes; ++i)
    data[i] = plane_byte(static_cast<const uint8_t*>(img->data), g, i, &inexact);
  std::vector<BlockWork> works(g.n_blocks);
  for (uint32_t k = 0; k < g.n_blocks; ++k)
    compress_block(data.data(), g.n_bytes, k * BLOCK,
                   k + 1u < g.n_blocks ? BLOCK : g.n_bytes - k * BLOCK, k + 1u == g.n_blocks, &works[k]);
  std::vector<BlockInfo> info(g.n_blocks);
  TileInfo ti;
  scan_tile(g, works.data(), inexact, info.data(), &ti);
  if (ti.status == RSX_OK && t->out)
    for (uint64_t j = 0; j < ti.bytes; ++j)
      t->out[j] = stream_byte(g, ti, works.data(), info.data(), data.data(), j);
  res->status = ti.status, res->adler = ti.adler, res->bytes = ti.bytes;
  res->blocks = ti.blocks, res->stored_blocks = ti.stored_blocks;
  return ti.status;
}

uint64_t rsx_fpwrite_host_deflate_bound(const rsx_dng_deflate_desc* d,
                                        const rsx_fpwrite_deflate_tile* t, const rsx_image* img) {
  using namespace rsx_deflate;
  if (!d || !t || !img ||
      validate_tile(*d, t->tile_w, t->tile_h, t->off_x, t->off_y, t->width, t->height, *img))
    return 0;
  return bound_of(uint64_t(d->bps / 8) * t->tile_w * t->tile_h);
}

// the limiter alone: n counts -> n lengths limited to maxbits; returns the used symbols or -1
int rsx_fpwrite_host_limit(const uint32_t* freq, int n, int maxbits, uint8_t* len) {
  if (!freq || !len || n < 1 || n > rsx_deflate::NLL || maxbits < 1 || maxbits > 15)
    return -2;
  std::vector<rsx_deflate::BlockWork> w(1);
  return rsx_deflate::build_lengths(freq, n, maxbits, len, &w[0]);
}

// the parse of the first block of `n` raw bytes: out[0] matches, out[1] distance codes used
void rsx_fpwrite_host_block_stats(const uint8_t* data, uint32_t n, uint32_t* out) {
  using namespace rsx_deflate;
  std::vector<BlockWork> w(1);
  compress_block(data, n, 0, n < BLOCK ? n : BLOCK, n <= BLOCK, &w[0]);
  out[0] = w[0].matches;
  out[1] = w[0].distances_used;
}

// a block of raw bytes (no image): compress `n` bytes as one tile's bytes; for the tests of the
// parse and the tables.  out: bound_of(n) bytes.  Returns the stream's length.
uint64_t rsx_fpwrite_host_deflate_bytes(const uint8_t* data, uint32_t n, uint8_t* out,
                                        rsx_fpwrite_deflate_result* res) {
  using namespace rsx_deflate;
  TileGeom g;
  std::memset(&g, 0, sizeof g);
  g.n_bytes = n, g.n_blocks = blocks_of(n), g.out_cap = bound_of(n);
  std::vector<BlockWork> works(g.n_blocks);
  for (uint32_t k = 0; k < g.n_blocks; ++k)
    compress_block(data, n, k * BLOCK, k + 1u < g.n_blocks ? BLOCK : n - k * BLOCK,
                   k + 1u == g.n_blocks, &works[k]);
  std::vector<BlockInfo> info(g.n_blocks);
  TileInfo ti;
  scan_tile(g, works.data(), false, info.data(), &ti);
  for (uint64_t j = 0; j < ti.bytes; ++j)
    out[j] = stream_byte(g, ti, works.data(), info.data(), data, j);
  if (res) {
    res->status = ti.status, res->adler = ti.adler, res->bytes = ti.bytes;
    res->blocks = ti.blocks, res->stored_blocks = ti.stored_blocks;
  }
  return ti.bytes;
}

} // extern "C"

#ifdef RSX_FPWRITE_HOST_MAIN
#include <algorithm>

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return uint32_t(rng_state >> 16);
}

// Every pattern p of the narrow format: narrow(widen(p)) == p.  Every binary32 pattern one unit
// in the last place above or below an image: exact iff it is itself an image (membership by
// search in the sorted list of all images, not by the code under test).
int check_narrowing(int bps) {
  const uint32_t n = 1u << bps;
  std::vector<uint32_t> images(n);
  for (uint32_t p = 0; p < n; ++p) {
    images[p] = rsx_fpwrite_host_widen(p, bps);
    uint32_t back = 0;
    if (!rsx_fpwrite_host_narrow(images[p], bps, &back) || back != p ||
        !(bps == 16 ? fits_fp<10, 5>(images[p]) : fits_fp<16, 7>(images[p])))
      return std::printf("narrow %d: pattern %x -> %x -> %x\n", bps, p, images[p], back), 1;
  }
  std::vector<uint32_t> sorted(images);
  std::sort(sorted.begin(), sorted.end());
  if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
    return std::printf("narrow %d: two patterns with one image\n", bps), 1;
  uint64_t inexact = 0;
  for (uint32_t p = 0; p < n; ++p)
    for (uint32_t y : {images[p] + 1u, images[p] - 1u}) {
      const bool image = std::binary_search(sorted.begin(), sorted.end(), y);
      uint32_t back = 0;
      const bool exact = rsx_fpwrite_host_narrow(y, bps, &back) != 0;
      if ((bps == 16 ? fits_fp<10, 5>(y) : fits_fp<16, 7>(y)) != exact)
        return std::printf("narrow %d: the predicate on %x\n", bps, y), 1;
      if (exact != image || (exact && rsx_fpwrite_host_widen(back, bps) != y))
        return std::printf("narrow %d: neighbour %x of %x\n", bps, y, images[p]), 1;
      inexact += exact ? 0 : 1;
    }
  // binary32 subnormals, and the exponents from one above the narrow maximum up to 254
  const int frac = bps == 16 ? 10 : 16, expw = bps == 16 ? 5 : 7;
  const uint32_t top = 127u + ((1u << (expw - 1)) - 1u) + 1u; // narrow exponent all ones: inf / NaN
  for (uint32_t sign = 0; sign < 2; ++sign) {
    uint32_t back;
    for (uint32_t f = 1; f < (1u << 23); f += (f < 4096 ? 1 : 4093))
      if (rsx_fpwrite_host_narrow(sign << 31 | f, bps, &back))
        return std::printf("narrow %d: subnormal %x\n", bps, f), 1;
    if (rsx_fpwrite_host_narrow(sign << 31 | 0x7FFFFFu, bps, &back))
      return std::printf("narrow %d: largest subnormal\n", bps), 1;
    for (uint32_t e = top; e < 255u; ++e)
      for (uint32_t f : {0u, 1u << (23 - frac), 0x7FFFFFu & ~((1u << (23 - frac)) - 1u)})
        if (rsx_fpwrite_host_narrow(sign << 31 | e << 23 | f, bps, &back))
          return std::printf("narrow %d: exponent %u\n", bps, e), 1;
  }
  // the predicate of the fit is narrow_fp's verdict on patterns of every exponent
  for (uint32_t k = 0; k < (1u << 24); ++k) {
    const uint32_t x = rnd() << 16 ^ rnd(), y = x & ~((1u << (rnd() % 24)) - 1u);
    uint32_t back;
    for (uint32_t v : {x, y})
      if ((rsx_fpwrite_host_narrow(v, bps, &back) != 0) !=
          (bps == 16 ? fits_fp<10, 5>(v) : fits_fp<16, 7>(v)))
        return std::printf("narrow %d: the predicate on %x\n", bps, v), 1;
  }
  std::printf("narrow %d: %u patterns, %llu inexact neighbours\n", bps, n,
              static_cast<unsigned long long>(inexact));
  return 0;
}

// a binary32 pattern with a narrow pattern under bps
uint32_t exact_sample(int bps) {
  return rsx_fpwrite_host_widen(rnd() & uint32_t((1ull << bps) - 1u), bps);
}

int check_pack() {
  int n = 0;
  for (int bps : {16, 24, 32})
    for (int order : {int(RSX_ORDER_LSB), int(RSX_ORDER_MSB)})
      for (int cpp = 1; cpp <= 3; ++cpp)
        for (int h = 1; h <= 4; ++h)
          for (int w = 1; w <= 23; ++w)
            for (int crop_x : {0, 2})
              for (int pad : {0, 3}) {
                const int cols = w * cpp, bytesps = bps / 8;
                const int pitch = cols * bytesps + pad;
                if (bps != 32 && h * pitch < 4)
                  continue;
                const int dim_x = w + crop_x, row = dim_x * cpp + 1;
                std::vector<uint32_t> img(size_t(h + 1) * row);
                for (uint32_t& v : img)
                  v = exact_sample(bps);
                rsx_image im{img.data(), uint32_t(4 * row), dim_x, h + 1, cpp, 1};
                rsx_unpack_desc d{crop_x, 1, w, h, pitch, bps, order};
                const size_t cap = size_t(round_up4(uint64_t(h) * pitch));
                std::vector<uint8_t> out(cap, uint8_t(0xEE));
                rsx_fpwrite_pack_result res;
                if (rsx_fpwrite_host_pack(&d, &im, out.data(), cap, &res) != RSX_OK ||
                    res.bytes_written != cap || res.inexact != 0)
                  return std::printf("pack: status bps %d order %d %dx%d\n", bps, order, w, h), 1;
                const int x0 = bps == 32 ? crop_x * cpp : crop_x;
                for (int r = 0; r < h; ++r) {
                  for (int c = 0; c < cols; ++c) {
                    uint32_t v = 0;
                    for (int j = 0; j < bytesps; ++j) {
                      const uint32_t byte = out[size_t(r) * pitch + size_t(c) * bytesps + j];
                      const bool big = bps != 32 && order == RSX_ORDER_MSB;
                      v |= byte << (big ? 8 * (bytesps - 1 - j) : 8 * j);
                    }
                    if (rsx_fpwrite_host_widen(v, bps) != img[size_t(r + 1) * row + x0 + c])
                      return std::printf("pack: sample bps %d order %d %dx%d\n", bps, order, w, h), 1;
                  }
                  for (size_t i = size_t(r) * pitch + size_t(cols) * bytesps;
                       i < size_t(r + 1) * pitch; ++i)
                    if (out[i] != 0)
                      return std::printf("pack: padding\n"), 1;
                }
                for (size_t i = size_t(h) * pitch; i < cap; ++i)
                  if (out[i] != 0)
                    return std::printf("pack: tail\n"), 1;
                // one inexact sample: counted once, nothing reported as written
                if (bps != 32) {
                  img[size_t(1 + rnd() % h) * row + x0 + rnd() % cols] = 0x3F800001u;
                  if (rsx_fpwrite_host_pack(&d, &im, out.data(), cap, &res) != RSX_ERR_VALUE_RANGE ||
                      res.bytes_written != 0 || res.inexact != 1)
                    return std::printf("pack: inexact bps %d %dx%d\n", bps, w, h), 1;
                }
                ++n;
              }
  std::printf("pack: %d geometries round-trip\n", n);
  return 0;
}

int check_fit() {
  const int w = 37, h = 9;
  std::vector<uint32_t> img(size_t(w) * h);
  for (uint32_t& v : img)
    v = exact_sample(16);
  rsx_image im{img.data(), uint32_t(4 * w), w, h, 1, 1};
  const rsx_fpwrite_window win[4] = {{0, 0, w, h}, {1, 1, 5, 3}, {30, 6, 7, 3}, {0, 8, 37, 1}};
  int32_t got[4];
  if (rsx_fpwrite_host_fit(&im, 4, win, got) || got[0] != 16 || got[1] != 16 || got[2] != 16 ||
      got[3] != 16)
    return std::printf("fit: all 16\n"), 1;
  img[size_t(8) * w + 36] = 0x3F800080u; // 1 + 2^-16: binary24, in the last row and column
  if (rsx_fpwrite_host_fit(&im, 4, win, got) || got[0] != 24 || got[1] != 16 || got[2] != 24 ||
      got[3] != 24)
    return std::printf("fit: one 24\n"), 1;
  img[size_t(2) * w + 3] = 0x3F800001u;
  if (rsx_fpwrite_host_fit(&im, 4, win, got) || got[0] != 32 || got[1] != 32 || got[2] != 24)
    return std::printf("fit: one 32\n"), 1;
  const rsx_fpwrite_window bad = {30, 6, 8, 3};
  if (rsx_fpwrite_host_fit(&im, 1, &bad, got) != RSX_ERR_INVALID_ARG)
    return std::printf("fit: window outside\n"), 1;
  std::printf("fit: windows\n");
  return 0;
}



// The deflate shape list of tests/fpwrite_files.py as a file of 32-bit words: per case bps,
// predictor, cpp, the six numbers of the geometry, pitch, dim_x, dim_y, then pitch dim_y / 4 words
// of image.  Every tile is written into exactly the bytes it takes, into one byte less
// (RSX_ERR_INPUT_OVERFLOW, nothing written) and with its window's last sample made inexact.
int check_deflate_file(const char* path) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f)
    return std::printf("deflate: cannot open %s\n", path), 1;
  int n = 0;
  uint32_t h[12];
  while (std::fread(h, 4, 12, f) == 12) {
    std::vector<uint32_t> px(size_t(h[9]) / 4 * h[11]);
    if (std::fread(px.data(), 4, px.size(), f) != px.size())
      return std::printf("deflate: short file\n"), 1;
    rsx_dng_deflate_desc d{int32_t(h[0]), int32_t(h[1])};
    rsx_image im{px.data(), h[9], int32_t(h[10]), int32_t(h[11]), int32_t(h[2]), 0};
    rsx_fpwrite_deflate_tile t{nullptr, 0, h[3], h[4], h[5], h[6], h[7], h[8]};
    const uint64_t bound = rsx_fpwrite_host_deflate_bound(&d, &t, &im);
    std::vector<uint8_t> big(bound);
    t.out = big.data(), t.out_cap = bound;
    rsx_fpwrite_deflate_result r, r2;
    if (bound == 0 || rsx_fpwrite_host_deflate(&d, &t, &im, &r) != RSX_OK || r.bytes > bound)
      return std::printf("deflate: case %d\n", n), 1;
    std::vector<uint8_t> exact(r.bytes), tight(r.bytes - 1);
    t.out = exact.data(), t.out_cap = exact.size();
    if (rsx_fpwrite_host_deflate(&d, &t, &im, &r2) != RSX_OK || r2.bytes != r.bytes ||
        std::memcmp(exact.data(), big.data(), exact.size()) != 0)
      return std::printf("deflate: case %d into its own size\n", n), 1;
    t.out = tight.data(), t.out_cap = tight.size();
    if (rsx_fpwrite_host_deflate(&d, &t, &im, &r2) != RSX_ERR_INPUT_OVERFLOW || r2.bytes != 0)
      return std::printf("deflate: case %d one byte short\n", n), 1;
    if (d.bps != 32) {
      px[size_t(h[9]) / 4 * (h[6] + h[8] - 1) + h[5] + h[7] - 1] = 0x3F800001u;
      t.out = big.data(), t.out_cap = bound;
      if (rsx_fpwrite_host_deflate(&d, &t, &im, &r2) != RSX_ERR_VALUE_RANGE || r2.bytes != 0)
        return std::printf("deflate: case %d inexact\n", n), 1;
    }
    ++n;
  }
  std::fclose(f);
  std::printf("deflate: %d tiles\n", n);
  return 0;
}

} // namespace

int main(int argc, char** argv) {
  if (argc > 1)
    return check_deflate_file(argv[1]) ? 1 : (std::printf("rsx_fpwrite_host_check OK\n"), 0);
  if (check_narrowing(16) || check_narrowing(24) || check_pack() || check_fit())
    return 1;
  std::printf("rsx_fpwrite_host_check OK\n");
  return 0;
}
#endif
