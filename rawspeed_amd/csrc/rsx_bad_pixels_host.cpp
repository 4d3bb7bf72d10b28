// rsx_bad_pixels_core.h as host C++ (librsx_bad_pixels_host.so): the same validation, word-wise
// search and interpolation as the kernels of rsx_bad_pixels.hip, driven by loops that mirror them
// -- the row map from map_in and the positions, the column map by column_word, then every set bit
// of every row-map word below fix_end -- so that the test cases meet the code on the CPU first.
// Compiled with -ffp-contract=off.  With -DRSX_BAD_PIXELS_HOST_MAIN the file is a program (built
// with AddressSanitizer and UBSan where g++ has them) that runs built-in cases, and the case file
// a test hands it, against a pixel-at-a-time restatement of fixBadPixelsThread / fixBadPixel.
#include "rsx_bad_pixels_core.h"

#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <thread>
#include <vector>

using namespace rsx_bp;

extern "C" int rsx_bad_pixels_host_validate(const rsx_bad_pixels_desc* desc, const rsx_image* img) {
  return validate(desc, img);
}

namespace {

// rows [y0, y1) of the scan; returns the pixels it fixed
uint64_t fix_rows(const Geo& g, const uint64_t* rowmap, const uint64_t* colmap, uint8_t* data,
                  uint32_t y0, uint32_t y1) {
  uint64_t n_fixed = 0;
  for (uint32_t y = y0; y < y1; ++y)
    for (uint32_t xw = 0; xw < g.wpr; ++xw) {
      uint64_t word = rowmap[size_t(y) * g.wpr + xw];
      while (word) {
        const uint32_t x = xw * 64u + uint32_t(ctz64(word));
        word &= word - 1ull;
        if (x >= g.fix_end)
          continue;
        ++n_fixed;
        uint8_t* p = data + size_t(y) * g.pitch + size_t(x) * (g.is_f32 ? 4u : 2u);
        if (g.is_f32) {
          const uint32_t v = fix_f32(g, rowmap, colmap, data, x, y);
          std::memcpy(p, &v, 4);
        } else {
          const uint16_t v = fix_u16(g, rowmap, colmap, data, x, y);
          std::memcpy(p, &v, 2);
        }
      }
    }
  return n_fixed;
}

} // namespace

// rsx_bad_pixels_fix on the host: img->data in place (untouched unless RSX_OK).  threads > 1: the
// scan in row bands of ceil(h / threads) rows, RawImageData::startWorker's split (the bands write
// marked pixels and read unmarked ones: no two touch the same sample).
extern "C" int rsx_bad_pixels_host_fix_threads(const rsx_bad_pixels_desc* desc, const rsx_image* img,
                                               rsx_bad_pixels_result* result, int threads) {
  if (result)
    std::memset(result, 0, sizeof *result);
  if (int st = validate(desc, img))
    return st;
  if (!img->data)
    return RSX_ERR_INVALID_ARG;
  if (desc->n_positions == 0 && !desc->map_in)
    return RSX_OK;
  const Geo g = make_geo(uint32_t(img->dim_x), uint32_t(img->dim_y), img->pitch_bytes,
                         img->is_cfa != 0, desc->is_f32 != 0);
  std::vector<uint64_t> rowmap(size_t(g.wpr) * g.h, 0), colmap(size_t(g.wpc) * g.w, 0);
  if (desc->map_in)
    std::memcpy(rowmap.data(), desc->map_in, rowmap.size() * 8u);
  for (uint32_t i = 0; i < desc->n_positions; ++i) {
    const uint32_t x = desc->positions[i] & 0xFFFFu, y = desc->positions[i] >> 16;
    rowmap[size_t(y) * g.wpr + (x >> 6)] |= 1ull << (x & 63u);
  }
  uint64_t n_bad = 0, n_fixed = 0;
  for (uint32_t x = 0; x < g.w; ++x)
    for (uint32_t yw = 0; yw < g.wpc; ++yw) {
      const uint64_t c = column_word(g, rowmap.data(), x >> 6, x & 63u, yw);
      colmap[size_t(x) * g.wpc + yw] = c;
      n_bad += uint64_t(popc64(c));
    }
  uint8_t* data = static_cast<uint8_t*>(img->data);
  if (threads <= 1) {
    n_fixed = fix_rows(g, rowmap.data(), colmap.data(), data, 0, g.h);
  } else {
    const uint32_t per = (g.h + uint32_t(threads) - 1u) / uint32_t(threads);
    std::vector<uint64_t> counts(size_t(threads), 0);
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t) {
      const uint32_t y0 = std::min(uint32_t(t) * per, g.h), y1 = std::min((uint32_t(t) + 1u) * per, g.h);
      pool.emplace_back([&, t, y0, y1]() {
        counts[size_t(t)] = fix_rows(g, rowmap.data(), colmap.data(), data, y0, y1);
      });
    }
    for (std::thread& th : pool)
      th.join();
    for (uint64_t c : counts)
      n_fixed += c;
  }
  if (desc->map_out)
    std::memcpy(desc->map_out, rowmap.data(), rowmap.size() * 8u);
  if (result) {
    result->n_bad = n_bad;
    result->n_fixed = n_fixed;
    result->map_made = 1;
  }
  return RSX_OK;
}

extern "C" int rsx_bad_pixels_host_fix(const rsx_bad_pixels_desc* desc, const rsx_image* img,
                                       rsx_bad_pixels_result* result) {
  return rsx_bad_pixels_host_fix_threads(desc, img, result, 1);
}

#ifdef RSX_BAD_PIXELS_HOST_MAIN
namespace {

// fixBadPixelsThread and fixBadPixel restated: a byte map, one pixel at a time
struct Plain {
  int w, h, pitch, step;
  bool f32;
  uint32_t mp;
  std::vector<uint8_t> map;
  uint8_t* img;
  bool bad(int x, int y) const { return (map[size_t(mp) * y + (x >> 3)] >> (x & 7)) & 1; }
  uint16_t& u16(int x, int y) { return *reinterpret_cast<uint16_t*>(img + size_t(y) * pitch + 2 * x); }
  float& f(int x, int y) { return *reinterpret_cast<float*>(img + size_t(y) * pitch + 4 * x); }
  void fix_u(int x, int y) {
    int values[4] = {-1, -1, -1, -1}, dist[4] = {0, 0, 0, 0}, weight[4] = {0, 0, 0, 0};
    for (int q = x - step; q >= 0 && values[0] < 0; q -= step)
      if (!bad(q, y)) {
        values[0] = u16(q, y);
        dist[0] = x - q;
      }
    for (int q = x + step; q < w && values[1] < 0; q += step)
      if (!bad(q, y)) {
        values[1] = u16(q, y);
        dist[1] = q - x;
      }
    for (int q = y - step; q >= 0 && values[2] < 0; q -= step)
      if (!bad(x, q)) {
        values[2] = u16(x, q);
        dist[2] = y - q;
      }
    for (int q = y + step; q < h && values[3] < 0; q += step)
      if (!bad(x, q)) {
        values[3] = u16(x, q);
        dist[3] = q - y;
      }
    int shifts = 7;
    if (int t = dist[0] + dist[1]; t) {
      weight[0] = dist[0] ? (t - dist[0]) * 256 / t : 0;
      weight[1] = 256 - weight[0];
      ++shifts;
    }
    if (int t = dist[2] + dist[3]; t) {
      weight[2] = dist[2] ? (t - dist[2]) * 256 / t : 0;
      weight[3] = 256 - weight[2];
      ++shifts;
    }
    int total = 0;
    for (int i = 0; i < 4; ++i)
      if (values[i] >= 0)
        total += values[i] * weight[i];
    total >>= shifts;
    u16(x, y) = uint16_t(total > 65535 ? 65535 : total);
  }
  void fix_f(int x, int y) {
    float values[4] = {-1, -1, -1, -1}, dist[4] = {0, 0, 0, 0}, weight[4] = {0, 0, 0, 0};
    for (int q = x - step; q >= 0 && values[0] < 0; q -= step)
      if (!bad(q, y)) {
        values[0] = f(q, y);
        dist[0] = float(x - q);
      }
    for (int q = x + step; q < w && values[1] < 0; q += step)
      if (!bad(q, y)) {
        values[1] = f(q, y);
        dist[1] = float(q - x);
      }
    for (int q = y - step; q >= 0 && values[2] < 0; q -= step)
      if (!bad(x, q)) {
        values[2] = f(x, q);
        dist[2] = float(y - q);
      }
    for (int q = y + step; q < h && values[3] < 0; q += step)
      if (!bad(x, q)) {
        values[3] = f(x, q);
        dist[3] = float(q - y);
      }
    float div = 0.000001F;
    if (float t = dist[0] + dist[1]; t > 0) {
      weight[0] = dist[0] > 0.0F ? (t - dist[0]) / t : 0;
      weight[1] = 1.0F - weight[0];
      div += 1;
    }
    if (float t = dist[2] + dist[3]; t > 0) {
      weight[2] = dist[2] > 0.0F ? (t - dist[2]) / t : 0;
      weight[3] = 1.0F - weight[2];
      div += 1;
    }
    float total = 0;
    for (int i = 0; i < 4; ++i)
      if (values[i] >= 0)
        total += values[i] * weight[i];
    total /= div;
    if (total != total) {
      const uint32_t n = NAN_X86;
      std::memcpy(&f(x, y), &n, 4);
    } else {
      f(x, y) = total;
    }
  }
  void run() {
    const int gw = (w + 15) / 32;
    for (int y = 0; y < h; ++y)
      for (int b = 0; b < gw; ++b)
        for (int i = 0; i < 32; ++i)
          if ((map[size_t(mp) * y + 4 * b + i / 8] >> (i & 7)) & 1) {
            if (f32)
              fix_f(32 * b + i, y);
            else
              fix_u(32 * b + i, y);
          }
  }
};

uint32_t rng_state = 2463534242u;
uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

int fails = 0;
void expect(bool ok, const char* what, int id) {
  if (!ok) {
    std::fprintf(stderr, "FAILED: %s (case %d)\n", what, id);
    ++fails;
  }
}

// one case through the host functions and through the restatement
void run_case(int id, int w, int h, int pitch, bool cfa, bool f32, const std::vector<uint32_t>& pos,
              const std::vector<uint8_t>* map_in, std::vector<uint8_t> image,
              const std::vector<uint8_t>* want_img, const std::vector<uint8_t>* want_map) {
  const uint32_t mp = map_pitch(uint32_t(w));
  std::vector<uint8_t> mine = image, map_out(size_t(mp) * h, 0xAA);
  rsx_bad_pixels_desc d;
  std::memset(&d, 0, sizeof d);
  d.positions = pos.empty() ? nullptr : pos.data();
  d.n_positions = uint32_t(pos.size());
  d.map_pitch = mp;
  d.map_in = map_in ? map_in->data() : nullptr;
  d.map_out = map_out.data();
  d.is_f32 = f32;
  rsx_image img{mine.data(), uint32_t(pitch), w, h, 1, cfa ? 1 : 0};
  rsx_bad_pixels_result r;
  expect(rsx_bad_pixels_host_fix(&d, &img, &r) == RSX_OK, "status", id);
  Plain p{w, h, pitch, cfa ? 2 : 1, f32, mp, {}, image.data()};
  p.map.assign(size_t(mp) * h, 0);
  if (map_in)
    p.map = *map_in;
  for (uint32_t q : pos)
    p.map[size_t(mp) * (q >> 16) + ((q & 0xFFFFu) >> 3)] |= uint8_t(1u << (q & 7u));
  const bool made = !pos.empty() || map_in;
  if (made)
    p.run();
  expect(mine == image, "image against the restatement", id);
  expect(r.map_made == (made ? 1 : 0), "map_made", id);
  if (made)
    expect(map_out == p.map, "map against the restatement", id);
  if (want_img)
    expect(mine == *want_img, "image against the case file", id);
  if (want_map && made)
    expect(map_out == *want_map, "map against the case file", id);
}

bool rd(std::FILE* f, void* p, size_t n) { return std::fread(p, 1, n, f) == n; }

// the case file of tests/bad_pixels_files.py: uint32 count, then per case a 64-byte name, uint32 w,
// h, pitch, cfa, f32, n_pos, has_map; the positions; the map; the image; the expected image; the
// expected map
int run_file(const char* path) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f)
    return 2;
  uint32_t n = 0;
  if (!rd(f, &n, 4))
    return 2;
  for (uint32_t c = 0; c < n; ++c) {
    char name[64];
    uint32_t hd[7];
    if (!rd(f, name, sizeof name) || !rd(f, hd, sizeof hd))
      return 2;
    const uint32_t mp = map_pitch(hd[0]);
    std::vector<uint32_t> pos(hd[5]);
    std::vector<uint8_t> map(hd[6] ? size_t(mp) * hd[1] : 0), image(size_t(hd[2]) * hd[1]),
        want(image.size()), want_map(size_t(mp) * hd[1]);
    if ((hd[5] && !rd(f, pos.data(), 4u * hd[5])) || (hd[6] && !rd(f, map.data(), map.size())) ||
        !rd(f, image.data(), image.size()) || !rd(f, want.data(), want.size()) ||
        !rd(f, want_map.data(), want_map.size()))
      return 2;
    run_case(int(c), int(hd[0]), int(hd[1]), int(hd[2]), hd[3] != 0, hd[4] != 0, pos,
             hd[6] ? &map : nullptr, image, &want, &want_map);
  }
  std::fclose(f);
  std::printf("%u file cases\n", n);
  return 0;
}

} // namespace

int main(int argc, char** argv) {
  if (argc > 1)
    if (int e = run_file(argv[1]))
      return e;
  struct G { int w, h; };
  const G geos[] = {{16, 2}, {17, 3}, {33, 66}, {48, 5}, {95, 7}, {130, 130}, {1, 1}, {64, 64}, {129, 65}};
  int id = 1000;
  for (const G& g : geos)
    for (int cfa = 0; cfa < 2; ++cfa)
      for (int f32 = 0; f32 < 2; ++f32)
        for (int mode = 0; mode < 5; ++mode, ++id) {
          const int ss = f32 ? 4 : 2, pitch = g.w * ss + (mode & 1 ? 3 * ss : 0);
          std::vector<uint8_t> image(size_t(pitch) * g.h);
          for (int y = 0; y < g.h; ++y)
            for (int x = 0; x < pitch / ss; ++x) {
              if (f32) {
                const uint32_t k = rnd() % 16u;
                float v = k == 0 ? -float(rnd() % 1000u) : k == 1 ? -0.0F : float(rnd() % 60000u) / 7.0F;
                if (k == 2)
                  v = __builtin_nanf("");
                if (k == 3)
                  v = __builtin_inff();
                std::memcpy(&image[size_t(y) * pitch + 4 * x], &v, 4);
              } else {
                const uint16_t v = uint16_t(rnd() % 3u == 0 ? (rnd() & 1u ? 65535u : 0u) : rnd());
                std::memcpy(&image[size_t(y) * pitch + 2 * x], &v, 2);
              }
            }
          // density by mode: nothing, sparse, half, nearly all, all
          const uint32_t per1024[] = {0u, 20u, 512u, 1000u, 1024u};
          std::vector<uint32_t> pos;
          std::vector<uint8_t> map(size_t(map_pitch(uint32_t(g.w))) * g.h, 0);
          for (int y = 0; y < g.h; ++y)
            for (int x = 0; x < g.w; ++x)
              if (rnd() % 1024u < per1024[mode]) {
                if (rnd() & 1u)
                  pos.push_back(uint32_t(y) << 16 | uint32_t(x));
                else
                  map[size_t(map_pitch(uint32_t(g.w))) * y + (x >> 3)] |= uint8_t(1u << (x & 7));
              }
          if (!pos.empty())
            pos.push_back(pos[0]); // (a duplicate)
          run_case(id, g.w, g.h, pitch, cfa != 0, f32 != 0, pos, mode >= 2 ? &map : nullptr, image,
                   nullptr, nullptr);
        }
  // the verdicts
  {
    std::vector<uint16_t> px(40 * 4, 7);
    rsx_image img{px.data(), 80, 40, 4, 1, 1};
    rsx_bad_pixels_desc d;
    std::memset(&d, 0, sizeof d);
    const uint32_t out_x = 40u, out_y = 4u << 16;
    d.positions = &out_x;
    d.n_positions = 1;
    expect(rsx_bad_pixels_host_fix(&d, &img, nullptr) == RSX_ERR_INVALID_ARG, "x outside", 0);
    d.positions = &out_y;
    expect(rsx_bad_pixels_host_fix(&d, &img, nullptr) == RSX_ERR_INVALID_ARG, "y outside", 0);
    rsx_image three = img;
    three.cpp = 3;
    three.dim_x = 13;
    expect(rsx_bad_pixels_host_fix(&d, &three, nullptr) == RSX_ERR_UNSUPPORTED, "cpp 3", 0);
    std::vector<uint8_t> map(16 * 4, 0);
    map[5] = 1; // (x = 40)
    d.n_positions = 0;
    d.map_in = map.data();
    d.map_pitch = 16;
    expect(rsx_bad_pixels_host_fix(&d, &img, nullptr) == RSX_ERR_INVALID_ARG, "map bit outside", 0);
    d.map_pitch = 32;
    expect(rsx_bad_pixels_host_fix(&d, &img, nullptr) == RSX_ERR_INVALID_ARG, "map pitch", 0);
    for (uint16_t v : px)
      expect(v == 7, "untouched", 0);
  }
  if (fails)
    return 1;
  std::puts("rsx_bad_pixels_host_check OK");
  return 0;
}
#endif
