// rsx_jpeg_core.h as host C++: the lossy-JPEG tile decode of rsx_dng_jpeg.hip with one "lane" --
// the same header parse, segment table, bit walk, transform and pixel arithmetic, segment after
// segment and block after block.  The tests hold it against libjpeg-turbo's recorded images
// (tests/golden/dng_jpeg_ref.json) and the device against the same.  With -DRSX_JPEG_HOST_MAIN
// the file is a program (built with AddressSanitizer and UBSan) that decodes a corpus file and
// seeded corruptions of its streams.
#include "rsx_jpeg_core.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace rsx_jpeg;

namespace {

struct MemSrc {
  const uint8_t* p;
  uint8_t at(uint32_t i) const { return p[i]; }
};

} // namespace

extern "C" int rsx_jpeg_host_validate(const rsx_dng_jpeg_tile* tile, const rsx_image* img,
                                      rsx_dng_jpeg_info* info) {
  return validate_call(tile, img, info);
}

// The tile into the host image `img` (data = row 0): the status of the device's run.
extern "C" int rsx_jpeg_host_decode(const rsx_dng_jpeg_tile* tile, const rsx_image* img) {
  if (!tile || !img || !img->data)
    return RSX_ERR_INVALID_ARG;
  Header H;
  if (int st = validate_tile(tile->in, tile->in_bytes, tile->off_x, tile->off_y, *img, &H))
    return st;
  std::vector<Segment> segs;
  if (int st = scan_segments(tile->in, tile->in_bytes, H,
                             [&](uint32_t, uint32_t first, uint32_t n, uint32_t a, uint32_t b) {
                               segs.push_back(Segment{0, first, n, a, b});
                             }))
    return st;
  std::vector<Tables> tables(1);
  fill_tables(H, &tables[0]);
  Tile T;
  const uint64_t plane_bytes = fill_tile(H, tile->off_x, tile->off_y, *img, 0, &T);
  std::vector<uint8_t> planes(plane_bytes);
  const MemSrc src{tile->in};
  uint8_t order[64];
  for (uint32_t k = 0; k < 64; ++k)
    order[k] = uint8_t(natural_order(k));
  int verdict = RSX_OK;
  for (const Segment& S : segs) {
    Bits<MemSrc> B;
    B.init(&src, S.start, S.end);
    int32_t pred[3] = {0, 0, 0};
    const uint32_t per_mcu = T.ncomp == 1 ? 1u : uint32_t(T.hs) * T.vs + 2u;
    int st = RSX_OK;
    for (uint64_t b = 0; b < uint64_t(S.n_mcus) * per_mcu && st == RSX_OK; ++b) {
      uint32_t comp;
      uint64_t at;
      block_place(T, S, uint32_t(b), &comp, &at);
      int16_t coef[64] = {0};
      int32_t ws[64];
      st = decode_block(B, tables[0].dc[comp], tables[0].ac[comp], order, &pred[comp], coef);
      if (st != RSX_OK)
        break;
      for (uint32_t c = 0; c < 8; ++c)
        if (!idct_column(coef, tables[0].q[comp], c, ws))
          st = RSX_ERR_UNSUPPORTED;
      for (uint32_t r = 0; r < 8; ++r)
        idct_row(ws, r, &planes[at + uint64_t(r) * T.plane_w[comp]]);
    }
    if (st > verdict)
      verdict = st;
  }
  if (verdict != RSX_OK)
    return verdict;
  uint8_t* const base = static_cast<uint8_t*>(img->data);
  for (uint32_t y = 0; y < T.copy_h; ++y) {
    uint16_t* row = reinterpret_cast<uint16_t*>(base + uint64_t(T.off_y + y) * T.pitch) +
                    uint64_t(T.off_x) * T.ncomp;
    for (uint32_t x = 0; x < T.copy_w; ++x) {
      uint32_t px[3];
      pixel_at(planes.data(), T, x, y, px);
      for (uint32_t c = 0; c < T.ncomp; ++c)
        row[uint64_t(x) * T.ncomp + c] = uint16_t(px[c]);
    }
  }
  return RSX_OK;
}

#ifdef RSX_JPEG_HOST_MAIN
// rsx_jpeg_host_check CORPUS N_RANDOM: the corpus is "RSXJ", a count, then per stream its length
// and its bytes.  Every stream is decoded as it is (into an image that cuts its right and bottom
// edge), then N_RANDOM seeded corruptions of the streams: byte changes, truncations, insertions.
// Prints the counts; the exit status is 0 unless the corpus is unreadable.
namespace {

uint32_t g_state = 12345u;
uint32_t rnd() {
  g_state = g_state * 1664525u + 1013904223u;
  return g_state >> 8;
}

int run_one(const std::vector<uint8_t>& s, uint32_t off_x, uint32_t off_y) {
  // (a heap copy of exactly the stream's size: a read past it is AddressSanitizer's)
  std::vector<uint8_t> bytes(s);
  rsx_dng_jpeg_tile t;
  t.in = bytes.data();
  t.in_bytes = bytes.size();
  t.off_x = off_x;
  t.off_y = off_y;
  int best = RSX_ERR_INVALID_ARG;
  for (int cpp = 1; cpp <= 3; cpp += 2) {
    rsx_image img;
    std::memset(&img, 0, sizeof img);
    img.dim_x = 37;
    img.dim_y = 29;
    img.cpp = cpp;
    img.pitch_bytes = uint32_t(img.dim_x * cpp * 2 + 6);
    std::vector<uint8_t> px(size_t(img.pitch_bytes) * size_t(img.dim_y));
    img.data = px.data();
    if (!bytes.empty()) {
      const int st = rsx_jpeg_host_decode(&t, &img);
      if (st != RSX_ERR_INVALID_ARG)
        best = st;
    }
  }
  return best;
}

} // namespace

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s CORPUS N_RANDOM\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f)
    return 2;
  std::vector<std::vector<uint8_t>> corpus;
  char magic[4];
  uint32_t n = 0;
  if (std::fread(magic, 1, 4, f) != 4 || std::memcmp(magic, "RSXJ", 4) != 0 || std::fread(&n, 4, 1, f) != 1) {
    std::fclose(f);
    return 2;
  }
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t len = 0;
    if (std::fread(&len, 4, 1, f) != 1 || len > (1u << 24)) {
      std::fclose(f);
      return 2;
    }
    std::vector<uint8_t> s(len);
    if (len && std::fread(s.data(), 1, len, f) != len) {
      std::fclose(f);
      return 2;
    }
    corpus.push_back(std::move(s));
  }
  std::fclose(f);
  if (corpus.empty())
    return 2;
  int ok = 0, refused = 0;
  for (const auto& s : corpus)
    (run_one(s, 0, 0) == RSX_OK ? ok : refused)++;
  const int n_random = std::atoi(argv[2]);
  int r_ok = 0, r_refused = 0;
  for (int i = 0; i < n_random; ++i) {
    std::vector<uint8_t> s = corpus[rnd() % corpus.size()];
    const uint32_t kind = rnd() % 8u;
    if (kind == 0 && !s.empty()) {
      s.resize(rnd() % s.size());
    } else if (kind == 1 && !s.empty()) {
      const size_t at = rnd() % s.size();
      s.insert(s.begin() + long(at), uint8_t(0xFF));
    } else if (kind == 2 && s.size() > 2) {
      const size_t at = rnd() % (s.size() - 1);
      s.erase(s.begin() + long(at));
    } else {
      const uint32_t changes = 1u + rnd() % 3u;
      for (uint32_t c = 0; c < changes && !s.empty(); ++c)
        s[rnd() % s.size()] = uint8_t(rnd());
    }
    (run_one(s, rnd() % 37u, rnd() % 29u) == RSX_OK ? r_ok : r_refused)++;
  }
  std::printf("corpus: %d decoded, %d refused; corruptions: %d decoded, %d refused\n", ok, refused,
              r_ok, r_refused);
  return 0;
}
#endif
