// rsx_fuji_core.h as host C++ (librsx_fuji_host.so): the container parse, the validation and the
// strip decode of rsx_fuji.hip with one "lane" -- per pass the records of both lines, then the
// chain over them, the helper columns, and per line the copy-out and the rotation.  The tests hold
// it against the reference's recorded answers (tests/golden/fuji_ref.json) and the Python model,
// and the device against the same.  The strips of a frame run on `threads` threads.  With
// -DRSX_FUJI_HOST_MAIN the file is a program (built with AddressSanitizer and UBSan where g++ has
// them) that decodes the containers of a case file, each from a heap copy of exactly its size.
#include "rsx_fuji_core.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

using namespace rsx_fuji;

namespace {

struct MemSrc {
  const uint8_t* p;
  uint32_t size;
  uint32_t word(uint32_t k) const {
    uint32_t w = 0;
    for (uint32_t b = 0; b < 4; ++b) {
      const uint64_t at = 4ull * k + b;
      w = w << 8 | (at < size ? p[at] : 0u);
    }
    return w;
  }
};

// One strip into the image rows at `out` (the strip's first pixel), `width` columns of it.
int decode_strip(const Params& P, const uint8_t* bytes, uint32_t size, int32_t total_lines,
                 int32_t width, uint8_t* out, uint32_t pitch) {
  if (size < 4)
    return RSX_ERR_IO;
  const MemSrc src{bytes, size};
  Bits<MemSrc> B;
  B.init(&src, size);
  std::vector<uint16_t> lines(size_t(LTOTAL) * STRIDE, 0);
  std::vector<int32_t> ge(TABLE_INTS), go(TABLE_INTS);
  for (int32_t i = 0; i < TABLE_INTS; i += 2) {
    ge[i] = go[i] = P.max_diff;
    ge[i + 1] = go[i + 1] = 1;
  }
  std::vector<uint32_t> ev(MAX_LW), od(2 * MAX_LW);
  const int32_t half = P.lw / 2;
  uint16_t* L = lines.data();
  for (int32_t line = 0; line < total_lines; ++line) {
    for (int32_t row = 0; row < 6; ++row) {
      int32_t c[2];
      pass_lines(row, &c[0], &c[1]);
      for (int32_t comp = 0; comp < 2; ++comp)
        for (int32_t col = 0; col < half; ++col) {
          const bool no_bits = P.xtrans && xtrans_no_bits(row, col, comp);
          const uint32_t rec =
              even_record(L + (c[comp] - 1) * STRIDE, L + (c[comp] - 2) * STRIDE, col, no_bits);
          ev[comp * (MAX_LW / 2) + col] = rec;
          if (no_bits)
            L[c[comp] * STRIDE + 1 + 2 * col] = uint16_t(rec & 0xFFFFu);
          odd_record(L + (c[comp] - 1) * STRIDE, col, &od[(comp * (MAX_LW / 2) + col) * 2],
                     &od[(comp * (MAX_LW / 2) + col) * 2 + 1]);
        }
      const int32_t t = (row % 3) * GRADS * 2;
      if (int st = walk(B, P, L + c[0] * STRIDE, L + c[1] * STRIDE, 0, half + 4, ev.data(),
                        od.data(), ge.data() + t, go.data() + t))
        return st;
      for (int32_t comp = 0; comp < 2; ++comp) {
        const int32_t k = c[comp] < G0 ? 0 : c[comp] < B0 ? 1 : 2;
        for (int32_t i = colour_first(k) + 2; i < colour_first(k) + colour_count(k); ++i)
          extend_one(L, i, P.lw);
      }
    }
    for (int32_t r = 0; r < 6; ++r) {
      uint16_t* dst = reinterpret_cast<uint16_t*>(out + size_t(6 * line + r) * pitch);
      for (int32_t x = 0; x < width; ++x)
        dst[x] = L[out_index(P.xtrans != 0, r, x)];
    }
    if (line + 1 == total_lines)
      break;
    for (int32_t k = 0; k < 3; ++k) {
      const int32_t a = colour_first(k), b = colour_count(k);
      std::memcpy(L + a * STRIDE, L + (a + b - 2) * STRIDE, 2 * STRIDE * sizeof(uint16_t));
      L[(a + 2) * STRIDE + P.lw + 1] = L[(a + 1) * STRIDE + P.lw];
    }
  }
  return RSX_OK;
}

} // namespace

extern "C" int rsx_fuji_host_parse(const uint8_t* in, size_t in_bytes, rsx_fuji_desc* desc) {
  return parse(in, in_bytes, desc);
}

extern "C" int rsx_fuji_host_validate(const rsx_fuji_desc* desc, const rsx_image* img) {
  return validate(desc, img);
}

// The frame into the host image `img`; strip_status (may be NULL) gets a status per strip.  The
// status of the lowest-numbered failing strip; the strips that decode are written either way.
extern "C" int rsx_fuji_host_decode(const rsx_fuji_desc* desc, const uint8_t* in, size_t in_bytes,
                                    const rsx_image* img, int32_t* strip_status, int threads) {
  if (!in || !img || !img->data)
    return RSX_ERR_INVALID_ARG;
  if (int st = validate(desc, img))
    return st;
  if (int st = check_strips(*desc, in_bytes))
    return st;
  Params P;
  params_init(&P, desc->raw_type, desc->raw_bits);
  const int32_t n = desc->n_strips;
  std::vector<int32_t> st(size_t(n), RSX_OK);
  auto one = [&](int32_t s) {
    st[size_t(s)] = decode_strip(P, in + desc->strip_offset[s], desc->strip_bytes[s],
                                 desc->total_lines, strip_width(desc->raw_width, s),
                                 static_cast<uint8_t*>(img->data) + size_t(s) * BLOCK * 2,
                                 img->pitch_bytes);
  };
  if (threads <= 1) {
    for (int32_t s = 0; s < n; ++s)
      one(s);
  } else {
    std::vector<std::thread> pool;
    for (int32_t t = 0; t < threads && t < n; ++t)
      pool.emplace_back([&, t]() {
        for (int32_t s = t; s < n; s += threads)
          one(s);
      });
    for (std::thread& t : pool)
      t.join();
  }
  int rc = RSX_OK;
  for (int32_t s = n - 1; s >= 0; --s) {
    if (strip_status)
      strip_status[s] = st[size_t(s)];
    if (st[size_t(s)] != RSX_OK)
      rc = st[size_t(s)];
  }
  return rc;
}

#ifdef RSX_FUJI_HOST_MAIN
// rsx_fuji_host_check CASES: the file is "RSXF", a count, then per case its length and its
// container bytes.  Prints per case "parse validate decode s0 s1 ..." (a step not reached: -1).
int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s CASES\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f)
    return 2;
  char magic[4];
  uint32_t n = 0;
  if (std::fread(magic, 1, 4, f) != 4 || std::memcmp(magic, "RSXF", 4) != 0 ||
      std::fread(&n, 4, 1, f) != 1) {
    std::fclose(f);
    return 2;
  }
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t len = 0;
    if (std::fread(&len, 4, 1, f) != 1 || len > (1u << 26)) {
      std::fclose(f);
      return 2;
    }
    // (a heap block of exactly the container's size: a read past it is AddressSanitizer's)
    uint8_t* bytes = static_cast<uint8_t*>(std::malloc(len ? len : 1));
    if (len && std::fread(bytes, 1, len, f) != len) {
      std::fclose(f);
      return 2;
    }
    rsx_fuji_desc d;
    int pst = parse(bytes, len, &d), vst = -1, dst = -1;
    std::vector<int32_t> ss;
    if (pst == RSX_OK) {
      rsx_image img;
      std::memset(&img, 0, sizeof img);
      img.dim_x = d.raw_width;
      img.dim_y = d.raw_height;
      img.cpp = 1;
      img.pitch_bytes = uint32_t(d.raw_width > 0 ? d.raw_width : 0) * 2u + 6u;
      vst = validate(&d, &img);
      if (vst == RSX_OK) {
        std::vector<uint8_t> px(size_t(img.pitch_bytes) * size_t(img.dim_y));
        img.data = px.data();
        ss.assign(size_t(d.n_strips), -1);
        dst = rsx_fuji_host_decode(&d, bytes, len, &img, ss.data(), 1);
      }
    }
    std::printf("%d %d %d", pst, vst, dst);
    for (int32_t s : ss)
      std::printf(" %d", s);
    std::printf("\n");
    std::free(bytes);
  }
  std::fclose(f);
  return 0;
}
#endif
