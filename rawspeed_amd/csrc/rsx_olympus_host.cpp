// rsx_olympus_core.h as host C++ (librsx_olympus_host.so): the validation, the walk through the
// bits (the differences mod 2^16 into the image, as olympus_parse_kernel leaves them) and the
// reconstruction in place, plane by plane (as olympus_recon_kernel does it).  The tests hold it
// against the reference's recorded answers (tests/golden/olympus_ref.json) and the Python model,
// and the device against the same.  With -DRSX_OLYMPUS_HOST_MAIN the file is a program (built with
// AddressSanitizer and UBSan where g++ has them) that decodes the streams of a case file, each
// from a heap copy of exactly its size.
#include "rsx_olympus_core.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace rsx_olympus;

namespace {

struct MemSrc {
  const uint8_t* p;
  uint64_t size;
  uint32_t word(uint64_t k) const {
    uint32_t w = 0;
    for (uint32_t b = 0; b < 4; ++b) {
      const uint64_t at = 4ull * k + b;
      w = w << 8 | (at < size ? p[at] : 0u);
    }
    return w;
  }
};

inline uint16_t* row_ptr(uint8_t* data, uint32_t pitch, int32_t row) {
  return reinterpret_cast<uint16_t*>(data + size_t(row) * pitch);
}

// The walk: uint16(diff) of every pixel into the image; the reader's verdict.
int parse(const uint8_t* bits, uint64_t size, uint8_t* data, uint32_t pitch, int32_t w, int32_t h) {
  const MemSrc src{bits, size};
  Bits<MemSrc> B;
  B.init(&src, size);
  for (int32_t row = 0; row < h; ++row) {
    Carry s[2] = {{0, 0, 0}, {0, 0, 0}};
    uint16_t* out = row_ptr(data, pitch, row);
    for (int32_t col = 0; col < w; ++col) {
      if (!B.fill())
        return RSX_ERR_INPUT_OVERFLOW;
      int32_t diff;
      B.skip(symbol(s[col & 1], B.peek32(), &diff));
      out[col] = uint16_t(diff);
    }
  }
  return RSX_OK;
}

// Differences into pixels, in place: the four planes one after another.
void reconstruct(uint8_t* data, uint32_t pitch, int32_t w, int32_t h) {
  for (int32_t plane = 0; plane < 4; ++plane) {
    const int32_t pr = plane >> 1, pc = plane & 1;
    for (int32_t i = 0; i < h / 2; ++i) {
      uint16_t* cur = row_ptr(data, pitch, 2 * i + pr);
      const uint16_t* above = i ? row_ptr(data, pitch, 2 * i + pr - 2) : nullptr;
      for (int32_t j = 0; j < w / 2; ++j) {
        const int32_t x = 2 * j + pc;
        const int32_t left = j ? cur[x - 2] : 0, up = i ? above[x] : 0,
                      nw = (i && j) ? above[x - 2] : 0;
        cur[x] = uint16_t(pred(i, j, left, up, nw) + int32_t(cur[x]));
      }
    }
  }
}

} // namespace

extern "C" int rsx_olympus_host_validate(size_t in_bytes, const rsx_image* img) {
  return validate(in_bytes, img);
}

// The frame into the host image `img`; a failing call leaves the image as it was.
extern "C" int rsx_olympus_host_decode(const uint8_t* in, size_t in_bytes, const rsx_image* img) {
  if (!in || !img || !img->data)
    return RSX_ERR_INVALID_ARG;
  if (int st = validate(in_bytes, img))
    return st;
  const int32_t w = img->dim_x, h = img->dim_y;
  const uint32_t pitch = uint32_t(w) * 2u;
  std::vector<uint8_t> tmp(size_t(pitch) * size_t(h));
  if (int st = parse(in + SKIP, in_bytes - SKIP, tmp.data(), pitch, w, h))
    return st;
  reconstruct(tmp.data(), pitch, w, h);
  for (int32_t r = 0; r < h; ++r)
    std::memcpy(static_cast<uint8_t*>(img->data) + size_t(r) * img->pitch_bytes,
                tmp.data() + size_t(r) * pitch, pitch);
  return RSX_OK;
}

// fill_limit and the closed form of the over-read rule, for the tests
extern "C" uint64_t rsx_olympus_host_fill_limit(uint64_t size) { return fill_limit(size); }

#ifdef RSX_OLYMPUS_HOST_MAIN
// rsx_olympus_host_check CASES: the file is "RSXO", a count, then per case its width, height,
// pitch, stream length (u32 each) and the stream.  Prints per case "validate decode fnv" (a step
// not reached: -1; fnv: FNV-1a of the rows without padding, 0 where nothing was decoded).
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
  if (std::fread(magic, 1, 4, f) != 4 || std::memcmp(magic, "RSXO", 4) != 0 ||
      std::fread(&n, 4, 1, f) != 1) {
    std::fclose(f);
    return 2;
  }
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t hd[4];
    if (std::fread(hd, 4, 4, f) != 4 || hd[3] > (1u << 28)) {
      std::fclose(f);
      return 2;
    }
    const uint32_t len = hd[3];
    // (a heap block of exactly the stream's size: a read past it is AddressSanitizer's)
    uint8_t* bytes = static_cast<uint8_t*>(std::malloc(len ? len : 1));
    if (len && std::fread(bytes, 1, len, f) != len) {
      std::fclose(f);
      return 2;
    }
    rsx_image img;
    std::memset(&img, 0, sizeof img);
    img.dim_x = int32_t(hd[0]);
    img.dim_y = int32_t(hd[1]);
    img.cpp = 1;
    img.pitch_bytes = hd[2];
    int vst = validate(len, &img), dst = -1;
    uint64_t fnv = 0;
    if (vst == RSX_OK) {
      std::vector<uint8_t> px(size_t(img.pitch_bytes) * size_t(img.dim_y), 0xA5);
      img.data = px.data();
      dst = rsx_olympus_host_decode(bytes, len, &img);
      if (dst == RSX_OK) {
        fnv = 0xcbf29ce484222325ull;
        for (int32_t r = 0; r < img.dim_y; ++r)
          for (uint32_t b = 0; b < uint32_t(img.dim_x) * 2u; ++b)
            fnv = (fnv ^ px[size_t(r) * img.pitch_bytes + b]) * 0x100000001b3ull;
      }
    }
    std::printf("%d %d %016llx\n", vst, dst, static_cast<unsigned long long>(fnv));
    std::free(bytes);
  }
  std::fclose(f);
  return 0;
}
#endif
