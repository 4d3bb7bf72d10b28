// rsx_kodak_core.h as host C++ (librsx_kodak_host.so): the validation and a decode that goes
// from segment to segment with the closed forms the kernels use -- the segment's size from the sum
// of its lengths, every field from the prefix sum in front of it -- instead of the reference's
// reader.  The tests hold it against the reference's recorded answers
// (tests/golden/kodak_ref.json) and the Python model, whose decoder is that reader, and the device
// against the same.  With -DRSX_KODAK_HOST_MAIN the file is a program (built with
// AddressSanitizer and UBSan where g++ has them) that decodes the streams of a case file, each
// from a heap copy of exactly its size.
#include "rsx_kodak_core.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace rsx_kodak;

namespace {

// One segment of `len` pixels at `in + at` into out[0 .. len); *at moves behind it.
int segment(const uint8_t* in, uint64_t in_bytes, uint64_t* at, uint32_t len,
            const rsx_kodak_desc* desc, uint16_t* out) {
  const uint64_t o = *at;
  if (o + len / 2u > in_bytes)
    return RSX_ERR_IO; // (inside the lengths)
  uint32_t sum = 0;
  for (uint32_t k = 0; k < len / 2u; ++k)
    sum += nibble_sum(in[o + k]);
  const uint32_t size = segment_bytes(len, sum);
  if (o + size > in_bytes)
    return RSX_ERR_IO; // (inside the up-front unit or a read of 4 bytes)
  const uint8_t* area = in + o + len / 2u;
  int32_t pred[2] = {0, 0};
  uint32_t cum = 0;
  for (uint32_t i = 0; i < len; ++i) {
    const uint32_t b = in[o + i / 2u];
    const uint32_t n = (i & 1u) ? b >> 4 : b & 15u;
    pred[i & 1u] += extend(field_at(area, cum, n), n);
    cum += n;
    if (out_of_range(pred[i & 1u], desc->bps))
      return RSX_ERR_VALUE_RANGE;
    out[i] = store_value(pred[i & 1u], desc->table_mode, desc->table);
  }
  *at = o + size;
  return RSX_OK;
}

} // namespace

extern "C" int rsx_kodak_host_validate(const rsx_kodak_desc* desc, const rsx_image* img,
                                       size_t in_bytes) {
  return validate(desc, img, in_bytes);
}

// The frame into the host image `img`; a failing call leaves the image as it was.  *consumed (may
// be NULL) = the bytes the segments took.
extern "C" int rsx_kodak_host_decode(const rsx_kodak_desc* desc, const uint8_t* in, size_t in_bytes,
                                     const rsx_image* img, uint64_t* consumed) {
  if (!in || !img || !img->data)
    return RSX_ERR_INVALID_ARG;
  if (int st = validate(desc, img, in_bytes))
    return st;
  const int32_t w = img->dim_x, h = img->dim_y;
  std::vector<uint16_t> tmp(size_t(w) * size_t(h));
  uint64_t at = 0;
  for (int32_t row = 0; row < h; ++row)
    for (int32_t col = 0; col < w; col += SEGMENT) {
      const uint32_t len = uint32_t(w - col < SEGMENT ? w - col : SEGMENT);
      if (int st = segment(in, in_bytes, &at, len, desc, tmp.data() + size_t(row) * w + col))
        return st;
    }
  for (int32_t r = 0; r < h; ++r)
    std::memcpy(static_cast<uint8_t*>(img->data) + size_t(r) * img->pitch_bytes,
                tmp.data() + size_t(r) * w, size_t(w) * 2u);
  if (consumed)
    *consumed = at;
  return RSX_OK;
}

// the closed forms, for the tests
extern "C" uint32_t rsx_kodak_host_segment_bytes(uint32_t len, uint32_t sum) {
  return segment_bytes(len, sum);
}
extern "C" uint64_t rsx_kodak_host_image_bound(int32_t dim_x, int32_t dim_y) {
  return image_bound(dim_x, dim_y);
}

#ifdef RSX_KODAK_HOST_MAIN
// rsx_kodak_host_check CASES: the file is "RSXK", a count, then per case its width, height, pitch,
// bps, table mode, table entries and stream length (u32 each), the table (u16 each) and the
// stream.  Prints per case "validate decode fnv" (a step not reached: -1; fnv: FNV-1a of the rows
// without padding, 0 where nothing was decoded).
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
  if (std::fread(magic, 1, 4, f) != 4 || std::memcmp(magic, "RSXK", 4) != 0 ||
      std::fread(&n, 4, 1, f) != 1) {
    std::fclose(f);
    return 2;
  }
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t hd[7];
    if (std::fread(hd, 4, 7, f) != 7 || hd[5] > (1u << 14) || hd[6] > (1u << 28)) {
      std::fclose(f);
      return 2;
    }
    const uint32_t entries = hd[5], len = hd[6];
    // (heap blocks of exactly the sizes: a read past one is AddressSanitizer's)
    uint16_t* table = static_cast<uint16_t*>(std::malloc(entries ? entries * 2u : 2u));
    uint8_t* bytes = static_cast<uint8_t*>(std::malloc(len ? len : 1));
    if ((entries && std::fread(table, 2, entries, f) != entries) ||
        (len && std::fread(bytes, 1, len, f) != len)) {
      std::fclose(f);
      return 2;
    }
    rsx_image img;
    std::memset(&img, 0, sizeof img);
    img.dim_x = int32_t(hd[0]);
    img.dim_y = int32_t(hd[1]);
    img.cpp = 1;
    img.pitch_bytes = hd[2];
    rsx_kodak_desc desc;
    desc.bps = int32_t(hd[3]);
    desc.table_mode = int32_t(hd[4]);
    desc.table = entries ? table : nullptr;
    int vst = validate(&desc, &img, len), dst = -1;
    uint64_t fnv = 0;
    if (vst == RSX_OK) {
      std::vector<uint8_t> px(size_t(img.pitch_bytes) * size_t(img.dim_y), 0xA5);
      img.data = px.data();
      dst = rsx_kodak_host_decode(&desc, bytes, len, &img, nullptr);
      if (dst == RSX_OK) {
        fnv = 0xcbf29ce484222325ull;
        for (int32_t r = 0; r < img.dim_y; ++r)
          for (uint32_t b = 0; b < uint32_t(img.dim_x) * 2u; ++b)
            fnv = (fnv ^ px[size_t(r) * img.pitch_bytes + b]) * 0x100000001b3ull;
      }
    }
    std::printf("%d %d %016llx\n", vst, dst, static_cast<unsigned long long>(fnv));
    std::free(bytes);
    std::free(table);
  }
  std::fclose(f);
  return 0;
}
#endif
