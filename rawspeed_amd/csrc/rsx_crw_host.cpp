// rsx_crw_core.h as host C++ (librsx_crw_host.so): the validation and a decode that un-stuffs the
// scan up to its first marker and then goes from symbol to symbol with the closed forms the
// kernels use -- a symbol from the next 32 bits, the reader's overflow as a threshold on the bit
// a symbol starts at -- instead of the reference's reader.  The tests hold it against the
// reference's recorded answers (tests/golden/crw_ref.json) and the Python model, whose decoder is
// that reader, and the device against the same.  With -DRSX_CRW_HOST_MAIN the file is a program
// (built with AddressSanitizer and UBSan where g++ has them) that decodes the streams of a case
// file, each from a heap copy of exactly its size.
#include "rsx_crw_core.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace rsx_crw;

namespace {

// the next 32 bits at bit `c` of the un-stuffed scan (zeros behind it)
inline uint32_t peek32(const std::vector<uint8_t>& data, uint64_t c) {
  const uint64_t b = c >> 3;
  uint64_t v = 0;
  for (int k = 0; k < 5; ++k)
    v = v << 8 | data[b + k];
  return uint32_t(v >> (8u - (c & 7u)));
}

} // namespace

extern "C" int rsx_crw_host_validate(const rsx_crw_desc* desc, const rsx_image* img,
                                     size_t in_bytes, size_t low_bytes) {
  return validate(desc, img, in_bytes, low_bytes);
}

// The frame into the host image `img`; a failing call leaves the image as it was.
extern "C" int rsx_crw_host_decode(const rsx_crw_desc* desc, const uint8_t* in, size_t in_bytes,
                                   const uint8_t* low, size_t low_bytes, const rsx_image* img) {
  if (!in || !img || !img->data || (desc && desc->has_lowbits && !low))
    return RSX_ERR_INVALID_ARG;
  if (int st = validate(desc, img, in_bytes, low_bytes))
    return st;
  const int32_t w = img->dim_x, h = img->dim_y;
  const uint32_t n_blocks = uint32_t(w) * uint32_t(h) / 64u;
  const uint64_t size64 = in_bytes < image_bound(w, h) ? in_bytes : image_bound(w, h);
  const uint32_t size = uint32_t(size64);
  // the data bytes in front of the first marker, then zeros
  std::vector<uint8_t> data;
  data.reserve(size_t(size) + 64);
  bool marker = false;
  for (uint32_t j = 0; j < size; ++j) {
    if (in[j] == 0xFF && j + 1 < size && in[j + 1] != 0) {
      marker = true;
      break;
    }
    if (in[j] == 0 && j > 0 && in[j - 1] == 0xFF)
      continue;
    data.push_back(in[j]);
  }
  const uint32_t n_data = uint32_t(data.size());
  data.resize(size_t(n_data) + 64, 0);
  const uint32_t limit =
      marker ? NO_THRESHOLD : overflow_threshold(size, n_data, in[size - 1] == 0xFF);
  const int64_t fill_at = marker ? marker_fill_threshold(n_data) : 0;
  bool met = false;
  uint32_t marker_limit = NO_THRESHOLD;

  Tables tables;
  build_tables(desc->dec_table, &tables);
  std::vector<uint16_t> tmp(size_t(w) * size_t(h));
  uint64_t c = 0;
  int32_t carry = 0, base[2] = {512, 512};
  uint32_t p = 0; // the frame's pixel in row-major order
  for (uint32_t b = 0; b < n_blocks; ++b) {
    int32_t diff[64] = {0};
    int32_t i = 0;
    do {
      if (marker && !met && int64_t(c) > fill_at) {
        met = true;
        marker_limit = marker_overflow_threshold(uint32_t(c));
      }
      if (c > limit || c > marker_limit)
        return RSX_ERR_INPUT_OVERFLOW;
      const Symbol s = symbol(&tables, peek32(data, c), i);
      if (s.used == 0)
        return RSX_ERR_BAD_HUFFMAN_CODE;
      c += s.used;
      if (s.at >= 0)
        diff[s.at] = s.diff;
      i = s.next;
    } while (i != 0);
    carry += diff[0];
    diff[0] = carry;
    for (uint32_t k = 0; k < 64; ++k, ++p) {
      if (p % uint32_t(w) == 0)
        base[0] = base[1] = 512;
      base[k & 1] += diff[k];
      if (out_of_range(base[k & 1]))
        return RSX_ERR_VALUE_RANGE;
      tmp[p] = uint16_t(base[k & 1]);
    }
  }
  if (desc->has_lowbits)
    for (uint32_t q = 0; q < uint32_t(w) * uint32_t(h); ++q)
      tmp[q] = merge_low(tmp[q], low[q / 4u], q & 3u, w);
  for (int32_t r = 0; r < h; ++r)
    std::memcpy(static_cast<uint8_t*>(img->data) + size_t(r) * img->pitch_bytes,
                tmp.data() + size_t(r) * w, size_t(w) * 2u);
  return RSX_OK;
}

#ifdef RSX_CRW_HOST_MAIN
// rsx_crw_host_check CASES: the file is "RSXC", a count, then per case its width, height, pitch,
// table number, low-bit flag, low-bit length and stream length (u32 each), the low bits and the
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
  if (std::fread(magic, 1, 4, f) != 4 || std::memcmp(magic, "RSXC", 4) != 0 ||
      std::fread(&n, 4, 1, f) != 1) {
    std::fclose(f);
    return 2;
  }
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t hd[7];
    if (std::fread(hd, 4, 7, f) != 7 || hd[5] > (1u << 28) || hd[6] > (1u << 28)) {
      std::fclose(f);
      return 2;
    }
    const uint32_t low_len = hd[5], len = hd[6];
    // (heap blocks of exactly the sizes: a read past one is AddressSanitizer's)
    uint8_t* low = static_cast<uint8_t*>(std::malloc(low_len ? low_len : 1));
    uint8_t* bytes = static_cast<uint8_t*>(std::malloc(len ? len : 1));
    if ((low_len && std::fread(low, 1, low_len, f) != low_len) ||
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
    rsx_crw_desc desc;
    desc.dec_table = hd[3];
    desc.has_lowbits = hd[4];
    int vst = validate(&desc, &img, len, low_len), dst = -1;
    uint64_t fnv = 0;
    if (vst == RSX_OK) {
      std::vector<uint8_t> px(size_t(img.pitch_bytes) * size_t(img.dim_y), 0xA5);
      img.data = px.data();
      dst = rsx_crw_host_decode(&desc, bytes, len, low, low_len, &img);
      if (dst == RSX_OK) {
        fnv = 0xcbf29ce484222325ull;
        for (int32_t r = 0; r < img.dim_y; ++r)
          for (uint32_t b = 0; b < uint32_t(img.dim_x) * 2u; ++b)
            fnv = (fnv ^ px[size_t(r) * img.pitch_bytes + b]) * 0x100000001b3ull;
      }
    }
    std::printf("%d %d %016llx\n", vst, dst, static_cast<unsigned long long>(fnv));
    std::free(bytes);
    std::free(low);
  }
  std::fclose(f);
  return 0;
}
#endif
