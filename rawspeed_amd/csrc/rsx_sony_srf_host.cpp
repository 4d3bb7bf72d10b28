// rsx_sony_srf_core.h as host C++ (librsx_sony_srf_host.so): the reference's loop restated on one
// thread (the 128-entry ring of ArwDecoder::SonyDecrypt), the same stream made the way the device
// makes it (chunks that start from a jump and grow by the doubling identity), and decodeSRF's
// widening.  The tests hold both against the Python model.  With -DRSX_SONY_SRF_HOST_MAIN the file
// is a program (built with AddressSanitizer and UBSan where g++ has them) that runs both over heap
// blocks of exactly their sizes and compares them.
#include "rsx_sony_srf_core.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace rsx_sony_srf;

extern "C" int rsx_sony_srf_host_validate(size_t in_bytes, const rsx_image* img) {
  return validate(in_bytes, img);
}

// SonyDecrypt (:524-560) as it stands: the ring, p & 127.  in == out is allowed.
extern "C" void rsx_sony_srf_host_decrypt(const uint8_t* in, uint8_t* out, uint64_t n_words,
                                          uint32_t key) {
  if (n_words == 0)
    return;
  uint32_t pad[128];
  table_from_key(key, pad, PAD);
  pad[127] = 0;
  uint32_t p = 127;
  for (uint64_t i = 0; i != n_words; ++i, ++p) {
    pad[p & 127u] = pad[(p + 1u) & 127u] ^ pad[(p + 1u + 64u) & 127u];
    uint32_t bv;
    std::memcpy(&bv, in + 4u * i, 4);
    bv ^= pad[p & 127u];
    std::memcpy(out + 4u * i, &bv, 4);
  }
}

// The words w[first .. first + count) of the stream the way a workgroup makes them: 127 by the
// jump, the rest by the doubling identity.  out has 127 + count entries; the stream words are
// out[127 ..] when first is the index of the chunk's first OUTPUT word (w[127 + i] belongs to i).
static void chunk_words(const uint32_t* table, uint64_t first, uint32_t count, uint32_t* s) {
  const Poly c = x_pow(first);
  for (int m = 0; m < PAD; ++m)
    s[m] = jump_word(c, table, m);
  const uint32_t total = uint32_t(PAD) + count;
  uint32_t known = PAD;
  while (known < total) {
    const int k = doubling_shift(known);
    uint32_t step = 63u << k;
    if (step > total - known)
      step = total - known;
    for (uint32_t t = known; t < known + step; ++t)
      s[t] = s[t - (127u << k)] ^ s[t - (63u << k)];
    known += step;
  }
}

// ... the same bytes as rsx_sony_srf_host_decrypt, chunk by chunk in any order (here: last first)
extern "C" void rsx_sony_srf_host_decrypt_chunked(const uint8_t* in, uint8_t* out,
                                                  uint64_t n_words, uint32_t key) {
  uint32_t table[TABLE];
  table_from_key(key, table, TABLE);
  std::vector<uint32_t> s(size_t(PAD) + CHUNK);
  const uint64_t n_chunks = (n_words + CHUNK - 1) / CHUNK;
  for (uint64_t c = n_chunks; c-- > 0;) {
    const uint64_t first = c * CHUNK;
    const uint32_t count = uint32_t(n_words - first < CHUNK ? n_words - first : CHUNK);
    chunk_words(table, first, count, s.data());
    for (uint32_t i = 0; i < count; ++i) {
      uint32_t bv;
      std::memcpy(&bv, in + 4u * (first + i), 4);
      bv ^= s[size_t(PAD) + i];
      std::memcpy(out + 4u * (first + i), &bv, 4);
    }
  }
}

// w[n .. n + 127) by the jump, for the tests
extern "C" void rsx_sony_srf_host_jump(uint32_t key, uint64_t n, uint32_t* out) {
  uint32_t table[TABLE];
  table_from_key(key, table, TABLE);
  const Poly c = x_pow(n);
  for (int m = 0; m < PAD; ++m)
    out[m] = jump_word(c, table, m);
}

// decodeSRF behind the key: decrypt 2 w h bytes, read them as 16-bit big-endian rows of pitch 2 w
extern "C" int rsx_sony_srf_host_decode(const uint8_t* in, size_t in_bytes, uint32_t key,
                                        const rsx_image* img) {
  if (!in || !img || !img->data)
    return RSX_ERR_INVALID_ARG;
  if (int st = validate(in_bytes, img))
    return st;
  const size_t w = size_t(img->dim_x), h = size_t(img->dim_y), len = 2 * w * h;
  std::vector<uint8_t> dec(len);
  rsx_sony_srf_host_decrypt(in, dec.data(), len / 4, key);
  for (size_t y = 0; y < h; ++y) {
    uint8_t* row = static_cast<uint8_t*>(img->data) + y * img->pitch_bytes;
    for (size_t x = 0; x < w; ++x) {
      const uint8_t* b = dec.data() + 2 * (y * w + x);
      const uint16_t v = uint16_t(b[0] << 8 | b[1]);
      std::memcpy(row + 2 * x, &v, 2);
    }
  }
  return RSX_OK;
}

#ifdef RSX_SONY_SRF_HOST_MAIN
// rsx_sony_srf_host_check: ring against chunks for sizes around the pad and the chunk, and one
// small image.  Prints one line per case and "ok" at the end; exit status 1 on a difference.
int main() {
  const uint64_t sizes[] = {1, 62, 63, 64, 126, 127, 128, 129, 254, 255, CHUNK - 1, CHUNK,
                            CHUNK + 1, 2 * CHUNK + 1, 4099, 100000};
  const uint32_t keys[] = {0u, 1u, 0xFFFFFFFFu, 0x9E3779B9u};
  int bad = 0;
  for (uint64_t n : sizes)
    for (uint32_t key : keys) {
      // (heap blocks of exactly the sizes: an access past one is AddressSanitizer's)
      uint8_t* in = static_cast<uint8_t*>(std::malloc(size_t(4 * n)));
      uint8_t* a = static_cast<uint8_t*>(std::malloc(size_t(4 * n)));
      uint8_t* b = static_cast<uint8_t*>(std::malloc(size_t(4 * n)));
      uint32_t lcg = key ^ uint32_t(n);
      for (uint64_t i = 0; i < 4 * n; ++i)
        in[i] = uint8_t((lcg = lcg * 1664525u + 1013904223u) >> 24);
      rsx_sony_srf_host_decrypt(in, a, n, key);
      rsx_sony_srf_host_decrypt_chunked(in, b, n, key);
      const bool same = std::memcmp(a, b, size_t(4 * n)) == 0;
      rsx_sony_srf_host_decrypt(a, a, n, key); // in place, and twice is the identity
      const bool back = std::memcmp(a, in, size_t(4 * n)) == 0;
      std::printf("%llu %08x %d %d\n", static_cast<unsigned long long>(n), key, int(same),
                  int(back));
      bad += !same || !back;
      std::free(in);
      std::free(a);
      std::free(b);
    }
  {
    rsx_image img;
    std::memset(&img, 0, sizeof img);
    img.dim_x = 63;
    img.dim_y = 2;
    img.cpp = 1;
    img.pitch_bytes = 128;
    std::vector<uint8_t> px(size_t(img.pitch_bytes) * 2, 0xA5), in(252, 0x5A);
    img.data = px.data();
    const int st = rsx_sony_srf_host_decode(in.data(), in.size(), 7u, &img);
    std::printf("decode %d %d\n", st, int(px[126] == 0xA5 && px[127] == 0xA5));
    bad += st != RSX_OK || px[126] != 0xA5;
  }
  std::printf(bad ? "FAILED\n" : "ok\n");
  return bad ? 1 : 0;
}
#endif
