// rsx_image_hash_core.h as host C++ (librsx_image_hash_host.so): the image hash with its rows on
// one or more threads (a row the way a lane of the device takes it, the digests through the
// streaming hasher), a plain md5(bytes), the checks and the two tables.  The tests hold them against
// hashlib and numpy; the benchmark uses the image hash as its host yardstick.  With
// -DRSX_IMAGE_HASH_HOST_MAIN the file is a program (built with AddressSanitizer and UBSan where g++
// has them) that runs RFC 1321's test suite, every length around the padding edge in every
// alignment and in pieces, and images over heap blocks of exactly their sizes.
#include "rsx_image_hash_core.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

using namespace rsx_imghash;

extern "C" int rsx_image_hash_host_validate(const rsx_image* img, int32_t sample_bytes) {
  return validate(img, sample_bytes);
}

extern "C" void rsx_image_hash_host_md5(const uint8_t* data, size_t n, uint8_t out[16]) {
  Md5 m;
  m.update(data, n);
  m.final(out);
}

// ... the same message handed over in pieces of `piece` bytes (>= 1)
extern "C" void rsx_image_hash_host_md5_pieces(const uint8_t* data, size_t n, size_t piece,
                                               uint8_t out[16]) {
  Md5 m;
  for (size_t at = 0; at < n; at += piece)
    m.update(data + at, n - at < piece ? n - at : piece);
  m.final(out);
}

extern "C" void rsx_image_hash_host_tables(uint32_t sines[64], int32_t shifts[64],
                                           int32_t words[64]) {
  for (int i = 0; i < 64; ++i) {
    sines[i] = sine_constant(i);
    shifts[i] = step_shift(i);
    words[i] = step_word(i);
  }
}

// Section 4g on the host.  line_md5 (16 dim_y bytes) may be NULL; n_threads < 1 counts as 1.  The
// rows are split into n_threads runs of consecutive rows; the sums are exact integers, so the
// split changes nothing.
extern "C" int rsx_image_hash_host(const rsx_image* img, int32_t sample_bytes, uint8_t* line_md5,
                                   rsx_image_hash_result* out, int n_threads) {
  if (!img || !img->data || !out)
    return RSX_ERR_INVALID_ARG;
  if (int st = validate(img, sample_bytes))
    return st;
  const uint32_t row_bytes = uint32_t(img->dim_x) * uint32_t(img->cpp) * uint32_t(sample_bytes);
  const size_t h = size_t(img->dim_y);
  std::vector<uint8_t> own;
  if (!line_md5) {
    own.resize(16 * h);
    line_md5 = own.data();
  }
  const size_t nt = n_threads < 1 ? 1 : size_t(n_threads) > h ? h : size_t(n_threads);
  std::vector<uint64_t> bytes(nt, 0), halves(nt, 0);
  auto rows = [&](size_t t) {
    for (size_t y = h * t / nt; y < h * (t + 1) / nt; ++y) {
      uint32_t s[4];
      uint64_t b, v;
      hash_row(static_cast<const uint8_t*>(img->data) + y * img->pitch_bytes, row_bytes, s, &b, &v);
      store_digest(s, line_md5 + 16 * y);
      bytes[t] += b;
      halves[t] += v;
    }
  };
  if (nt == 1) {
    rows(0);
  } else {
    std::vector<std::thread> pool;
    for (size_t t = 0; t < nt; ++t)
      pool.emplace_back(rows, t);
    for (std::thread& t : pool)
      t.join();
  }
  Md5 m;
  m.update(line_md5, 16 * h);
  m.final(out->md5);
  out->byte_sum = out->sample_sum = 0;
  for (size_t t = 0; t < nt; ++t) {
    out->byte_sum += bytes[t];
    out->sample_sum += sample_bytes == 2 ? halves[t] : 0;
  }
  return RSX_OK;
}

#ifdef RSX_IMAGE_HASH_HOST_MAIN
// rsx_image_hash_host_check: prints one line per group and "ok" at the end; exit status 1 on a
// difference.
static bool digest_is(const uint8_t d[16], const char* hex) {
  char text[33];
  for (int i = 0; i < 16; ++i)
    std::snprintf(text + 2 * i, 3, "%02x", d[i]);
  return std::strcmp(text, hex) == 0;
}

int main() {
  int bad = 0;
  // RFC 1321, A.5
  const char* suite[][2] = {
      {"", "d41d8cd98f00b204e9800998ecf8427e"},
      {"a", "0cc175b9c0f1b6a831c399e269772661"},
      {"abc", "900150983cd24fb0d6963f7d28e17f72"},
      {"message digest", "f96b697d7cb7938d525a2f31aaf161d0"},
      {"abcdefghijklmnopqrstuvwxyz", "c3fcd3d76192e4007dfb496cca67e13b"},
      {"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789",
       "d174ab98d277d9f5a5611c2c9f419d9f"},
      {"1234567890123456789012345678901234567890123456789012345678901234567890123456789"
       "0",
       "57edf4a22be3c955ac49da2e2107b67a"}};
  int suite_ok = 0;
  for (auto& c : suite) {
    uint8_t d[16];
    rsx_image_hash_host_md5(reinterpret_cast<const uint8_t*>(c[0]), std::strlen(c[0]), d);
    suite_ok += digest_is(d, c[1]);
  }
  std::printf("suite %d\n", suite_ok);
  bad += suite_ok != 7;
  // every length 0 .. 200 at every alignment 0 .. 3 of a heap block of exactly its size (an
  // access past one is AddressSanitizer's): whole, in pieces of 1, 7 and 64 bytes, and as a row
  int same = 0, cases = 0;
  for (size_t n = 0; n <= 200; ++n)
    for (size_t a = 0; a < 4; ++a) {
      uint8_t* block = static_cast<uint8_t*>(std::malloc(n + a + 1));
      uint8_t* p = block + a;
      uint32_t lcg = uint32_t(n * 4 + a);
      for (size_t i = 0; i < n; ++i)
        p[i] = uint8_t((lcg = lcg * 1664525u + 1013904223u) >> 24);
      uint8_t whole[16], d[16];
      rsx_image_hash_host_md5(p, n, whole);
      bool ok = true;
      for (size_t piece : {size_t(1), size_t(7), size_t(64)}) {
        rsx_image_hash_host_md5_pieces(p, n, piece, d);
        ok = ok && std::memcmp(d, whole, 16) == 0;
      }
      uint32_t s[4];
      uint64_t b = 0, v = 0, want_b = 0;
      hash_row(p, uint32_t(n), s, &b, &v);
      store_digest(s, d);
      for (size_t i = 0; i < n; ++i)
        want_b += p[i];
      ok = ok && std::memcmp(d, whole, 16) == 0 && b == want_b;
      same += ok;
      ++cases;
      std::free(block);
    }
  std::printf("lengths %d %d\n", cases, same);
  bad += same != cases;
  // images: tight and padded pitch, 1 and 3 threads, the padding rewritten in between
  int images = 0, images_ok = 0;
  for (int32_t sb : {2, 4})
    for (int32_t w : {1, 27, 28, 32, 95})
      for (uint32_t pad : {0u, 4u, 16u}) {
        rsx_image img;
        std::memset(&img, 0, sizeof img);
        img.dim_x = w;
        img.dim_y = 7;
        img.cpp = sb == 2 ? 3 : 1;
        const uint32_t row_bytes = uint32_t(w * img.cpp * sb);
        img.pitch_bytes = row_bytes + pad;
        const size_t size = size_t(img.pitch_bytes) * 6 + row_bytes; // (no padding behind the last row)
        uint8_t* px = static_cast<uint8_t*>(std::malloc(size));
        uint32_t lcg = uint32_t(w * 8 + sb);
        for (size_t i = 0; i < size; ++i)
          px[i] = uint8_t((lcg = lcg * 1664525u + 1013904223u) >> 24);
        img.data = px;
        rsx_image_hash_result r1, r3;
        uint8_t lines[16 * 7];
        int st = rsx_image_hash_host(&img, sb, lines, &r1, 1);
        for (size_t y = 0; y + 1 < 7; ++y)
          std::memset(px + y * img.pitch_bytes + row_bytes, int(y), pad);
        st |= rsx_image_hash_host(&img, sb, nullptr, &r3, 3);
        uint64_t want = 0;
        for (size_t y = 0; y < 7; ++y)
          for (size_t i = 0; i < row_bytes; ++i)
            want += px[y * img.pitch_bytes + i];
        uint8_t d[16];
        rsx_image_hash_host_md5(lines, sizeof lines, d);
        images_ok += st == RSX_OK && std::memcmp(&r1, &r3, sizeof r1) == 0 &&
                     std::memcmp(d, r1.md5, 16) == 0 && r1.byte_sum == want &&
                     (sb == 2) == (r1.sample_sum != 0);
        ++images;
        std::free(px);
      }
  std::printf("images %d %d\n", images, images_ok);
  bad += images_ok != images;
  std::printf(bad ? "FAILED\n" : "ok\n");
  return bad ? 1 : 0;
}
#endif
