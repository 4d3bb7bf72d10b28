// Records what the reference's RawImageData::scaleBlackWhite() makes of the recorded cases of
// tests/scale_files.py: tests/golden/scale_ref.json comes from this program's output.  It is not
// part of any build or test; it needs the reference's sources (REF below) and the reference
// library that oracle/Makefile builds.  From the repository root:
//
//   python tests/scale_files.py --write-cases /tmp/scale_cases.bin
//   /opt/rocm/lib/llvm/bin/clang++ -std=c++20 -O2 -fopenmp -march=x86-64-v2 -w \
//       -Ioracle/ref_config -I$REF/src/librawspeed -I$REF/src/external \
//       scripts/record_scale_ref.cpp oracle/_ref/librawspeed_ref.so \
//       -Wl,-rpath,$PWD/oracle/_ref -Wl,-rpath,/opt/rocm/lib/llvm/lib -o /tmp/record_scale_ref
//   /tmp/record_scale_ref /tmp/scale_cases.bin > /tmp/scale_ref.jsonl
//   python tests/scale_files.py --golden /tmp/scale_ref.jsonl
//
// Per case it makes a RawImage (UINT16 or F32) of the case's size and components, copies the
// case's samples in, sets subFrame, blackAreas, blackLevel, whitePoint, blackLevelSeparate,
// mDitherScale and isCFA, calls scaleBlackWhite() on four threads, and prints one JSON line: the
// SHA-256 of the input rows and of the rows afterwards (without padding), whether the call
// returned (false: it threw), and the levels it left.  The reference build has WITH_SSE2: what
// that keeps from being recorded is listed in tests/scale_files.py.
// Behind the cases it times the call on an 8192 x 5464 CFA image (SSE2 variant with dither, levels
// given) on 1 and on 16 threads, best of 5, on stderr: bench_scale.py's README quotes those.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "common/RawImage.h"
#include "decoders/RawDecoderException.h"
#include "metadata/BlackArea.h"

extern "C" void ref_set_threads(int n);

namespace {

struct Sha256 {
  uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                   0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
  uint8_t buf[64];
  uint64_t total = 0;
  size_t fill = 0;
  static uint32_t rotr(uint32_t v, int n) { return v >> n | v << (32 - n); }
  void block(const uint8_t* p) {
    static const uint32_t k[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u,
        0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu,
        0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu,
        0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u,
        0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu,
        0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu,
        0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u,
        0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
        0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u,
        0xc67178f2u};
    uint32_t w[64];
    for (int i = 0; i < 16; ++i)
      w[i] = uint32_t(p[4 * i]) << 24 | uint32_t(p[4 * i + 1]) << 16 | uint32_t(p[4 * i + 2]) << 8 |
             p[4 * i + 3];
    for (int i = 16; i < 64; ++i) {
      const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ w[i - 15] >> 3;
      const uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ w[i - 2] >> 10;
      w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t v[8];
    std::memcpy(v, h, sizeof v);
    for (int i = 0; i < 64; ++i) {
      const uint32_t s1 = rotr(v[4], 6) ^ rotr(v[4], 11) ^ rotr(v[4], 25);
      const uint32_t t1 = v[7] + s1 + ((v[4] & v[5]) ^ (~v[4] & v[6])) + k[i] + w[i];
      const uint32_t s0 = rotr(v[0], 2) ^ rotr(v[0], 13) ^ rotr(v[0], 22);
      const uint32_t t2 = s0 + ((v[0] & v[1]) ^ (v[0] & v[2]) ^ (v[1] & v[2]));
      for (int j = 7; j > 0; --j)
        v[j] = v[j - 1];
      v[4] += t1;
      v[0] = t1 + t2;
    }
    for (int i = 0; i < 8; ++i)
      h[i] += v[i];
  }
  void update(const void* data, size_t n) {
    const uint8_t* p = static_cast<const uint8_t*>(data);
    total += n;
    while (n) {
      const size_t take = n < 64 - fill ? n : 64 - fill;
      std::memcpy(buf + fill, p, take);
      fill += take;
      p += take;
      n -= take;
      if (fill == 64) {
        block(buf);
        fill = 0;
      }
    }
  }
  std::string hex() {
    const uint64_t bits = total * 8;
    const uint8_t one = 0x80, zero = 0;
    update(&one, 1);
    while (fill != 56)
      update(&zero, 1);
    uint8_t len[8];
    for (int i = 0; i < 8; ++i)
      len[i] = uint8_t(bits >> (56 - 8 * i));
    update(len, 8);
    char out[65];
    for (int i = 0; i < 8; ++i)
      std::snprintf(out + 8 * i, 9, "%08x", h[i]);
    return out;
  }
};

bool rd(std::FILE* f, void* p, size_t n) { return std::fread(p, 1, n, f) == n; }

void time_reference(int threads) {
  using namespace rawspeed;
  const int w = 8192, h = 5464;
  ref_set_threads(threads);
  double best = 1e30;
  for (int rep = 0; rep < 5; ++rep) {
    RawImage raw = RawImage::create(iPoint2D(w, h), RawImageType::UINT16, 1);
    const Array2DRef<uint16_t> px = raw->getU16DataAsUncroppedArray2DRef();
    uint32_t s = 12345u;
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        s = s * 1664525u + 1013904223u;
        px(y, x) = uint16_t(256u + (s >> 18));
      }
    raw->blackLevel = 256;
    raw->whitePoint = 16383;
    raw->blackLevelSeparateStorage = {256, 257, 258, 259};
    raw->blackLevelSeparate = Array2DRef<int>(raw->blackLevelSeparateStorage.data(), 2, 2);
    raw->mDitherScale = true;
    const auto t0 = std::chrono::steady_clock::now();
    raw->scaleBlackWhite();
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    best = ms < best ? ms : best;
  }
  std::fprintf(stderr, "scaleBlackWhite 8192 x 5464 uint16, SSE2 variant with dither, %d thread(s): %.2f ms\n",
               threads, best);
}

} // namespace

int main(int argc, char** argv) {
  using namespace rawspeed;
  if (argc != 2)
    return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  uint32_t n = 0;
  if (!f || !rd(f, &n, 4))
    return 2;
  ref_set_threads(4);
  for (uint32_t c = 0; c < n; ++c) {
    char name[65] = {0};
    // w, h, cpp, pitch, cfa, off_x, off_y, crop_x, crop_y, is_f32, black_level, has_white,
    // white_point, has_separate, black_separate[4], dither, host_sse2, n_areas, status
    int32_t hd[22];
    if (!rd(f, name, 64) || !rd(f, hd, sizeof hd))
      return 2;
    const int w = hd[0], h = hd[1], cpp = hd[2], pitch = hd[3], ss = hd[9] ? 4 : 2;
    std::vector<uint32_t> areas(4 * size_t(hd[20]));
    std::vector<uint8_t> image(size_t(pitch) * h), skip(image.size());
    if ((!areas.empty() && !rd(f, areas.data(), 4 * areas.size())) ||
        !rd(f, image.data(), image.size()) || !rd(f, skip.data(), skip.size()))
      return 2;
    const size_t row = size_t(w) * cpp * ss;
    Sha256 in;
    for (int y = 0; y < h; ++y)
      in.update(&image[size_t(y) * pitch], row);

    RawImage raw = RawImage::create(iPoint2D(w, h), hd[9] ? RawImageType::F32 : RawImageType::UINT16,
                                    uint32_t(cpp));
    raw->isCFA = false; // (subFrame would shift a CFA this image does not have)
    const Array2DRef<std::byte> bytes = raw->getByteDataAsUncroppedArray2DRef();
    for (int y = 0; y < h; ++y)
      std::memcpy(&bytes(y, 0), &image[size_t(y) * pitch], row);
    if (hd[5] != 0 || hd[6] != 0 || hd[7] != w || hd[8] != h)
      raw->subFrame(iRectangle2D(hd[5], hd[6], hd[7], hd[8]));
    if (raw->getCropOffset() != iPoint2D(hd[5], hd[6]) || raw->dim != iPoint2D(hd[7], hd[8]))
      return 3;
    raw->isCFA = hd[4] != 0;
    for (size_t a = 0; a < areas.size(); a += 4)
      raw->blackAreas.emplace_back(int(areas[a]), int(areas[a + 1]), areas[a + 2] != 0);
    raw->blackLevel = hd[10];
    if (hd[11])
      raw->whitePoint = hd[12];
    if (hd[13]) {
      raw->blackLevelSeparateStorage = {hd[14], hd[15], hd[16], hd[17]};
      raw->blackLevelSeparate = Array2DRef<int>(raw->blackLevelSeparateStorage.data(), 2, 2);
    }
    raw->mDitherScale = hd[18] != 0;
    bool ok = true;
    try {
      raw->scaleBlackWhite();
    } catch (const RawDecoderException&) {
      ok = false;
    }
    Sha256 out;
    for (int y = 0; y < h; ++y)
      out.update(&bytes(y, 0), row);
    int sep[4] = {0, 0, 0, 0};
    if (ok && raw->blackLevelSeparate)
      for (int i = 0; i < 4; ++i)
        sep[i] = raw->blackLevelSeparateStorage[size_t(i)];
    std::printf("{\"name\": \"%s\", \"input\": \"%s\", \"ok\": %s, \"image\": \"%s\", \"black\": %d, "
                "\"white\": %d, \"sep\": [%d, %d, %d, %d]}\n",
                name, in.hex().c_str(), ok ? "true" : "false", out.hex().c_str(), raw->blackLevel,
                raw->whitePoint ? *raw->whitePoint : 0, sep[0], sep[1], sep[2], sep[3]);
  }
  time_reference(1);
  time_reference(16);
  return 0;
}
