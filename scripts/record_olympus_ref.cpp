// Records what the reference's OlympusDecompressor makes of the streams of tests/olympus_files.py:
// tests/golden/olympus_ref.json comes from this program's output.  It is not part of any build or
// test; it needs the reference's sources (REF below) and the reference library that
// oracle/Makefile builds.  From the repository root:
//
//   python tests/olympus_files.py --write-cases /tmp/olympus_cases.bin
//   /opt/rocm/lib/llvm/bin/clang++ -std=c++20 -O2 -fopenmp -march=x86-64-v2 -w \
//       -Ioracle/ref_config -I$REF/src/librawspeed -I$REF/src/external \
//       scripts/record_olympus_ref.cpp oracle/_ref/librawspeed_ref.so \
//       -Wl,-rpath,$PWD/oracle/_ref -Wl,-rpath,/opt/rocm/lib/llvm/lib -o /tmp/record_olympus_ref
//   /tmp/record_olympus_ref /tmp/olympus_cases.bin > /tmp/olympus_ref.jsonl
//   python tests/olympus_files.py --golden /tmp/olympus_ref.jsonl
//
// The case file is "RSXO", a count, then per case its width, height, pitch and length (u32 each)
// and the stream.  Per case the program makes a RawImage (UINT16, one component) of width x
// height -- for a width or height below 1, which no image can have, an empty one with those
// dimensions set --, runs the OlympusDecompressor constructor and decompress(), and prints one
// JSON line: whether both returned, the exception's class and message if not, and the SHA-256 of
// the image rows without padding.
//
//   /tmp/record_olympus_ref --time FRAME W H     (bench_olympus.py --write-frame FRAME)
// times decompress() of one stream, best of 5, on stderr: profiles/olympus/README.md quotes that
// as another machine's CPU.  The reference's loop is single-threaded.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "common/RawImage.h"
#include "common/RawspeedException.h"
#include "decoders/RawDecoderException.h"
#include "decompressors/OlympusDecompressor.h"
#include "io/Buffer.h"
#include "io/ByteStream.h"
#include "io/Endianness.h"
#include "io/IOException.h"

namespace {

struct Sha256 {
  uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                   0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
  uint8_t buf[64];
  uint64_t total = 0;
  size_t fill = 0;
  uint32_t k[64];
  Sha256() {
    // the fractional parts of the cube roots of the first 64 primes
    int n = 0;
    for (uint32_t p = 2; n < 64; ++p) {
      bool prime = true;
      for (uint32_t d = 2; d * d <= p; ++d)
        prime = prime && p % d != 0;
      if (!prime)
        continue;
      long double r = __builtin_cbrtl((long double)p);
      r -= (long double)(uint64_t)r;
      k[n++] = uint32_t(r * 4294967296.0L);
    }
  }
  static uint32_t rotr(uint32_t v, int n) { return v >> n | v << (32 - n); }
  void block(const uint8_t* p) {
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
    for (; n; --n) {
      buf[fill++] = *p++;
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

using namespace rawspeed;

struct Verdict {
  bool ok = false;
  std::string cls, msg;
};

std::string json_escape(const std::string& s) {
  std::string o;
  for (char c : s) {
    if (c == '"' || c == '\\')
      o += '\\';
    o += (unsigned char)c < 0x20 ? ' ' : c;
  }
  return o;
}

Verdict decode(const std::vector<uint8_t>& c, int w, int h, RawImage* out, double* ms) {
  Verdict v;
  try {
    RawImage raw = RawImage::create(RawImageType::UINT16);
    if (w > 0 && h > 0)
      raw = RawImage::create(iPoint2D(w, h), RawImageType::UINT16, 1);
    else
      raw->dim = iPoint2D(w, h);
    const Buffer b(c.data(), Buffer::size_type(c.size()));
    OlympusDecompressor o(raw);
    const auto t0 = std::chrono::steady_clock::now();
    o.decompress(ByteStream(DataBuffer(b, Endianness::big)));
    if (ms)
      *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *out = raw;
    v.ok = true;
  } catch (const RawDecoderException& e) {
    v.cls = "RawDecoderException";
    v.msg = e.what();
  } catch (const IOException& e) {
    v.cls = "IOException";
    v.msg = e.what();
  } catch (const RawspeedException& e) {
    v.cls = "RawspeedException";
    v.msg = e.what();
  }
  return v;
}

} // namespace

int main(int argc, char** argv) {
  if (argc == 5 && std::string(argv[1]) == "--time") {
    std::FILE* f = std::fopen(argv[2], "rb");
    if (!f)
      return 2;
    std::vector<uint8_t> c;
    uint8_t chunk[65536];
    for (size_t n; (n = std::fread(chunk, 1, sizeof chunk, f)) != 0;)
      c.insert(c.end(), chunk, chunk + n);
    std::fclose(f);
    const int w = std::atoi(argv[3]), h = std::atoi(argv[4]);
    double best = 1e30;
    for (int rep = 0; rep < 5; ++rep) {
      RawImage raw = RawImage::create(RawImageType::UINT16);
      double ms = 0;
      if (!decode(c, w, h, &raw, &ms).ok)
        return 1;
      best = ms < best ? ms : best;
    }
    std::fprintf(stderr, "OlympusDecompressor::decompress %d x %d, 1 thread: %.2f ms\n", w, h, best);
    return 0;
  }
  if (argc != 2)
    return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  char magic[4];
  uint32_t n = 0;
  if (!f || std::fread(magic, 1, 4, f) != 4 || std::memcmp(magic, "RSXO", 4) != 0 ||
      std::fread(&n, 4, 1, f) != 1)
    return 2;
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t hd[4];
    if (std::fread(hd, 4, 4, f) != 4)
      return 2;
    std::vector<uint8_t> c(hd[3]);
    if (hd[3] && std::fread(c.data(), 1, hd[3], f) != hd[3])
      return 2;
    RawImage raw = RawImage::create(RawImageType::UINT16);
    const Verdict v = decode(c, int(hd[0]), int(hd[1]), &raw, nullptr);
    Sha256 sha;
    if (v.ok) {
      const Array2DRef<uint16_t> px = raw->getU16DataAsUncroppedArray2DRef();
      for (int y = 0; y < px.height(); ++y)
        sha.update(&px(y, 0), size_t(px.width()) * 2);
    }
    std::printf("{\"ok\": %s, \"exception\": \"%s\", \"message\": \"%s\", \"sha256\": \"%s\"}\n",
                v.ok ? "true" : "false", v.cls.c_str(), json_escape(v.msg).c_str(),
                v.ok ? sha.hex().c_str() : "");
  }
  std::fclose(f);
  return 0;
}
