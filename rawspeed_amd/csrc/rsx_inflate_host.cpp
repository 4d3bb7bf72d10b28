// The inflate core of rsx_dng_deflate.hip as host C++ (librsx_inflate_host.so): the same bit
// reader, table builder and symbol loop with a wave of one lane, so that the test corpora --
// valid streams and damaged ones -- meet it on the CPU first.  Reads and writes touch exactly
// [in, in + in_bytes) and [out, out + dst_len): a sanitizer build (build.py) sees every slip.
#include "rsx_inflate_core.h"

#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

namespace {

struct HostWave {
  static constexpr uint32_t N = 1;
  uint32_t lane = 0, skip = 0;
  const uint8_t* in = nullptr;
  uint64_t in_bytes = 0;
  uint32_t uni(uint32_t x) const { return x; }
  void sync() const {}
  uint64_t ballot(bool p) const { return p ? 1u : 0u; }
  uint64_t lt_mask() const { return 0; }
  uint64_t reduce_add(uint64_t x) const { return x; }
  uint32_t word(uint32_t i) const {
    uint32_t v = 0;
    for (uint32_t k = 0; k < 4; ++k) {
      const uint64_t at = uint64_t(i) * 4u + k;
      if (at < in_bytes)
        v |= uint32_t(in[at]) << (8u * k);
    }
    return v;
  }
  uint8_t byte(uint64_t i) const { return in[i]; }
  void store16(uint8_t* dst, const rsx_inflate::U4& v) const { std::memcpy(dst, &v, 16); }
};

} // namespace

// Returns 0 (whole, right and exactly dst_len bytes, all in `out`), 1 (whole and right, fewer
// bytes) or 2 (anything libz rejects); -1 without memory.
extern "C" int rsx_inflate_host(const uint8_t* in, size_t in_bytes, uint8_t* out, uint32_t dst_len,
                                uint32_t* produced, uint32_t* consumed) {
  if (in_bytes >= (size_t(1) << 32))
    return -1;
  std::unique_ptr<rsx_inflate::Shared> S(new (std::nothrow) rsx_inflate::Shared);
  if (!S)
    return -1;
  HostWave w;
  w.in = in;
  w.in_bytes = in_bytes;
  uint32_t p = 0, c = 0;
  const int v = rsx_inflate::inflate_stream(w, *S, uint32_t(in_bytes), out, dst_len, &p, &c);
  if (produced)
    *produced = p;
  if (consumed)
    *consumed = c;
  return v;
}

extern "C" uint32_t rsx_inflate_host_shared_bytes(void) { return uint32_t(sizeof(rsx_inflate::Shared)); }

#ifdef RSX_INFLATE_HOST_MAIN
// The sanitizer run: a corpus file of records { u32 in_bytes, u32 dst_len, bytes } in, one line
// "verdict produced consumed fnv1a(out)" per record out.  Every record gets allocations of exactly
// its sizes.
int main(int argc, char** argv) {
  if (argc != 2)
    return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f)
    return 2;
  uint32_t head[2];
  while (std::fread(head, 4, 2, f) == 2) {
    std::vector<uint8_t> buf(head[0]);
    if (head[0] && std::fread(buf.data(), 1, head[0], f) != head[0])
      return 2;
    uint8_t* in = static_cast<uint8_t*>(std::malloc(head[0] ? head[0] : 1));
    uint8_t* out = static_cast<uint8_t*>(std::malloc(head[1] ? head[1] : 1));
    if (!in || !out)
      return 2;
    if (head[0])
      std::memcpy(in, buf.data(), head[0]);
    std::memset(out, 0, head[1]);
    uint32_t produced = 0, consumed = 0;
    // (an empty input still gets a pointer, and never a byte read behind it)
    const int v = rsx_inflate_host(in, head[0], out, head[1], &produced, &consumed);
    uint32_t h = 2166136261u;
    if (v == 0)
      for (uint32_t i = 0; i < head[1]; ++i)
        h = (h ^ out[i]) * 16777619u;
    std::printf("%d %u %u %u\n", v, produced, consumed, h);
    std::free(in);
    std::free(out);
  }
  std::fclose(f);
  return 0;
}
#endif
