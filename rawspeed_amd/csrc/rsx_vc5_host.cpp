// rsx_vc5_core.h as host C++ (librsx_vc5_host.so): the same table, segment walks, filters and
// merge as the kernels of rsx_vc5.hip, driven by a loop that mirrors the band kernel -- windows
// of `lanes` segments, every segment parsed from a guessed entry and re-parsed until no entry
// changes, then the write -- so that the test corpora meet the code on the CPU first.  Reads
// touch exactly [in, in + bytes), writes exactly out[0, n): a sanitizer build sees every slip.
#include "rsx_vc5_core.h"

#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

namespace {

using namespace rsx_vc5;

struct HostReader {
  const uint8_t* in;
  uint32_t bytes;
  uint64_t bit0; // the window's first bit
  uint32_t peek27(uint32_t pos) const {
    const uint64_t bit = bit0 + pos, at = bit >> 3;
    uint64_t v = 0;
    for (uint64_t k = 0; k < 5; ++k)
      v = (v << 8) | (at + k < bytes ? in[at + k] : 0u);
    return uint32_t(v >> (13u - uint32_t(bit & 7u))) & 0x07FFFFFFu;
  }
};

int32_t window_limit(uint32_t bytes, uint64_t bit0) {
  const int64_t d = int64_t(start_limit(bytes)) - int64_t(bit0);
  return int32_t(d < -1 ? -1 : (d > (1 << 30) ? (1 << 30) : d));
}

} // namespace

extern "C" int rsx_vc5_host_table(const Code* codes, int n, Table* out) {
  return build_table(codes, n, out) ? 0 : 1;
}

// One high-pass band.  Returns the band's verdict (B_*), -1 for a code book the table builder
// refuses; out[0, n) is zeroed first.  *windows / *rounds: windows walked and parse rounds.
extern "C" int rsx_vc5_host_band(const Code* codes, int n_codes, const uint8_t* in, uint32_t bytes,
                                 int32_t quant, uint32_t n, int16_t* out, uint32_t lanes,
                                 uint32_t* windows, uint32_t* rounds) {
  std::unique_ptr<Table> T(new Table);
  if (!build_table(codes, n_codes, T.get()) || lanes < 1)
    return -1;
  const TableRef t{T->l1, T->start, T->info};
  std::memset(out, 0, size_t(n) * 2);
  std::vector<uint32_t> entry(lanes), exits(lanes), next(lanes);
  std::vector<SegCount> res(lanes);
  uint32_t base = 0, carry = 0, n_win = 0, n_rounds = 0, verdict = B_NONE;
  const uint64_t win_bits = uint64_t(lanes) * SEG_BITS;
  for (uint64_t w = 0; verdict == B_NONE; ++w) {
    const HostReader rd{in, bytes, w * win_bits};
    const int32_t lim = window_limit(bytes, rd.bit0);
    if (rd.bit0 > start_limit(bytes) + win_bits) { // (cannot be reached: the limit ends a walk)
      verdict = B_OVERREAD;
      break;
    }
    ++n_win;
    for (uint32_t l = 0; l < lanes; ++l) {
      entry[l] = l == 0 ? carry : 0u;
      res[l] = parse_count(rd, t, quant, l * SEG_BITS + entry[l], (l + 1) * SEG_BITS, lim);
    }
    for (;;) { // every lane takes the exit of the lane in front of it, as of the round before
      ++n_rounds;
      bool changed = false;
      for (uint32_t l = 0; l < lanes; ++l)
        exits[l] = res[l].exit;
      for (uint32_t l = 1; l < lanes; ++l)
        if (exits[l - 1] != entry[l]) {
          entry[l] = exits[l - 1];
          res[l] = parse_count(rd, t, quant, l * SEG_BITS + entry[l], (l + 1) * SEG_BITS, lim);
          changed = true;
        }
      if (!changed)
        break;
    }
    uint32_t p = base;
    for (uint32_t l = 0; l < lanes && verdict == B_NONE; ++l) {
      verdict = parse_write(rd, t, quant, l * SEG_BITS + entry[l], (l + 1) * SEG_BITS, lim, p, n, out);
      p += res[l].ncoef;
    }
    base = p;
    carry = res[lanes - 1].exit;
  }
  if (windows)
    *windows = n_win;
  if (rounds)
    *rounds = n_rounds;
  return int(verdict);
}

// One level of one channel: out is 2w x 2h, pitch 2w
extern "C" void rsx_vc5_host_level(const int16_t* b0, uint32_t pitch0, const int16_t* b1,
                                   const int16_t* b2, const int16_t* b3, uint32_t w, uint32_t h,
                                   int32_t shift, int32_t clamp, int16_t* out) {
  const LevelView L{b0, b1, b2, b3, pitch0, w, h, shift, clamp};
  for (uint32_t r = 0; r < h; ++r)
    for (uint32_t c = 0; c < w; ++c) {
      int16_t v[4];
      level_cell(L, r, c, v);
      int16_t* o = out + (size_t(2) * r) * (2 * w) + 2 * c;
      o[0] = v[0], o[1] = v[1], o[2 * w] = v[2], o[2 * w + 1] = v[3];
    }
}

// The merge: four planes of pitch `ppitch`, w2 x h2 cells, into an image of `pitch` samples a row
extern "C" void rsx_vc5_host_merge(const int16_t* const planes[4], uint32_t ppitch, uint32_t w2,
                                   uint32_t h2, int phase, const uint16_t* table, uint16_t* img,
                                   uint32_t pitch) {
  for (uint32_t r = 0; r < h2; ++r)
    for (uint32_t c = 0; c < w2; ++c) {
      const size_t i = size_t(r) * ppitch + c;
      uint16_t px[4];
      merge_cell(planes[0][i], planes[1][i], planes[2][i], planes[3][i], phase, table, px);
      uint16_t* o = img + size_t(2 * r) * pitch + 2 * c;
      o[0] = px[0], o[1] = px[1], o[pitch] = px[2], o[pitch + 1] = px[3];
    }
}

#ifdef RSX_VC5_HOST_MAIN
// The sanitizer run: a corpus file in, one line per record out.  The file starts with u32 n_codes
// and n_codes records { u32 bits, u32 size, u32 count, i32 value }; then records
//   { u32 kind = 1, u32 bytes, i32 quant, u32 n, u32 lanes, bytes }           a band
//   { u32 kind = 2, u32 w, u32 h, u32 pitch0, i32 shift, i32 clamp, i16 b0[pitch0 h], b1, b2, b3 [w h] }
// Every buffer is an allocation of exactly its size.
namespace {
uint32_t fnv(const void* p, size_t n) {
  uint32_t h = 2166136261u;
  for (size_t i = 0; i < n; ++i)
    h = (h ^ static_cast<const uint8_t*>(p)[i]) * 16777619u;
  return h;
}
template <class T> T* exact(FILE* f, size_t n) {
  T* p = static_cast<T*>(std::malloc(n * sizeof(T) ? n * sizeof(T) : 1));
  if (!p || (n && std::fread(p, sizeof(T), n, f) != n))
    std::exit(2);
  return p;
}
} // namespace

int main(int argc, char** argv) {
  if (argc != 2)
    return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f)
    return 2;
  uint32_t n_codes = 0;
  if (std::fread(&n_codes, 4, 1, f) != 1 || n_codes > 4096)
    return 2;
  std::vector<Code> codes(n_codes);
  for (Code& c : codes) {
    uint32_t r[4];
    if (std::fread(r, 4, 4, f) != 4)
      return 2;
    c.bits = r[0], c.size = uint8_t(r[1]), c.count = uint16_t(r[2]), c.value = int16_t(int32_t(r[3]));
  }
  uint32_t kind;
  while (std::fread(&kind, 4, 1, f) == 1) {
    if (kind == 1) {
      uint32_t h[4];
      if (std::fread(h, 4, 4, f) != 4)
        return 2;
      uint8_t* in = exact<uint8_t>(f, h[0]);
      int16_t* out = static_cast<int16_t*>(std::malloc(h[2] ? size_t(h[2]) * 2 : 1));
      uint32_t windows = 0, rounds = 0;
      const int v = rsx_vc5_host_band(codes.data(), int(n_codes), in, h[0], int32_t(h[1]), h[2], out,
                                      h[3], &windows, &rounds);
      std::printf("band %d %u %u %u\n", v, windows, rounds, v == 0 ? fnv(out, size_t(h[2]) * 2) : 0u);
      std::free(in);
      std::free(out);
    } else if (kind == 2) {
      uint32_t h[5];
      if (std::fread(h, 4, 5, f) != 5)
        return 2;
      const size_t w = h[0], hh = h[1];
      int16_t* b0 = exact<int16_t>(f, size_t(h[2]) * hh);
      int16_t* b1 = exact<int16_t>(f, w * hh);
      int16_t* b2 = exact<int16_t>(f, w * hh);
      int16_t* b3 = exact<int16_t>(f, w * hh);
      int16_t* out = static_cast<int16_t*>(std::malloc(4 * w * hh * 2));
      rsx_vc5_host_level(b0, h[2], b1, b2, b3, h[0], h[1], int32_t(h[3]), int32_t(h[4]), out);
      std::printf("level %u\n", fnv(out, 4 * w * hh * 2));
      std::free(b0), std::free(b1), std::free(b2), std::free(b3), std::free(out);
    } else {
      return 2;
    }
  }
  std::fclose(f);
  return 0;
}
#endif
