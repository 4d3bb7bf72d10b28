// rsx_dng_post_core.h as host C++ (librsx_dng_post_host.so): the same parse, tables and lane as
// the kernel of rsx_dng_post.hip, driven by a loop that mirrors the kernel -- every lane of every
// row goes through the whole list and the look-up, the hits are collected and composed -- so that
// the test cases meet the code on the CPU first.  Compiled with -ffp-contract=off.  With
// -DRSX_DNG_POST_HOST_MAIN the file is a program (built with AddressSanitizer and UBSan where g++
// has them): without arguments it holds the fused pass against a pass-per-opcode restatement with
// a stepped generator on built-in lists and runs 200 randomly damaged lists; every argument is a
// case file a test wrote (the layout is at read_case) whose expected verdict, image and positions
// it checks.
#include "rsx_dng_post_core.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace rsx_dngpost;

extern "C" int rsx_dng_post_host_validate(const rsx_dng_post_desc* desc, const rsx_image* img,
                                          rsx_dng_post_result* result, uint32_t* bad,
                                          uint32_t bad_cap) {
  if (!bad && bad_cap != 0)
    return RSX_ERR_INVALID_ARG;
  return validate(desc, img, result, bad, bad_cap);
}

// rsx_dng_post on the host: img->data is processed in place (untouched unless RSX_OK, or
// RSX_ERR_UNSUPPORTED for a position list past bad_cap)
extern "C" int rsx_dng_post_host_apply(const rsx_dng_post_desc* desc, const rsx_image* img,
                                       rsx_dng_post_result* result, uint32_t* bad,
                                       uint32_t bad_cap) {
  if (!desc || !img || !img->data || (!bad && bad_cap != 0))
    return RSX_ERR_INVALID_ARG;
  Parsed P;
  if (int st = parse(desc, img, &P))
    return st;
  JobDev J;
  fill_job(desc, img, P, &J);
  const std::vector<uint32_t> pw = dither_powers8(J.vpr ? J.vpr : 1u);
  const uint32_t N = J.is_f32 ? 4u : 8u;
  std::vector<uint64_t> hit_list;
  for (uint32_t row = 0; row < J.h; ++row) {
    uint8_t* line = static_cast<uint8_t*>(img->data) + size_t(row) * J.pitch;
    for (uint32_t v = 0; v < J.vpr; ++v) {
      const uint32_t s0 = N * v, n = J.ws - s0 < N ? J.ws - s0 : N;
      uint32_t px[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      uint64_t hits[2] = {0, 0};
      for (uint32_t i = 0; i < n; ++i) {
        if (J.is_f32)
          std::memcpy(&px[i], line + 4 * size_t(s0 + i), 4);
        else {
          uint16_t t;
          std::memcpy(&t, line + 2 * size_t(s0 + i), 2);
          px[i] = t;
        }
      }
      const uint32_t touched =
          J.is_f32 ? lane<true>(J, P.ops.data(), P.tables.data(), P.deltas.data(), P.lut.data(),
                                pw.data(), row, s0, n, px, hits)
                   : lane<false>(J, P.ops.data(), P.tables.data(), P.deltas.data(), P.lut.data(),
                                 pw.data(), row, s0, n, px, hits);
      for (uint32_t i = 0; i < n; ++i)
        if (touched >> i & 1u) {
          if (J.is_f32)
            std::memcpy(line + 4 * size_t(s0 + i), &px[i], 4);
          else {
            const uint16_t t = uint16_t(px[i]);
            std::memcpy(line + 2 * size_t(s0 + i), &t, 2);
          }
        }
      for (uint32_t half = 0; half < 2; ++half)
        for (uint32_t bit = 0; bit < 64; ++bit)
          if (hits[half] >> bit & 1u) {
            const uint32_t o = half * 8u + (bit >> 3);
            hit_list.push_back(hit_entry(o, row - P.ops[o].y0, s0 + (bit & 7u) - P.ops[o].x0));
          }
    }
  }
  std::vector<uint32_t> out;
  compose_bad(P, hit_list, &out);
  fill_result(P, out.size(), result);
  if (out.size() > bad_cap)
    return RSX_ERR_UNSUPPORTED;
  if (!out.empty())
    std::memcpy(bad, out.data(), out.size() * sizeof(uint32_t));
  return RSX_OK;
}

// the state doLookup's generator has when it looks sample x of row y up, through the jump the
// lanes take (x >= 8: the reduced seed times a power; x < 8: stepped from the seed)
extern "C" uint32_t rsx_dng_post_host_dither_state(uint32_t dim_x, uint32_t y, uint32_t x) {
  const uint32_t seed = (dim_x + 13u * y) ^ 0x45694584u;
  const uint32_t s0 = x & ~7u;
  uint32_t r = seed;
  if (s0 != 0u) {
    const std::vector<uint32_t> pw = dither_powers8((s0 >> 3) + 1u);
    const uint64_t reduced = seed >= DITHER_M ? seed - DITHER_M : seed;
    r = uint32_t(reduced * pw[s0 >> 3] % DITHER_M);
  }
  for (uint32_t i = s0; i <= x; ++i)
    r = dither_step(r);
  return r;
}

#ifdef RSX_DNG_POST_HOST_MAIN
namespace {

int fails = 0;
void expect(bool ok, const char* what, int k = -1) {
  if (!ok) {
    std::fprintf(stderr, "FAILED: %s (%d)\n", what, k);
    ++fails;
  }
}

uint32_t rng_state = 4242;
uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

void be32(std::vector<uint8_t>& o, uint32_t v) {
  for (int s = 24; s >= 0; s -= 8)
    o.push_back(uint8_t(v >> s));
}
void bef(std::vector<uint8_t>& o, float f) {
  uint32_t b;
  std::memcpy(&b, &f, 4);
  be32(o, b);
}

struct PlainOp {
  uint32_t code, top, left, bottom, right, first, planes, rp, cp, value;
  std::vector<float> deltas;
  std::vector<uint16_t> table;
};

void emit(std::vector<uint8_t>& list, const PlainOp& op) {
  std::vector<uint8_t> b;
  if (op.code == 4) {
    be32(b, op.value);
    be32(b, 0);
  } else {
    be32(b, op.top);
    be32(b, op.left);
    be32(b, op.bottom);
    be32(b, op.right);
    if (op.code != 6) {
      be32(b, op.first);
      be32(b, op.planes);
      be32(b, op.rp);
      be32(b, op.cp);
      if (op.code == 7) {
        be32(b, uint32_t(op.table.size()));
        for (uint16_t t : op.table) {
          b.push_back(uint8_t(t >> 8));
          b.push_back(uint8_t(t));
        }
      } else {
        be32(b, uint32_t(op.deltas.size()));
        for (float f : op.deltas)
          bef(b, f);
      }
    }
  }
  be32(list, op.code);
  be32(list, 0x01030000);
  be32(list, 0);
  be32(list, uint32_t(b.size()));
  list.insert(list.end(), b.begin(), b.end());
}

// a pass per opcode, PixelOpcode::applyOP's loops; then doLookup with a stepped generator
void plain(const std::vector<PlainOp>& ops, std::vector<uint16_t>& img, int w, int h, int cpp,
           int pitch_px, int cx, int cy, int cw, int ch, const std::vector<uint16_t>& table,
           std::vector<uint32_t>* bad) {
  for (const PlainOp& op : ops) {
    if (op.code == 6) {
      cx += int(op.left);
      cy += int(op.top);
      cw = int(op.right - op.left);
      ch = int(op.bottom - op.top);
      continue;
    }
    if (op.code == 4) {
      for (int r = 0; r < ch; ++r)
        for (int c = 0; c < cw; ++c)
          if (img[size_t(cy + r) * pitch_px + cx + c] == op.value)
            bad->push_back((uint32_t(cx) | uint32_t(cy) << 16) + (uint32_t(r) << 16 | uint32_t(c)));
      continue;
    }
    const uint32_t ny = (op.bottom - op.top + op.rp - 1) / op.rp, nx = (op.right - op.left + op.cp - 1) / op.cp;
    for (uint32_t y = 0; y < ny; ++y)
      for (uint32_t x = 0; x < nx; ++x)
        for (uint32_t p = 0; p < op.planes; ++p) {
          uint16_t& px = img[size_t(cy + op.top + op.rp * y) * pitch_px + size_t(cx) * cpp + op.first +
                             size_t(op.left + op.cp * x) * cpp + p];
          const uint32_t k = (op.code == 10 || op.code == 12) ? y : x;
          if (op.code == 7)
            px = op.table[px < op.table.size() ? px : op.table.size() - 1];
          else if (op.code <= 11)
            px = uint16_t(clamp16(int(65535.0F * op.deltas[k]) + px));
          else
            px = uint16_t(clamp16((int(1024.0F * op.deltas[k]) * px + 512) >> 10));
        }
  }
  if (table.empty())
    return;
  std::vector<uint32_t> lut;
  build_lut(table.data(), uint32_t(table.size()), &lut);
  for (int y = 0; y < h; ++y) { // (every uncropped row: APPLY_LOOKUP is a FULL_IMAGE task)
    uint32_t v = uint32_t(w + y * 13) ^ 0x45694584u;
    for (int x = 0; x < w * cpp; ++x) {
      uint16_t& p = img[size_t(y) * pitch_px + x];
      v = 15700u * (v & 65535u) + (v >> 16);
      const uint32_t pix = (lut[p] & 0xFFFFu) + (((lut[p] >> 16) * (v & 2047u) + 1024u) >> 12);
      p = uint16_t(pix > 65535u ? 65535u : pix);
    }
  }
}

std::vector<PlainOp> random_list(int cw, int ch, int cpp) {
  std::vector<PlainOp> ops;
  const int n = 1 + int(rnd() % 6);
  for (int k = 0; k < n; ++k) {
    PlainOp op{};
    const uint32_t codes[] = {7, 10, 11, 12, 13, 6, 4};
    op.code = codes[rnd() % (cpp == 1 ? 7 : 6)];
    if (op.code == 4) {
      op.value = rnd() % 4;
      ops.push_back(op);
      continue;
    }
    if (cw < 3 || ch < 3)
      break;
    op.left = rnd() % uint32_t(cw - 1);
    op.top = rnd() % uint32_t(ch - 1);
    op.right = op.left + 1 + rnd() % uint32_t(cw - int(op.left));
    op.bottom = op.top + 1 + rnd() % uint32_t(ch - int(op.top));
    if (op.code == 6) {
      if (op.right - op.left < 3 || op.bottom - op.top < 3)
        continue;
      cw = int(op.right - op.left);
      ch = int(op.bottom - op.top);
      ops.push_back(op);
      continue;
    }
    op.first = rnd() % uint32_t(cpp);
    op.planes = 1 + rnd() % uint32_t(cpp - int(op.first));
    op.rp = 1 + rnd() % std::min<uint32_t>(3, op.bottom - op.top);
    op.cp = 1 + rnd() % std::min<uint32_t>(3, op.right - op.left);
    if (op.code == 7) {
      op.table.resize(1 + rnd() % 300);
      for (uint16_t& t : op.table)
        t = uint16_t(rnd());
    } else {
      const bool by_col = op.code == 11 || op.code == 13;
      const uint32_t ext = by_col ? op.right - op.left : op.bottom - op.top, pitch = by_col ? op.cp : op.rp;
      op.deltas.resize((ext + pitch - 1) / pitch);
      for (float& f : op.deltas)
        f = op.code <= 11 ? (float(rnd() % 2001) - 1000.0F) / 1000.0F : float(rnd() % 4000) / 1000.0F;
    }
    ops.push_back(op);
  }
  return ops;
}

// A case file: 12 little-endian int32 (w, h, cpp, is_f32, pitch_bytes, crop x y w h, table_count,
// opcodes_bytes, n_expected_bad), then int32 expected status, list_status, n_applied, 4 x final
// crop; the table, the list, the image (pitch_bytes * h), the expected image, the expected
// positions.
bool read_case(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f)
    return false;
  std::vector<uint8_t> all;
  uint8_t buf[4096];
  size_t got;
  while ((got = std::fread(buf, 1, sizeof buf, f)) > 0)
    all.insert(all.end(), buf, buf + got);
  std::fclose(f);
  if (all.size() < 19 * 4)
    return false;
  int32_t hd[19];
  std::memcpy(hd, all.data(), sizeof hd);
  size_t at = sizeof hd;
  const size_t img_bytes = size_t(hd[4]) * size_t(hd[1]);
  if (all.size() != at + 2 * size_t(hd[9]) + size_t(hd[10]) + 2 * img_bytes + 4 * size_t(hd[11]))
    return false;
  std::vector<uint16_t> table(size_t(hd[9]) + 1);
  std::memcpy(table.data(), all.data() + at, 2 * size_t(hd[9]));
  at += 2 * size_t(hd[9]);
  std::vector<uint8_t> list(all.begin() + at, all.begin() + at + hd[10]);
  at += size_t(hd[10]);
  std::vector<uint8_t> img(all.begin() + at, all.begin() + at + img_bytes);
  at += img_bytes;
  std::vector<uint8_t> want(all.begin() + at, all.begin() + at + img_bytes);
  at += img_bytes;
  std::vector<uint32_t> want_bad(size_t(hd[11]) + 1);
  std::memcpy(want_bad.data(), all.data() + at, 4 * size_t(hd[11]));
  rsx_dng_post_desc d{};
  d.opcodes = list.empty() ? nullptr : list.data();
  d.opcodes_bytes = uint32_t(list.size());
  d.table = hd[9] ? table.data() : nullptr;
  d.table_count = uint32_t(hd[9]);
  d.is_f32 = hd[3];
  d.crop_x = hd[5];
  d.crop_y = hd[6];
  d.crop_w = hd[7];
  d.crop_h = hd[8];
  rsx_image v{img.data(), uint32_t(hd[4]), hd[0], hd[1], hd[2], 1};
  rsx_dng_post_result r{};
  std::vector<uint32_t> bad(size_t(hd[11]) + 1);
  const int st = rsx_dng_post_host_apply(&d, &v, &r, bad.data(), uint32_t(hd[11]));
  bool ok = st == hd[12];
  if (st == RSX_OK)
    ok = ok && r.list_status == hd[13] && r.n_applied == hd[14] && r.crop_x == hd[15] &&
         r.crop_y == hd[16] && r.crop_w == hd[17] && r.crop_h == hd[18] &&
         r.n_bad == uint64_t(hd[11]) &&
         std::memcmp(bad.data(), want_bad.data(), 4 * size_t(hd[11])) == 0;
  return ok && img == want;
}

} // namespace

int main(int argc, char** argv) {
  for (int a = 1; a < argc; ++a)
    expect(read_case(argv[a]), argv[a]);
  if (argc > 1) {
    if (fails)
      return 1;
    std::printf("rsx_dng_post_host_check OK: %d case files\n", argc - 1);
    return 0;
  }
  struct Geo { int w, h, cpp, pitch_px, cx, cy, cw, ch; };
  const Geo geos[] = {{64, 20, 1, 64, 0, 0, 64, 20}, {70, 20, 1, 75, 3, 2, 60, 15},
                      {22, 9, 3, 71, 1, 1, 20, 7},   {8, 6, 1, 8, 0, 0, 8, 6},
                      {1100, 4, 1, 1100, 5, 0, 1090, 3}};
  int k = 0;
  for (const Geo& g : geos)
    for (int rep = 0; rep < 40; ++rep, ++k) {
      const std::vector<PlainOp> ops = random_list(g.cw, g.ch, g.cpp);
      std::vector<uint8_t> list;
      be32(list, uint32_t(ops.size()));
      for (const PlainOp& op : ops)
        emit(list, op);
      std::vector<uint16_t> table(rep % 3 == 0 ? 0 : 1 + rnd() % 700);
      for (uint16_t& t : table)
        t = uint16_t(rnd());
      std::vector<uint16_t> a(size_t(g.pitch_px) * g.h), b;
      for (uint16_t& v : a)
        v = uint16_t(rnd() % 5 == 0 ? rnd() % 4 : rnd());
      b = a;
      rsx_dng_post_desc d{};
      d.opcodes = list.data();
      d.opcodes_bytes = uint32_t(list.size());
      d.table = table.empty() ? nullptr : table.data();
      d.table_count = uint32_t(table.size());
      d.crop_x = g.cx;
      d.crop_y = g.cy;
      d.crop_w = g.cw;
      d.crop_h = g.ch;
      rsx_image img{a.data(), uint32_t(2 * g.pitch_px), g.w, g.h, g.cpp, 1};
      rsx_dng_post_result r{};
      std::vector<uint32_t> bad(size_t(g.w) * g.h * 8), want_bad;
      const int st = rsx_dng_post_host_apply(&d, &img, &r, bad.data(), uint32_t(bad.size()));
      expect(st == RSX_OK && r.list_status == RSX_OK && r.n_applied == int(ops.size()), "status", k);
      plain(ops, b, g.w, g.h, g.cpp, g.pitch_px, g.cx, g.cy, g.cw, g.ch, table, &want_bad);
      expect(a == b, "fused pass against pass per opcode", k);
      bad.resize(size_t(r.n_bad));
      expect(bad == want_bad, "positions", k);
      // the same list, damaged: truncated, a byte changed, a length changed -- whatever the
      // verdict, no read outside the list and an image that is untouched unless RSX_OK
      for (int m = 0; m < 1; ++m) {
        std::vector<uint8_t> bent = list;
        const uint32_t how = rnd() % (bent.size() >= 20 ? 3 : 2);
        if (how == 0)
          bent.resize(rnd() % bent.size());
        else if (how == 1)
          bent[rnd() % bent.size()] ^= uint8_t(1u << (rnd() % 8));
        else
          bent[4 + 12 + rnd() % 4] = uint8_t(rnd());
        std::vector<uint8_t> exact(bent); // (its own allocation: a read past the end is seen)
        d.opcodes = exact.empty() ? nullptr : exact.data();
        d.opcodes_bytes = uint32_t(exact.size());
        std::vector<uint16_t> c = b, keep = b;
        rsx_image im2{c.data(), uint32_t(2 * g.pitch_px), g.w, g.h, g.cpp, 1};
        bad.assign(size_t(g.w) * g.h * 8, 0u);
        const int st2 = rsx_dng_post_host_apply(&d, &im2, &r, bad.data(), uint32_t(bad.size()));
        expect(st2 == RSX_OK || c == keep, "a refused list touched the image", k);
      }
    }
  if (fails)
    return 1;
  std::printf("rsx_dng_post_host_check OK: %d lists, %d damaged\n", k, k);
  return 0;
}
#endif
