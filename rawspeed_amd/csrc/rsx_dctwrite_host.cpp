// rsx_dctwrite_host.cpp -- rsx_dctwrite_core.h as host C++: the single-threaded reference walk of
// a whole tile that the kernels of rsx_dctwrite.hip are held against, built into
// rawspeed_amd/librsx_dctwrite_host.so.  With -DRSX_DCTWRITE_HOST_MAIN the same source is a
// program (AddressSanitizer + UBSan where the runtimes exist) that proves the reciprocal quantiser
// equal to the division for every (|x| <= 32767, q), walks small frames of every sampling, size
// and restart interval through the writer, and checks their headers, sizes and bounds.
#include "rsx_dctwrite_core.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace rsx_dctw;

namespace {

// the quantised coefficients of real block w in zig-zag order
void block_coefficients(const Geom& g, const uint8_t* base, const Where& w, const uint16_t* q,
                        int16_t* zz, bool* over) {
  int ws[64];
  for (uint32_t r = 0; r < 8; ++r) {
    block_row(g, base, w, r, ws + 8 * r, over);
    fdct_pass<true>(ws + 8 * r);
  }
  for (uint32_t c = 0; c < 8; ++c) {
    int col[8];
    for (uint32_t r = 0; r < 8; ++r)
      col[r] = ws[8 * r + c];
    fdct_pass<false>(col);
    for (uint32_t r = 0; r < 8; ++r)
      ws[8 * r + c] = col[r];
  }
  for (uint32_t k = 0; k < 64; ++k) {
    const uint32_t n = ZIGZAG[k];
    zz[k] = int16_t(quantise(ws[n], q[n], recip_of(q[n])));
  }
}

struct BitSink {
  std::vector<uint8_t>* out;
  uint64_t acc = 0;
  uint32_t n = 0;
  uint64_t bits = 0;
  void byte(uint8_t b) {
    out->push_back(b);
    if (b == 0xFF)
      out->push_back(0);
  }
  void put(uint32_t v, uint32_t len) {
    acc = (acc << len) | v;
    n += len;
    bits += len;
    while (n >= 8) {
      byte(uint8_t(acc >> (n - 8)));
      n -= 8;
    }
  }
  void close() {
    if (n) {
      const uint32_t pad = 8 - n;
      byte(uint8_t((acc << pad) | ((1u << pad) - 1u)));
    }
    acc = 0, n = 0;
  }
};

int encode(const rsx_dctwrite_desc& d, const rsx_image& img, std::vector<uint8_t>* out,
           rsx_dctwrite_result* res) {
  Geom g;
  geom_of(d, img, 0, 0, 0, &g);
  HuffEnc h;
  build_huff(&h);
  out->clear();
  write_header(d, out);
  const size_t hdr = out->size();
  const uint8_t* base = static_cast<const uint8_t*>(img.data);
  BitSink sink{out};
  bool over = false;
  int pred[3] = {0, 0, 0};
  int16_t zz[64];
  for (uint32_t lb = 0; lb < g.n_blocks; ++lb) {
    const uint32_t m = lb / g.bpm;
    if (lb % g.bpm == 0 && m % g.ri == 0) {
      if (m) {
        sink.close();
        out->push_back(0xFF);
        out->push_back(uint8_t(0xD0 + (m / g.ri - 1) % 8));
      }
      pred[0] = pred[1] = pred[2] = 0;
    }
    const Where w = where_of(g, lb);
    const uint32_t t = w.comp ? 1u : 0u;
    int diff = 0;
    if (!w.dummy) {
      block_coefficients(g, base, w, d.qtables[t], zz, &over);
      diff = zz[0] - pred[w.comp];
      pred[w.comp] = zz[0];
    }
    walk_block(h, t, diff, w.dummy, [&](uint32_t k) { return int(zz[k]); }, sink);
  }
  sink.close();
  res->scan_bytes = out->size() - hdr;
  out->push_back(0xFF);
  out->push_back(0xD9);
  res->symbol_bits = sink.bits;
  res->bytes = out->size();
  res->status = over ? RSX_ERR_VALUE_RANGE : RSX_OK;
  return res->status;
}

} // namespace

extern "C" {

int rsx_dctwrite_host_quality_tables(int quality, uint16_t* luma, uint16_t* chroma) {
  return quality_tables(quality, luma, chroma);
}

int rsx_dctwrite_host_validate(const rsx_dctwrite_desc* d, const rsx_image* img) {
  return validate(d, img);
}

uint64_t rsx_dctwrite_host_bound(const rsx_dctwrite_desc* d, const rsx_image* img) {
  if (validate(d, img) != RSX_OK)
    return 0;
  Geom g;
  geom_of(*d, *img, 0, 0, 0, &g);
  return bound_of(g);
}

// the quantised coefficients of every block of the scan (dummies: zeros), 64 a block in zig-zag
// order; returns the number of blocks, or 0 for a refused descriptor
uint32_t rsx_dctwrite_host_coefficients(const rsx_dctwrite_desc* d, const rsx_image* img,
                                        int16_t* out, uint32_t cap_blocks) {
  if (validate(d, img) != RSX_OK || !img->data)
    return 0;
  Geom g;
  geom_of(*d, *img, 0, 0, 0, &g);
  bool over = false;
  for (uint32_t lb = 0; lb < g.n_blocks && lb < cap_blocks; ++lb) {
    const Where w = where_of(g, lb);
    std::memset(out + 64 * size_t(lb), 0, 128);
    if (!w.dummy)
      block_coefficients(g, static_cast<const uint8_t*>(img->data), w, d->qtables[w.comp ? 1 : 0],
                         out + 64 * size_t(lb), &over);
  }
  return g.n_blocks;
}

// img->data: the image in host memory.  Returns the tile's status; res as the device reports it.
int rsx_dctwrite_host(const rsx_dctwrite_desc* d, const rsx_image* img, uint8_t* out, size_t out_cap,
                      rsx_dctwrite_result* res) {
  if (!d || !img || !img->data || !res || (!out && out_cap))
    return RSX_ERR_INVALID_ARG;
  std::memset(res, 0, sizeof *res);
  if (int st = validate(d, img))
    return res->status = st;
  std::vector<uint8_t> s;
  int st = encode(*d, *img, &s, res);
  if (st == RSX_OK && s.size() > out_cap)
    st = RSX_ERR_INPUT_OVERFLOW;
  if (st != RSX_OK) {
    std::memset(res, 0, sizeof *res);
    return res->status = st;
  }
  std::memcpy(out, s.data(), s.size());
  return RSX_OK;
}

} // extern "C"

#ifdef RSX_DCTWRITE_HOST_MAIN
namespace {

int fail(const char* what, long a = 0, long b = 0) {
  std::fprintf(stderr, "ERROR %s (%ld, %ld)\n", what, a, b);
  return 1;
}

} // namespace

int main() {
  // the reciprocal is the division
  for (uint32_t q = 1; q <= 255; ++q) {
    const uint32_t r = recip_of(q);
    for (int x = 0; x <= 32767; ++x) {
      const int want = int((uint32_t(x) + 4u * q) / (8u * q));
      if (quantise(x, q, r) != want || quantise(-x, q, r) != -want)
        return fail("reciprocal", x, q);
    }
  }
  std::printf("quantise: 32768 x 255 pairs equal the division\n");
  // the predictor rule of the kernels against the walk's running predictors
  uint32_t frames = 0;
  const int samp[4][3] = {{1, 1, 1}, {3, 1, 1}, {3, 2, 1}, {3, 2, 2}};
  for (const auto& s : samp)
    for (uint32_t w : {1u, 8u, 16u, 17u, 33u})
      for (uint32_t h : {1u, 8u, 16u, 17u})
        for (uint32_t ri : {0u, 1u, 2u, 3u}) {
          rsx_dctwrite_desc d;
          std::memset(&d, 0, sizeof d);
          d.width = w + 3, d.height = h + 2; // (past the image's edge)
          d.components = s[0], d.h_samp = s[1], d.v_samp = s[2];
          d.restart_interval = ri;
          d.flags = frames & 1u;
          quality_tables(int(1 + (frames * 7) % 100), d.qtables[0], d.qtables[1]);
          std::vector<uint16_t> px(size_t(w) * h * s[0]);
          uint32_t x = 12345u + frames;
          for (uint16_t& v : px)
            v = uint16_t((x = x * 1664525u + 1013904223u) >> 24);
          rsx_image img{px.data(), uint32_t(2 * w * s[0]), int32_t(w), int32_t(h), s[0], 0};
          if (validate(&d, &img) != RSX_OK)
            return fail("validate", w, h);
          Geom g;
          geom_of(d, img, 0, 0, 0, &g);
          // predictor_block against a running predictor over the scan order
          int last[3] = {-1, -1, -1};
          for (uint32_t lb = 0; lb < g.n_blocks; ++lb) {
            if (lb % g.bpm == 0 && (lb / g.bpm) % g.ri == 0)
              last[0] = last[1] = last[2] = -1;
            const Where wh = where_of(g, lb);
            uint32_t p = 0;
            const bool has = predictor_block(g, lb, &p);
            if (has != (last[wh.comp] >= 0) || (has && int(p) != last[wh.comp]))
              return fail("predictor_block", lb, frames);
            if (!wh.dummy)
              last[wh.comp] = int(lb);
            else if (lb % g.bpm == 0)
              return fail("dummy at block 0", lb, frames);
          }
          const uint64_t bound = rsx_dctwrite_host_bound(&d, &img);
          std::vector<uint8_t> out(bound);
          rsx_dctwrite_result res;
          if (rsx_dctwrite_host(&d, &img, out.data(), out.size(), &res) != RSX_OK)
            return fail("encode", w, h);
          std::vector<uint8_t> hdr;
          write_header(d, &hdr);
          if (hdr.size() != g.hdr_bytes || std::memcmp(hdr.data(), out.data(), hdr.size()) != 0)
            return fail("header", long(hdr.size()), g.hdr_bytes);
          if (res.bytes > bound || res.bytes != g.hdr_bytes + res.scan_bytes + 2 ||
              out[res.bytes - 2] != 0xFF || out[res.bytes - 1] != 0xD9)
            return fail("sizes", long(res.bytes), long(bound));
          std::vector<uint8_t> tight(res.bytes);
          rsx_dctwrite_result r2;
          if (rsx_dctwrite_host(&d, &img, tight.data(), tight.size(), &r2) != RSX_OK ||
              std::memcmp(tight.data(), out.data(), tight.size()) != 0)
            return fail("exact capacity", w, h);
          if (rsx_dctwrite_host(&d, &img, tight.data(), tight.size() - 1, &r2) !=
                  RSX_ERR_INPUT_OVERFLOW || r2.bytes != 0)
            return fail("one byte short", w, h);
          px[px.size() / 2] = 256;
          if (rsx_dctwrite_host(&d, &img, out.data(), out.size(), &r2) != RSX_ERR_VALUE_RANGE ||
              r2.bytes != 0)
            return fail("value range", w, h);
          ++frames;
        }
  std::printf("frames: %u written, bounded and refused\n", frames);
  std::printf("rsx_dctwrite_host_check OK\n");
  return 0;
}
#endif
