// rsx_fuji_rotate_core.h as host C++ (librsx_fuji_rotate_host.so): the reference's loop restated on
// one thread (clear, then scatter), and the gather the device runs.  The tests hold both against
// the Python model.  With -DRSX_FUJI_ROTATE_HOST_MAIN the file is a program (built with
// AddressSanitizer and UBSan where g++ has them) that runs both over heap blocks of exactly their
// sizes for every small geometry and compares them.
#include "rsx_fuji_rotate_core.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace rsx_fujirot;

extern "C" int rsx_fuji_rotate_host_geometry(const rsx_raf_rotate_desc* desc, int32_t* out_dim_x,
                                             int32_t* out_dim_y, int32_t* rotation_pos) {
  return geometry(desc, out_dim_x, out_dim_y, rotation_pos);
}

extern "C" int rsx_fuji_rotate_host_validate(const rsx_raf_rotate_desc* desc, const rsx_image* src,
                                             const rsx_image* dst) {
  return validate(desc, src, dst);
}

// applyCorrections :246-269: clearArea over the R samples of every row, then the scatter
extern "C" int rsx_fuji_rotate_host_scatter(const rsx_raf_rotate_desc* desc, const rsx_image* src,
                                            const rsx_image* dst) {
  if (!src || !dst || !src->data || !dst->data)
    return RSX_ERR_INVALID_ARG;
  if (int st = validate(desc, src, dst))
    return st;
  const uint8_t* s = static_cast<const uint8_t*>(src->data);
  uint8_t* o = static_cast<uint8_t*>(dst->data);
  for (int32_t r = 0; r < dst->dim_y; ++r)
    std::memset(o + size_t(r) * dst->pitch_bytes, 0, size_t(dst->dim_x) * 2u);
  for (int32_t y = 0; y < desc->size_y; ++y)
    for (int32_t x = 0; x < desc->size_x; ++x) {
      int32_t h, w;
      forward(desc->size_x, desc->size_y, desc->alt_layout, x, y, &h, &w);
      std::memcpy(o + size_t(h) * dst->pitch_bytes + 2u * size_t(w),
                  s + size_t(desc->crop_y + y) * src->pitch_bytes + 2u * size_t(desc->crop_x + x), 2);
    }
  return RSX_OK;
}

// every destination sample from the inverse map, as the kernels make it
extern "C" int rsx_fuji_rotate_host_gather(const rsx_raf_rotate_desc* desc, const rsx_image* src,
                                           const rsx_image* dst) {
  if (!src || !dst || !src->data || !dst->data)
    return RSX_ERR_INVALID_ARG;
  if (int st = validate(desc, src, dst))
    return st;
  uint8_t* o = static_cast<uint8_t*>(dst->data);
  for (int32_t h = 0; h < dst->dim_y; ++h)
    for (int32_t w = 0; w < dst->dim_x; ++w) {
      const uint16_t v = gather(static_cast<const uint8_t*>(src->data), src->pitch_bytes,
                                desc->crop_x, desc->crop_y, desc->size_x, desc->size_y,
                                desc->alt_layout, h, w);
      std::memcpy(o + size_t(h) * dst->pitch_bytes + 2u * size_t(w), &v, 2);
    }
  return RSX_OK;
}

// the maps, for the tests
extern "C" void rsx_fuji_rotate_host_forward(int32_t W, int32_t H, int32_t alt, int32_t x, int32_t y,
                                             int32_t* h, int32_t* w) {
  forward(W, H, alt, x, y, h, w);
}
extern "C" void rsx_fuji_rotate_host_inverse(int32_t W, int32_t alt, int32_t h, int32_t w,
                                             int32_t* x, int32_t* y) {
  inverse(W, alt, h, w, x, y);
}

#ifdef RSX_FUJI_ROTATE_HOST_MAIN
// rsx_fuji_rotate_host_check: scatter against gather for every W, H <= 24, both layouts, a crop of
// (1, 2) in a source of (W + 3) x (H + 2), padded pitches.  Prints the number of geometries that ran
// and were refused, then "ok"; exit status 1 on a difference.
int main() {
  int ran = 0, refused = 0, bad = 0;
  for (int32_t alt = 0; alt < 2; ++alt)
    for (int32_t W = 1; W <= 24; ++W)
      for (int32_t H = 1; H <= 24; ++H) {
        rsx_raf_rotate_desc d;
        std::memset(&d, 0, sizeof d);
        d.crop_x = 1;
        d.crop_y = 2;
        d.size_x = W;
        d.size_y = H;
        d.alt_layout = alt;
        int32_t R = 0, Rm = 0, pos = 0;
        const int gst = geometry(&d, &R, &Rm, &pos);
        if (gst != RSX_OK) {
          ++refused;
          continue;
        }
        rsx_image src, dst;
        std::memset(&src, 0, sizeof src);
        std::memset(&dst, 0, sizeof dst);
        src.dim_x = W + 3;
        src.dim_y = H + 2;
        src.cpp = dst.cpp = 1;
        src.pitch_bytes = uint32_t(2 * src.dim_x + 6);
        dst.dim_x = R;
        dst.dim_y = Rm;
        dst.pitch_bytes = uint32_t(2 * R + 4);
        // (heap blocks of exactly the rows' span: an access past one is AddressSanitizer's)
        const size_t sb = size_t(image_span(&src)), db = size_t(image_span(&dst));
        uint8_t* s = static_cast<uint8_t*>(std::malloc(sb));
        uint8_t* a = static_cast<uint8_t*>(std::malloc(db));
        uint8_t* b = static_cast<uint8_t*>(std::malloc(db));
        for (size_t i = 0; i < sb; ++i)
          s[i] = uint8_t(i * 131u + 7u);
        std::memset(a, 0xA5, db);
        std::memset(b, 0xA5, db);
        src.data = s;
        dst.data = a;
        const int st_a = rsx_fuji_rotate_host_scatter(&d, &src, &dst);
        dst.data = b;
        const int st_b = rsx_fuji_rotate_host_gather(&d, &src, &dst);
        if (st_a != RSX_OK || st_b != RSX_OK || std::memcmp(a, b, db) != 0) {
          std::printf("differs: alt %d W %d H %d (%d %d)\n", alt, W, H, st_a, st_b);
          ++bad;
        }
        ++ran;
        std::free(s);
        std::free(a);
        std::free(b);
      }
  std::printf("ran %d refused %d\n", ran, refused);
  std::printf(bad ? "FAILED\n" : "ok\n");
  return bad ? 1 : 0;
}
#endif
