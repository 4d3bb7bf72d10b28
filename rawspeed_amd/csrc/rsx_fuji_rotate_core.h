// RafDecoder::applyCorrections, the 45 degree rotation of SuperCCD frames (include/rsx.h section
// 3y), shared by the kernels of rsx_fuji_rotate.hip and by a host build (rsx_fuji_rotate_host.cpp):
// the rotated size (decoders/RafDecoder.cpp:233-244), the scatter's map (:257-263), its inverse for
// a gather, and the validation.  Plain integers.
//
// With W x H = new_size and (cx, cy) = crop_offset, src(cy + y, cx + x) goes to dst(h, w):
//   normal  R = W + H / 2   h = W - 1 - x + (y >> 1)           w = ((y + 1) >> 1) + x
//   alt     R = H + W / 2   h = R - (H + 1 - y + (x >> 1))     w = ((x + 1) >> 1) + y
// dst is R wide and R - 1 tall and zero where nothing lands.  Both maps are restrictions of a
// bijection of the integer plane:
//   normal  w + h = W - 1 + y,  w - h + W - 1 = 2 x + (y & 1)
//           -> y = w + h - (W - 1),  x = (w - h + W - 1) >> 1
//   alt     w - h = x - (W / 2 - 1)  (W even)
//           -> x = w - h + (W / 2 - 1),  y = w - ((x + 1) >> 1)
// so a destination sample is src at the inverse if that lies in [0, W) x [0, H), else 0.
// Where the scatter leaves the image (w < R always holds):
//   normal  h <= W - 1 + ((H - 1) >> 1): R - 2 for even H, but R - 1 = dim.y for odd H -- the
//           reference throws "Trying to write out of bounds" at (y = H - 1, x = 0)
//   alt     0 <= h <= R - 2 for even W; for odd W, (y = 0, x = W - 1) has h = -1, which the
//           reference's `h < dim.y` on signed ints lets through
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "rsx.h"

#if defined(__HIPCC__)
#define RSX_FR_FN __host__ __device__ __forceinline__
#else
#define RSX_FR_FN inline
#endif

namespace rsx_fujirot {

constexpr int32_t MAX_R = 65535; // RawImage::createData refuses a larger dimension

// rotatedsize
RSX_FR_FN int64_t rotated_size(int32_t W, int32_t H, int32_t alt) {
  return alt ? int64_t(H) + W / 2 : int64_t(W) + H / 2;
}

// the scatter: where (x, y) of the crop lands
RSX_FR_FN void forward(int32_t W, int32_t H, int32_t alt, int32_t x, int32_t y, int32_t* h,
                       int32_t* w) {
  if (alt) {
    const int32_t R = int32_t(rotated_size(W, H, 1));
    *h = R - (H + 1 - y + (x >> 1));
    *w = ((x + 1) >> 1) + y;
  } else {
    *h = W - 1 - x + (y >> 1);
    *w = ((y + 1) >> 1) + x;
  }
}

// the gather: which (x, y) lands on (h, w); any integers come back, the caller asks `inside`
RSX_FR_FN void inverse(int32_t W, int32_t alt, int32_t h, int32_t w, int32_t* x, int32_t* y) {
  if (alt) {
    *x = w - h + (W / 2 - 1);
    *y = w - ((*x + 1) >> 1);
  } else {
    *y = w + h - (W - 1);
    *x = (w - h + W - 1) >> 1;
  }
}

RSX_FR_FN bool inside(int32_t W, int32_t H, int32_t x, int32_t y) {
  return x >= 0 && x < W && y >= 0 && y < H;
}

// the descriptor's own checks, in the order of validate() below
inline int check_desc(const rsx_raf_rotate_desc* d) {
  if (d->size_x < 1 || d->size_y < 1)
    return RSX_ERR_INVALID_ARG;
  if (d->crop_x < 0 || d->crop_y < 0)
    return RSX_ERR_INVALID_ARG;
  return RSX_OK;
}
inline int check_size(const rsx_raf_rotate_desc* d) {
  const int64_t R = rotated_size(d->size_x, d->size_y, d->alt_layout);
  return R < 2 || R > MAX_R ? RSX_ERR_INVALID_ARG : RSX_OK;
}
// what the reference's loop does not survive
inline int check_layout(const rsx_raf_rotate_desc* d) {
  if (!d->alt_layout && d->size_y % 2 != 0)
    return RSX_ERR_INVALID_ARG; // "Trying to write out of bounds"
  if (d->alt_layout && d->size_x % 2 != 0)
    return RSX_ERR_UNSUPPORTED; // a write to row -1
  return RSX_OK;
}

inline int geometry(const rsx_raf_rotate_desc* d, int32_t* out_dim_x, int32_t* out_dim_y,
                    int32_t* rotation_pos) {
  if (!d)
    return RSX_ERR_INVALID_ARG;
  int st;
  if ((st = check_desc(d)) || (st = check_size(d)) || (st = check_layout(d)))
    return st;
  const int32_t R = int32_t(rotated_size(d->size_x, d->size_y, d->alt_layout));
  if (out_dim_x)
    *out_dim_x = R;
  if (out_dim_y)
    *out_dim_y = R - 1;
  if (rotation_pos)
    *rotation_pos = d->alt_layout ? d->size_x / 2 - 1 : d->size_x - 1;
  return RSX_OK;
}

// the bytes of an image its rows cover
inline uint64_t image_span(const rsx_image* img) {
  return uint64_t(img->pitch_bytes) * uint64_t(img->dim_y - 1) + 2ull * uint64_t(img->dim_x);
}

inline int validate(const rsx_raf_rotate_desc* d, const rsx_image* src, const rsx_image* dst) {
  if (!d || !src || !dst)
    return RSX_ERR_INVALID_ARG;
  if (src->cpp != 1 || dst->cpp != 1)
    return RSX_ERR_INVALID_ARG;
  if (src->dim_x <= 0 || src->dim_y <= 0 || dst->dim_x <= 0 || dst->dim_y <= 0)
    return RSX_ERR_INVALID_ARG;
  if (src->pitch_bytes < 2u * uint32_t(src->dim_x) || src->pitch_bytes % 2u != 0 ||
      dst->pitch_bytes < 2u * uint32_t(dst->dim_x) || dst->pitch_bytes % 2u != 0)
    return RSX_ERR_INVALID_ARG;
  if (int st = check_desc(d))
    return st;
  // (the reference would read outside its image)
  if (int64_t(d->crop_x) + d->size_x > src->dim_x || int64_t(d->crop_y) + d->size_y > src->dim_y)
    return RSX_ERR_INVALID_ARG;
  if (int st = check_size(d))
    return st;
  const int32_t R = int32_t(rotated_size(d->size_x, d->size_y, d->alt_layout));
  if (dst->dim_x != R || dst->dim_y != R - 1)
    return RSX_ERR_INVALID_ARG;
  if (src->data && dst->data) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(src->data);
    const uintptr_t b = reinterpret_cast<uintptr_t>(dst->data);
    if (a < b + image_span(dst) && b < a + image_span(src))
      return RSX_ERR_INVALID_ARG;
  }
  return check_layout(d);
}

// One destination sample: the whole of the gather.
RSX_FR_FN uint16_t gather(const uint8_t* src, uint32_t src_pitch, int32_t cx, int32_t cy, int32_t W,
                          int32_t H, int32_t alt, int32_t h, int32_t w) {
  int32_t x, y;
  inverse(W, alt, h, w, &x, &y);
  if (!inside(W, H, x, y))
    return 0;
  const uint8_t* p = src + size_t(cy + y) * src_pitch + 2u * size_t(cx + x);
  return *reinterpret_cast<const uint16_t*>(p);
}

} // namespace rsx_fujirot
