// RawImageData::scaleBlackWhite (include/rsx.h section 6), shared by the kernels of rsx_scale.hip
// and by a host build (rsx_scale_host.cpp): the validation of a call, what follows the reductions
// (the estimate's use, the skip rule, the levels, the refusals, the variant and its constants) and
// the arithmetic of one sample of each variant (common/RawImageDataU16.cpp:60-392,
// common/RawImageDataFloat.cpp:51-170).
//
// Everything is as the reference's code is written.  The integer variants wrap where the
// reference's int arithmetic would overflow (x86-64 wraps; plain_sample says when it did).  In
// binary32 every operation is rounded on its own: this header turns contraction off for the
// translation unit that includes it, the host build is compiled with -ffp-contract=off; division
// is the correctly rounded one on both.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "rsx.h"
#include "rsx_dither_dev.h"

#if defined(__HIPCC__)
#define RSX_SC_FN __host__ __device__ __forceinline__
#else
#define RSX_SC_FN inline
#endif

namespace rsx_sc {

#if defined(__HIPCC__)
#pragma clang fp contract(off)
#endif
RSX_SC_FN float f_sub(float a, float b) { return a - b; }
RSX_SC_FN float f_mul(float a, float b) { return a * b; }
RSX_SC_FN float f_div(float a, float b) { return a / b; }

constexpr int32_t MAX_DIM = 65536, MAX_CPP = 4;
constexpr int VARIANT_PLAIN = 0, VARIANT_SSE2 = 1, VARIANT_F32 = 2;
constexpr uint32_t HIST_CELLS = 4u * 65536u;
// the eight 16-bit generators of the SSE2 variant leave a checkpoint every CHK_BLOCKS blocks
constexpr uint32_t CHK_BLOCKS = 8;

typedef rsx::Mwc<18000> Gen; // scaleValues_plain's generator

// One image of a call or a plan as the lanes see it: the descriptor's scalars and what follows
// from them alone.
struct Job {
  uint64_t img_offset;
  uint64_t hist_off; // the job's 4 x 65536 counters (use_areas)
  uint64_t chk_off;  // the job's checkpoints: crop_y rows of n_chk x 8 states (may_sse2_dither)
  uint32_t pitch;
  int32_t dim_x, dim_y, cpp, is_cfa;
  int32_t off_x, off_y, crop_x, crop_y;
  int32_t is_f32, black_level, has_white, white_point, has_separate;
  int32_t bs[4];
  int32_t dither, host_sse2;
  uint32_t n_areas, area_first; // its areas in the plan's list
  int32_t totalpixels;          // calculateBlackAreas' count in front of its division
  uint32_t need_estimate, use_areas, empty_crop, may_sse2_dither;
  uint32_t n_blocks, n_chk;     // SSE2: blocks of 8 a row, checkpoints a row
  // the estimate's window: cropped rows [er0, er1), cropped samples [ec0, ec1)
  int32_t er0, er1, ec0, ec1;
};

// what the reductions leave
struct Acc {
  int32_t mn, mx;     // uint16 estimate
  uint32_t fmin_key;  // F32 estimate: f_key of the minimum
  uint32_t nan;       // ... a NaN in the window
  unsigned long long n_wrapped;
};

// the levels and the pass's constants
struct Rec {
  int32_t status;
  int32_t black_level, white_point, bs[4];
  int32_t estimated, skipped, variant;
  int32_t mul[4], sub[4]; // plain, by cropped parity 2 (y & 1) + (x & 1)
  float fmul[4], fsub[4]; // F32
  int32_t full_scale_fp, half_scale_fp;
  uint32_t sse_sub[2], sse_mul[2]; // SSE2, by uncropped row parity: two 16-bit lanes a word
  uint32_t sse_fs[2];              // full_scale_fp of an even and an odd 16-bit lane
  uint32_t sse_round;              // 512 + (half_scale_fp >> 4)
};

// a monotonic key of a binary32 that is no NaN
RSX_SC_FN uint32_t f_key(uint32_t bits) { return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
RSX_SC_FN uint32_t f_unkey(uint32_t key) { return key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu); }
RSX_SC_FN uint32_t f_bits(float f) {
  union { float f; uint32_t u; } c;
  c.f = f;
  return c.u;
}
RSX_SC_FN float f_from(uint32_t u) {
  union { float f; uint32_t u; } c;
  c.u = u;
  return c.f;
}

RSX_SC_FN void acc_init(Acc* a) {
  a->mn = 65536;
  a->mx = 0;
  a->fmin_key = f_key(f_bits(100000000.0F));
  a->nan = 0;
  a->n_wrapped = 0;
}

// rsx_scale_validate: the order is the header's
inline int validate(const rsx_scale_desc* d, const rsx_image* img) {
  if (!d || !img || (d->n_areas != 0 && !d->areas))
    return RSX_ERR_INVALID_ARG;
  const uint32_t ss = d->is_f32 ? 4u : 2u;
  if (img->cpp < 1 || img->dim_x <= 0 || img->dim_y <= 0)
    return RSX_ERR_INVALID_ARG;
  if (uint64_t(img->pitch_bytes) < uint64_t(img->dim_x) * uint64_t(img->cpp) * ss ||
      img->pitch_bytes % ss != 0)
    return RSX_ERR_INVALID_ARG;
  if (d->off_x < 0 || d->off_y < 0 || d->crop_x < 0 || d->crop_y < 0 ||
      int64_t(d->off_x) + d->crop_x > img->dim_x || int64_t(d->off_y) + d->crop_y > img->dim_y)
    return RSX_ERR_INVALID_ARG;
  if (img->dim_x > MAX_DIM || img->dim_y > MAX_DIM || img->cpp > MAX_CPP)
    return RSX_ERR_UNSUPPORTED;
  if (d->is_f32) {
    if (!d->has_white || d->n_areas != 0)
      return RSX_ERR_UNSUPPORTED;
    return RSX_OK;
  }
  if (!d->has_separate && d->crop_x != 0 && d->crop_y != 0)
    for (uint32_t i = 0; i < d->n_areas; ++i) {
      const rsx_scale_area& a = d->areas[i];
      const uint32_t size = a.size - (a.size & 1u);
      // (static_cast<int>(offset) + static_cast<int>(size) > the dimension, RawImageDataU16.cpp:81,97)
      const int64_t end = int64_t(int32_t(a.offset)) + int64_t(int32_t(size));
      if (int32_t(a.offset) < 0 || int32_t(size) < 0 || end > (a.is_vertical ? img->dim_x : img->dim_y))
        return RSX_ERR_INVALID_ARG;
    }
  return RSX_OK;
}

// a validated call's job
inline Job make_job(const rsx_scale_desc* d, const rsx_image* img) {
  Job J = Job();
  J.pitch = img->pitch_bytes;
  J.dim_x = img->dim_x;
  J.dim_y = img->dim_y;
  J.cpp = img->cpp;
  J.is_cfa = img->is_cfa != 0;
  J.off_x = d->off_x;
  J.off_y = d->off_y;
  J.crop_x = d->crop_x;
  J.crop_y = d->crop_y;
  J.is_f32 = d->is_f32 != 0;
  J.black_level = d->black_level;
  J.has_white = d->has_white != 0;
  J.white_point = d->white_point;
  J.has_separate = d->has_separate != 0;
  for (int i = 0; i < 4; ++i)
    J.bs[i] = d->black_separate[i];
  J.dither = d->dither != 0;
  J.host_sse2 = d->host_sse2 != 0;
  J.n_areas = d->n_areas;
  J.empty_crop = (d->crop_x == 0 || d->crop_y == 0) ? 1u : 0u;
  const bool no_levels = d->n_areas == 0 && !J.has_separate && d->black_level < 0;
  if (J.is_f32) {
    J.need_estimate = no_levels ? 1u : 0u;
    J.er0 = 150 * J.cpp;
    J.er1 = J.crop_y - 150;
    J.ec0 = 150;
    J.ec1 = (J.crop_x - 150) * J.cpp;
  } else {
    J.need_estimate = (no_levels || !J.has_white) ? 1u : 0u;
    // img(row, skipBorder + col), col from skipBorder: the reference's double offset
    J.er0 = 250;
    J.er1 = J.crop_y - 250;
    J.ec0 = 500;
    J.ec1 = (J.crop_x - 250) * J.cpp + 250;
    J.use_areas = (!J.has_separate && !J.empty_crop) ? 1u : 0u;
    uint32_t total = 0;
    if (J.use_areas)
      for (uint32_t i = 0; i < d->n_areas; ++i) {
        const uint32_t size = d->areas[i].size - (d->areas[i].size & 1u);
        total += size * uint32_t(d->areas[i].is_vertical ? J.crop_y : J.crop_x);
      }
    J.totalpixels = int32_t(total);
    J.may_sse2_dither = (J.dither && J.host_sse2) ? 1u : 0u;
    J.n_blocks = uint32_t(J.dim_x) / 8u;
    J.n_chk = (J.n_blocks + CHK_BLOCKS - 1u) / CHK_BLOCKS;
  }
  return J;
}

// the median walk of one histogram (RawImageDataU16.cpp:126-135): cells of 16 bits
inline int32_t median_walk(const uint32_t* hist, int32_t total) {
  int acc = int(hist[0] & 0xFFFFu), v = 0;
  while (acc <= total && v < 65535) {
    ++v;
    acc += int(hist[v] & 0xFFFFu);
  }
  return v;
}

RSX_SC_FN bool fits_i32(int64_t v) { return v >= INT32_MIN && v <= INT32_MAX; }

// Everything between the reductions and the pass.  med: the four median walks (use_areas with
// totalpixels != 0).  R->status other than RSX_OK, or R->skipped: the pass does nothing.
RSX_SC_FN void resolve(const Job& J, const Acc& A, const int32_t* med, Rec* R) {
  *R = Rec();
  int32_t black = J.black_level, white = J.white_point;
  bool has_white = J.has_white != 0;
  if (J.need_estimate) {
    R->estimated = 1;
    if (J.is_f32) {
      if (A.nan) {
        R->status = RSX_ERR_UNSUPPORTED;
        return;
      }
      const float b = f_from(f_unkey(A.fmin_key));
      if (b < -2147483648.0F) {
        R->status = RSX_ERR_UNSUPPORTED;
        return;
      }
      if (black < 0)
        black = int32_t(b);
    } else {
      if (black < 0)
        black = A.mn;
      if (!has_white) {
        white = A.mx;
        has_white = true;
      }
    }
  }
  R->black_level = black;
  R->white_point = white;
  for (int i = 0; i < 4; ++i)
    R->bs[i] = J.has_separate ? J.bs[i] : 0;
  if (!J.is_f32 &&
      ((J.n_areas == 0 && black == 0 && white == 65535 && !J.has_separate) || J.empty_crop)) {
    R->skipped = 1;
    return;
  }
  if (!J.has_separate) {
    if (J.is_f32 || J.totalpixels == 0) {
      for (int i = 0; i < 4; ++i)
        R->bs[i] = black;
    } else {
      int32_t total = 0;
      for (int i = 0; i < 4; ++i) {
        R->bs[i] = med[i];
        total += med[i];
      }
      if (!J.is_cfa)
        for (int i = 0; i < 4; ++i)
          R->bs[i] = (total + 2) >> 2;
    }
  }
  for (int i = 0; i < 4; ++i)
    if (int64_t d = int64_t(white) - R->bs[i]; d <= 0 || !fits_i32(d)) {
      R->status = RSX_ERR_UNSUPPORTED;
      return;
    }
  // sub[i], mul[i] of cropped parity i: the level of uncropped parity v
  const int flip = (J.off_x & 1) | ((J.off_y & 1) << 1);
  if (J.is_f32) {
    R->variant = VARIANT_F32;
    for (int i = 0; i < 4; ++i) {
      R->fmul[i] = f_div(65535.0F, float(white - R->bs[i ^ flip]));
      R->fsub[i] = float(R->bs[i ^ flip]);
    }
    return;
  }
  const float app_scale = f_div(65535.0F, float(white - R->bs[0]));
  R->full_scale_fp = int32_t(f_mul(app_scale, 4.0F));
  R->half_scale_fp = int32_t(f_mul(app_scale, 4095.0F));
  if (J.host_sse2 && app_scale < 63.0F) {
    R->variant = VARIANT_SSE2;
    for (int r = 0; r < 2; ++r) {
      const int32_t b0 = R->bs[2 * r + (J.off_x & 1)], b1 = R->bs[2 * r + ((J.off_x + 1) & 1)];
      const int32_t m0 = int32_t(f_div(f_mul(1024.0F, 65535.0F), float(white - b0)));
      const int32_t m1 = int32_t(f_div(f_mul(1024.0F, 65535.0F), float(white - b1)));
      R->sse_sub[r] = uint32_t(b0) | (uint32_t(b1) << 16);
      R->sse_mul[r] = uint32_t(m0) | (uint32_t(m1) << 16);
    }
    const uint32_t fs = uint32_t(R->full_scale_fp) | (uint32_t(R->full_scale_fp) << 16);
    R->sse_fs[0] = fs & 0xFFFFu;
    R->sse_fs[1] = fs >> 16;
    R->sse_round = 512u + uint32_t(R->half_scale_fp >> 4);
    return;
  }
  R->variant = VARIANT_PLAIN;
  // the last row's seed crop_x + y 36969 as an int
  if (int64_t(J.crop_x) + int64_t(J.crop_y - 1) * 36969 > INT32_MAX) {
    R->status = RSX_ERR_UNSUPPORTED;
    return;
  }
  for (int i = 0; i < 4; ++i) {
    R->mul[i] = int32_t(f_div(f_mul(16384.0F, 65535.0F), float(white - R->bs[i ^ flip])));
    R->sub[i] = R->bs[i ^ flip];
  }
}

// ---- plain variant (RawImageDataU16.cpp:374-391) ----
RSX_SC_FN uint32_t plain_seed(const Job& J, uint32_t y) { return uint32_t(J.crop_x) + y * 36969u; }
// the dither term of a state that has been stepped for its sample
RSX_SC_FN int32_t plain_rand(const Rec& R, uint32_t v) {
  return int32_t(uint32_t(R.half_scale_fp) - uint32_t(R.full_scale_fp) * (v & 2047u));
}
// sub, mul: the sample's parity's.  *wrapped: the reference's int arithmetic left int32 on the way
// (undefined there).  The product is one 32 x 32 -> 64 multiplication: a difference that left
// int32 is wrapped first, and counted whatever the product does.
RSX_SC_FN uint16_t plain_sample(int32_t sub, int32_t mul, uint32_t p, int32_t rnd, bool* wrapped) {
  const int64_t d = int64_t(p) - sub, prod = int64_t(int32_t(uint32_t(uint64_t(d)))) * int64_t(mul);
  const int64_t t1 = int64_t(int32_t(uint32_t(uint64_t(prod)))) + 8192,
                t2 = int64_t(int32_t(uint32_t(uint64_t(t1)))) + rnd;
  *wrapped = !fits_i32(d) || !fits_i32(prod) || !fits_i32(t1) || !fits_i32(t2);
  const int32_t s = int32_t(uint32_t(t2)) >> 14;
  return uint16_t(s < 0 ? 0 : s > 65535 ? 65535 : s);
}

// ---- SSE2 variant (RawImageDataU16.cpp:277-340) ----
// generator g of 8 of cropped row y: a half of one of the four words of :281-282
RSX_SC_FN uint32_t sse2_seed(const Job& J, uint32_t y, uint32_t g) {
  const uint32_t cx = uint32_t(J.crop_x);
  const uint32_t a[4] = {1234u, 4272u, 2342u, 1676u}, b[4] = {23464u, 12123u, 34311u, 18000u};
  const uint32_t e = cx * a[g >> 1] + y * b[g >> 1];
  return (e >> (16u * (g & 1u))) & 0xFFFFu;
}
// s' = mulhi_epi16(s, c) ^ mullo_epi16(s, c)
RSX_SC_FN uint32_t sse2_step(uint32_t s, uint32_t g) {
  const int32_t c = (g & 1u) ? 0x4d9f : 0x1d32;
  const uint32_t prod = uint32_t(int32_t(int16_t(uint16_t(s))) * c);
  return ((prod >> 16) ^ prod) & 0xFFFFu;
}
// pixel j of 8 of a block of an uncropped row of parity `row`; s: generator j's state stepped for
// the block, or 0 without dither
RSX_SC_FN uint16_t sse2_pixel(const Rec& R, uint32_t row, uint32_t j, uint32_t p, uint32_t s) {
  const uint32_t sub = (R.sse_sub[row] >> (16u * (j & 1u))) & 0xFFFFu;
  const uint32_t mul = (R.sse_mul[row] >> (16u * (j & 1u))) & 0xFFFFu;
  const uint32_t d = p > sub ? p - sub : 0u;
  const uint32_t rnd = ((s & 0xFFu) * R.sse_fs[j & 1u]) & 0xFFFFu;
  int32_t t = int32_t(d * mul + R.sse_round - rnd) >> 10;
  t -= 32768;
  t = t < -32768 ? -32768 : t > 32767 ? 32767 : t;
  return uint16_t(uint32_t(t) ^ 0x8000u);
}

// ---- F32 (RawImageDataFloat.cpp:165-169) ----
RSX_SC_FN float f32_sample(const Rec& R, float p, uint32_t par) {
  return f_mul(f_sub(p, R.fsub[par]), R.fmul[par]);
}

} // namespace rsx_sc
