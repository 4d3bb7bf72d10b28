// rsx_scale_core.h as host C++ (librsx_scale_host.so): the same validation, level resolution and
// per-sample arithmetic as the kernels of rsx_scale.hip, driven by plain loops -- the estimate, the
// area histograms with 32-bit counters truncated in front of the median walk, resolve(), then the
// pass of the variant resolve() chose -- so that the test cases meet the code on the CPU first.
// The plain variant's rows start every run of eight samples from a generator JUMP, as the lanes
// do.  Compiled with -ffp-contract=off.  With -DRSX_SCALE_HOST_MAIN the file is a program (built
// with AddressSanitizer and UBSan where g++ has them) that runs built-in cases, and the case file
// a test hands it.
#include "rsx_scale_core.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace rsx_sc;

extern "C" int rsx_scale_host_validate(const rsx_scale_desc* desc, const rsx_image* img) {
  return validate(desc, img);
}

// the generator's state n steps behind `seed`: by the jump the lanes use, and step by step
extern "C" uint32_t rsx_scale_host_jump(uint32_t seed, uint32_t n) {
  if (n < Gen::SETTLE) {
    for (uint32_t i = 0; i < n; ++i)
      seed = Gen::step(seed);
    return seed;
  }
  return Gen::jump_settled(seed, Gen::powers(n - Gen::SETTLE, 2)[1]);
}
extern "C" uint32_t rsx_scale_host_steps(uint32_t seed, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i)
    seed = Gen::step(seed);
  return seed;
}

namespace {

template <typename T>
T& at(uint8_t* data, const Job& J, int64_t row, int64_t sample) {
  return *reinterpret_cast<T*>(data + size_t(row) * J.pitch + size_t(sample) * sizeof(T));
}

void estimate(const Job& J, uint8_t* data, Acc* A) {
  for (int64_t r = J.er0; r < J.er1; ++r)
    for (int64_t c = J.ec0; c < J.ec1; ++c) {
      const int64_t row = J.off_y + r, s = int64_t(J.off_x) * J.cpp + c;
      if (J.is_f32) {
        const uint32_t bits = at<uint32_t>(data, J, row, s);
        if ((bits & 0x7FFFFFFFu) > 0x7F800000u)
          A->nan = 1;
        else if (f_key(bits) < A->fmin_key)
          A->fmin_key = f_key(bits);
      } else {
        const int32_t p = at<uint16_t>(data, J, row, s);
        A->mn = p < A->mn ? p : A->mn;
        A->mx = p > A->mx ? p : A->mx;
      }
    }
}

void areas(const Job& J, const rsx_scale_area* list, uint8_t* data, uint32_t* hist) {
  for (uint32_t i = 0; i < J.n_areas; ++i) {
    const uint32_t off = list[i].offset, size = list[i].size - (list[i].size & 1u);
    if (!list[i].is_vertical) {
      for (uint32_t y = off; y < off + size; ++y)
        for (int x = J.off_x; x < J.crop_x + J.off_x; ++x)
          ++hist[(2u * (y & 1u) + (uint32_t(x) & 1u)) * 65536u + at<uint16_t>(data, J, y, J.off_x)];
    } else {
      for (int y = J.off_y; y < J.crop_y + J.off_y; ++y)
        for (uint32_t x = off; x < off + size; ++x)
          ++hist[(2u * (uint32_t(y) & 1u) + (x & 1u)) * 65536u + at<uint16_t>(data, J, y, off)];
    }
  }
}

void pass(const Job& J, const Rec& R, uint8_t* data, uint64_t* n_wrapped) {
  const int64_t gw = int64_t(J.crop_x) * J.cpp, s0 = int64_t(J.off_x) * J.cpp;
  if (R.variant == VARIANT_F32) {
    for (int y = 0; y < J.crop_y; ++y)
      for (int64_t x = 0; x < gw; ++x) {
        float& p = at<float>(data, J, J.off_y + y, s0 + x);
        p = f32_sample(R, p, 2u * (uint32_t(y) & 1u) + (uint32_t(x) & 1u));
      }
    return;
  }
  if (R.variant == VARIANT_SSE2) {
    for (int y = 0; y < J.crop_y; ++y) {
      uint32_t s[8];
      for (uint32_t g = 0; g < 8; ++g)
        s[g] = J.dither ? sse2_seed(J, uint32_t(y), g) : 0u;
      const uint32_t row = uint32_t(y + J.off_y) & 1u;
      for (uint32_t b = 0; b < J.n_blocks; ++b)
        for (uint32_t j = 0; j < 8; ++j) {
          if (J.dither)
            s[j] = sse2_step(s[j], j);
          uint16_t& p = at<uint16_t>(data, J, J.off_y + y, 8u * b + j);
          p = sse2_pixel(R, row, j, p, s[j]);
        }
    }
    return;
  }
  const std::vector<uint32_t> pw = Gen::powers(1, uint32_t(gw) + 1u);
  for (int y = 0; y < J.crop_y; ++y) {
    const uint32_t seed = plain_seed(J, uint32_t(y));
    for (int64_t x0 = 0; x0 < gw; x0 += 8) {
      uint32_t v = x0 == 0 ? seed : Gen::jump_settled(seed, pw[size_t(x0) - Gen::SETTLE]);
      for (int64_t x = x0; x < x0 + 8 && x < gw; ++x) {
        int32_t rnd = 0;
        if (J.dither) {
          v = Gen::step(v);
          rnd = plain_rand(R, v);
        }
        bool wrapped;
        uint16_t& p = at<uint16_t>(data, J, J.off_y + y, s0 + x);
        const uint32_t par = 2u * (uint32_t(y) & 1u) + (uint32_t(x) & 1u);
        p = plain_sample(R.sub[par], R.mul[par], p, rnd, &wrapped);
        *n_wrapped += wrapped ? 1u : 0u;
      }
    }
  }
}

} // namespace

// rsx_scale_black_white on the host: img->data in place (untouched unless RSX_OK)
extern "C" int rsx_scale_host_black_white(const rsx_scale_desc* desc, const rsx_image* img,
                                          rsx_scale_result* result) {
  if (result)
    std::memset(result, 0, sizeof *result);
  if (int st = validate(desc, img))
    return st;
  if (!img->data)
    return RSX_ERR_INVALID_ARG;
  const Job J = make_job(desc, img);
  uint8_t* data = static_cast<uint8_t*>(img->data);
  Acc A;
  acc_init(&A);
  if (J.need_estimate)
    estimate(J, data, &A);
  int32_t med[4] = {0, 0, 0, 0};
  if (J.use_areas && J.n_areas != 0 && J.totalpixels != 0) {
    std::vector<uint32_t> hist(HIST_CELLS, 0u);
    areas(J, desc->areas, data, hist.data());
    for (int i = 0; i < 4; ++i)
      med[i] = median_walk(hist.data() + size_t(i) * 65536u, J.totalpixels / 8);
  }
  Rec R;
  resolve(J, A, med, &R);
  if (R.status)
    return R.status;
  uint64_t n_wrapped = 0;
  if (!R.skipped)
    pass(J, R, data, &n_wrapped);
  if (result) {
    result->black_level = R.black_level;
    result->white_point = R.white_point;
    for (int i = 0; i < 4; ++i)
      result->black_separate[i] = R.bs[i];
    result->estimated = R.estimated;
    result->skipped = R.skipped;
    result->variant = R.variant;
    result->n_wrapped = n_wrapped;
  }
  return RSX_OK;
}

#ifdef RSX_SCALE_HOST_MAIN
namespace {

uint32_t rng_state = 2463534242u;
uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

int fails = 0;
void expect(bool ok, const char* what, int id) {
  if (!ok) {
    std::fprintf(stderr, "FAILED: %s (case %d)\n", what, id);
    ++fails;
  }
}

bool rd(std::FILE* f, void* p, size_t n) { return std::fread(p, 1, n, f) == n; }

// the case file of tests/scale_files.py: uint32 count, then per case a 64-byte name, int32 w, h,
// cpp, pitch, cfa, then the descriptor's int32 scalars off_x, off_y, crop_x, crop_y, is_f32,
// black_level, has_white, white_point, has_separate, black_separate[4], dither, host_sse2,
// n_areas, the expected status; the areas (offset, size, is_vertical, 0); the image; the expected
// image
int run_file(const char* path) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f)
    return 2;
  uint32_t n = 0;
  if (!rd(f, &n, 4))
    return 2;
  for (uint32_t c = 0; c < n; ++c) {
    char name[64];
    int32_t hd[22];
    if (!rd(f, name, sizeof name) || !rd(f, hd, sizeof hd))
      return 2;
    std::vector<rsx_scale_area> ar{size_t(hd[20]), rsx_scale_area()};
    std::vector<uint8_t> image(size_t(hd[3]) * size_t(hd[1])), want(image.size());
    if ((!ar.empty() && !rd(f, ar.data(), ar.size() * sizeof(rsx_scale_area))) ||
        !rd(f, image.data(), image.size()) || !rd(f, want.data(), want.size()))
      return 2;
    rsx_scale_desc d;
    std::memset(&d, 0, sizeof d);
    d.off_x = hd[5];
    d.off_y = hd[6];
    d.crop_x = hd[7];
    d.crop_y = hd[8];
    d.is_f32 = hd[9];
    d.black_level = hd[10];
    d.has_white = hd[11];
    d.white_point = hd[12];
    d.has_separate = hd[13];
    for (int i = 0; i < 4; ++i)
      d.black_separate[i] = hd[14 + i];
    d.dither = hd[18];
    d.host_sse2 = hd[19];
    d.n_areas = uint32_t(hd[20]);
    d.areas = ar.empty() ? nullptr : ar.data();
    rsx_image img{image.data(), uint32_t(hd[3]), hd[0], hd[1], hd[2], hd[4]};
    rsx_scale_result r;
    expect(rsx_scale_host_black_white(&d, &img, &r) == hd[21], "status against the case file", int(c));
    expect(image == want, "image against the case file", int(c));
  }
  std::fclose(f);
  std::printf("%u file cases\n", n);
  return 0;
}

} // namespace

int main(int argc, char** argv) {
  if (argc > 1)
    if (int e = run_file(argv[1]))
      return e;
  // the jump against the steps: the seeds around the modulus, the largest, and random ones
  const uint32_t m = uint32_t(Gen::MOD);
  std::vector<uint32_t> seeds = {0u, 1u, m - 1u, m, m + 1u, 0x7FFFFFFFu, 0x7FFFFFFEu};
  for (int i = 0; i < 200; ++i)
    seeds.push_back(rnd() << 7 & 0x7FFFFFFFu);
  for (uint32_t s : seeds)
    for (uint32_t n : {0u, 1u, 2u, 3u, 8u, 4093u, 196608u})
      expect(rsx_scale_host_jump(s, n) == rsx_scale_host_steps(s, n), "jump", int(n));
  // random images through every variant: nothing outside the pass's samples is written, and a
  // second run of the same call gives the same image (no state is kept)
  int id = 1000;
  for (int f32 = 0; f32 < 2; ++f32)
    for (int sse2 = 0; sse2 < 2; ++sse2)
      for (int dither = 0; dither < 2; ++dither)
        for (int cpp = 1; cpp <= 3; cpp += 2, ++id) {
          const int w = 37, h = 7, ss = f32 ? 4 : 2, pitch = (w * cpp + 3) * ss;
          std::vector<uint8_t> image(size_t(pitch) * h);
          for (uint8_t& b : image)
            b = uint8_t(rnd());
          if (f32)
            for (size_t i = 0; i < image.size(); i += 4) {
              const float v = float(rnd() % 70000u) / 3.0F;
              std::memcpy(&image[i], &v, 4);
            }
          rsx_scale_desc d;
          std::memset(&d, 0, sizeof d);
          d.off_x = 3;
          d.off_y = 1;
          d.crop_x = 30;
          d.crop_y = 5;
          d.is_f32 = f32;
          d.black_level = 100;
          d.has_white = 1;
          d.white_point = 16000;
          d.has_separate = 1;
          d.black_separate[0] = 90;
          d.black_separate[1] = 110;
          d.black_separate[2] = 15990;
          d.black_separate[3] = 4000;
          d.dither = dither;
          d.host_sse2 = sse2;
          std::vector<uint8_t> a = image, b = image;
          rsx_image ia{a.data(), uint32_t(pitch), w, h, cpp, 1}, ib{b.data(), uint32_t(pitch), w, h, cpp, 1};
          rsx_scale_result ra, rb;
          expect(rsx_scale_host_black_white(&d, &ia, &ra) == RSX_OK, "status", id);
          expect(rsx_scale_host_black_white(&d, &ib, &rb) == RSX_OK, "status", id);
          expect(a == b, "two runs agree", id);
          expect(ra.variant == (f32 ? 2 : sse2 ? 1 : 0), "variant", id);
          const bool wide = ra.variant == 1; // (the SSE2 variant covers uncropped samples 0 .. 32)
          for (int y = 0; y < h; ++y)
            for (int s = 0; s < pitch / ss; ++s) {
              const bool row_in = y >= 1 && y < 6;
              const bool in = row_in && (wide ? s < 32 : (s >= 3 * cpp && s < 33 * cpp));
              if (!in)
                expect(std::memcmp(&a[size_t(y) * pitch + size_t(s) * ss],
                                   &image[size_t(y) * pitch + size_t(s) * ss], size_t(ss)) == 0,
                       "untouched outside", id);
            }
        }
  // the verdicts leave the image alone
  {
    std::vector<uint16_t> px(40 * 4, 7);
    rsx_image img{px.data(), 80, 40, 4, 1, 1};
    rsx_scale_desc d;
    std::memset(&d, 0, sizeof d);
    d.crop_x = 40;
    d.crop_y = 4;
    d.black_level = 10;
    d.has_white = 1;
    d.white_point = 10;
    expect(rsx_scale_host_black_white(&d, &img, nullptr) == RSX_ERR_UNSUPPORTED, "white == black", 0);
    d.white_point = 1000;
    d.crop_x = 41;
    expect(rsx_scale_host_black_white(&d, &img, nullptr) == RSX_ERR_INVALID_ARG, "crop outside", 0);
    d.crop_x = 40;
    const rsx_scale_area past{3, 2, 0, 0};
    d.areas = &past;
    d.n_areas = 1;
    expect(rsx_scale_host_black_white(&d, &img, nullptr) == RSX_ERR_INVALID_ARG, "area past", 0);
    for (uint16_t v : px)
      expect(v == 7, "untouched", 0);
  }
  if (fails)
    return 1;
  std::puts("rsx_scale_host_check OK");
  return 0;
}
#endif
