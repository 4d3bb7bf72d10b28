// What the kernels that store through the dithering TableLookUp share (rsx_sony_arw2.hip,
// rsx_nikon_snef.hip): RawImageDataU16::setWithLookUp (common/RawImage.h:335-353) looks a value
// up as base + ((delta (r & 2047) + 1024) >> 12) mod 2^16 and then steps its generator
// r' = 15700 (r & 65535) + (r >> 16).  That is a lag-1 multiply-with-carry: r_n = r_0 15700^n
// mod m, m = 15700 * 2^16 - 1, for seeds r_0 < m (rsx_ljpeg_recon.hip has the argument;
// tests/test_dither_jump_model.py checks it; the seeds are 24 bits, and 0 stays 0), so the state
// in front of a lane's first sample is one multiplication mod m away from the row's seed.
// Device code: included by those two sources only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

namespace rsx {

namespace {

constexpr uint64_t DITHER_MOD = 15700ull * 65536ull - 1ull; // the generator's modulus

// the state `n` steps behind `seed`, pw = 15700^n mod m (dither_powers)
__device__ __forceinline__ uint32_t dither_jump(uint32_t seed, uint32_t pw) {
  return uint32_t((uint64_t(seed) * pw) % DITHER_MOD);
}

// one look-up through a table entry e = base | delta << 16, and the generator's step
__device__ __forceinline__ uint32_t dither_lookup(uint32_t e, uint32_t& r) {
  const uint32_t v = ((e & 0xFFFFu) + (((e >> 16) * (r & 2047u) + 1024u) >> 12)) & 0xFFFFu;
  r = 15700u * (r & 65535u) + (r >> 16);
  return v;
}

// [k] = 15700^(stride k) mod m, k < n
inline std::vector<uint32_t> dither_powers(uint32_t stride, uint32_t n) {
  std::vector<uint32_t> p(n);
  uint64_t step = 1;
  for (uint32_t i = 0; i < stride; ++i)
    step = step * 15700u % DITHER_MOD;
  uint64_t x = 1;
  for (uint32_t k = 0; k < n; ++k) {
    p[k] = uint32_t(x);
    x = x * step % DITHER_MOD;
  }
  return p;
}

} // namespace

} // namespace rsx
