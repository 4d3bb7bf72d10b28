// What the kernels that store through the dithering TableLookUp share (rsx_sony_arw2.hip,
// rsx_nikon_snef.hip): RawImageDataU16::setWithLookUp (common/RawImage.h:335-353) looks a value
// up as base + ((delta (r & 2047) + 1024) >> 12) mod 2^16 and then steps its generator
// r' = 15700 (r & 65535) + (r >> 16).  That is a lag-1 multiply-with-carry: r_n = r_0 15700^n
// mod m, m = 15700 * 2^16 - 1, for seeds r_0 < m (rsx_ljpeg_recon.hip has the argument;
// tests/test_dither_jump_model.py checks it; the seeds are 24 bits, and 0 stays 0), so the state
// in front of a lane's first sample is one multiplication mod m away from the row's seed.
//
// The generator with any multiplier A is Mwc<A>: 2^16 r' = (m + 1) lo + 2^16 hi = r (mod m), and
// A 2^16 = 1 (mod m), so r' = A r (mod m); a state <= m steps to a state <= m, and only m itself
// (= 0 mod m, a fixed point like 0) steps to m.  RawImageDataU16::scaleValues_plain runs A = 18000
// (rsx_scale_core.h), whose seeds are not all below m: Mwc<A>::jump_settled.
// The dither_* functions are device code: included by the two sources above; Mwc also builds as
// host C++.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RSX_MWC_FN __host__ __device__ __forceinline__
#else
#define RSX_MWC_FN inline
#endif

#include <cstdint>
#include <vector>

namespace rsx {

namespace {

template <uint32_t A>
struct Mwc {
  static constexpr uint64_t MOD = uint64_t(A) * 65536ull - 1ull; // the generator's modulus
  static RSX_MWC_FN uint32_t step(uint32_t r) { return A * (r & 65535u) + (r >> 16); }
  // the state `n` steps behind `seed` < MOD, pw = A^n mod m (powers)
  static RSX_MWC_FN uint32_t jump(uint32_t seed, uint32_t pw) {
    return uint32_t((uint64_t(seed) * pw) % MOD);
  }
  // A seed of 31 bits that is not MOD itself is below MOD after SETTLE steps, and MOD stays MOD
  // (scripts/scale_seed_settle.cpp runs every such seed): the state n >= SETTLE steps behind ANY
  // seed < 2^31, pw = A^(n - SETTLE) mod m.
  static constexpr uint32_t SETTLE = 2;
  static RSX_MWC_FN uint32_t jump_settled(uint32_t seed, uint32_t pw) {
    const uint32_t s = step(step(seed));
    return uint64_t(s) == MOD ? s : jump(s, pw);
  }
  // [k] = A^(stride k) mod m, k < n
  static inline std::vector<uint32_t> powers(uint32_t stride, uint32_t n) {
    std::vector<uint32_t> p(n);
    uint64_t st = 1;
    for (uint32_t i = 0; i < stride; ++i)
      st = st * A % MOD;
    uint64_t x = 1;
    for (uint32_t k = 0; k < n; ++k) {
      p[k] = uint32_t(x);
      x = x * st % MOD;
    }
    return p;
  }
};

constexpr uint64_t DITHER_MOD = Mwc<15700>::MOD;

#if defined(__HIPCC__)
// the state `n` steps behind `seed`, pw = 15700^n mod m (dither_powers)
__device__ __forceinline__ uint32_t dither_jump(uint32_t seed, uint32_t pw) {
  return Mwc<15700>::jump(seed, pw);
}

// one look-up through a table entry e = base | delta << 16, and the generator's step
__device__ __forceinline__ uint32_t dither_lookup(uint32_t e, uint32_t& r) {
  const uint32_t v = ((e & 0xFFFFu) + (((e >> 16) * (r & 2047u) + 1024u) >> 12)) & 0xFFFFu;
  r = Mwc<15700>::step(r);
  return v;
}
#endif

// [k] = 15700^(stride k) mod m, k < n
inline std::vector<uint32_t> dither_powers(uint32_t stride, uint32_t n) {
  return Mwc<15700>::powers(stride, n);
}

} // namespace

} // namespace rsx
