// extendBinaryFloatingPoint<Narrow, Binary32> (common/FloatingPoint.h:109-145) in integer
// arithmetic: exact, subnormals renormalised, NaN payload kept.  Shared by the F32 unpack kernels
// (rsx_unpack.hip) and the deflate DNG row kernel (rsx_dng_deflate.hip).
#pragma once
#include <stdint.h>

template <int FRAC, int EXPW>
__device__ __forceinline__ uint32_t widen_fp(uint32_t narrow) {
  constexpr int BIAS = (1 << (EXPW - 1)) - 1;
  const uint32_t sign = (narrow >> (FRAC + EXPW)) & 1u;
  const uint32_t ne = (narrow >> FRAC) & ((1u << EXPW) - 1u);
  const uint32_t nf = narrow & ((1u << FRAC) - 1u);
  uint32_t we = ne - BIAS + 127;
  uint32_t wf = nf << (23 - FRAC);
  if (ne == (1u << EXPW) - 1u) {
    we = 255; // infinity / NaN, fraction widened
  } else if (ne == 0) {
    if (nf == 0) {
      we = 0;
      wf = 0;
    } else {
      // subnormal: normalise (shift until the hidden bit appears)
      const uint32_t sh = uint32_t(__builtin_clz(wf)) - 8u; // wf < 2^23
      we = 1 - BIAS + 127 - sh;
      wf = (wf << sh) & 0x7FFFFFu;
    }
  }
  return (sign << 31) | (we << 23) | wf;
}
