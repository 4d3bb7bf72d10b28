// The inverse of widen_fp<FRAC, EXPW> (rsx_fp_widen.h; extendBinaryFloatingPoint,
// common/FloatingPoint.h:109-145) in integer arithmetic, for the device and the host: binary32 ->
// binary16 (10, 5) or binary24 (16, 7).  narrow_fp is defined only where widen(narrow(x)) == x as
// 32-bit patterns; everything else is reported inexact.  No rounding mode and no clamping: the
// writers stand behind bit-exact decoders.  The rule is bitwise: -0, the infinities and NaN
// payloads (their low 23 - FRAC fraction bits must be zero) are covered; a binary32 normal that is
// a subnormal of the narrow format is exact iff the bits shifted out are zero; no binary32
// subnormal other than +-0 exists in either narrow format.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RSX_FPN_HD __host__ __device__ __forceinline__
#else
#define RSX_FPN_HD inline
#endif

// widen_fp's arithmetic without its clz, for host code (the exhaustive check of the host core)
template <int FRAC, int EXPW>
RSX_FPN_HD uint32_t widen_fp_plain(uint32_t narrow) {
  constexpr int BIAS = (1 << (EXPW - 1)) - 1;
  const uint32_t sign = (narrow >> (FRAC + EXPW)) & 1u;
  const uint32_t ne = (narrow >> FRAC) & ((1u << EXPW) - 1u);
  const uint32_t nf = narrow & ((1u << FRAC) - 1u);
  uint32_t we = ne - BIAS + 127;
  uint32_t wf = nf << (23 - FRAC);
  if (ne == (1u << EXPW) - 1u) {
    we = 255;
  } else if (ne == 0) {
    if (nf == 0) {
      we = 0;
    } else {
      we = 1 - BIAS + 127;
      while (!(wf & 0x800000u)) {
        wf <<= 1;
        --we;
      }
      wf &= 0x7FFFFFu;
    }
  }
  return (sign << 31) | (we << 23) | wf;
}

// true and *out = the narrow pattern iff x has one
template <int FRAC, int EXPW>
RSX_FPN_HD bool narrow_fp(uint32_t x, uint32_t* out) {
  constexpr int BIAS = (1 << (EXPW - 1)) - 1;
  constexpr uint32_t EMAX = (1u << EXPW) - 1u;
  constexpr int SH = 23 - FRAC;
  const uint32_t sign = (x >> 31) << (FRAC + EXPW);
  const uint32_t we = (x >> 23) & 0xFFu;
  const uint32_t wf = x & 0x7FFFFFu;
  if (we == 255u) { // infinity / NaN: the payload's top FRAC bits are all the narrow format keeps
    *out = sign | (EMAX << FRAC) | (wf >> SH);
    return (wf & ((1u << SH) - 1u)) == 0;
  }
  if (we == 0u) { // +-0; a binary32 subnormal is below the least narrow subnormal
    *out = sign;
    return wf == 0;
  }
  const int e = int(we) - 127 + BIAS;
  if (e >= int(EMAX)) { // above the narrow maximum
    *out = sign;
    return false;
  }
  if (e >= 1) {
    *out = sign | (uint32_t(e) << FRAC) | (wf >> SH);
    return (wf & ((1u << SH) - 1u)) == 0;
  }
  // a subnormal of the narrow format: the hidden bit joins the fraction, shifted by 1 - e more
  const uint32_t m = 0x800000u | wf;
  const int shift = SH + 1 - e;
  if (shift > 23) { // (the hidden bit itself would be shifted out)
    *out = sign;
    return false;
  }
  *out = sign | (m >> shift);
  return (m & ((1u << shift) - 1u)) == 0;
}

// Whether narrow_fp<FRAC, EXPW>(x) is exact, without the pattern: the cases of narrow_fp as one
// count of fraction bits that must be zero (23 - FRAC for a normal, an infinity or a NaN; 1 - e more
// for a subnormal of the narrow format, whose hidden bit survives only while the count is <= 23).
template <int FRAC, int EXPW>
RSX_FPN_HD bool fits_fp(uint32_t x) {
  constexpr int BIAS = (1 << (EXPW - 1)) - 1;
  constexpr int EMAX = (1 << EXPW) - 1;
  constexpr int SH = 23 - FRAC;
  const uint32_t we = (x >> 23) & 0xFFu;
  const uint32_t wf = x & 0x7FFFFFu;
  if (we == 0u)
    return wf == 0u;
  const int e = int(we) - 127 + BIAS;
  if (we != 255u && e >= EMAX)
    return false;
  const int z = e < 1 ? SH + 1 - e : SH;
  return z <= 23 && (wf & ((1u << z) - 1u)) == 0u;
}

// The width class of a binary32 pattern: 0 if it has a binary16 pattern, 1 if a binary24 one, 2
// otherwise (a binary16 value always has a binary24 pattern: more fraction and more exponent).
RSX_FPN_HD uint32_t fp_fit_class(uint32_t x) {
  if (fits_fp<10, 5>(x))
    return 0u;
  return fits_fp<16, 7>(x) ? 1u : 2u;
}

// narrow at run-time bps (16, 24 or 32: 32 is the identity)
RSX_FPN_HD bool narrow_fp_bps(uint32_t x, uint32_t bps, uint32_t* out) {
  if (bps == 16u)
    return narrow_fp<10, 5>(x, out);
  if (bps == 24u)
    return narrow_fp<16, 7>(x, out);
  *out = x;
  return true;
}
