// What the Panasonic kernels share (rsx_panasonic.hip: V5, V6, V7; rsx_panasonic_v4.hip: V4): a
// job's geometry on the device, a packet half at any byte address, and the store of a
// workgroup's pixel run from LDS along the output's 16-byte grid.  Device code: included by
// those two sources only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rsx {

namespace {

constexpr int PN_THREADS = 256;
constexpr uint32_t PN_V5_BLOCK = 0x4000, PN_V5_SPLIT = 0x1FF8, PN_V5_PACKETS = 1024;

struct PnJobDev {
  uint64_t in_off;     // first byte of the job in the plan's input
  uint64_t img_offset; // first byte of the image in the plan's output
  uint32_t pitch, width;
};

// 8 bytes at any byte address: 8-byte aligned -> one load; else the three dwords that hold them
// (all three hold bytes of the 8: no dword reaches past the last byte)
__device__ __forceinline__ void pn_load8(const uint8_t* p, bool aligned, uint32_t& w0, uint32_t& w1) {
  if (aligned) {
    const uint2 v = *reinterpret_cast<const uint2*>(p);
    w0 = v.x, w1 = v.y;
    return;
  }
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  const uint32_t* d = reinterpret_cast<const uint32_t*>(a & ~uintptr_t(3));
  const uint32_t s = uint32_t(a & 3u);
  const uint32_t d0 = d[0], d1 = d[1];
  const uint32_t d2 = s ? d[2] : 0u;
  w0 = __builtin_amdgcn_alignbyte(d1, d0, s);
  w1 = __builtin_amdgcn_alignbyte(d2, d1, s);
}

// bits [POS, POS + LEN) of the packet (constants after unrolling)
template <int POS, int LEN> __device__ __forceinline__ uint32_t pn_bits(const uint32_t (&w)[4]) {
  static_assert(POS >= 0 && LEN >= 1 && LEN <= 16 && POS + LEN <= 128, "field outside the packet");
  constexpr int lo = POS >> 5, s = POS & 31;
  constexpr uint32_t mask = (1u << LEN) - 1u;
  if constexpr (s + LEN == 32)
    return w[lo] >> s;
  else if constexpr (s + LEN < 32)
    return (w[lo] >> s) & mask;
  else
    return __builtin_amdgcn_alignbit(w[lo + 1], w[lo], s) & mask;
}

// The run of `cnt` values in LDS = the pixels [P0, P0 + cnt) of the job's image, out along the
// output's 16-byte grid.  Row r starts sh(r) = (its address & 15) / 2 values behind a grid line,
// so piece j of a row holds the columns [8 j - sh, 8 j - sh + 8); a row has at most CR pieces.
// The pieces of the run are numbered through from the one that holds P0.
__device__ __forceinline__ void pn_store(const uint32_t* stage, uint8_t* out, const PnJobDev& J,
                                         uint32_t P0, uint32_t cnt) {
  const uint32_t W = J.width;
  const uint32_t CR = (W + 6u) / 8u + 1u;
  const uint32_t r0 = P0 / W, c0 = P0 - r0 * W;
  const uint32_t last = P0 + cnt - 1u;
  const uint32_t r1 = last / W, c1 = last - r1 * W;
  const uint32_t a0 = uint32_t(reinterpret_cast<uintptr_t>(out));
  const uint32_t jlo = (c0 + (((a0 + r0 * J.pitch) & 15u) >> 1)) >> 3;
  const uint32_t jhi = (c1 + (((a0 + r1 * J.pitch) & 15u) >> 1)) >> 3;
  const uint32_t total = (r1 - r0) * CR + jhi + 1u - jlo;
  const uint16_t* s16 = reinterpret_cast<const uint16_t*>(stage);
  for (uint32_t v = threadIdx.x; v < total; v += PN_THREADS) {
    const uint32_t vv = v + jlo;
    const uint32_t q = vv / CR, j = vv - q * CR;
    const uint32_t r = r0 + q;
    const int32_t sh = int32_t(((a0 + r * J.pitch) & 15u) >> 1);
    const int32_t col = int32_t(8u * j) - sh;
    const int32_t L = int32_t(r * W - P0) + col; // the piece's first value in the run
    uint8_t* dst = out + uint64_t(r) * J.pitch + int64_t(col) * 2;
    if (col >= 0 && uint32_t(col) + 8u <= W && L >= 0 && uint32_t(L) + 8u <= cnt) {
      const uint32_t* d = stage + (uint32_t(L) >> 1);
      const uint32_t s = (uint32_t(L) & 1u) * 2u;
      const uint32_t d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3], d4 = d[4];
      *reinterpret_cast<uint4*>(dst) =
          make_uint4(__builtin_amdgcn_alignbyte(d1, d0, s), __builtin_amdgcn_alignbyte(d2, d1, s),
                     __builtin_amdgcn_alignbyte(d3, d2, s), __builtin_amdgcn_alignbyte(d4, d3, s));
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int32_t c = col + i, l = L + i;
        if (c >= 0 && uint32_t(c) < W && l >= 0 && uint32_t(l) < cnt)
          reinterpret_cast<uint16_t*>(dst)[i] = s16[l];
      }
    }
  }
}

} // namespace

} // namespace rsx
