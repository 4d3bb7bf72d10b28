// SamsungV0Decompressor on the device (include/rsx.h section 3k).
//
// What the reference does (decompressors/SamsungV0Decompressor.cpp:92-204): every image row is
// a bit stream of its own (BitStreamerMSB32 over exactly the row's bytes, zeros behind them),
// cut into blocks of 16 columns.  A block header is a direction bit, four 2-bit ops on the four
// running bit lengths and a 4-bit field per op 3; 8 even and 8 odd adjustments follow.  With
// dir = 0 all eight pixels of a parity are adj + the parity's last pixel of the block before
// (128 at column 0); with dir = 1 an even pixel is adj + the pixel one row up, an odd one adj +
// the pixel two rows up.  After all rows out(row, col + 1) and out(row + 1, col) are swapped
// for even row, col.  Two things follow from that:
//   * the bit lengths come from the headers alone, never from decoded values: one lane can
//     walk a row's headers -- a step per block, 347 at the widest frame -- and the rows can be
//     parsed independently of one another;
//   * per parity the only value that travels along a row is a block's last pixel, and a
//     dir = 1 block restarts that chain from the rows above: a segmented scan makes every
//     pixel LOCAL -- relative to the root of its run, which is 128 or a pixel of the rows above.
//
//   sv0_parse_kernel  one workgroup per row (192 lanes, two passes of a block a lane; 5546 / 16
//                     -> 347 blocks):
//                     1. the row's bytes -> LDS as little-endian words, zero behind them;
//                     2. lane 0 walks the block headers -- a step is a peek, a table look-up on
//                        the eight op bits and byte-parallel arithmetic on the four lengths -- and
//                        leaves per block the bit offset of its pixels, the four lengths and dir,
//                        and decides the row's status in stream order (size < 4, over-read, length
//                        range, upward prediction);
//                     3. a lane extracts the 16 adjustments of its block;
//                     4. a segmented scan mod 2^16 of the blocks' last adjustments per parity,
//                        restarted by dir = 1 blocks, which also carries the last such block;
//                     5. the lane writes its 16 local values (128 folded in where the run starts
//                        at column 0) to the plan's scratch plane, and a root code per block:
//                        0 = nothing to add, b0 + 1 = add the rows above at column 16 b0 + 14
//                        (+ 1 for odd pixels), SV0_UP = every pixel adds its own column.
//   sv0_recon_kernel  one workgroup per frame, marching down the rows; lane b owns block b.
//                     The last three pre-swap rows sit in LDS.  A row step is a gather from
//                     the two rows above, an add, a 32-byte LDS write and one barrier; local
//                     values and codes are loaded a group of rows ahead (they depend on nothing).
//                     Both pixels a swap exchanges lie in one block, so a lane keeps the two
//                     rows before in registers and stores each row, swapped, one step later.
//
// Bit-exact against the numpy model of exactly this decomposition (tests/srw_v0_files.py),
// which tests/test_samsung_v0_model.py holds against the reference's whole-file decode.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "rsx_internal.h"
#include "rsx_ljpeg_dev.h"
#include "rsx_plan_host.h"
#include "rsx_samsung_v0.h"

namespace rsx {

namespace {

constexpr int SV0_THREADS = 384; // reconstruction: one lane per block of 16 columns (5546 / 16 -> 347)
// parse: two blocks a lane.  The walk is one lane's chain of dependent steps, so what counts is
// how many rows a CU walks at once: 10 workgroups of 192 (the LDS allows no more) instead of 5 of 384.
constexpr int SV0_PARSE_THREADS = 192;
constexpr int SV0_PARSE_WAVES = SV0_PARSE_THREADS / 64;
constexpr int SV0_PASSES = SV0_THREADS / SV0_PARSE_THREADS;
constexpr uint32_t SV0_UP = 0xFFFFu; // root code of a dir = 1 block
constexpr int32_t SV0_MIN_W = 16, SV0_MAX_W = 5546, SV0_MAX_H = 3714; // SamsungV0Decompressor.cpp:54
constexpr uint32_t SV0_BLOCK_BITS = 281; // 9 + 4 x 4 + 16 x 16
// LDS of the parse in front of the row's words: per block the bit offset of its pixels | dir << 31
// and its four lengths + 1 as bytes, the scan's per-wave totals of either pass, the row's status,
// and what the eight op bits of a header mean
constexpr int SV0_LDS_LUT = 2 * SV0_THREADS + 16; // the header table: 256 entries of two words
constexpr int SV0_LDS_HEAD = SV0_LDS_LUT + 512;
constexpr int SV0_LDS_STATUS = 2 * SV0_THREADS + 2 * SV0_PARSE_WAVES * SV0_PASSES;
static_assert(SV0_LDS_STATUS < SV0_LDS_HEAD, "the status lies behind the totals");
#ifndef RSX_SV0_AHEAD
#define RSX_SV0_AHEAD 4
#endif
constexpr int SV0_AHEAD = RSX_SV0_AHEAD; // rows of a group of the reconstruction (even)

struct Sv0RowDev {
  uint64_t off;   // first byte of the row in the plan's input
  uint32_t bytes; // row size
  uint32_t job;
  uint32_t row;
  uint32_t pad;
};

struct Sv0JobDev {
  uint64_t img_offset;
  uint64_t blk_base; // first block of the job in the scratch plane (16 values) and in codes[]
  uint32_t pitch, width, height; // height 0: rejected by the host
  uint32_t nblk;
  uint32_t row_base; // first entry of the job in rows[] / row_status[]
  uint32_t words;    // words of a row in LDS (a bound on what its blocks can read, + 3)
};

struct Sv0Args {
  const uint8_t* in_base;
  uint8_t* out_base;
  const Sv0RowDev* rows;
  const Sv0JobDev* jobs;
  uint16_t* local;      // [block of the plan][16]
  uint32_t* codes;      // [block of the plan]
  uint32_t* row_status; // [row of the plan]: rsx_status
  uint32_t* job_status; // [job]: first failing row << 8 | status, STATUS_NONE = fine
};

__host__ __device__ inline uint32_t sv0_row_words(uint32_t nblk) {
  return nblk * SV0_BLOCK_BITS / 32u + 3u;
}

// Workgroup barrier that orders LDS accesses only: loads issued rows ahead stay in flight.
__device__ __forceinline__ void sv0_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// The 32 bits at bit offset q (BitStreamerMSB32: little-endian words, MSB first)
__device__ __forceinline__ uint32_t sv0_peek(const uint32_t* w, uint32_t q) {
  const uint32_t k = q >> 5;
  const uint64_t v = (uint64_t(w[k]) << 32) | w[k + 1];
  return uint32_t((v << (q & 31u)) >> 32);
}

// the low half of a, the high half of b
__device__ __forceinline__ uint32_t sv0_halves(uint32_t a, uint32_t b) {
  return (a & 0xFFFFu) | (b & 0xFFFF0000u);
}

// both halves added mod 2^16 (v_pk_add_u16)
typedef unsigned short sv0_u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t sv0_add16(uint32_t a, uint32_t b) {
  sv0_u16x2 x, y;
  __builtin_memcpy(&x, &a, 4);
  __builtin_memcpy(&y, &b, 4);
  x += y;
  uint32_t r;
  __builtin_memcpy(&r, &x, 4);
  return r;
}

// last adjustments per parity: sum (16 bits) | (last dir = 1 block + 1) << 16; a then b
__device__ __forceinline__ uint32_t sv0_combine(uint32_t a, uint32_t b) {
  return (b >> 16) ? b : ((a & 0xFFFF0000u) | ((a + b) & 0xFFFFu));
}

__global__ void __launch_bounds__(SV0_PARSE_THREADS) sv0_parse_kernel(Sv0Args A) {
  extern __shared__ __attribute__((aligned(16))) uint32_t sv0_lds[];
  uint32_t* blk_pos = sv0_lds;
  uint32_t* blk_len = sv0_lds + SV0_THREADS;
  uint32_t* totals = sv0_lds + 2 * SV0_THREADS; // [pass][wave][parity]
  uint32_t* W = sv0_lds + SV0_LDS_HEAD;
  const int tid = threadIdx.x;
  const Sv0RowDev R = A.rows[blockIdx.x];
  const Sv0JobDev J = A.jobs[R.job];
  const uint32_t width = J.width, nblk = J.nblk;

  // What a header's eight op bits (op 0 in the top two) do to the four lengths, kept + 1 as the
  // bytes of one word (length i in byte i): word 0 = for an op 3 the byte of the spread fields its
  // value comes from (v_perm_b32), word 1 = per byte the op's step + 1 (bits 0-1) and "op 3" (bit
  // 2), and in bits 4-6 the number of ops 3.
  for (uint32_t e = tid; e < 256u; e += SV0_PARSE_THREADS) {
    uint32_t sel = 0, w1 = 0, n3 = 0;
    for (int i = 0; i < 4; ++i) {
      const uint32_t op = (e >> (6 - 2 * i)) & 3u;
      if (op == 3u) {
        sel |= (3u - n3) << (8 * i);
        w1 |= 4u << (8 * i);
        ++n3;
      }
      w1 |= (op == 1u ? 2u : op == 2u ? 0u : 1u) << (8 * i);
    }
    sv0_lds[SV0_LDS_LUT + 2 * e] = sel;
    sv0_lds[SV0_LDS_LUT + 2 * e + 1] = w1 | (n3 << 4);
  }

  // 1. the row -> LDS.  Rows start at any byte: each word is two aligned dwords shifted
  // together; only dwords that hold bytes of the row are read, bytes behind it are zero.
  {
    const uintptr_t a = reinterpret_cast<uintptr_t>(A.in_base + R.off);
    const uint32_t* d = reinterpret_cast<const uint32_t*>(a & ~uintptr_t(3));
    const uint32_t sh = uint32_t(a & 3u) * 8u;
    const uint64_t nd = R.bytes ? (((a & 3u) + uint64_t(R.bytes) + 3u) >> 2) : 0u; // dwords
    for (uint32_t k = tid; k < J.words; k += SV0_PARSE_THREADS) {
      uint32_t v = 0;
      if (4ull * k < R.bytes) {
        const uint32_t lo = d[k];
        const uint32_t hi = k + 1u < nd ? d[k + 1] : 0u;
        v = sh ? (lo >> sh) | (hi << (32u - sh)) : lo;
        const uint64_t rem = uint64_t(R.bytes) - 4ull * k;
        if (rem < 4u)
          v &= (1u << (8u * uint32_t(rem))) - 1u;
      }
      W[k] = v;
    }
  }
  __syncthreads();

  // 2. the walk: per block where its pixels start and how long they are; the row's status is
  // that of the first exception in stream order
  if (tid == 0) {
    uint32_t st = R.bytes < 4u ? uint32_t(RSX_ERR_IO) : uint32_t(RSX_OK);
    // A request that ends at bit `end` refills up to word ceil(end / 32); the refill at byte
    // 4 (k - 1) throws when that is more than size + 8 (BitStreamer.h:100-132): end > limit
    const uint64_t limit64 = 32ull * ((uint64_t(R.bytes) + 8u) / 4u + 1u);
    const uint32_t limit = limit64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(limit64);
    constexpr uint32_t ONES = 0x01010101u;
    uint32_t B = (R.row < 2u ? 8u : 5u) * ONES; // the lengths + 1: 7 resp. 4 at the start (:116-118)
    uint32_t pos = 0;
    for (uint32_t b = 0; b < nblk && st == RSX_OK; ++b) {
      const uint32_t w = sv0_peek(W, pos);
      const uint32_t dir = w >> 31, e = (w >> 23) & 0xFFu;
      const uint2 T = *reinterpret_cast<const uint2*>(sv0_lds + SV0_LDS_LUT + 2u * e);
      // the 16 bits behind the header, as four bytes: the first 4-bit field in byte 3
      const uint32_t x = (w >> 7) & 0xFFFFu, x2 = (x | (x << 8)) & 0x00FF00FFu;
      const uint32_t N = (x2 | (x2 << 4)) & 0x0F0F0F0Fu;
      const uint32_t F = __builtin_amdgcn_perm(N, N, T.x); // the field of every op 3 in its length's byte
      const uint32_t m3 = ((T.y >> 2) & ONES) * 255u;
      const uint32_t q = 9u + 4u * ((T.y >> 4) & 7u);
      // op 1: + 1, op 2: - 1 (bytes never borrow: length + 1 >= 1), op 3: the field
      const uint32_t S = B + (T.y & 0x03030303u) - ONES;
      const uint32_t Bn = (S & ~m3) | ((F + ONES) & m3);
      // the pixels: the last one of a length > 0 ends where the block ends
      const uint32_t end = pos + q + 4u * (__builtin_amdgcn_sad_u8(Bn, 0u, 0u) - 4u);
      const uint32_t below = (Bn - ONES) & ~Bn & 0x80808080u; // some byte 0: a length of -1
      const uint32_t above = (Bn + 0x6E6E6E6Eu) & 0x80808080u; // some byte > 17: a length > 16
      const bool updir = dir && (R.row < 2u || 16u * b + 16u >= width);
      // (requests only grow: no over-read at the block's end means none before it; a length
      // that left 0..16 may make `end` meaningless, but then the ordered checks decide)
      if ((below | above) != 0u || updir || end > limit || pos + 32u > limit) {
        // the first exception in stream order (:122-160)
        uint32_t qq = 9;
        if (pos + 32u > limit) // bits.fill()
          st = RSX_ERR_INPUT_OVERFLOW;
        for (int i = 0; i < 4 && st == RSX_OK; ++i) {
          const uint32_t op = (e >> (6 - 2 * i)) & 3u;
          int l = int((B >> (8 * i)) & 0xFFu) - 1;
          if (op == 3u) {
            if (pos + qq + 4u > limit)
              st = RSX_ERR_INPUT_OVERFLOW;
            qq += 4u;
            l = int((F >> (8 * i)) & 0xFFu);
          } else if (op == 2u) {
            --l;
          } else if (op == 1u) {
            ++l;
          }
          if (st == RSX_OK && (l < 0 || l > 16)) // (:147-150)
            st = RSX_ERR_VALUE_RANGE;
        }
        if (st == RSX_OK && updir) // (:156-160)
          st = RSX_ERR_INVALID_ARG;
        if (st == RSX_OK)
          st = RSX_ERR_INPUT_OVERFLOW; // (a pixel)
        break;
      }
      B = Bn;
      blk_pos[b] = (pos + q) | (dir << 31);
      blk_len[b] = Bn;
      pos = end;
    }
    sv0_lds[SV0_LDS_STATUS] = st;
    A.row_status[J.row_base + R.row] = st;
    if (st != RSX_OK)
      atomicMin(&A.job_status[R.job], (R.row << 8) | st);
  }
  __syncthreads();

  const bool ok = sv0_lds[SV0_LDS_STATUS] == RSX_OK;
  const int lane = tid & 63, wave = tid >> 6;
  uint32_t before0 = 0, before1 = 0; // the scan over the passes so far
  for (int pass = 0; pass < SV0_PASSES; ++pass) {
    const uint32_t b = uint32_t(pass * SV0_PARSE_THREADS + tid);
    if (uint32_t(pass * SV0_PARSE_THREADS) >= nblk)
      break;
    // 3. lane b: the 16 adjustments of block b, mod 2^16 (a failed row: all zero, dir = 0)
    const bool live = b < nblk;
    const uint32_t info = (live && ok) ? blk_len[b] : 0x01010101u; // (lengths + 1)
    const uint32_t where = (live && ok) ? blk_pos[b] : 0u;
    const uint32_t dir = where >> 31;
    uint32_t adj[16]; // 0..7 the even pixels, 8..15 the odd ones
    {
      uint32_t p = where & 0x7FFFFFFFu;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const uint32_t n = ((info >> (8 * g)) & 0xFFu) - 1u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          uint32_t v = 0;
          if (n) // signExtend(getBits(n), n) (:104-108)
            v = uint32_t(int32_t(sv0_peek(W, p)) >> (32u - n));
          adj[4 * g + j] = v;
          p += n;
        }
      }
    }

    // 4. the segmented scan of the blocks' last adjustments, both parities at once
    const uint32_t mark = dir ? (b + 1u) << 16 : 0u;
    uint32_t s0 = live ? ((adj[7] & 0xFFFFu) | mark) : 0u;
    uint32_t s1 = live ? ((adj[15] & 0xFFFFu) | mark) : 0u;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t t0 = __shfl_up(s0, d, 64), t1 = __shfl_up(s1, d, 64);
      if (lane >= d) {
        s0 = sv0_combine(t0, s0);
        s1 = sv0_combine(t1, s1);
      }
    }
    uint32_t* tot = totals + 2 * SV0_PARSE_WAVES * pass;
    if (lane == 63) {
      tot[2 * wave] = s0;
      tot[2 * wave + 1] = s1;
    }
    __syncthreads();
    uint32_t e0 = __shfl_up(s0, 1, 64), e1 = __shfl_up(s1, 1, 64);
    if (lane == 0)
      e0 = e1 = 0;
    uint32_t w0 = before0, w1 = before1;
    for (int v = 0; v < SV0_PARSE_WAVES; ++v) {
      if (v == wave) {
        e0 = sv0_combine(w0, e0);
        e1 = sv0_combine(w1, e1);
      }
      w0 = sv0_combine(w0, tot[2 * v]);
      w1 = sv0_combine(w1, tot[2 * v + 1]);
    }
    before0 = w0;
    before1 = w1;
    const uint32_t carry0 = e0, carry1 = e1;
    if (!live)
      continue;

    // 5. local values and the root code
    uint32_t code, add0, add1;
    if (dir) {
      code = SV0_UP;
      add0 = add1 = 0;
    } else {
      code = carry0 >> 16; // (the same block for both parities)
      add0 = (carry0 & 0xFFFFu) + (code ? 0u : 128u); // (:184, :194)
      add1 = (carry1 & 0xFFFFu) + (code ? 0u : 128u);
    }
    uint32_t px[8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
      px[i] = ((adj[i] + add0) & 0xFFFFu) | ((adj[8 + i] + add1) << 16);
    const uint64_t blk = J.blk_base + uint64_t(R.row) * nblk + b;
    uint4* dst = reinterpret_cast<uint4*>(A.local + blk * 16u);
    dst[0] = make_uint4(px[0], px[1], px[2], px[3]);
    dst[1] = make_uint4(px[4], px[5], px[6], px[7]);
    A.codes[blk] = code;
  }
}

// The first `npix` of a block's 16 pixels to `out`: w[] holds the pixel pairs, `last` the word
// of the single last pixel of an odd npix (which has no partner to swap with).  Any even address.
__device__ __forceinline__ void sv0_store_narrow(uint8_t* out, const uint32_t* w, const uint32_t* last,
                                                 uint32_t npix) {
  if ((reinterpret_cast<uintptr_t>(out) & 3u) == 0u) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (uint32_t(2 * i + 1) < npix)
        reinterpret_cast<uint32_t*>(out)[i] = w[i];
      else if (uint32_t(2 * i) < npix)
        reinterpret_cast<uint16_t*>(out)[2 * i] = uint16_t(last[i]);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (uint32_t(2 * i + 1) < npix) {
        reinterpret_cast<uint16_t*>(out)[2 * i] = uint16_t(w[i]);
        reinterpret_cast<uint16_t*>(out)[2 * i + 1] = uint16_t(w[i] >> 16);
      } else if (uint32_t(2 * i) < npix) {
        reinterpret_cast<uint16_t*>(out)[2 * i] = uint16_t(last[i]);
      }
    }
  }
}

// Up to three pixel pairs a0, a1, a2 and, for an odd count of pixels, the single pixel behind them
// (the low half of the pair's word m0..m3 it falls into) to the 8-byte aligned `p`.
__device__ __forceinline__ void sv0_store_rest(uint8_t* p, uint32_t pairs, bool single, uint32_t a0,
                                               uint32_t a1, uint32_t a2, uint32_t m0, uint32_t m1,
                                               uint32_t m2, uint32_t m3) {
  if (pairs & 2u)
    *reinterpret_cast<uint2*>(p) = make_uint2(a0, a1);
  if (pairs & 1u)
    reinterpret_cast<uint32_t*>(p)[pairs & 2u] = (pairs & 2u) ? a2 : a0;
  if (single) {
    const uint32_t m = pairs == 0u ? m0 : pairs == 1u ? m1 : pairs == 2u ? m2 : m3;
    reinterpret_cast<uint16_t*>(p)[2u * pairs] = uint16_t(m);
  }
}

// The first `npix` < 16 pixels of a block on the 16-byte grid, in at most four stores: 16, 8, 4
// and 2 bytes.  (Branches, not selects, between the block's halves: a select between two
// elements of an array becomes an indexed access, and the array goes to scratch memory.)
__device__ __forceinline__ void sv0_store_partial(uint8_t* out, const uint32_t* w, const uint32_t* last,
                                                  uint32_t npix) {
  const uint32_t nw = npix >> 1; // whole pairs, 0..7
  if (nw >= 4u) {
    *reinterpret_cast<uint4*>(out) = make_uint4(w[0], w[1], w[2], w[3]);
    sv0_store_rest(out + 16, nw & 3u, npix & 1u, w[4], w[5], w[6], last[4], last[5], last[6], last[7]);
  } else {
    sv0_store_rest(out, nw & 3u, npix & 1u, w[0], w[1], w[2], last[0], last[1], last[2], last[3]);
  }
}

// One frame.  GRID: the image's rows start on the 16-byte grid, so a whole block goes out as two
// 16-byte stores.  Then the row step has no branch but the narrow stores of a partial last block:
// lanes without a block load block 0's values, and they and the lane of a partial block send their
// two 16-byte stores to an already consumed place of the scratch plane, each to another one.  With every load and store on one path the compiler
// counts them, and a wait for a loaded row leaves the stores of the rows before it in flight.
template <bool GRID>
__device__ __forceinline__ void sv0_recon_frame(const Sv0Args& A, const Sv0JobDev& J, uint32_t* rows) {
  const uint32_t nblk = J.nblk, h = J.height;
  const uint32_t t = threadIdx.x; // the lane's place in the LDS rows (a place of its own even without a block)
  const bool live = t < nblk;
  const uint32_t b = live ? t : 0u;
  // a row in LDS: the blocks' words 0..3, then their words 4..7 -- neighbouring lanes 16 bytes
  // apart in either half (8 words a block in one piece: 32 bytes apart, an 8-way bank conflict on
  // every 16-byte access, which was most of a row step)
  const uint32_t stride = 8u * SV0_THREADS, half = 4u * SV0_THREADS;
  uint32_t* cur = rows;               // the row being made
  uint32_t* up1 = rows + stride;      // one row up
  uint32_t* up2 = rows + 2u * stride; // two rows up
  uint4* local = reinterpret_cast<uint4*>(A.local + (J.blk_base + b) * 16u);
  const uint32_t* codes = A.codes + J.blk_base + b;
  uint8_t* out = A.out_base + J.img_offset + 32ull * b;
  const uint32_t npix = min(16u, J.width - 16u * b);
  // where a lane's two 16-byte stores of row r go: its block of the image, or -- without a whole
  // block -- local values of row r that have been consumed (each such lane another block's)
  const bool whole = live && npix == 16u;
  uint8_t* d16_base = whole ? out : reinterpret_cast<uint8_t*>(A.local + (J.blk_base + t % nblk) * 16u);
  const uint32_t d16_step = whole ? J.pitch : 32u * nblk;

  // Local values and codes depend on nothing: the next group of SV0_AHEAD rows is loaded while
  // this one is made -- all of it during the group's first half, so that the loads have landed
  // when the group ends and the registers change hands.
  uint4 qa[SV0_AHEAD], qb[SV0_AHEAD], na[SV0_AHEAD], nb[SV0_AHEAD];
  uint32_t qc[SV0_AHEAD], nc[SV0_AHEAD];
#pragma unroll
  for (int k = 0; k < SV0_AHEAD; ++k) {
    const uint64_t r = uint64_t(min(uint32_t(k), h - 1u)) * nblk;
    qa[k] = local[2ull * r];
    qb[k] = local[2ull * r + 1u];
    qc[k] = codes[r];
  }
  uint32_t p1[8], p2[8]; // the rows one and two up, before the swap
#pragma unroll
  for (int i = 0; i < 8; ++i)
    p1[i] = p2[i] = 0;

  // The image row `r` of this block: final(r, odd c) = pre(r + 1, c - 1) and final(r + 1,
  // even c) = pre(r, c + 1) for even r < h - 1 where c + 1 < width (:98-101); both pixels lie
  // in this block.  odd: the partner is the row above, else the one below; swap: r has a partner.
  auto emit = [&](const uint32_t r, const bool odd, const bool swap, const uint32_t* own,
                  const uint32_t* partner) {
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (!swap)
        w[i] = own[i];
      else if (odd) // its partner is the row above it
        w[i] = (partner[i] >> 16) | (own[i] & 0xFFFF0000u);
      else          // its partner is the row below it
        w[i] = (own[i] & 0xFFFFu) | (partner[i] << 16);
    }
    // (the single last pixel of an odd width has no partner: it goes out from `own`)
    uint8_t* dst = out + uint64_t(r) * J.pitch;
    if (GRID) {
      // (what is no whole block of the image goes where nobody reads any more: local values of row r)
      uint4* d16 = reinterpret_cast<uint4*>(d16_base + uint64_t(r) * d16_step);
      d16[0] = make_uint4(w[0], w[1], w[2], w[3]);
      d16[1] = make_uint4(w[4], w[5], w[6], w[7]);
      if (live && npix < 16u)
        sv0_store_partial(dst, w, own, npix);
    } else if (live) {
      if (npix == 16u && (reinterpret_cast<uintptr_t>(dst) & 3u) == 0u) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
          reinterpret_cast<uint32_t*>(dst)[i] = w[i];
      } else {
        sv0_store_narrow(dst, w, own, npix);
      }
    }
  };

  // one row: `k` is its place in the group (and its parity), `ahead`: load the next group
  auto step = [&](const int k, const uint32_t row, const bool ahead) {
    if (ahead && 2 * k < SV0_AHEAD) {
#pragma unroll
      for (int j = 2 * k; j < 2 * k + 2 && j < SV0_AHEAD; ++j) {
        const uint64_t nx = uint64_t(min(row - uint32_t(k) + uint32_t(SV0_AHEAD + j), h - 1u)) * nblk;
        na[j] = local[2ull * nx];
        nb[j] = local[2ull * nx + 1u];
        nc[j] = codes[nx];
      }
    }
    uint32_t px[8] = {qa[k].x, qa[k].y, qa[k].z, qa[k].w, qb[k].x, qb[k].y, qb[k].z, qb[k].w};
    const uint32_t code = qc[k];
    {
      // One add word per pixel pair: low half from one row up (even pixels), high half from two
      // rows up (odd pixels).  A dir = 1 block takes its own columns, a block behind one the last
      // pixels of block code - 1, a run from column 0 nothing.  No lane branches: nearly every
      // wave with a dir = 1 block holds blocks of all kinds.
      const bool up = code == SV0_UP;
      uint32_t e[8], o[8];
#pragma unroll
      for (int i = 0; i < 8; ++i)
        e[i] = o[i] = 0;
      if (__any(up)) { // (wave-uniform: a wave without a dir = 1 block reads two words a lane)
        const uint4 a0 = *reinterpret_cast<const uint4*>(up1 + 4u * t);
        const uint4 a1 = *reinterpret_cast<const uint4*>(up1 + half + 4u * t);
        const uint4 c0 = *reinterpret_cast<const uint4*>(up2 + 4u * t);
        const uint4 c1 = *reinterpret_cast<const uint4*>(up2 + half + 4u * t);
        e[0] = a0.x, e[1] = a0.y, e[2] = a0.z, e[3] = a0.w, e[4] = a1.x, e[5] = a1.y, e[6] = a1.z, e[7] = a1.w;
        o[0] = c0.x, o[1] = c0.y, o[2] = c0.z, o[3] = c0.w, o[4] = c1.x, o[5] = c1.y, o[6] = c1.z, o[7] = c1.w;
      }
      // (code - 1 is a block for 1 <= code <= nblk only: 0 wraps around, SV0_UP - 1 is no block;
      // such a lane reads its own place and drops it)
      const bool rooted = code - 1u < uint32_t(SV0_THREADS);
      const uint32_t rb = rooted ? code - 1u : t;
      const uint32_t rw = sv0_halves(up1[half + 4u * rb + 3u], up2[half + 4u * rb + 3u]);
      const uint32_t root = rooted ? rw : 0u;
#pragma unroll
      for (int i = 0; i < 8; ++i)
        px[i] = sv0_add16(px[i], up ? sv0_halves(e[i], o[i]) : root);
      *reinterpret_cast<uint4*>(cur + 4u * t) = make_uint4(px[0], px[1], px[2], px[3]);
      *reinterpret_cast<uint4*>(cur + half + 4u * t) = make_uint4(px[4], px[5], px[6], px[7]);
    }
    sv0_barrier();
    uint32_t* t = up2;
    up2 = up1;
    up1 = cur;
    cur = t;
    // the row above goes out now that its partner is known
    if (row > 0u)
      emit(row - 1u, !(k & 1), true, p1, (k & 1) ? px : p2);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      p2[i] = p1[i];
      p1[i] = px[i];
    }
  };
  // whole groups of SV0_AHEAD rows, then the rows that are left, which load nothing
  uint32_t row0 = 0;
  for (; row0 + SV0_AHEAD <= h; row0 += SV0_AHEAD) {
#pragma unroll
    for (int k = 0; k < SV0_AHEAD; ++k)
      step(k, row0 + uint32_t(k), true);
#pragma unroll
    for (int k = 0; k < SV0_AHEAD; ++k) {
      qa[k] = na[k];
      qb[k] = nb[k];
      qc[k] = nc[k];
    }
  }
#pragma unroll
  for (int k = 0; k < SV0_AHEAD - 1; ++k)
    if (row0 + uint32_t(k) < h)
      step(k, row0 + uint32_t(k), false);
  // the last row: the odd row of a pair, or the single last row of an odd height
  emit(h - 1u, true, ((h - 1u) & 1u) != 0u, p1, p2);
}

__global__ void __launch_bounds__(SV0_THREADS) sv0_recon_kernel(Sv0Args A) {
  extern __shared__ __attribute__((aligned(16))) uint32_t sv0_rows[]; // three pre-swap rows, 8 words a lane
  const Sv0JobDev J = A.jobs[blockIdx.x];
  if (J.height == 0u)
    return;
  const bool grid = ((reinterpret_cast<uintptr_t>(A.out_base) + J.img_offset) & 15u) == 0u && (J.pitch & 15u) == 0u;
  if (grid)
    sv0_recon_frame<true>(A, J, sv0_rows);
  else
    sv0_recon_frame<false>(A, J, sv0_rows);
}

} // namespace

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
namespace {
struct Sv0Plan final : DecoderPlan {
  rsx_ctx* ctx = nullptr;
  std::vector<Sv0JobDev> jobs;
  JobStatus status;
  DeviceBuffer d_jobs, d_rows, d_row_status, d_local, d_codes;
  std::vector<uint32_t> h_row_status;
  uint32_t total_rows = 0, max_words = 0, max_nblk = 0;
  uint64_t total_blocks = 0;
  bool launched = false;
  int run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) override;
  int results(hipStream_t s, bool ran, int32_t* job_status, uint32_t* job_consumed) override;
  int row_status(hipStream_t s, int job, int32_t* statuses) override;
};
} // namespace

int samsung_v0_validate(const uint32_t* row_offsets, int n_offsets, size_t in_bytes,
                        const rsx_image& img) {
  // the constructor, SamsungV0Decompressor.cpp:44-58
  if (img.cpp != 1)
    return RSX_ERR_INVALID_ARG;
  if (img.dim_x < SV0_MIN_W || img.dim_x > SV0_MAX_W || img.dim_y <= 0 || img.dim_y > SV0_MAX_H)
    return RSX_ERR_INVALID_ARG;
  if (img.pitch_bytes < uint32_t(img.dim_x) * 2u)
    return RSX_ERR_INVALID_ARG;
  if (uint64_t(in_bytes) >= (1ull << 32))
    return RSX_ERR_UNSUPPORTED; // (the offsets are 32-bit)
  // bso.peekStream(height, 4)
  if (!row_offsets || n_offsets < img.dim_y)
    return RSX_ERR_IO;
  // computeStripes (:61-90): bsr.skipBytes(first offset), then pair by pair the sequence check
  // and bsr.getStream(size)
  if (row_offsets[0] > in_bytes)
    return RSX_ERR_IO;
  for (int y = 0; y < img.dim_y; ++y) {
    const uint64_t lo = row_offsets[y];
    const uint64_t hi = y + 1 < img.dim_y ? uint64_t(row_offsets[y + 1]) : uint64_t(in_bytes);
    if (lo >= hi)
      return RSX_ERR_INVALID_ARG; // "Line offsets are out of sequence or slice is empty."
    if (hi > in_bytes)
      return RSX_ERR_IO;
  }
  return RSX_OK;
}

int samsung_v0_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_samsung_v0_job* jobs,
                           std::unique_ptr<DecoderPlan>* out) {
  auto p = std::make_unique<Sv0Plan>();
  p->ctx = ctx;
  p->status.host.assign(n_jobs, RSX_OK);
  p->jobs.resize(n_jobs);
  std::vector<Sv0RowDev> rows;
  for (int i = 0; i < n_jobs; ++i) {
    const rsx_samsung_v0_job& j = jobs[i];
    Sv0JobDev& J = p->jobs[i];
    std::memset(&J, 0, sizeof J);
    int st = samsung_v0_validate(j.row_offsets, j.n_offsets, size_t(j.in_bytes), j.img);
    if (st == RSX_OK && (j.img_offset % 2 != 0 || j.img.pitch_bytes % 2 != 0))
      st = RSX_ERR_INVALID_ARG;
    p->status.host[i] = st;
    if (st != RSX_OK)
      continue;
    J.img_offset = j.img_offset;
    J.blk_base = p->total_blocks;
    J.pitch = j.img.pitch_bytes;
    J.width = uint32_t(j.img.dim_x);
    J.height = uint32_t(j.img.dim_y);
    J.nblk = (J.width + 15u) / 16u;
    J.row_base = p->total_rows;
    J.words = sv0_row_words(J.nblk);
    p->max_words = std::max(p->max_words, J.words);
    p->max_nblk = std::max(p->max_nblk, J.nblk);
    for (uint32_t y = 0; y < J.height; ++y) {
      const uint64_t lo = j.row_offsets[y];
      const uint64_t hi = y + 1 < J.height ? uint64_t(j.row_offsets[y + 1]) : j.in_bytes;
      rows.push_back(Sv0RowDev{j.in_offset + lo, uint32_t(hi - lo), uint32_t(i), y, 0u});
    }
    p->total_rows += J.height;
    p->total_blocks += uint64_t(J.height) * J.nblk;
  }
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int st;
  if ((st = upload(ctx, p->d_jobs, p->jobs)) || (st = upload(ctx, p->d_rows, rows)) ||
      (st = p->d_row_status.ensure(size_t(p->total_rows) * 4 + 16)) || (st = p->status.init()) ||
      (st = p->d_local.ensure(size_t(p->total_blocks) * 32 + 16)) ||
      (st = p->d_codes.ensure(size_t(p->total_blocks) * 4 + 16)))
    return st;
  *out = std::move(p);
  return RSX_OK;
}

int Sv0Plan::run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) {
  if (total_rows == 0)
    return RSX_OK; // (every job was rejected by the host)
  if (timer)
    timer->begin(s);
  Sv0Args A{};
  A.in_base = static_cast<const uint8_t*>(in_dev);
  A.out_base = static_cast<uint8_t*>(out_dev);
  A.rows = static_cast<const Sv0RowDev*>(d_rows.ptr);
  A.jobs = static_cast<const Sv0JobDev*>(d_jobs.ptr);
  A.local = static_cast<uint16_t*>(d_local.ptr);
  A.codes = static_cast<uint32_t*>(d_codes.ptr);
  A.row_status = static_cast<uint32_t*>(d_row_status.ptr);
  A.job_status = static_cast<uint32_t*>(status.dev.ptr);
  if (int st = status.reset(ctx, s))
    return st;
  const size_t lds = (size_t(SV0_LDS_HEAD) + max_words) * 4;
  hipLaunchKernelGGL(sv0_parse_kernel, dim3(total_rows), dim3(SV0_PARSE_THREADS), lds, s, A);
  if (timer)
    timer->mark("sv0_parse_kernel");
  RSX_HIP_CHECK(ctx, hipGetLastError());
  hipLaunchKernelGGL(sv0_recon_kernel, dim3(uint32_t(jobs.size())), dim3(SV0_THREADS),
                     size_t(3) * 8 * SV0_THREADS * 4, s, A);
  if (timer)
    timer->mark("sv0_recon_kernel");
  RSX_HIP_CHECK(ctx, hipGetLastError());
  launched = true;
  return RSX_OK;
}

int Sv0Plan::results(hipStream_t s, bool ran, int32_t* job_status, uint32_t* job_consumed) {
  if (job_consumed)
    std::fill(job_consumed, job_consumed + jobs.size(), 0u);
  return status.fold(ctx, s, ran && total_rows != 0, 0xFFu, FoldOrder::LAST_FAILING, job_status);
}

int Sv0Plan::row_status(hipStream_t s, int job, int32_t* statuses) {
  if (job < 0 || size_t(job) >= jobs.size() || !launched || jobs[job].height == 0)
    return RSX_ERR_INVALID_ARG;
  return fetch_words(ctx, s, d_row_status, jobs[job].row_base, jobs[job].height, h_row_status,
                     statuses);
}

} // namespace rsx
