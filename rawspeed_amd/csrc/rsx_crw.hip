// CrwDecompressor (Canon CRW) on gfx950: include/rsx.h section 3x, DESIGN.md 4.22.
//
// A frame's scan is one serial chain of Huffman symbols with no marker to enter it at, but a
// parser's state is only (bit position, coefficient index), so the chain is found the way
// vc5_band_kernel finds its bands' -- parse segments from guessed entries, hand the exits forward,
// repeat until nothing changes; segment k is final after k rounds whatever the stream -- on two
// levels, because here one stream is the whole frame.  A run is, over all jobs (frames) of a plan:
//
// crw_zero_kernel      the images' rows to zero (the differences are kept in the image itself);
//                      in front of it the run zeroes the compact buffer and the coefficient-0 list.
// crw_count_kernel     per 4096 raw bytes: the bytes that are not the 00 of an FF 00, and the
//                      first marker (FF xx, xx != 00) by an atomic minimum.
// crw_compact_kernel   the data bytes in front of the marker, packed (a workgroup sums the counts
//                      of the chunks in front of it); the buffer is zero behind them, which is
//                      what the reader supplies there.  Records the number of data bytes, from
//                      which the reader's overflow becomes a threshold on bit positions.
// crw_parse_kernel     round 0: one workgroup a WINDOW of RSX_CRW_WIN_SEGS segments of
//                      RSX_CRW_SEG_BITS bits, held in LDS; a lane parses its segment from the
//                      guess (the segment's first bit, coefficient 1; lane 0 of window 0 from the
//                      truth), exits are handed to the next lane and re-parsed until a workgroup
//                      vote finds no change.  Publishes the window's exit.  Rounds 1..R (launches,
//                      no host read in between): a window whose predecessor's exit differs from
//                      the head it used settles again from that head; only lanes whose entry
//                      changed parse.  Exits are double-buffered between rounds.
// crw_settle_kernel    one workgroup a frame walks the windows in order and re-settles those whose
//                      head is still not their predecessor's exit: nothing to do when the rounds
//                      sufficed, and exact whatever the stream.
// crw_scan_kernel      blocks begun in front of every segment (a prefix sum), and the overflow
//                      threshold (with a marker it hangs on the symbol start that met it).
// crw_write_kernel     every lane walks its segment from its true entry and writes the
//                      differences as int16 at pixel 64 block + coefficient; coefficient 0 also
//                      into a list of its own.  The first symbol that fails to parse: an atomic
//                      minimum over its bit position.
// crw_carry_kernel     coefficient 0's running sum over the frame's blocks.
// crw_recon_kernel     one workgroup a row: two scans by column parity from 512, the range check
//                      (an atomic minimum over the pixel), the low bits, 16-byte stores where the
//                      row's address allows.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "rsx_crw.h"
#include "rsx_crw_core.h"
#include "rsx_ljpeg_dev.h"
#include "rsx_plan_host.h"

// bits of a segment (a multiple of 32, at least 64) and segments of a window (= lanes of a
// workgroup, a multiple of 64, at most 1024)
#ifndef RSX_CRW_SEG_BITS
#define RSX_CRW_SEG_BITS 1024
#endif
#ifndef RSX_CRW_WIN_SEGS
#define RSX_CRW_WIN_SEGS 256
#endif

namespace rsx {

using namespace rsx_crw;

namespace {

constexpr uint32_t SEG_BITS = RSX_CRW_SEG_BITS;
constexpr uint32_t SEG_WORDS = SEG_BITS / 32u;
constexpr uint32_t SEG_BYTES = SEG_BITS / 8u;
constexpr uint32_t WIN_SEGS = RSX_CRW_WIN_SEGS;
constexpr uint32_t WIN_WORDS = WIN_SEGS * SEG_WORDS;
// A segment's words and, behind them, the next segment's first word (a symbol that starts in the
// segment's last word ends there); the odd stride also spreads the lanes over the 64 LDS banks.
constexpr uint32_t ROW_WORDS = SEG_WORDS + 1u;
static_assert(SEG_BITS % 32u == 0 && SEG_BITS >= 64u && SEG_BITS <= 32768u, "segment size");
static_assert(SEG_WORDS % 2u == 0, "the row stride must be odd");
static_assert(WIN_SEGS % 64u == 0 && WIN_SEGS <= 1024u, "window size");
static_assert(WIN_SEGS * ROW_WORDS * 4u <= 60u * 1024u, "a window lives in LDS");

constexpr int CHUNK_THREADS = 256;
constexpr uint32_t CHUNK_BYTES = 16u * CHUNK_THREADS; // raw bytes a workgroup compacts
constexpr int SCAN_THREADS = 1024;
constexpr int ROW_THREADS = 256;

// A parser's state at a segment's edge: bits 0..4 how far the first symbol starts behind the edge
// (a symbol has at most 31 bits), bits 5..10 the coefficient index, or DEAD behind a bad code.
constexpr uint32_t ST_DEAD = 0x8000u;
constexpr uint32_t ST_GUESS = 1u << 5;
constexpr uint32_t ST_TRUTH = 0u;

// words of a job's status block
enum { W_PARSE = 0 /* and 1 */, W_RANGE = 2, W_CUT = 3, W_NDATA = 4, W_LIMIT = 5, STATUS_WORDS = 8 };
enum { KIND_BAD_CODE = 0, KIND_OVERFLOW = 1 };
enum { S_INNER = 1, S_OUTER = 2, S_SETTLE = 3 };

struct CrwJobDev {
  uint64_t in_off;  // the scan, from the run's input base
  uint64_t low_off; // the low bits, from the run's input base
  uint64_t out_off; // the image's first pixel, from the run's output base
  uint64_t cb_off;  // the job's compact bytes in cb[]
  uint64_t seg_off; // its segments in entries[], nb[], block_base[]
  uint64_t blk_off; // its blocks in c0[], carry[]
  uint32_t in_bytes; // bytes of the scan that can be read
  uint32_t cb_words; // words of its compact buffer
  uint32_t n_segs, n_wins;
  uint32_t win_off;   // its windows in wexit[][], whead[]
  uint32_t chunk_off; // its chunks in chunk_cnt[]
  uint32_t n_chunks;
  uint32_t n_blocks;
  uint32_t pitch;
  uint32_t job;
  int32_t dim_x, dim_y;
  uint32_t table;
  uint32_t has_low;
};

struct CrwArgs {
  const uint8_t* in_base;
  uint8_t* out_base;
  const CrwJobDev* jobs;
  const Tables* tables; // [table number]
  uint8_t* cb;
  uint32_t* chunk_cnt;
  uint16_t* entries; // per segment: the state it is entered in
  uint16_t* nb;      // per segment: blocks begun in it from that state
  uint32_t* block_base;
  uint16_t* wexit; // [2][total_wins]: the windows' exits, by the parity of the round
  uint16_t* whead; // per window: the head it was settled from
  int16_t* c0;
  int32_t* carry;
  uint32_t* status; // [job of the plan][STATUS_WORDS]
  uint32_t* stats;  // [job of the plan][4]
  uint32_t total_wins;
};

__device__ __forceinline__ uint32_t wave_scan_u32(uint32_t v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t u = __shfl_up(v, d);
    v += lane >= d ? u : 0u;
  }
  return v; // inclusive
}

// inclusive sum over the workgroup's threads in thread order; `sums` has one word a wave
template <int THREADS>
__device__ __forceinline__ uint32_t block_scan_u32(uint32_t v, uint32_t* sums) {
  const int t = int(threadIdx.x), lane = t & 63, wave = t >> 6;
  const uint32_t incl = wave_scan_u32(v, lane);
  __syncthreads(); // (sums may still be read from a call before)
  if (lane == 63)
    sums[wave] = incl;
  __syncthreads();
  uint32_t ex = 0;
  for (int w = 0; w < wave; ++w)
    ex += sums[w];
  return incl + ex;
}

__global__ void __launch_bounds__(ROW_THREADS) crw_zero_kernel(CrwArgs A) {
  const CrwJobDev J = A.jobs[blockIdx.y];
  if (blockIdx.x >= uint32_t(J.dim_y))
    return;
  uint16_t* row =
      reinterpret_cast<uint16_t*>(A.out_base + J.out_off + uint64_t(blockIdx.x) * J.pitch);
  for (uint32_t x = threadIdx.x; x < uint32_t(J.dim_x); x += ROW_THREADS)
    row[x] = 0;
}

// The thread's 16 raw bytes from r0 (0 behind the scan), the byte in front (0 at the start) and
// the byte behind.  keep bit k: byte r0 + k is inside the scan and not the 00 of an FF 00;
// mark bit k: it is an FF with a byte other than 00 behind it inside the scan.
__device__ __forceinline__ void crw_classify(const uint8_t* in, uint32_t size, uint32_t r0,
                                             uint8_t (&b)[16], uint32_t* keep, uint32_t* mark) {
  uint32_t prev = r0 > 0 && r0 - 1u < size ? in[r0 - 1u] : 0u;
  uint32_t k_bits = 0, m_bits = 0;
#pragma unroll
  for (uint32_t k = 0; k < 16; ++k) {
    const uint32_t j = r0 + k;
    const uint32_t v = j < size ? in[j] : 0u;
    b[k] = uint8_t(v);
    if (j < size && !(v == 0u && prev == 0xFFu))
      k_bits |= 1u << k;
    if (prev == 0xFFu && v != 0u && j < size && k > 0)
      m_bits |= 1u << (k - 1u);
    prev = v;
  }
  // (the thread's last byte looks at the byte behind the thread's range)
  if (b[15] == 0xFFu && r0 + 16u < size && in[r0 + 16u] != 0u)
    m_bits |= 1u << 15;
  *keep = k_bits;
  *mark = m_bits;
}

__global__ void __launch_bounds__(CHUNK_THREADS) crw_count_kernel(CrwArgs A) {
  __shared__ uint32_t sums[CHUNK_THREADS / 64];
  const CrwJobDev J = A.jobs[blockIdx.y];
  if (blockIdx.x >= J.n_chunks)
    return;
  const uint8_t* in = A.in_base + J.in_off;
  const uint32_t r0 = blockIdx.x * CHUNK_BYTES + 16u * threadIdx.x;
  uint8_t b[16];
  uint32_t keep, mark;
  crw_classify(in, J.in_bytes, r0, b, &keep, &mark);
  if (mark)
    atomicMin(&A.status[J.job * STATUS_WORDS + W_CUT], r0 + uint32_t(__ffs(int(mark))) - 1u);
  const uint32_t total = block_scan_u32<CHUNK_THREADS>(uint32_t(__popc(keep)), sums);
  if (threadIdx.x == CHUNK_THREADS - 1)
    A.chunk_cnt[J.chunk_off + blockIdx.x] = total;
}

__global__ void __launch_bounds__(CHUNK_THREADS) crw_compact_kernel(CrwArgs A) {
  __shared__ uint32_t sums[CHUNK_THREADS / 64];
  const CrwJobDev J = A.jobs[blockIdx.y];
  if (blockIdx.x >= J.n_chunks)
    return;
  const uint8_t* in = A.in_base + J.in_off;
  const uint32_t cut = A.status[J.job * STATUS_WORDS + W_CUT]; // STATUS_NONE: no marker
  const uint32_t end = cut < J.in_bytes ? cut : J.in_bytes;    // the raw bytes that count
  // data bytes in front of this chunk
  uint32_t part = 0;
  for (uint32_t q = threadIdx.x; q < blockIdx.x; q += CHUNK_THREADS)
    part += A.chunk_cnt[J.chunk_off + q];
  const uint32_t base = block_scan_u32<CHUNK_THREADS>(part, sums);
  __shared__ uint32_t base_all;
  if (threadIdx.x == CHUNK_THREADS - 1)
    base_all = base;
  __syncthreads();
  const uint32_t r0 = blockIdx.x * CHUNK_BYTES + 16u * threadIdx.x;
  uint8_t b[16];
  uint32_t keep, mark;
  crw_classify(in, J.in_bytes, r0, b, &keep, &mark);
  const uint32_t n = uint32_t(__popc(keep));
  uint32_t dest = base_all + block_scan_u32<CHUNK_THREADS>(n, sums) - n;
  uint8_t* out = A.cb + J.cb_off;
  if (end == 0 && r0 == 0)
    A.status[J.job * STATUS_WORDS + W_NDATA] = 0;
#pragma unroll
  for (uint32_t k = 0; k < 16; ++k) {
    const uint32_t j = r0 + k;
    if (j < end && ((keep >> k) & 1u))
      out[dest++] = b[k]; // (dest < in_bytes: inside the job's compact buffer)
    if (j + 1u == end)
      A.status[J.job * STATUS_WORDS + W_NDATA] = dest;
  }
}

// The window's words (and the first one behind it) into LDS, byte-swapped: bit 31 of a word is
// the first bit.  Words behind the job's buffer are zero.
__device__ __forceinline__ void crw_load_window(const CrwArgs& A, const CrwJobDev& J, uint32_t W,
                                                uint32_t* lds) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(A.cb + J.cb_off); // (cb_off: 16-aligned)
  const uint32_t w0 = W * WIN_WORDS;
  for (uint32_t g = threadIdx.x; g <= WIN_WORDS; g += WIN_SEGS) {
    const uint32_t v = w0 + g < J.cb_words ? __builtin_bswap32(src[w0 + g]) : 0u;
    const uint32_t row = g / SEG_WORDS, col = g % SEG_WORDS;
    if (row < WIN_SEGS)
      lds[row * ROW_WORDS + col] = v;
    if (col == 0 && row > 0)
      lds[(row - 1u) * ROW_WORDS + SEG_WORDS] = v;
  }
}

__device__ __forceinline__ void crw_load_tables(const CrwArgs& A, const CrwJobDev& J, Tables* t) {
  const uint16_t* src = reinterpret_cast<const uint16_t*>(A.tables + J.table);
  uint16_t* dst = reinterpret_cast<uint16_t*>(t);
  for (uint32_t k = threadIdx.x; k < sizeof(Tables) / 2u; k += blockDim.x)
    dst[k] = src[k];
}

// the next 32 bits at bit c of the segment whose row starts at `row`
__device__ __forceinline__ uint32_t crw_peek(const uint32_t* row, uint32_t c) {
  const uint32_t k = c >> 5;
  const uint64_t two = uint64_t(row[k]) << 32 | row[k + 1u];
  return uint32_t((two << (c & 31u)) >> 32);
}

// A segment from state `entry`: the state at the next segment's edge and the blocks begun.
__device__ __forceinline__ uint32_t crw_parse_segment(const uint32_t* row, const Tables* t,
                                                      uint32_t entry, uint32_t* begun) {
  *begun = 0;
  if (entry & ST_DEAD)
    return ST_DEAD;
  uint32_t c = entry & 31u, n = 0;
  int32_t i = int32_t(entry >> 5);
  while (c < SEG_BITS) {
    n += i == 0 ? 1u : 0u;
    const Symbol s = symbol(t, crw_peek(row, c), i);
    if (s.used == 0)
      return ST_DEAD;
    c += s.used;
    i = s.next;
  }
  *begun = n;
  return (c - SEG_BITS) | uint32_t(i) << 5;
}

// Window W of job J from state `head`.  first: every lane parses, from the guess; else the lanes
// start from the entries of the window's last settling and only those whose entry changes parse.
// Returns the window's exit (to every thread) and leaves entries[] and nb[] final for this head.
__device__ __forceinline__ uint32_t crw_settle_window(const CrwArgs& A, const CrwJobDev& J,
                                                      uint32_t W, uint32_t head, bool first,
                                                      uint32_t old_exit, uint32_t* lds, Tables* tab,
                                                      uint16_t* ent, uint8_t* flag) {
  const uint32_t t = threadIdx.x, s = W * WIN_SEGS + t;
  const bool valid = s < J.n_segs;
  __syncthreads(); // (LDS may still be read from a window before)
  crw_load_window(A, J, W, lds);
  crw_load_tables(A, J, tab);
  uint32_t mine = first ? ST_GUESS : (valid ? uint32_t(A.entries[J.seg_off + s]) : ST_DEAD);
  bool changed = first;
  if (t == 0) {
    changed = first || mine != head;
    mine = head;
    ent[WIN_SEGS] = uint16_t(first ? ST_DEAD : old_exit);
  }
  ent[t] = uint16_t(mine);
  __syncthreads();
  uint32_t begun = 0, rounds = 0;
  bool parsed = false;
  for (;;) {
    uint32_t ex = ST_DEAD;
    const bool work = changed;
    if (work) {
      mine = ent[t];
      if (valid)
        ex = crw_parse_segment(lds + t * ROW_WORDS, tab, mine, &begun);
      parsed = true;
    }
    // hand the exit forward: lane t + 1 parses again if it is not what it started from
    const bool moves = work && ex != uint32_t(ent[t + 1u]);
    __syncthreads();
    if (work)
      ent[t + 1u] = uint16_t(ex);
    flag[t + 1u] = moves ? 1 : 0;
    ++rounds;
    const int any = __syncthreads_or(moves && t + 1u < WIN_SEGS);
    changed = t > 0 && flag[t] != 0;
    if (!any || rounds > WIN_SEGS)
      break;
  }
  if (valid && parsed) {
    A.entries[J.seg_off + s] = uint16_t(mine);
    A.nb[J.seg_off + s] = uint16_t(begun);
  }
  if (t == 0)
    atomicMax(&A.stats[J.job * 4u + S_INNER], rounds);
  return ent[WIN_SEGS];
}

#define CRW_WINDOW_LDS()                                   \
  __shared__ uint32_t lds[WIN_SEGS * ROW_WORDS];           \
  __shared__ Tables tab;                                   \
  __shared__ uint16_t ent[WIN_SEGS + 1];                   \
  __shared__ uint8_t flag[WIN_SEGS + 1]

__global__ void __launch_bounds__(WIN_SEGS) crw_parse_kernel(CrwArgs A, uint32_t round) {
  CRW_WINDOW_LDS();
  const CrwJobDev J = A.jobs[blockIdx.y];
  const uint32_t W = blockIdx.x;
  if (W >= J.n_wins)
    return;
  uint16_t* cur = A.wexit + (round & 1u) * A.total_wins + J.win_off;
  const uint16_t* prev = A.wexit + ((round + 1u) & 1u) * A.total_wins + J.win_off;
  uint32_t head, old_exit = ST_DEAD;
  if (round == 0) {
    head = W == 0 ? ST_TRUTH : ST_GUESS;
  } else {
    head = W == 0 ? ST_TRUTH : uint32_t(prev[W - 1u]);
    old_exit = prev[W];
    if (head == uint32_t(A.whead[J.win_off + W])) {
      if (threadIdx.x == 0)
        cur[W] = uint16_t(old_exit);
      return;
    }
  }
  const uint32_t ex = crw_settle_window(A, J, W, head, round == 0, old_exit, lds, &tab, ent, flag);
  if (threadIdx.x == 0) {
    cur[W] = uint16_t(ex);
    A.whead[J.win_off + W] = uint16_t(head);
    if (round != 0)
      atomicMax(&A.stats[J.job * 4u + S_OUTER], round);
  }
}

// `last`: the round whose exits are the newest
__global__ void __launch_bounds__(WIN_SEGS) crw_settle_kernel(CrwArgs A, uint32_t last) {
  CRW_WINDOW_LDS();
  const CrwJobDev& J = A.jobs[blockIdx.x]; // (read where used: the loop keeps few of its fields)
  const uint16_t* exits = A.wexit + (last & 1u) * A.total_wins + J.win_off;
  uint32_t before = exits[0]; // (window 0 started from the truth)
  for (uint32_t W = 1; W < J.n_wins; ++W) {
    if (uint32_t(A.whead[J.win_off + W]) == before) {
      before = exits[W];
      continue;
    }
    const uint32_t head = before;
    before = crw_settle_window(A, J, W, head, false, exits[W], lds, &tab, ent, flag);
    if (threadIdx.x == 0) {
      A.whead[J.win_off + W] = uint16_t(head);
      A.stats[J.job * 4u + S_SETTLE] = 1;
    }
  }
}

// the next 32 bits at bit c of the job's compact bytes
__device__ __forceinline__ uint32_t crw_peek_bytes(const uint8_t* cb, uint32_t c) {
  const uint8_t* p = cb + (c >> 3);
  const uint64_t v = uint64_t(p[0]) << 32 | uint64_t(p[1]) << 24 | uint64_t(p[2]) << 16 |
                     uint64_t(p[3]) << 8 | p[4];
  return uint32_t(v >> (8u - (c & 7u)));
}

__global__ void __launch_bounds__(SCAN_THREADS) crw_scan_kernel(CrwArgs A) {
  __shared__ uint32_t sums[SCAN_THREADS / 64];
  __shared__ Tables tab;
  const CrwJobDev J = A.jobs[blockIdx.x];
  crw_load_tables(A, J, &tab);
  const uint16_t* nb = A.nb + J.seg_off;
  const uint16_t* entries = A.entries + J.seg_off;
  const uint32_t per = (J.n_segs + SCAN_THREADS - 1u) / SCAN_THREADS;
  const uint32_t s0 = min(threadIdx.x * per, J.n_segs), s1 = min(s0 + per, J.n_segs);
  uint32_t sum = 0;
  for (uint32_t s = s0; s < s1; ++s)
    sum += (entries[s] & ST_DEAD) ? 0u : nb[s];
  uint32_t at = block_scan_u32<SCAN_THREADS>(sum, sums) - sum;
  for (uint32_t s = s0; s < s1; ++s) {
    A.block_base[J.seg_off + s] = at;
    at += (entries[s] & ST_DEAD) ? 0u : nb[s];
  }
  if (threadIdx.x != 0)
    return;
  // the overflow threshold (rsx_crw_core.h)
  uint32_t* st = A.status + J.job * STATUS_WORDS;
  const uint32_t n_data = st[W_NDATA];
  uint32_t limit = NO_THRESHOLD;
  if (n_data > J.in_bytes) {
    // (cannot be: crw_compact_kernel counts bytes of the scan)
  } else if (st[W_CUT] >= J.in_bytes) {
    const uint8_t* in = A.in_base + J.in_off;
    limit = overflow_threshold(J.in_bytes, n_data, in[J.in_bytes - 1u] == 0xFFu);
  } else {
    // the symbol start that takes the fill which meets the marker
    const int64_t fill_at = marker_fill_threshold(n_data);
    if (fill_at < 0) {
      limit = marker_overflow_threshold(0u);
    } else {
      const uint32_t s = uint32_t(fill_at + 1) / SEG_BITS; // (below 8 n_data: a segment of the job)
      const uint32_t e = entries[s];
      if (!(e & ST_DEAD)) {
        const uint8_t* cb = A.cb + J.cb_off;
        uint32_t c = s * SEG_BITS + (e & 31u);
        int32_t i = int32_t(e >> 5);
        bool ok = true;
        while (ok && int64_t(c) <= fill_at) { // (at most a segment and a symbol of steps)
          const Symbol sy = symbol(&tab, crw_peek_bytes(cb, c), i);
          ok = sy.used != 0;
          c += sy.used;
          i = sy.next;
        }
        if (ok)
          limit = marker_overflow_threshold(c);
      }
    }
  }
  st[W_LIMIT] = limit;
}

__global__ void __launch_bounds__(WIN_SEGS) crw_write_kernel(CrwArgs A) {
  __shared__ uint32_t lds[WIN_SEGS * ROW_WORDS];
  __shared__ Tables tab;
  const CrwJobDev J = A.jobs[blockIdx.y];
  const uint32_t W = blockIdx.x;
  if (W >= J.n_wins)
    return;
  crw_load_window(A, J, W, lds);
  crw_load_tables(A, J, &tab);
  __syncthreads();
  const uint32_t s = W * WIN_SEGS + threadIdx.x;
  if (s >= J.n_segs)
    return;
  const uint32_t e = A.entries[J.seg_off + s];
  if (e & ST_DEAD)
    return;
  uint32_t cnt = A.block_base[J.seg_off + s];
  const uint32_t limit = A.status[J.job * STATUS_WORDS + W_LIMIT];
  unsigned long long* fail =
      reinterpret_cast<unsigned long long*>(A.status + J.job * STATUS_WORDS + W_PARSE);
  const uint32_t* row = lds + threadIdx.x * ROW_WORDS;
  uint8_t* out = A.out_base + J.out_off;
  const uint32_t w = uint32_t(J.dim_x);
  uint32_t c = e & 31u;
  int32_t i = int32_t(e >> 5);
  while (c < SEG_BITS) {
    if (i == 0)
      ++cnt;
    if (cnt == 0 || cnt > J.n_blocks)
      return; // (behind the frame's last block)
    const uint32_t b = cnt - 1u, at_bit = s * SEG_BITS + c;
    if (at_bit > limit) {
      atomicMin(fail, uint64_t(at_bit) << 32 | b << 2 | KIND_OVERFLOW);
      return;
    }
    const Symbol sy = symbol(&tab, crw_peek(row, c), i);
    if (sy.used == 0) {
      atomicMin(fail, uint64_t(at_bit) << 32 | b << 2 | KIND_BAD_CODE);
      return;
    }
    if (sy.at >= 0) {
      const uint32_t p = 64u * b + uint32_t(sy.at);
      *reinterpret_cast<int16_t*>(out + uint64_t(p / w) * J.pitch + 2u * (p % w)) =
          int16_t(sy.diff);
      if (sy.at == 0)
        A.c0[J.blk_off + b] = int16_t(sy.diff);
    }
    c += sy.used;
    i = sy.next;
  }
}

__global__ void __launch_bounds__(SCAN_THREADS) crw_carry_kernel(CrwArgs A) {
  __shared__ uint32_t sums[SCAN_THREADS / 64];
  const CrwJobDev J = A.jobs[blockIdx.x];
  const int16_t* c0 = A.c0 + J.blk_off;
  const uint32_t per = (J.n_blocks + SCAN_THREADS - 1u) / SCAN_THREADS;
  const uint32_t b0 = min(threadIdx.x * per, J.n_blocks), b1 = min(b0 + per, J.n_blocks);
  uint32_t sum = 0; // (two's complement: the sums wrap like the int32 they stand for)
  for (uint32_t b = b0; b < b1; ++b)
    sum += uint32_t(int32_t(c0[b]));
  uint32_t at = block_scan_u32<SCAN_THREADS>(sum, sums) - sum;
  for (uint32_t b = b0; b < b1; ++b) {
    at += uint32_t(int32_t(c0[b]));
    A.carry[J.blk_off + b] = int32_t(at);
  }
}

// the eight differences of pixels p0 .. p0 + 7 of the row at `px` (n of them inside the row)
__device__ __forceinline__ void crw_load8(const uint8_t* px, bool wide, uint32_t n,
                                          const int32_t* carry, uint32_t p0, int32_t (&d)[8]) {
  int16_t v[8];
  if (wide && n == 8u) {
    *reinterpret_cast<uint4*>(v) = *reinterpret_cast<const uint4*>(px);
  } else {
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k)
      v[k] = k < n ? reinterpret_cast<const int16_t*>(px)[k] : int16_t(0);
  }
#pragma unroll
  for (uint32_t k = 0; k < 8; ++k)
    d[k] = ((p0 + k) & 63u) == 0u && k < n ? carry[(p0 + k) >> 6] : int32_t(v[k]);
}

__global__ void __launch_bounds__(ROW_THREADS) crw_recon_kernel(CrwArgs A) {
  __shared__ uint32_t sums[ROW_THREADS / 64];
  const CrwJobDev J = A.jobs[blockIdx.y];
  const uint32_t y = blockIdx.x;
  if (y >= uint32_t(J.dim_y))
    return;
  const uint32_t w = uint32_t(J.dim_x);
  uint8_t* row = A.out_base + J.out_off + uint64_t(y) * J.pitch;
  const bool wide = (reinterpret_cast<uintptr_t>(row) & 15u) == 0;
  const int32_t* carry = A.carry + J.blk_off;
  const uint8_t* low = A.in_base + J.low_off;
  // a thread takes `per` groups of 8 pixels in a row
  const uint32_t groups = (w + 7u) / 8u, per = (groups + ROW_THREADS - 1u) / ROW_THREADS;
  const uint32_t g0 = min(threadIdx.x * per, groups), g1 = min(g0 + per, groups);
  int32_t even = 0, odd = 0;
  for (uint32_t g = g0; g < g1; ++g) {
    int32_t d[8];
    const uint32_t x = 8u * g;
    crw_load8(row + 2u * x, wide, min(8u, w - x), carry, y * w + x, d);
    even += d[0] + d[2] + d[4] + d[6];
    odd += d[1] + d[3] + d[5] + d[7];
  }
  // (two's complement sums; a frame that decodes never wraps)
  int32_t e = int32_t(block_scan_u32<ROW_THREADS>(uint32_t(even), sums)) - even + 512;
  int32_t o = int32_t(block_scan_u32<ROW_THREADS>(uint32_t(odd), sums)) - odd + 512;
  uint32_t first_bad = STATUS_NONE;
  for (uint32_t g = g0; g < g1; ++g) {
    int32_t d[8];
    const uint32_t x = 8u * g, n = min(8u, w - x), p0 = y * w + x;
    crw_load8(row + 2u * x, wide, n, carry, p0, d);
    uint16_t v[8];
    const uint32_t lo0 = J.has_low ? low[p0 >> 2] : 0u;
    const uint32_t lo1 = J.has_low && n > 4u ? low[(p0 >> 2) + 1u] : 0u;
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) {
      int32_t& acc = (k & 1u) ? o : e;
      acc += d[k];
      if (k < n && out_of_range(acc) && first_bad == STATUS_NONE)
        first_bad = p0 + k;
      v[k] = J.has_low ? merge_low(uint32_t(acc) & 1023u, k < 4 ? lo0 : lo1, k & 3u, J.dim_x)
                       : uint16_t(acc);
    }
    if (wide && n == 8u) {
      uint4 q;
      q.x = uint32_t(v[0]) | uint32_t(v[1]) << 16;
      q.y = uint32_t(v[2]) | uint32_t(v[3]) << 16;
      q.z = uint32_t(v[4]) | uint32_t(v[5]) << 16;
      q.w = uint32_t(v[6]) | uint32_t(v[7]) << 16;
      *reinterpret_cast<uint4*>(row + 2u * x) = q;
    } else {
#pragma unroll
      for (uint32_t k = 0; k < 8; ++k)
        if (k < n)
          reinterpret_cast<uint16_t*>(row + 2u * x)[k] = v[k];
    }
  }
  if (first_bad != STATUS_NONE)
    atomicMin(&A.status[J.job * STATUS_WORDS + W_RANGE], first_bad);
}

uint32_t crw_blocks(uint64_t n, uint32_t per) { return uint32_t((n + per - 1) / per); }

} // namespace

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
namespace {
struct CrwPlan final : DecoderPlan {
  rsx_ctx* ctx = nullptr;
  std::vector<CrwJobDev> jobs; // the jobs that go to the device
  std::vector<int> dev_of;     // per job of the plan: its index in `jobs`, or -1
  std::vector<uint32_t> h_stats;
  JobStatus status;
  DeviceBuffer d_jobs, d_tables, d_cb, d_chunks, d_entries, d_nb, d_base, d_wexit, d_whead, d_c0,
      d_carry, d_stats;
  uint64_t cb_bytes = 0, total_blocks = 0;
  uint32_t total_wins = 0, max_wins = 0, max_chunks = 0, max_rows = 0;
  uint32_t spec_rounds = 0;
  int run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) override;
  int results(hipStream_t s, bool ran, int32_t* job_status, uint32_t* job_consumed) override;
};
} // namespace

int crw_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_crw_job* jobs,
                    std::unique_ptr<DecoderPlan>* out) {
  auto p = std::make_unique<CrwPlan>();
  p->ctx = ctx;
  p->spec_rounds = ctx->crw_spec_rounds;
  p->status.host.assign(n_jobs, RSX_OK);
  p->dev_of.assign(n_jobs, -1);
  p->h_stats.assign(size_t(n_jobs) * 4, 0);
  uint64_t segs = 0, chunks = 0;
  for (int i = 0; i < n_jobs; ++i) {
    const rsx_crw_job& j = jobs[i];
    int st = validate(&j.desc, &j.img, j.in_bytes, j.low_bytes);
    if (st == RSX_OK && (j.img_offset % 2 != 0 || j.img.pitch_bytes % 2 != 0))
      st = RSX_ERR_INVALID_ARG;
    p->status.host[i] = st;
    if (st != RSX_OK)
      continue;
    CrwJobDev D;
    std::memset(&D, 0, sizeof D);
    D.in_off = j.in_offset;
    D.low_off = j.low_offset;
    D.out_off = j.img_offset;
    // (at most 9.7e7: what an image of 4104 x 3048 can take; bit positions stay below 2^30)
    D.in_bytes = uint32_t(std::min<uint64_t>(j.in_bytes, image_bound(j.img.dim_x, j.img.dim_y)));
    // the data bytes and the zeros a parse can reach behind them (the thresholds of
    // rsx_crw_core.h lie within 8 n + 223 bits), then one segment that is only ever peeked into
    D.n_segs = crw_blocks(uint64_t(D.in_bytes) + 64u, SEG_BYTES);
    D.cb_words = (D.n_segs + 1u) * SEG_WORDS;
    D.n_wins = crw_blocks(D.n_segs, WIN_SEGS);
    D.n_chunks = crw_blocks(D.in_bytes, CHUNK_BYTES);
    D.n_blocks = uint32_t(j.img.dim_x) * uint32_t(j.img.dim_y) / 64u;
    D.pitch = j.img.pitch_bytes;
    D.job = uint32_t(i);
    D.dim_x = j.img.dim_x;
    D.dim_y = j.img.dim_y;
    D.table = j.desc.dec_table;
    D.has_low = j.desc.has_lowbits != 0;
    D.cb_off = p->cb_bytes;
    p->cb_bytes += (uint64_t(D.cb_words) * 4u + 15u) / 16u * 16u;
    D.seg_off = segs;
    segs += D.n_segs;
    D.win_off = p->total_wins;
    p->total_wins += D.n_wins;
    D.chunk_off = uint32_t(chunks);
    chunks += D.n_chunks;
    D.blk_off = p->total_blocks;
    p->total_blocks += D.n_blocks;
    p->max_wins = std::max(p->max_wins, D.n_wins);
    p->max_chunks = std::max(p->max_chunks, D.n_chunks);
    p->max_rows = std::max(p->max_rows, uint32_t(D.dim_y));
    p->h_stats[size_t(i) * 4] = D.n_wins;
    p->dev_of[i] = int(p->jobs.size());
    p->jobs.push_back(D);
  }
  if (p->jobs.size() > 65535u || chunks > 0xFFFFFFFFull)
    return RSX_ERR_UNSUPPORTED; // (a job is a row of the launches' grids)
  std::vector<Tables> tables(3);
  for (uint32_t t = 0; t < 3; ++t)
    build_tables(t, &tables[t]);
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int st;
  if ((st = upload(ctx, p->d_jobs, p->jobs)) || (st = upload(ctx, p->d_tables, tables)) ||
      (st = p->d_cb.ensure(p->cb_bytes + 16)) || (st = p->d_chunks.ensure(chunks * 4 + 16)) ||
      (st = p->d_entries.ensure(segs * 2 + 16)) || (st = p->d_nb.ensure(segs * 2 + 16)) ||
      (st = p->d_base.ensure(segs * 4 + 16)) ||
      (st = p->d_wexit.ensure(uint64_t(p->total_wins) * 4 + 16)) ||
      (st = p->d_whead.ensure(uint64_t(p->total_wins) * 2 + 16)) ||
      (st = p->d_c0.ensure(p->total_blocks * 2 + 16)) ||
      (st = p->d_carry.ensure(p->total_blocks * 4 + 16)) ||
      (st = p->d_stats.ensure(size_t(n_jobs) * 16 + 16)) || (st = p->status.init(STATUS_WORDS)))
    return st;
  *out = std::move(p);
  return RSX_OK;
}

int CrwPlan::run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) {
  if (jobs.empty())
    return RSX_OK; // (every job was rejected by the host)
  CrwArgs A{};
  A.in_base = static_cast<const uint8_t*>(in_dev);
  A.out_base = static_cast<uint8_t*>(out_dev);
  A.jobs = static_cast<const CrwJobDev*>(d_jobs.ptr);
  A.tables = static_cast<const Tables*>(d_tables.ptr);
  A.cb = static_cast<uint8_t*>(d_cb.ptr);
  A.chunk_cnt = static_cast<uint32_t*>(d_chunks.ptr);
  A.entries = static_cast<uint16_t*>(d_entries.ptr);
  A.nb = static_cast<uint16_t*>(d_nb.ptr);
  A.block_base = static_cast<uint32_t*>(d_base.ptr);
  A.wexit = static_cast<uint16_t*>(d_wexit.ptr);
  A.whead = static_cast<uint16_t*>(d_whead.ptr);
  A.c0 = static_cast<int16_t*>(d_c0.ptr);
  A.carry = static_cast<int32_t*>(d_carry.ptr);
  A.status = static_cast<uint32_t*>(status.dev.ptr);
  A.stats = static_cast<uint32_t*>(d_stats.ptr);
  A.total_wins = total_wins;
  if (int st = status.reset(ctx, s))
    return st;
  if (timer)
    timer->begin(s);
  // (the compact bytes are zero behind the data, a block's coefficient 0 is zero unless written;
  // in a timed run the three fills count with crw_zero_kernel, the launch behind them)
  RSX_HIP_CHECK(ctx, hipMemsetAsync(d_cb.ptr, 0, cb_bytes, s));
  RSX_HIP_CHECK(ctx, hipMemsetAsync(d_c0.ptr, 0, total_blocks * 2, s));
  RSX_HIP_CHECK(ctx, hipMemsetAsync(d_stats.ptr, 0, h_stats.size() * 4, s));
  const uint32_t n_dev = uint32_t(jobs.size());
  hipLaunchKernelGGL(crw_zero_kernel, dim3(max_rows, n_dev), dim3(ROW_THREADS), 0, s, A);
  if (timer)
    timer->mark("crw_zero_kernel");
  hipLaunchKernelGGL(crw_count_kernel, dim3(max_chunks, n_dev), dim3(CHUNK_THREADS), 0, s, A);
  if (timer)
    timer->mark("crw_count_kernel");
  hipLaunchKernelGGL(crw_compact_kernel, dim3(max_chunks, n_dev), dim3(CHUNK_THREADS), 0, s, A);
  if (timer)
    timer->mark("crw_compact_kernel");
  for (uint32_t round = 0; round <= spec_rounds; ++round) {
    hipLaunchKernelGGL(crw_parse_kernel, dim3(max_wins, n_dev), dim3(WIN_SEGS), 0, s, A, round);
    if (timer)
      timer->mark("crw_parse_kernel");
  }
  hipLaunchKernelGGL(crw_settle_kernel, dim3(n_dev), dim3(WIN_SEGS), 0, s, A, spec_rounds);
  if (timer)
    timer->mark("crw_settle_kernel");
  hipLaunchKernelGGL(crw_scan_kernel, dim3(n_dev), dim3(SCAN_THREADS), 0, s, A);
  if (timer)
    timer->mark("crw_scan_kernel");
  hipLaunchKernelGGL(crw_write_kernel, dim3(max_wins, n_dev), dim3(WIN_SEGS), 0, s, A);
  if (timer)
    timer->mark("crw_write_kernel");
  hipLaunchKernelGGL(crw_carry_kernel, dim3(n_dev), dim3(SCAN_THREADS), 0, s, A);
  if (timer)
    timer->mark("crw_carry_kernel");
  hipLaunchKernelGGL(crw_recon_kernel, dim3(max_rows, n_dev), dim3(ROW_THREADS), 0, s, A);
  if (timer)
    timer->mark("crw_recon_kernel");
  RSX_HIP_CHECK(ctx, hipGetLastError());
  return RSX_OK;
}

// A job's parse word is the least (bit position, block, kind) of the symbols that failed to
// parse, its range word the least failing pixel.  The reference parses block b, then sums its
// pixels: the parse failure decides unless a pixel of an earlier block is out of range.
int CrwPlan::results(hipStream_t s, bool ran, int32_t* job_status, uint32_t* job_consumed) {
  if (job_consumed)
    std::fill(job_consumed, job_consumed + status.host.size(), 0u);
  const bool ran_with_work = ran && !jobs.empty();
  if (ran_with_work) {
    if (int st = status.fetch(ctx, s))
      return st;
    std::vector<uint32_t> got(h_stats.size());
    if (int st = fetch_words(ctx, s, d_stats, 0, got.size(), got.data()))
      return st;
    for (size_t i = 0; i < status.host.size(); ++i)
      for (int k = 1; k < 4; ++k)
        h_stats[4 * i + k] = got[4 * i + k];
  }
  return fold_jobs(status.host.size(), FoldOrder::LAST_FAILING, job_status, [&](size_t i) {
    if (status.host[i] != RSX_OK || !ran_with_work)
      return int(status.host[i]);
    const uint32_t* w = status.words.data() + i * STATUS_WORDS;
    const bool parse = w[W_PARSE] != STATUS_NONE || w[W_PARSE + 1] != STATUS_NONE;
    const bool range = w[W_RANGE] != STATUS_NONE;
    if (parse && (!range || (w[W_PARSE] >> 2) <= w[W_RANGE] / 64u))
      return int((w[W_PARSE] & 3u) == KIND_OVERFLOW ? RSX_ERR_INPUT_OVERFLOW
                                                    : RSX_ERR_BAD_HUFFMAN_CODE);
    return int(range ? RSX_ERR_VALUE_RANGE : RSX_OK);
  });
}

int crw_plan_stats(DecoderPlan* plan, int job, uint32_t* stats) {
  CrwPlan* p = dynamic_cast<CrwPlan*>(plan);
  if (!p || !stats || job < 0 || size_t(job) >= p->dev_of.size())
    return RSX_ERR_INVALID_ARG;
  for (int k = 0; k < 4; ++k)
    stats[k] = p->h_stats[size_t(job) * 4 + k];
  return RSX_OK;
}

} // namespace rsx
