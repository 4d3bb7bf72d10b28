// rsx_dctwrite.hip -- baseline-DCT JPEG tile writer for gfx950: the inverse of rsx_dng_jpeg.hip,
// what libjpeg-turbo's default compressor writes (include/rsx.h section 7e).  The
// arithmetic is rsx_dctwrite_core.h.
//
// The jobs (tiles) of a plan share every launch; a workgroup finds its job by search in a start
// table.  Two grids: "block" workgroups of DCT_THREADS blocks of one job in scan order (dummy
// blocks have a place in it), and "word" workgroups of DCT_WORDS 32-bit words of one job's
// un-stuffed scratch stream, as many as the job's bound allows; those behind the job's last word
// leave at once.  Interval i of a job whose intervals begin at symbol bits S_i lies in the scratch
// words from (S_i >> 5) + i on: no two intervals share a word.  All bit offsets are 64-bit.
//   dctwrite_transform_kernel  a wavefront eight blocks at a time, a lane a (block, row): the
//                              gather with clamped coordinates, colour conversion and box filter
//                              fused in; the row pass; the transpose through LDS; the lane as
//                              (block, column): the column pass and the quantiser by reciprocal;
//                              again through LDS into zig-zag order, 16 bytes a lane to scratch.
//                              Dummy blocks are not transformed.  A sample above 255 sets the
//                              workgroup's flag word.
//   dctwrite_length_kernel     a lane a block: DC difference against the component's last real
//                              block of the interval, the block's symbol bits, the workgroup's sum.
//   dctwrite_scan_kernel       a workgroup a job: the exclusive scan of the workgroups' sums (phase
//                              two of three), the job's bits, the OR of its flags.
//   dctwrite_offsets_kernel    phase three: every block's first bit; S_i from the block that opens
//                              interval i.
//   dctwrite_zero_kernel       the job's scratch words up to its last one to zero.
//   dctwrite_emit_kernel       a lane a block: the symbols again into a 64-bit accumulator; whole
//                              words are plain stores, the block's first and a partial last word
//                              vector atomicOr on the zeroed stream.
//   dctwrite_count_kernel      a lane four scratch words: their bytes of the closed interval (1-bits
//                              applied), the FF bytes, 2 for the marker or EOI behind an interval.
//   dctwrite_place_kernel      a workgroup a job: the scan of those counts; the job's result.
//   dctwrite_stuff_kernel      header, bytes with their 00s, markers and EOI to their places;
//                              nothing for a job whose status is not RSX_OK.
// All stores are ordinary vector stores and vector atomics in plain HIP C++.
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <vector>

#include "rsx_dctwrite.h"
#include "rsx_dctwrite_core.h"
#include "rsx_ljpeg_dev.h"
#include "rsx_plan_host.h"

namespace rsx {

using namespace rsx_dctw;

namespace {

constexpr uint32_t DCT_THREADS = 256;
constexpr uint32_t DCT_WORDS = 4 * DCT_THREADS; // scratch words of a word workgroup
constexpr uint32_t FLAG_RANGE = 1u;

__constant__ uint8_t ZZ_DEV[64] = RSX_DCT_ZIGZAG;

struct Args {
  const uint8_t* in_base;
  uint8_t* out_base;
  const Geom* jobs;
  const uint32_t* bwg_starts; // first block workgroup of every job, and the total behind them
  const uint32_t* wwg_starts; // ... word workgroup
  const HuffEnc* huff;
  const uint16_t* qtab;    // 2 x 64 entries a job, natural order
  const uint8_t* headers;  // the jobs' SOI .. SOS bytes
  int16_t* coef;           // 64 a block, zig-zag order
  uint32_t* block_bits;    // a block's symbol bits
  uint64_t* block_off;     // ... and its first bit in the job
  uint32_t* bwg_bits;      // a block workgroup's symbol bits
  uint64_t* bwg_off;       // ... and its first bit in the job
  uint32_t* bwg_flags;     // FLAG_RANGE
  uint64_t* job_bits;      // a job's symbol bits
  uint32_t* job_flags;
  uint64_t* int_start;     // S_i of every interval
  uint32_t* scratch;       // stream bytes 4 k .. 4 k + 3 in word k, the first one on top
  uint32_t* wwg_count;     // a word workgroup's output bytes
  uint64_t* wwg_off;       // ... and its first byte behind the job's header
  rsx_dctwrite_result* results;
  uint32_t n_jobs;
};

__device__ __forceinline__ uint32_t find_job(const uint32_t* __restrict__ starts, uint32_t n,
                                             uint32_t at) {
  uint32_t lo = 0, hi = n - 1u;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1u) >> 1;
    if (starts[mid] <= at)
      lo = mid;
    else
      hi = mid - 1u;
  }
  return lo;
}

// exclusive scan over the workgroup's DCT_THREADS lanes and the total; lds: 4 entries
template <class T>
__device__ __forceinline__ T block_scan(T v, T* total, T* lds) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  T inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(inc, o, 64);
    if (lane >= uint32_t(o))
      inc += t;
  }
  __syncthreads(); // (the reads of the scan before are done)
  if (lane == 63u)
    lds[wave] = inc;
  __syncthreads();
  T base = 0, tot = 0;
#pragma unroll
  for (uint32_t w = 0; w < DCT_THREADS / 64; ++w) {
    const T x = lds[w];
    base += w < wave ? x : T(0);
    tot += x;
  }
  *total = tot;
  return base + inc - v;
}

__global__ __launch_bounds__(DCT_THREADS) void dctwrite_transform_kernel(Args A) {
  __shared__ int ws[32 * 72];       // a block's 8 x 8 behind the row pass, rows 9 apart
  __shared__ int16_t nat[32 * 64];  // quantised, natural order
  __shared__ uint16_t qq[128];
  __shared__ uint32_t rq[128];
  const uint32_t job = find_job(A.bwg_starts, A.n_jobs, blockIdx.x);
  const Geom g = A.jobs[job];
  if (threadIdx.x < 128u) {
    const uint32_t q = A.qtab[size_t(job) * 128u + threadIdx.x];
    qq[threadIdx.x] = uint16_t(q);
    rq[threadIdx.x] = recip_of(q);
  }
  __syncthreads();
  const uint32_t lb0 = (blockIdx.x - g.first_bwg) * DCT_THREADS;
  const uint32_t bl = threadIdx.x >> 3, r = threadIdx.x & 7u;
  bool over = false;
  for (uint32_t it = 0; it < DCT_THREADS / 32u; ++it) {
    const uint32_t lb = lb0 + it * 32u + bl;
    Where w{};
    bool active = lb < g.n_blocks;
    if (active) {
      w = where_of(g, lb);
      active = !w.dummy;
    }
    int d[8];
    if (active) {
      block_row(g, A.in_base, w, r, d, &over);
      fdct_pass<true>(d);
#pragma unroll
      for (uint32_t i = 0; i < 8; ++i)
        ws[bl * 72u + r * 9u + i] = d[i];
    }
    __syncthreads();
    if (active) {
      const uint32_t t = w.comp ? 64u : 0u;
#pragma unroll
      for (uint32_t i = 0; i < 8; ++i)
        d[i] = ws[bl * 72u + i * 9u + r];
      fdct_pass<false>(d);
#pragma unroll
      for (uint32_t i = 0; i < 8; ++i) {
        const uint32_t n = i * 8u + r;
        nat[bl * 64u + n] = int16_t(quantise(d[i], qq[t + n], rq[t + n]));
      }
    }
    __syncthreads();
    if (active) {
      uint32_t p[4];
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t lo = uint16_t(nat[bl * 64u + ZZ_DEV[r * 8u + 2u * j]]);
        const uint32_t hi = uint16_t(nat[bl * 64u + ZZ_DEV[r * 8u + 2u * j + 1u]]);
        p[j] = lo | (hi << 16);
      }
      uint4* dst = reinterpret_cast<uint4*>(A.coef + (size_t(g.first_block) + lb) * 64u) + r;
      *dst = make_uint4(p[0], p[1], p[2], p[3]);
    }
  }
  if (__syncthreads_or(over) && threadIdx.x == 0)
    A.bwg_flags[blockIdx.x] = FLAG_RANGE;
  else if (threadIdx.x == 0)
    A.bwg_flags[blockIdx.x] = 0u;
}

// a block's coefficients as the walk reads them: 16 bytes at a time, picked apart by selects
struct CoefReader {
  const uint4* p;
  uint4 cur;
  uint32_t have;
  __device__ __forceinline__ int operator()(uint32_t k) {
    const uint32_t c = k >> 3;
    if (c != have) {
      cur = p[c];
      have = c;
    }
    const uint32_t s = (k >> 1) & 3u;
    const uint32_t word = s == 0 ? cur.x : s == 1 ? cur.y : s == 2 ? cur.z : cur.w;
    return int(int16_t((k & 1u) ? word >> 16 : word & 0xFFFFu));
  }
};

struct CountSink {
  uint32_t bits;
  __device__ __forceinline__ void put(uint32_t, uint32_t len) { bits += len; }
};

struct EmitSink {
  uint32_t* w;
  uint64_t acc;
  uint32_t n;
  bool first;
  __device__ __forceinline__ void put(uint32_t v, uint32_t len) {
    acc = (acc << len) | v;
    n += len;
    if (n >= 32u) {
      const uint32_t word = uint32_t(acc >> (n - 32u));
      if (first) {
        atomicOr(w, word);
        first = false;
      } else {
        *w = word;
      }
      ++w;
      n -= 32u;
    }
  }
  __device__ __forceinline__ void finish() {
    if (n)
      atomicOr(w, uint32_t(acc << (32u - n)));
  }
};

__device__ __forceinline__ void load_huff(const Args& A, HuffEnc* h) {
  static_assert(sizeof(HuffEnc) % 4 == 0, "copied as words");
  const uint32_t* src = reinterpret_cast<const uint32_t*>(A.huff);
  uint32_t* dst = reinterpret_cast<uint32_t*>(h);
  for (uint32_t k = threadIdx.x; k < sizeof(HuffEnc) / 4; k += DCT_THREADS)
    dst[k] = src[k];
  __syncthreads();
}

// the symbols of block lb of the job into sink
template <class Sink>
__device__ __forceinline__ void block_symbols(const Args& A, const Geom& g, const HuffEnc& h,
                                              uint32_t lb, Sink& sink) {
  const Where w = where_of(g, lb);
  const int16_t* base = A.coef + size_t(g.first_block) * 64u;
  int diff = 0;
  if (!w.dummy) {
    uint32_t prev;
    const int pred = predictor_block(g, lb, &prev) ? int(base[size_t(prev) * 64u]) : 0;
    diff = int(base[size_t(lb) * 64u]) - pred;
  }
  CoefReader rd{reinterpret_cast<const uint4*>(base + size_t(lb) * 64u), make_uint4(0, 0, 0, 0), ~0u};
  walk_block(h, w.comp ? 1u : 0u, diff, w.dummy, rd, sink);
}

__global__ __launch_bounds__(DCT_THREADS) void dctwrite_length_kernel(Args A) {
  __shared__ HuffEnc huff;
  __shared__ uint32_t sums[4];
  const uint32_t job = find_job(A.bwg_starts, A.n_jobs, blockIdx.x);
  const Geom g = A.jobs[job];
  load_huff(A, &huff);
  const uint32_t lb = (blockIdx.x - g.first_bwg) * DCT_THREADS + threadIdx.x;
  CountSink sink{0u};
  if (lb < g.n_blocks) {
    block_symbols(A, g, huff, lb, sink);
    A.block_bits[size_t(g.first_block) + lb] = sink.bits;
  }
  uint32_t total;
  block_scan(sink.bits, &total, sums);
  if (threadIdx.x == 0)
    A.bwg_bits[blockIdx.x] = total;
}

__global__ __launch_bounds__(DCT_THREADS) void dctwrite_scan_kernel(Args A) {
  __shared__ uint64_t sums[4];
  const uint32_t job = blockIdx.x;
  const Geom g = A.jobs[job];
  const uint32_t n_bwg = A.bwg_starts[job + 1u] - g.first_bwg;
  uint64_t running = 0;
  uint32_t flags = 0;
  for (uint32_t base = 0; base < n_bwg; base += DCT_THREADS) {
    const uint32_t b = base + threadIdx.x;
    const uint64_t v = b < n_bwg ? A.bwg_bits[g.first_bwg + b] : 0u;
    flags |= b < n_bwg ? A.bwg_flags[g.first_bwg + b] : 0u;
    uint64_t total;
    const uint64_t off = running + block_scan(v, &total, sums);
    if (b < n_bwg)
      A.bwg_off[g.first_bwg + b] = off;
    running += total;
  }
  const bool range = __syncthreads_or(int(flags & FLAG_RANGE)) != 0;
  if (threadIdx.x == 0) {
    A.job_bits[job] = running;
    A.job_flags[job] = range ? FLAG_RANGE : 0u;
  }
}

__global__ __launch_bounds__(DCT_THREADS) void dctwrite_offsets_kernel(Args A) {
  __shared__ uint64_t sums[4];
  const uint32_t job = find_job(A.bwg_starts, A.n_jobs, blockIdx.x);
  const Geom g = A.jobs[job];
  const uint32_t lb = (blockIdx.x - g.first_bwg) * DCT_THREADS + threadIdx.x;
  const uint64_t v = lb < g.n_blocks ? A.block_bits[size_t(g.first_block) + lb] : 0u;
  uint64_t total;
  const uint64_t off = A.bwg_off[blockIdx.x] + block_scan(v, &total, sums);
  if (lb < g.n_blocks) {
    A.block_off[size_t(g.first_block) + lb] = off;
    const uint32_t per = g.ri * g.bpm; // blocks an interval
    if (lb % per == 0)
      A.int_start[size_t(g.first_int) + lb / per] = off;
  }
}

// the job's scratch words in use: interval i takes the words from (S_i >> 5) + i on
__device__ __forceinline__ uint64_t words_used(const Args& A, const Geom& g, uint32_t job) {
  return (A.job_bits[job] >> 5) + g.n_int;
}

__global__ __launch_bounds__(DCT_THREADS) void dctwrite_zero_kernel(Args A) {
  const uint32_t job = find_job(A.wwg_starts, A.n_jobs, blockIdx.x);
  const Geom g = A.jobs[job];
  const uint64_t wl = uint64_t(blockIdx.x - g.first_wwg) * DCT_WORDS + threadIdx.x * 4u;
  if (wl > words_used(A, g, job))
    return;
  *reinterpret_cast<uint4*>(A.scratch + g.first_word + wl) = make_uint4(0, 0, 0, 0);
}

__global__ __launch_bounds__(DCT_THREADS) void dctwrite_emit_kernel(Args A) {
  __shared__ HuffEnc huff;
  const uint32_t job = find_job(A.bwg_starts, A.n_jobs, blockIdx.x);
  const Geom g = A.jobs[job];
  load_huff(A, &huff);
  const uint32_t lb = (blockIdx.x - g.first_bwg) * DCT_THREADS + threadIdx.x;
  if (lb >= g.n_blocks)
    return;
  const uint32_t i = lb / (g.ri * g.bpm);
  const uint64_t S = A.int_start[size_t(g.first_int) + i];
  const uint64_t rel = A.block_off[size_t(g.first_block) + lb] - S;
  EmitSink sink{A.scratch + g.first_word + (S >> 5) + i + (rel >> 5), 0ull, uint32_t(rel & 31u), true};
  block_symbols(A, g, huff, lb, sink);
  sink.finish();
}

// scratch word wl of the job: the interval it lies in (interval *i is a guess at or below it), its
// bytes of the closed interval (first byte on top, the closing 1-bits applied), how many, and
// whether the interval ends in it
struct WordInfo {
  uint32_t v, n_bytes, interval;
  bool closes, last;
};

__device__ __forceinline__ uint64_t int_word(const Args& A, const Geom& g, uint32_t i) {
  return (A.int_start[size_t(g.first_int) + i] >> 5) + i;
}

__device__ __forceinline__ uint32_t interval_of(const Args& A, const Geom& g, uint64_t wl) {
  uint32_t lo = 0, hi = g.n_int - 1u;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1u) >> 1;
    if (int_word(A, g, mid) <= wl)
      lo = mid;
    else
      hi = mid - 1u;
  }
  return lo;
}

__device__ __forceinline__ WordInfo word_info(const Args& A, const Geom& g, uint32_t job, uint64_t wl,
                                              uint32_t i) {
  while (i + 1u < g.n_int && int_word(A, g, i + 1u) <= wl)
    ++i;
  WordInfo w{0u, 0u, i, false, i + 1u == g.n_int};
  const uint64_t S = A.int_start[size_t(g.first_int) + i];
  const uint64_t E = w.last ? A.job_bits[job] : A.int_start[size_t(g.first_int) + i + 1u];
  uint32_t ones;
  const uint64_t bytes = interval_bytes(E - S, &ones);
  const uint64_t at = (wl - ((S >> 5) + i)) * 4u;
  if (at >= bytes)
    return w;
  w.v = A.scratch[g.first_word + wl];
  const uint64_t left = bytes - at;
  w.n_bytes = left < 4u ? uint32_t(left) : 4u;
  if (left <= 4u) {
    w.v |= ((1u << ones) - 1u) << (8u * (4u - uint32_t(left)));
    w.closes = true;
  }
  return w;
}

__device__ __forceinline__ uint32_t stuffed_size(const WordInfo& w) {
  uint32_t n = w.n_bytes + (w.closes ? 2u : 0u);
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j)
    n += j < w.n_bytes && (w.v >> (24u - 8u * j) & 0xFFu) == 0xFFu ? 1u : 0u;
  return n;
}

__global__ __launch_bounds__(DCT_THREADS) void dctwrite_count_kernel(Args A) {
  __shared__ uint32_t sums[4];
  const uint32_t job = find_job(A.wwg_starts, A.n_jobs, blockIdx.x);
  const Geom g = A.jobs[job];
  const uint64_t used = words_used(A, g, job);
  const uint64_t wl0 = uint64_t(blockIdx.x - g.first_wwg) * DCT_WORDS;
  if (wl0 >= used)
    return; // (a workgroup's one answer)
  const uint64_t wl = wl0 + threadIdx.x * 4u;
  uint32_t n = 0;
  if (wl < used) {
    uint32_t i = interval_of(A, g, wl);
    for (uint32_t j = 0; j < 4 && wl + j < used; ++j) {
      const WordInfo w = word_info(A, g, job, wl + j, i);
      i = w.interval;
      n += stuffed_size(w);
    }
  }
  uint32_t total;
  block_scan(n, &total, sums);
  if (threadIdx.x == 0)
    A.wwg_count[blockIdx.x] = total;
}

__global__ __launch_bounds__(DCT_THREADS) void dctwrite_place_kernel(Args A) {
  __shared__ uint64_t sums[4];
  const uint32_t job = blockIdx.x;
  const Geom g = A.jobs[job];
  const uint64_t used = words_used(A, g, job);
  const uint32_t n_wwg = uint32_t((used + DCT_WORDS - 1u) / DCT_WORDS);
  uint64_t running = 0;
  for (uint32_t base = 0; base < n_wwg; base += DCT_THREADS) {
    const uint32_t b = base + threadIdx.x;
    const uint64_t v = b < n_wwg ? A.wwg_count[g.first_wwg + b] : 0u;
    uint64_t total;
    const uint64_t off = running + block_scan(v, &total, sums);
    if (b < n_wwg)
      A.wwg_off[g.first_wwg + b] = off;
    running += total;
  }
  if (threadIdx.x == 0) {
    rsx_dctwrite_result r;
    const uint64_t bytes = uint64_t(g.hdr_bytes) + running;
    r.status = (A.job_flags[job] & FLAG_RANGE) ? RSX_ERR_VALUE_RANGE
               : bytes > g.out_cap             ? RSX_ERR_INPUT_OVERFLOW
                                               : RSX_OK;
    r.reserved = 0;
    r.bytes = r.status == RSX_OK ? bytes : 0u;
    r.scan_bytes = r.status == RSX_OK ? running - 2u : 0u;
    r.symbol_bits = r.status == RSX_OK ? A.job_bits[job] : 0u;
    A.results[job] = r;
  }
}

__global__ __launch_bounds__(DCT_THREADS) void dctwrite_stuff_kernel(Args A) {
  __shared__ uint32_t sums[4];
  const uint32_t job = find_job(A.wwg_starts, A.n_jobs, blockIdx.x);
  if (A.results[job].status != RSX_OK)
    return; // (a workgroup's one answer: nothing of a failed job is written)
  const Geom g = A.jobs[job];
  const uint64_t used = words_used(A, g, job);
  const uint64_t wl0 = uint64_t(blockIdx.x - g.first_wwg) * DCT_WORDS;
  if (wl0 >= used)
    return;
  uint8_t* out = A.out_base + g.out_off;
  if (wl0 == 0)
    for (uint32_t k = threadIdx.x; k < g.hdr_bytes; k += DCT_THREADS)
      out[k] = A.headers[g.hdr_off + k];
  const uint64_t wl = wl0 + threadIdx.x * 4u;
  WordInfo w[4] = {};
  uint32_t n = 0;
  if (wl < used) {
    uint32_t i = interval_of(A, g, wl);
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      w[j] = wl + j < used ? word_info(A, g, job, wl + j, i) : WordInfo{0u, 0u, i, false, false};
      i = w[j].interval;
      n += stuffed_size(w[j]);
    }
  }
  uint32_t total;
  const uint32_t before = block_scan(n, &total, sums);
  if (wl >= used)
    return;
  uint8_t* dst = out + g.hdr_bytes + A.wwg_off[blockIdx.x] + before;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      if (k < w[j].n_bytes) {
        const uint8_t b = uint8_t(w[j].v >> (24u - 8u * k));
        *dst++ = b;
        if (b == 0xFFu)
          *dst++ = 0x00u;
      }
    }
    if (w[j].closes) {
      *dst++ = 0xFFu;
      *dst++ = w[j].last ? uint8_t(0xD9u) : uint8_t(0xD0u + w[j].interval % 8u);
    }
  }
}

struct DctWritePlan final : DecoderPlan {
  rsx_ctx* ctx = nullptr;
  std::vector<int32_t> host;  // validation result per job
  std::vector<int> dev_index; // the job's place among those that go to the device, or -1
  std::vector<Geom> jobs;     // the jobs that go to the device
  std::vector<uint32_t> bwg_starts, wwg_starts;
  std::vector<uint16_t> qtab;
  std::vector<uint8_t> headers;
  std::vector<rsx_dctwrite_result> fetched;
  bool have_results = false;
  DeviceBuffer d_jobs, d_bwg_starts, d_wwg_starts, d_huff, d_qtab, d_headers, d_coef, d_block_bits,
      d_block_off, d_bwg_bits, d_bwg_off, d_bwg_flags, d_job_bits, d_job_flags, d_int_start,
      d_scratch, d_wwg_count, d_wwg_off, d_results;
  uint64_t total_blocks = 0, total_bwg = 0, total_ints = 0, total_wwg = 0, total_words = 0;

  int finish() {
    if (jobs.empty())
      return RSX_OK;
    bwg_starts.push_back(uint32_t(total_bwg));
    wwg_starts.push_back(uint32_t(total_wwg));
    std::vector<HuffEnc> huff(1);
    build_huff(&huff[0]);
    RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (int st = upload(ctx, d_jobs, jobs))
      return st;
    if (int st = upload(ctx, d_bwg_starts, bwg_starts))
      return st;
    if (int st = upload(ctx, d_wwg_starts, wwg_starts))
      return st;
    if (int st = upload(ctx, d_huff, huff))
      return st;
    if (int st = upload(ctx, d_qtab, qtab))
      return st;
    if (int st = upload(ctx, d_headers, headers))
      return st;
    const size_t nb = size_t(total_blocks), nj = jobs.size(), nw = size_t(total_bwg);
    int st = d_coef.ensure(nb * 128 + 16);
    st = st ? st : d_block_bits.ensure(nb * 4 + 16);
    st = st ? st : d_block_off.ensure(nb * 8 + 16);
    st = st ? st : d_bwg_bits.ensure(nw * 4 + 16);
    st = st ? st : d_bwg_off.ensure(nw * 8 + 16);
    st = st ? st : d_bwg_flags.ensure(nw * 4 + 16);
    st = st ? st : d_job_bits.ensure(nj * 8 + 16);
    st = st ? st : d_job_flags.ensure(nj * 4 + 16);
    st = st ? st : d_int_start.ensure(size_t(total_ints) * 8 + 16);
    st = st ? st : d_scratch.ensure(size_t(total_words) * 4 + 16);
    st = st ? st : d_wwg_count.ensure(size_t(total_wwg) * 4 + 16);
    st = st ? st : d_wwg_off.ensure(size_t(total_wwg) * 8 + 16);
    st = st ? st : d_results.ensure(nj * sizeof(rsx_dctwrite_result) + 16);
    return st;
  }
  int run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) override {
    have_results = false;
    if (jobs.empty())
      return RSX_OK; // (every job was refused by the host)
    if (reinterpret_cast<uintptr_t>(in_dev) % 2u != 0)
      return RSX_ERR_INVALID_ARG;
    Args A{};
    A.in_base = static_cast<const uint8_t*>(in_dev);
    A.out_base = static_cast<uint8_t*>(out_dev);
    A.jobs = static_cast<const Geom*>(d_jobs.ptr);
    A.bwg_starts = static_cast<const uint32_t*>(d_bwg_starts.ptr);
    A.wwg_starts = static_cast<const uint32_t*>(d_wwg_starts.ptr);
    A.huff = static_cast<const HuffEnc*>(d_huff.ptr);
    A.qtab = static_cast<const uint16_t*>(d_qtab.ptr);
    A.headers = static_cast<const uint8_t*>(d_headers.ptr);
    A.coef = static_cast<int16_t*>(d_coef.ptr);
    A.block_bits = static_cast<uint32_t*>(d_block_bits.ptr);
    A.block_off = static_cast<uint64_t*>(d_block_off.ptr);
    A.bwg_bits = static_cast<uint32_t*>(d_bwg_bits.ptr);
    A.bwg_off = static_cast<uint64_t*>(d_bwg_off.ptr);
    A.bwg_flags = static_cast<uint32_t*>(d_bwg_flags.ptr);
    A.job_bits = static_cast<uint64_t*>(d_job_bits.ptr);
    A.job_flags = static_cast<uint32_t*>(d_job_flags.ptr);
    A.int_start = static_cast<uint64_t*>(d_int_start.ptr);
    A.scratch = static_cast<uint32_t*>(d_scratch.ptr);
    A.wwg_count = static_cast<uint32_t*>(d_wwg_count.ptr);
    A.wwg_off = static_cast<uint64_t*>(d_wwg_off.ptr);
    A.results = static_cast<rsx_dctwrite_result*>(d_results.ptr);
    A.n_jobs = uint32_t(jobs.size());
    const dim3 threads(DCT_THREADS), bwg{uint32_t(total_bwg)}, wwg{uint32_t(total_wwg)},
        per_job{A.n_jobs};
    if (timer)
      timer->begin(s);
    auto mark = [&](const char* name) {
      if (timer)
        timer->mark(name);
    };
    hipLaunchKernelGGL(dctwrite_transform_kernel, bwg, threads, 0, s, A);
    mark("dctwrite_transform_kernel");
    hipLaunchKernelGGL(dctwrite_length_kernel, bwg, threads, 0, s, A);
    mark("dctwrite_length_kernel");
    hipLaunchKernelGGL(dctwrite_scan_kernel, per_job, threads, 0, s, A);
    mark("dctwrite_scan_kernel");
    hipLaunchKernelGGL(dctwrite_offsets_kernel, bwg, threads, 0, s, A);
    mark("dctwrite_offsets_kernel");
    hipLaunchKernelGGL(dctwrite_zero_kernel, wwg, threads, 0, s, A);
    mark("dctwrite_zero_kernel");
    hipLaunchKernelGGL(dctwrite_emit_kernel, bwg, threads, 0, s, A);
    mark("dctwrite_emit_kernel");
    hipLaunchKernelGGL(dctwrite_count_kernel, wwg, threads, 0, s, A);
    mark("dctwrite_count_kernel");
    hipLaunchKernelGGL(dctwrite_place_kernel, per_job, threads, 0, s, A);
    mark("dctwrite_place_kernel");
    hipLaunchKernelGGL(dctwrite_stuff_kernel, wwg, threads, 0, s, A);
    mark("dctwrite_stuff_kernel");
    RSX_HIP_CHECK(ctx, hipGetLastError());
    return RSX_OK;
  }
  int results(hipStream_t s, bool ran, int32_t* job_status, uint32_t* job_consumed) override {
    fetched.assign(jobs.size(), rsx_dctwrite_result{});
    const bool with_work = ran && !jobs.empty();
    if (with_work) {
      RSX_HIP_CHECK(ctx, hipMemcpyAsync(fetched.data(), d_results.ptr,
                                        jobs.size() * sizeof(rsx_dctwrite_result),
                                        hipMemcpyDeviceToHost, s));
      RSX_HIP_CHECK(ctx, hipStreamSynchronize(s));
    }
    have_results = with_work;
    if (job_consumed)
      for (size_t i = 0; i < host.size(); ++i)
        job_consumed[i] = dev_index[i] >= 0 ? uint32_t(fetched[size_t(dev_index[i])].bytes) : 0u;
    return fold_jobs(host.size(), FoldOrder::LAST_FAILING, job_status, [&](size_t i) {
      return host[i] != RSX_OK || !with_work ? int(host[i]) : int(fetched[size_t(dev_index[i])].status);
    });
  }
  int dctwrite_result(int job, rsx_dctwrite_result* out) override {
    if (job < 0 || size_t(job) >= host.size() || !out)
      return RSX_ERR_INVALID_ARG;
    std::memset(out, 0, sizeof *out);
    if (host[size_t(job)] != RSX_OK) {
      out->status = host[size_t(job)];
      return RSX_OK;
    }
    if (!have_results)
      return RSX_ERR_INVALID_ARG;
    *out = fetched[size_t(dev_index[size_t(job)])];
    return RSX_OK;
  }
};

} // namespace

int dctwrite_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_dctwrite_job* jobs,
                         std::unique_ptr<DecoderPlan>* out) {
  auto p = std::make_unique<DctWritePlan>();
  p->ctx = ctx;
  p->host.assign(n_jobs, RSX_OK);
  p->dev_index.assign(n_jobs, -1);
  for (int i = 0; i < n_jobs; ++i) {
    const rsx_dctwrite_job& j = jobs[i];
    int st = validate(&j.desc, &j.img);
    if (st == RSX_OK && j.img_offset % 2u != 0)
      st = RSX_ERR_INVALID_ARG;
    p->host[i] = st;
    if (st != RSX_OK)
      continue;
    Geom g;
    geom_of(j.desc, j.img, j.img_offset, j.out_offset, j.out_cap, &g);
    const uint64_t n_bwg = (uint64_t(g.n_blocks) + DCT_THREADS - 1u) / DCT_THREADS;
    // (the words of the symbol bits, one more an interval, and the word behind the last)
    uint64_t words = (uint64_t(g.n_blocks) * BLOCK_BITS_MAX + 31u) / 32u + g.n_int + 2u;
    words = (words + DCT_WORDS - 1u) / DCT_WORDS * DCT_WORDS;
    if (p->total_blocks + g.n_blocks > 0x7FFFFFFFull || p->total_wwg + words / DCT_WORDS > 0x7FFFFFFFull)
      return RSX_ERR_UNSUPPORTED; // (a launch's grid)
    g.first_block = uint32_t(p->total_blocks);
    g.first_bwg = uint32_t(p->total_bwg);
    g.first_int = uint32_t(p->total_ints);
    g.first_wwg = uint32_t(p->total_wwg);
    g.first_word = p->total_words;
    g.words_bound = words;
    g.hdr_off = uint32_t(p->headers.size());
    g.q_index = uint32_t(p->jobs.size());
    write_header(j.desc, &p->headers);
    for (int t = 0; t < 2; ++t)
      for (int k = 0; k < 64; ++k) // (a grey job's second table is not read; any entry will do)
        p->qtab.push_back(j.desc.components > 1 || t == 0 ? j.desc.qtables[t][k] : uint16_t(1));
    p->bwg_starts.push_back(g.first_bwg);
    p->wwg_starts.push_back(g.first_wwg);
    p->total_blocks += g.n_blocks;
    p->total_bwg += n_bwg;
    p->total_ints += g.n_int;
    p->total_wwg += words / DCT_WORDS;
    p->total_words += words;
    p->dev_index[i] = int(p->jobs.size());
    p->jobs.push_back(g);
  }
  if (int st = p->finish())
    return st;
  *out = std::move(p);
  return RSX_OK;
}

} // namespace rsx
