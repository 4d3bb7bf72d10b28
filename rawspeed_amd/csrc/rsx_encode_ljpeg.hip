// rsx_encode_ljpeg.hip -- lossless-JPEG scan writer for gfx950: the inverse of
// LJpegDecompressor::decode, what PrefixCodeVectorEncoder::encodeDifference over a BitVacuumerJPEG
// writes (include/rsx.h section 7b and 7c).  The arithmetic is rsx_encode_core.h.
//
// A lane a sample, a workgroup LJPEG_RUN consecutive samples of one restart interval of one job
// (intervals start on workgroup boundaries); the jobs of a plan share every launch, a workgroup
// finds its job by search in the plan's start table.  A symbol word is at most 32 bits, so a
// workgroup's samples fill at most LJPEG_RUN words: interval i of a job owns the words of its
// workgroups in the plan's un-stuffed scratch stream, and run k of those words is workgroup k's to
// stuff.  All bit offsets are 64-bit.
//   encode_ljpeg_clear_kernel    the jobs' flag words (or the counts of a histogram plan) to zero:
//                                nothing relies on a memset having run.
//   encode_ljpeg_length_kernel   predictor, reduce, symbol length from the 17-entry tables of the
//                                job's components in LDS; the workgroup's bit total; the
//                                missing-category flag (a vector atomic OR on the job's word).  Its
//                                histogram form counts the categories per component in LDS and adds
//                                the non-zero cells with one vector atomic each.
//   encode_ljpeg_scan_kernel     a workgroup an interval: the exclusive scan of its workgroups'
//                                totals and the interval's total; it zeroes the scratch word at
//                                every workgroup's first bit and at the interval's end -- the only
//                                words two writers share.
//   encode_ljpeg_emit_kernel     the symbol words again, OR-ed at their offsets into LDS; whole
//                                32-bit words to the scratch stream, the first and a partial last
//                                one with vector atomicOr on the zeroed words.
//   encode_ljpeg_count_kernel    per run of LJPEG_RUN_BYTES scratch bytes: its bytes of the closed
//                                interval (tail rule applied) plus its FF bytes.
//   encode_ljpeg_place_kernel    a workgroup a job: the scan of those counts with 2 for every
//                                marker; the job's result (status, bytes, symbol bits).
//   encode_ljpeg_stuff_kernel    the bytes to their final places with the 00s, the interval tails
//                                and the markers; nothing for a job whose status is not RSX_OK.
// All stores are ordinary vector stores and vector atomics in plain HIP C++.
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <vector>

#include "rsx_encode.h"
#include "rsx_encode_core.h"
#include "rsx_ljpeg_dev.h"
#include "rsx_plan_host.h"

namespace rsx {

using namespace rsx_encode;

namespace {

constexpr uint32_t FLAG_MISSING = 1u;

struct EncArgs {
  const uint8_t* in_base;
  uint8_t* out_base;
  const LJpegGeom* jobs;
  const uint32_t* block_starts; // first_block of every job, and the total behind them
  const uint32_t* int_starts;   // first_int of every job, and the total behind them
  const EncTable* tables;
  uint32_t* flags;              // a word a job
  uint32_t* block_bits;         // a workgroup's symbol bits
  uint64_t* block_off;          // ... and its first bit, from the interval's
  uint64_t* int_bits;           // an interval's symbol bits
  uint32_t* scratch;            // LJPEG_RUN words a workgroup: stream bytes 4 k .. 4 k + 3 in word k,
                                // the first one on top
  uint32_t* run_count;          // a run's bytes plus its FF bytes
  uint64_t* run_off;            // ... and its first byte in the job's output
  rsx_encode_result* results;
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

// exclusive scan over the workgroup's LJPEG_THREADS lanes and the total; lds: 4 entries
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
  for (uint32_t w = 0; w < LJPEG_THREADS / 64; ++w) {
    const T x = lds[w];
    base += w < wave ? x : T(0);
    tot += x;
  }
  *total = tot;
  return base + inc - v;
}

// where a workgroup stands: its job, its interval and that interval's shape
struct Where {
  uint32_t job, interval, run; // run: the workgroup's number in the interval
  uint32_t first_block;        // of the interval, in the plan's list
  uint32_t r0;                 // the interval's first row
  uint64_t n;                  // its samples
  bool last;
};

__device__ __forceinline__ Where where_of(const EncArgs& A, const LJpegGeom& g, uint32_t job,
                                          uint32_t block) {
  Where w;
  w.job = job;
  const uint32_t lb = block - g.first_block;
  w.interval = lb / g.int_blocks;
  w.run = lb - w.interval * g.int_blocks;
  w.first_block = g.first_block + w.interval * g.int_blocks;
  w.r0 = w.interval * g.rpi;
  const uint32_t rows = g.rows - w.r0 < g.rpi ? g.rows - w.r0 : g.rpi;
  w.n = uint64_t(rows) * g.row_samples;
  w.last = w.interval + 1u == g.n_int;
  return w;
}

// the tables of the job's components into LDS (4 x 17 codes and lengths, 4 fix16 flags)
struct TablesLds {
  uint16_t code[4][N_CATEGORIES];
  uint8_t len[4][N_CATEGORIES];
  uint8_t fix16[4];
};

__device__ __forceinline__ void load_tables(const EncArgs& A, const LJpegGeom& g, TablesLds* t) {
  if (threadIdx.x < 4u * N_CATEGORIES) {
    const uint32_t c = threadIdx.x / N_CATEGORIES, k = threadIdx.x % N_CATEGORIES;
    const EncTable& e = A.tables[g.table_base + g.table[c < g.n_comp ? c : 0u]];
    t->code[c][k] = e.code[k];
    t->len[c][k] = e.len[k];
    if (k == 0)
      t->fix16[c] = e.fix16;
  }
  __syncthreads();
}

// the lane's sample of the workgroup at w: its difference and its component; false behind the end
__device__ __forceinline__ bool lane_difference(const EncArgs& A, const LJpegGeom& g, const Where& w,
                                                int32_t* d, uint32_t* c) {
  const uint64_t idx = uint64_t(w.run) * LJPEG_RUN + threadIdx.x;
  if (idx >= w.n)
    return false;
  const uint32_t r = w.r0 + uint32_t(idx / g.row_samples);
  const uint32_t s = uint32_t(idx % g.row_samples);
  *d = ljpeg_difference(A.in_base, g, r, s);
  *c = s % g.n_comp;
  return true;
}

__global__ __launch_bounds__(LJPEG_THREADS) void encode_ljpeg_clear_kernel(EncArgs A, bool hist) {
  const uint32_t i = blockIdx.x * LJPEG_THREADS + threadIdx.x;
  if (!hist) {
    if (i < A.n_jobs)
      A.flags[i] = 0u;
    return;
  }
  const uint32_t job = i / (4u * N_CATEGORIES), cell = i % (4u * N_CATEGORIES);
  if (job < A.n_jobs)
    reinterpret_cast<unsigned long long*>(A.out_base + A.jobs[job].out_off)[cell] = 0ull;
}

template <bool HIST>
__global__ __launch_bounds__(LJPEG_THREADS) void encode_ljpeg_length_kernel(EncArgs A) {
  __shared__ TablesLds tabs;
  __shared__ uint32_t cells[4 * N_CATEGORIES];
  __shared__ uint32_t sums[4];
  const uint32_t job = find_job(A.block_starts, A.n_jobs, blockIdx.x);
  const LJpegGeom& g = A.jobs[job]; // (in place: init_pred and table are indexed)
  const Where w = where_of(A, g, job, blockIdx.x);
  int32_t d = 0;
  uint32_t c = 0;
  if (HIST) {
    if (threadIdx.x < 4u * N_CATEGORIES)
      cells[threadIdx.x] = 0u;
    __syncthreads();
    if (lane_difference(A, g, w, &d, &c))
      atomicAdd(&cells[c * N_CATEGORIES + category(d)], 1u);
    __syncthreads();
    if (threadIdx.x < 4u * N_CATEGORIES && cells[threadIdx.x] != 0u)
      atomicAdd(reinterpret_cast<unsigned long long*>(A.out_base + g.out_off) + threadIdx.x,
                (unsigned long long)cells[threadIdx.x]);
    return;
  }
  load_tables(A, g, &tabs);
  uint32_t nb = 0;
  bool missing = false;
  if (lane_difference(A, g, w, &d, &c)) {
    symbol(tabs.code[c], tabs.len[c], tabs.fix16[c], d, &nb);
    missing = nb == 0;
  }
  if (__syncthreads_or(missing) && threadIdx.x == 0)
    atomicOr(&A.flags[job], FLAG_MISSING);
  uint32_t total;
  block_scan(nb, &total, sums);
  if (threadIdx.x == 0)
    A.block_bits[blockIdx.x] = total;
}

__global__ __launch_bounds__(LJPEG_THREADS) void encode_ljpeg_scan_kernel(EncArgs A) {
  __shared__ uint64_t sums[4];
  const uint32_t job = find_job(A.int_starts, A.n_jobs, blockIdx.x);
  const LJpegGeom& g = A.jobs[job]; // (in place: init_pred and table are indexed)
  const uint32_t i = blockIdx.x - g.first_int;
  const uint32_t first = g.first_block + i * g.int_blocks;
  const uint32_t n_blocks = i + 1u == g.n_int ? g.n_blocks - i * g.int_blocks : g.int_blocks;
  uint32_t* words = A.scratch + uint64_t(first) * LJPEG_RUN;
  uint64_t running = 0;
  for (uint32_t base = 0; base < n_blocks; base += LJPEG_THREADS) {
    const uint32_t b = base + threadIdx.x;
    const uint64_t v = b < n_blocks ? A.block_bits[first + b] : 0u;
    uint64_t total;
    const uint64_t off = running + block_scan(v, &total, sums);
    if (b < n_blocks) {
      A.block_off[first + b] = off;
      words[off >> 5] = 0u;
    }
    running += total;
  }
  if (threadIdx.x == 0) {
    A.int_bits[blockIdx.x] = running;
    words[running >> 5] = 0u;
  }
}

__global__ __launch_bounds__(LJPEG_THREADS) void encode_ljpeg_emit_kernel(EncArgs A) {
  __shared__ TablesLds tabs;
  __shared__ uint32_t buf[LJPEG_RUN + 4];
  __shared__ uint32_t sums[4];
  const uint32_t job = find_job(A.block_starts, A.n_jobs, blockIdx.x);
  const LJpegGeom& g = A.jobs[job]; // (in place: init_pred and table are indexed)
  const Where w = where_of(A, g, job, blockIdx.x);
  load_tables(A, g, &tabs);
  for (uint32_t k = threadIdx.x; k < LJPEG_RUN + 4; k += LJPEG_THREADS)
    buf[k] = 0u;
  int32_t d = 0;
  uint32_t c = 0, nb = 0, word = 0;
  if (lane_difference(A, g, w, &d, &c))
    word = symbol(tabs.code[c], tabs.len[c], tabs.fix16[c], d, &nb);
  uint32_t total;
  const uint32_t before = block_scan(nb, &total, sums); // (its barriers order the zeroing of buf)
  const uint64_t start = A.block_off[blockIdx.x];
  const uint32_t lead = uint32_t(start & 31u);
  if (nb) {
    const uint32_t rel = lead + before;
    const uint64_t t = uint64_t(word) << (64u - nb - (rel & 31u));
    atomicOr(&buf[rel >> 5], uint32_t(t >> 32));
    if (uint32_t(t))
      atomicOr(&buf[(rel >> 5) + 1u], uint32_t(t));
  }
  __syncthreads();
  const uint32_t n_words = (lead + total + 31u) >> 5;
  const bool open_end = ((lead + total) & 31u) != 0;
  uint32_t* words = A.scratch + uint64_t(w.first_block) * LJPEG_RUN + (start >> 5);
  for (uint32_t k = threadIdx.x; k < n_words; k += LJPEG_THREADS) {
    if (k == 0 || (k + 1u == n_words && open_end))
      atomicOr(&words[k], buf[k]);
    else
      words[k] = buf[k];
  }
}

// the lane's word of the workgroup's run of the closed interval: its bytes that exist (first byte
// on top), the interval's tail applied
__device__ __forceinline__ uint32_t run_word(const EncArgs& A, const LJpegGeom& g, const Where& w,
                                             uint32_t block, uint32_t* n_bytes) {
  uint32_t ones;
  const uint64_t T = A.int_bits[g.first_int + w.interval];
  const uint64_t bytes = interval_bytes(T, w.last, g.tail, &ones);
  const uint64_t at = (uint64_t(w.run) * LJPEG_RUN + threadIdx.x) * 4u;
  *n_bytes = 0;
  if (at >= bytes)
    return 0u;
  uint32_t v = A.scratch[uint64_t(w.first_block) * LJPEG_RUN + (at >> 2)];
  const uint64_t left = bytes - at;
  *n_bytes = left < 4u ? uint32_t(left) : 4u;
  if (left <= 4u)
    v |= ((1u << ones) - 1u) << (8u * (4u - uint32_t(left)));
  return v;
}

__device__ __forceinline__ uint32_t stuffed_size(uint32_t v, uint32_t n_bytes) {
  uint32_t n = n_bytes;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j)
    n += j < n_bytes && (v >> (24u - 8u * j) & 0xFFu) == 0xFFu ? 1u : 0u;
  return n;
}

__global__ __launch_bounds__(LJPEG_THREADS) void encode_ljpeg_count_kernel(EncArgs A) {
  __shared__ uint32_t sums[4];
  const uint32_t job = find_job(A.block_starts, A.n_jobs, blockIdx.x);
  const LJpegGeom& g = A.jobs[job]; // (in place: init_pred and table are indexed)
  const Where w = where_of(A, g, job, blockIdx.x);
  uint32_t n_bytes;
  const uint32_t v = run_word(A, g, w, blockIdx.x, &n_bytes);
  uint32_t total;
  block_scan(stuffed_size(v, n_bytes), &total, sums);
  if (threadIdx.x == 0)
    A.run_count[blockIdx.x] = total;
}

__global__ __launch_bounds__(LJPEG_THREADS) void encode_ljpeg_place_kernel(EncArgs A) {
  __shared__ uint64_t sums[4];
  const uint32_t job = blockIdx.x;
  const LJpegGeom& g = A.jobs[job]; // (in place: init_pred and table are indexed)
  uint64_t running = 0;
  for (uint32_t base = 0; base < g.n_blocks; base += LJPEG_THREADS) {
    const uint32_t b = base + threadIdx.x;
    // a marker stands in front of the first run of every interval but the first
    const uint64_t marker = b < g.n_blocks && b != 0 && b % g.int_blocks == 0 ? 2u : 0u;
    const uint64_t v = b < g.n_blocks ? A.run_count[g.first_block + b] + marker : 0u;
    uint64_t total;
    const uint64_t off = running + block_scan(v, &total, sums);
    if (b < g.n_blocks)
      A.run_off[g.first_block + b] = off + marker;
    running += total;
  }
  uint64_t bits = 0;
  for (uint32_t i = threadIdx.x; i < g.n_int; i += LJPEG_THREADS)
    bits += A.int_bits[g.first_int + i];
  uint64_t all_bits;
  block_scan(bits, &all_bits, sums);
  if (threadIdx.x == 0) {
    rsx_encode_result r;
    r.status = (A.flags[job] & FLAG_MISSING) ? RSX_ERR_BAD_HUFFMAN_CODE
               : running > g.out_cap         ? RSX_ERR_INPUT_OVERFLOW
                                             : RSX_OK;
    r.reserved = 0;
    r.bytes = r.status == RSX_OK ? running : 0u;
    r.symbol_bits = r.status == RSX_OK ? all_bits : 0u;
    A.results[job] = r;
  }
}

__global__ __launch_bounds__(LJPEG_THREADS) void encode_ljpeg_stuff_kernel(EncArgs A) {
  __shared__ uint32_t sums[4];
  const uint32_t job = find_job(A.block_starts, A.n_jobs, blockIdx.x);
  if (A.results[job].status != RSX_OK)
    return; // (a workgroup's one answer: nothing of a failed job is written)
  const LJpegGeom& g = A.jobs[job]; // (in place: init_pred and table are indexed)
  const Where w = where_of(A, g, job, blockIdx.x);
  uint32_t n_bytes;
  const uint32_t v = run_word(A, g, w, blockIdx.x, &n_bytes);
  uint32_t total;
  const uint32_t before = block_scan(stuffed_size(v, n_bytes), &total, sums);
  uint8_t* run = A.out_base + g.out_off + A.run_off[blockIdx.x];
  if (threadIdx.x == 0 && w.run == 0 && w.interval != 0) {
    run[-2] = 0xFFu;
    run[-1] = uint8_t(0xD0u + (w.interval - 1u) % 8u);
  }
  uint8_t* dst = run + before;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    if (j < n_bytes) {
      const uint8_t b = uint8_t(v >> (24u - 8u * j));
      *dst++ = b;
      if (b == 0xFFu)
        *dst++ = 0x00u;
    }
  }
}

struct EncodeLJpegPlan final : DecoderPlan {
  rsx_ctx* ctx = nullptr;
  bool hist = false;
  std::vector<int32_t> host;   // validation result per job
  std::vector<int> dev_index;  // the job's place among those that go to the device, or -1
  std::vector<LJpegGeom> jobs; // the jobs that go to the device
  std::vector<EncTable> tables;
  std::vector<uint32_t> block_starts, int_starts;
  std::vector<rsx_encode_result> fetched;
  bool have_results = false;
  DeviceBuffer d_jobs, d_block_starts, d_int_starts, d_tables, d_flags, d_block_bits, d_block_off,
      d_int_bits, d_scratch, d_run_count, d_run_off, d_results;
  uint64_t total_blocks = 0, total_ints = 0;

  int finish() {
    if (total_blocks > 0x7FFFFFFFull || total_ints > 0x7FFFFFFFull)
      return RSX_ERR_UNSUPPORTED; // (a launch's grid)
    for (const LJpegGeom& g : jobs) {
      block_starts.push_back(g.first_block);
      int_starts.push_back(g.first_int);
    }
    block_starts.push_back(uint32_t(total_blocks));
    int_starts.push_back(uint32_t(total_ints));
    if (tables.empty())
      tables.emplace_back();
    RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (int st = upload(ctx, d_jobs, jobs))
      return st;
    if (int st = upload(ctx, d_block_starts, block_starts))
      return st;
    if (int st = upload(ctx, d_int_starts, int_starts))
      return st;
    if (int st = upload(ctx, d_tables, tables))
      return st;
    if (hist)
      return RSX_OK;
    const size_t nb = size_t(total_blocks), nj = jobs.size();
    int st = d_flags.ensure(nj * 4 + 16);
    st = st ? st : d_block_bits.ensure(nb * 4 + 16);
    st = st ? st : d_block_off.ensure(nb * 8 + 16);
    st = st ? st : d_int_bits.ensure(size_t(total_ints) * 8 + 16);
    // (the word at an interval's end may be the first one behind its workgroups' words)
    st = st ? st : d_scratch.ensure((nb * LJPEG_RUN + 4) * 4);
    st = st ? st : d_run_count.ensure(nb * 4 + 16);
    st = st ? st : d_run_off.ensure(nb * 8 + 16);
    st = st ? st : d_results.ensure(nj * sizeof(rsx_encode_result) + 16);
    return st;
  }
  int run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) override {
    have_results = false;
    if (jobs.empty())
      return RSX_OK; // (every job was refused by the host)
    if (reinterpret_cast<uintptr_t>(in_dev) % 2u != 0 ||
        (hist && reinterpret_cast<uintptr_t>(out_dev) % 8u != 0))
      return RSX_ERR_INVALID_ARG;
    EncArgs A{};
    A.in_base = static_cast<const uint8_t*>(in_dev);
    A.out_base = static_cast<uint8_t*>(out_dev);
    A.jobs = static_cast<const LJpegGeom*>(d_jobs.ptr);
    A.block_starts = static_cast<const uint32_t*>(d_block_starts.ptr);
    A.int_starts = static_cast<const uint32_t*>(d_int_starts.ptr);
    A.tables = static_cast<const EncTable*>(d_tables.ptr);
    A.flags = static_cast<uint32_t*>(d_flags.ptr);
    A.block_bits = static_cast<uint32_t*>(d_block_bits.ptr);
    A.block_off = static_cast<uint64_t*>(d_block_off.ptr);
    A.int_bits = static_cast<uint64_t*>(d_int_bits.ptr);
    A.scratch = static_cast<uint32_t*>(d_scratch.ptr);
    A.run_count = static_cast<uint32_t*>(d_run_count.ptr);
    A.run_off = static_cast<uint64_t*>(d_run_off.ptr);
    A.results = static_cast<rsx_encode_result*>(d_results.ptr);
    A.n_jobs = uint32_t(jobs.size());
    const dim3 threads(LJPEG_THREADS), blocks{uint32_t(total_blocks)};
    const uint32_t cells = A.n_jobs * (hist ? 4u * N_CATEGORIES : 1u);
    if (timer)
      timer->begin(s);
    auto mark = [&](const char* name) {
      if (timer)
        timer->mark(name);
    };
    hipLaunchKernelGGL(encode_ljpeg_clear_kernel, dim3((cells + LJPEG_THREADS - 1u) / LJPEG_THREADS),
                       threads, 0, s, A, hist);
    mark("encode_ljpeg_clear_kernel");
    if (hist) {
      hipLaunchKernelGGL(encode_ljpeg_length_kernel<true>, blocks, threads, 0, s, A);
      mark("encode_ljpeg_histogram_kernel");
    } else {
      hipLaunchKernelGGL(encode_ljpeg_length_kernel<false>, blocks, threads, 0, s, A);
      mark("encode_ljpeg_length_kernel");
      hipLaunchKernelGGL(encode_ljpeg_scan_kernel, dim3(uint32_t(total_ints)), threads, 0, s, A);
      mark("encode_ljpeg_scan_kernel");
      hipLaunchKernelGGL(encode_ljpeg_emit_kernel, blocks, threads, 0, s, A);
      mark("encode_ljpeg_emit_kernel");
      hipLaunchKernelGGL(encode_ljpeg_count_kernel, blocks, threads, 0, s, A);
      mark("encode_ljpeg_count_kernel");
      hipLaunchKernelGGL(encode_ljpeg_place_kernel, dim3(A.n_jobs), threads, 0, s, A);
      mark("encode_ljpeg_place_kernel");
      hipLaunchKernelGGL(encode_ljpeg_stuff_kernel, blocks, threads, 0, s, A);
      mark("encode_ljpeg_stuff_kernel");
    }
    RSX_HIP_CHECK(ctx, hipGetLastError());
    return RSX_OK;
  }
  int results(hipStream_t s, bool ran, int32_t* job_status, uint32_t* job_consumed) override {
    fetched.assign(jobs.size(), rsx_encode_result{});
    const bool with_work = ran && !jobs.empty() && !hist;
    if (with_work) {
      RSX_HIP_CHECK(ctx, hipMemcpyAsync(fetched.data(), d_results.ptr,
                                        jobs.size() * sizeof(rsx_encode_result),
                                        hipMemcpyDeviceToHost, s));
      RSX_HIP_CHECK(ctx, hipStreamSynchronize(s));
    } else if (ran && !jobs.empty())
      RSX_HIP_CHECK(ctx, hipStreamSynchronize(s));
    have_results = with_work;
    if (job_consumed)
      for (size_t i = 0; i < host.size(); ++i)
        job_consumed[i] = dev_index[i] >= 0 ? uint32_t(fetched[size_t(dev_index[i])].bytes) : 0u;
    return fold_jobs(host.size(), FoldOrder::LAST_FAILING, job_status, [&](size_t i) {
      return host[i] != RSX_OK || !with_work ? int(host[i]) : int(fetched[size_t(dev_index[i])].status);
    });
  }
  int encode_result(int job, rsx_encode_result* out) override {
    if (job < 0 || size_t(job) >= host.size() || !out || hist)
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

int make_plan(rsx_ctx* ctx, int n_jobs, const rsx_encode_ljpeg_job* jobs, bool hist,
              std::unique_ptr<DecoderPlan>* out) {
  auto p = std::make_unique<EncodeLJpegPlan>();
  p->ctx = ctx;
  p->hist = hist;
  p->host.assign(n_jobs, RSX_OK);
  p->dev_index.assign(n_jobs, -1);
  for (int i = 0; i < n_jobs; ++i) {
    const rsx_encode_ljpeg_job& j = jobs[i];
    int st = validate_ljpeg(j.desc, j.img);
    if (st == RSX_OK)
      st = validate_ljpeg_subset(j.desc, j.img);
    if (st == RSX_OK && (j.flags > RSX_ENCODE_TAIL_VACUUMER || j.img_offset % 2u != 0 ||
                         (hist && j.out_offset % 8u != 0)))
      st = RSX_ERR_INVALID_ARG;
    p->host[i] = st;
    if (st != RSX_OK)
      continue;
    LJpegGeom g;
    ljpeg_geom(j.desc, j.img, j.img_offset, j.out_offset, j.out_cap, j.flags, &g);
    const uint64_t blocks = ljpeg_blocks(g);
    if (p->total_blocks + blocks > 0x7FFFFFFFull)
      return RSX_ERR_UNSUPPORTED;
    g.first_block = uint32_t(p->total_blocks);
    g.n_blocks = uint32_t(blocks);
    g.first_int = uint32_t(p->total_ints);
    g.table_base = uint32_t(p->tables.size());
    for (int t = 0; t < j.desc.n_tables; ++t) {
      p->tables.emplace_back();
      build_enc_table(j.desc.tables[t], &p->tables.back());
    }
    p->total_blocks += blocks;
    p->total_ints += g.n_int;
    p->dev_index[i] = int(p->jobs.size());
    p->jobs.push_back(g);
  }
  if (int st = p->finish())
    return st;
  *out = std::move(p);
  return RSX_OK;
}

} // namespace

int encode_ljpeg_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_encode_ljpeg_job* jobs,
                             std::unique_ptr<DecoderPlan>* out) {
  return make_plan(ctx, n_jobs, jobs, false, out);
}

int encode_histogram_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_encode_ljpeg_job* jobs,
                                 std::unique_ptr<DecoderPlan>* out) {
  return make_plan(ctx, n_jobs, jobs, true, out);
}

} // namespace rsx
