// PhaseOneDecompressor on the device (include/rsx.h section 3h).
//
// What the reference does (decompressors/PhaseOneDecompressor.cpp:85-136): every image row
// is a bit stream of its own (BitStreamerMSB32 over exactly the strip's bytes, zeros behind
// them).  Groups of 8 pixels start with two length headers (len[0] for the even columns,
// len[1] for the odd ones); the last w % 8 pixels have none and are raw.  A pixel is either
// a raw 16-bit value that resets the running sum of its column parity, or a difference
// added to it.  Two things follow from that:
//   * the bit lengths of a row come from the headers alone, never from decoded values:
//     one lane can walk a row's headers -- a step per group, ~1500 at the widest frame --
//     and note where every 64-pixel chunk starts;
//   * the values are two running sums mod 2^16 that a raw value resets: a segmented scan.
//
//   p1_row_kernel   one workgroup per row (192 lanes; 11976 / 64 -> 188 chunks):
//                   1. the strip's bytes -> LDS as little-endian words, zero behind the
//                      strip (they are NOT the next row's bytes, which lie right behind);
//                   2. lane 0 walks the group headers in LDS and writes a checkpoint --
//                      bit offset, len[0], len[1] -- every 8 groups, and decides the row's
//                      status (size < 4, the col-0 header, the over-read rule);
//                   3. lane i decodes pixels 64 i .. 64 i + 63 from checkpoint i into
//                      registers: local running sums per parity, where each was reset;
//                   4. a segmented scan mod 2^16 of the lanes' sums per parity across the
//                      workgroup, the carry added in front of each lane's first reset;
//                   5. each lane stores its 128 contiguous bytes.
//   (The walk as a kernel of its own, one lane per row reading the strip from global
//   memory, with the checkpoints handed over through HBM, is the A/B of DESIGN 4.6.)
//
// All of it is bit-exact against the reference's whole-file decode (tests/test_gpu_phase_one.py)
// and against a model of exactly this decomposition (tests/test_phase_one_model.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "rsx_internal.h"
#include "rsx_ljpeg_dev.h"
#include "rsx_plan_host.h"
#include "rsx_phase_one.h"

namespace rsx {

namespace {

constexpr int P1_THREADS = 192; // lanes of a row: 64 pixels each (11976 / 64 -> 188)
constexpr int P1_WAVES = P1_THREADS / 64;
constexpr int32_t P1_MAX_W = 11976, P1_MAX_H = 8854; // PhaseOneDecompressor.cpp:52-56
// len = {8, 7, 6, 9, 11, 10, 5, 12, 14, 13}[2 (j - 1) + b] (:93-94), a nibble each
constexpr uint64_t P1_LENGTHS = 0xDEC5AB9678ull;
// LDS in front of the row's words: checkpoints (bit offset, lengths) per chunk, the scan's
// per-wave totals, the row's status
constexpr int P1_LDS_HEAD = 2 * P1_THREADS + 16;

struct P1RowDev {
  uint64_t off;   // first byte of the strip in the plan's input
  uint32_t bytes; // strip size
  uint32_t job;
  uint32_t row;   // image row
  uint32_t words; // words of the row in LDS (a bound on what its pixels can read, + 2)
};

struct P1JobDev {
  uint64_t img_offset;
  uint32_t pitch, width;
  uint32_t row_base; // first entry of the job in rows[] / row_status[]
  uint32_t pad;
};

struct P1Args {
  const uint8_t* in_base;
  uint8_t* out_base;
  const P1RowDev* rows;
  const P1JobDev* jobs;
  uint32_t* row_status; // [row of the plan]: rsx_status
  uint32_t* job_status; // [job]: first failing row << 8 | status, STATUS_NONE = fine
};

// The most bits a row of `width` pixels can read: 12 header bits + 8 x 16 per group, 16 per
// trailing pixel.  Its words + 2 bound every peek (peeks read word q / 32 and the next one).
__host__ __device__ inline uint32_t p1_row_words(uint32_t width) {
  const uint32_t bits = (width >> 3) * 140u + (width & 7u) * 16u;
  return bits / 32u + 2u;
}

// The 32 bits at bit offset q (BitStreamerMSB32: little-endian words, MSB first)
__device__ __forceinline__ uint32_t p1_peek(const uint32_t* w, uint32_t q) {
  const uint32_t k = q >> 5;
  const uint64_t v = (uint64_t(w[k]) << 32) | w[k + 1];
  return uint32_t((v << (q & 31u)) >> 32);
}

// One length header at the top of `w` (:96-111): up to five 0-bits up to a 1-bit; j zeros
// > 0 -> one more bit b, len = P1_LENGTHS[2 (j - 1) + b]; j == 0 keeps len.  Returns the
// bits it takes; *one: a 1-bit inside the five (the col-0 error, :103-104).
__device__ __forceinline__ uint32_t p1_len(uint32_t w, uint32_t* len, bool* one) {
  const uint32_t z = __clz(w);
  *one = z < 5u;
  if (z == 0u)
    return 1u;
  const uint32_t j = z < 5u ? z : 5u;
  const uint32_t used = z < 5u ? j + 1u : 5u;
  const uint32_t b = (w << used) >> 31;
  *len = uint32_t(P1_LENGTHS >> (4u * (2u * (j - 1u) + b))) & 15u;
  return used + 1u;
}

__device__ __forceinline__ uint32_t p1_bits(uint32_t len) { return len == 14u ? 16u : len; }

// running sums per parity: value (16 bits) | reset seen << 16; a then b
__device__ __forceinline__ uint32_t p1_combine(uint32_t a, uint32_t b) {
  return (b & 0x10000u) ? b : ((a & 0x10000u) | ((a + b) & 0xFFFFu));
}

__global__ void __launch_bounds__(P1_THREADS) p1_row_kernel(P1Args A) {
  extern __shared__ uint32_t p1_lds[];
  uint32_t* cp_pos = p1_lds;
  uint32_t* cp_len = p1_lds + P1_THREADS;
  uint32_t* totals = p1_lds + 2 * P1_THREADS; // [wave][parity]
  uint32_t* W = p1_lds + P1_LDS_HEAD;
  const int tid = threadIdx.x;
  const P1RowDev R = A.rows[blockIdx.x];
  const P1JobDev J = A.jobs[R.job];
  const uint32_t width = J.width, ng = width >> 3, gw = width & ~7u, tail = width & 7u;

  // 1. the strip -> LDS.  Strips start at any byte: each word is two aligned dwords shifted
  // together; only dwords that hold bytes of the strip are read, bytes behind it are zero.
  {
    const uintptr_t a = reinterpret_cast<uintptr_t>(A.in_base + R.off);
    const uint32_t* d = reinterpret_cast<const uint32_t*>(a & ~uintptr_t(3));
    const uint32_t sh = uint32_t(a & 3u) * 8u;
    const uint32_t nd = R.bytes ? uint32_t((((a & 3u) + R.bytes + 3u) >> 2)) : 0u; // dwords
    for (uint32_t k = tid; k < R.words; k += P1_THREADS) {
      uint32_t v = 0;
      if (4u * k < R.bytes) {
        const uint32_t lo = d[k];
        const uint32_t hi = k + 1u < nd ? d[k + 1] : 0u;
        v = sh ? (lo >> sh) | (hi << (32u - sh)) : lo;
        const uint32_t rem = R.bytes - 4u * k;
        if (rem < 4u)
          v &= (1u << (8u * rem)) - 1u;
      }
      W[k] = v;
    }
  }
  __syncthreads();

  // 2. the walk: checkpoints and the row's status
  if (tid == 0) {
    uint32_t st = R.bytes < 4u ? uint32_t(RSX_ERR_IO) : uint32_t(RSX_OK);
    uint32_t pos = 0, l0 = 8, l1 = 8;
    uint32_t c_last = 16u * (width - 1u); // start bit of the last pixel (no groups)
    for (uint32_t g = 0; g < ng; ++g) {
      if ((g & 7u) == 0u) {
        cp_pos[g >> 3] = pos;
        cp_len[g >> 3] = l0 | (l1 << 8);
      }
      const uint32_t w = p1_peek(W, pos);
      bool o0, o1;
      uint32_t h = p1_len(w, &l0, &o0);
      h += p1_len(w << h, &l1, &o1);
      if (g == 0 && (o0 || o1) && st == RSX_OK)
        st = RSX_ERR_BAD_HUFFMAN_CODE;
      const uint32_t b0 = p1_bits(l0), b1 = p1_bits(l1);
      c_last = pos + h + 4u * b0 + 3u * b1; // (pixel 7 of the group)
      pos += h + 4u * (b0 + b1);
    }
    if (tail) {
      if ((ng & 7u) == 0u) {
        cp_pos[ng >> 3] = pos;
        cp_len[ng >> 3] = 14u | (14u << 8);
      }
      c_last = pos + 16u * (tail - 1u);
    }
    // fill(32) before every pixel: ceil(c / 32) + 1 refills by the one at bit c, the last at
    // byte 4 ceil(c / 32); it throws when that is more than size + 8 (BitStreamer.h:124-127)
    if (st == RSX_OK && 4ull * ((uint64_t(c_last) + 31u) >> 5) > uint64_t(R.bytes) + 8u)
      st = RSX_ERR_INPUT_OVERFLOW;
    A.row_status[J.row_base + R.row] = st;
    if (st != RSX_OK)
      atomicMin(&A.job_status[R.job], (R.row << 8) | st);
  }
  __syncthreads();

  // 3. lane i: pixels 64 i .. 64 i + 63 into registers, as local running sums per parity
  const uint32_t c0 = 64u * uint32_t(tid);
  const bool live = c0 < width;
  uint32_t px[32];
  uint32_t a0 = 0, a1 = 0, f0 = 64, f1 = 64; // sums, first reset in the lane
  if (live) {
    uint32_t pos = cp_pos[tid], lens = cp_len[tid];
    uint32_t l0 = lens & 0xFFu, l1 = lens >> 8;
#pragma unroll
    for (int k = 0; k < 64; ++k) {
      const uint32_t col = c0 + uint32_t(k);
      uint32_t v = 0;
      if (col < width) {
        uint32_t w = p1_peek(W, pos);
        uint32_t h = 0;
        if (col >= gw) {
          l0 = l1 = 14u;
        } else if ((k & 7) == 0) {
          bool o;
          h = p1_len(w, &l0, &o);
          h += p1_len(w << h, &l1, &o);
          w <<= h;
        }
        const uint32_t L = (k & 1) ? l1 : l0;
        uint32_t& acc = (k & 1) ? a1 : a0;
        if (L == 14u) {
          acc = w >> 16; // (:122-124)
          if (k & 1)
            f1 = min(f1, uint32_t(k));
          else
            f0 = min(f0, uint32_t(k));
          pos += h + 16u;
        } else {
          acc += (w >> (32u - L)) + 1u - (1u << (L - 1u)); // (:126-128)
          pos += h + L;
        }
        v = acc & 0xFFFFu;
      }
      if (k & 1)
        px[k >> 1] |= v << 16;
      else
        px[k >> 1] = v;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 32; ++k)
      px[k] = 0;
  }

  // 4. the segmented scan of the lanes' sums, both parities at once
  const int lane = tid & 63, wave = tid >> 6;
  uint32_t s0 = (a0 & 0xFFFFu) | (f0 < 64u ? 0x10000u : 0u);
  uint32_t s1 = (a1 & 0xFFFFu) | (f1 < 64u ? 0x10000u : 0u);
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t0 = __shfl_up(s0, d, 64), t1 = __shfl_up(s1, d, 64);
    if (lane >= d) {
      s0 = p1_combine(t0, s0);
      s1 = p1_combine(t1, s1);
    }
  }
  if (lane == 63) {
    totals[2 * wave] = s0;
    totals[2 * wave + 1] = s1;
  }
  __syncthreads();
  uint32_t e0 = __shfl_up(s0, 1, 64), e1 = __shfl_up(s1, 1, 64);
  if (lane == 0)
    e0 = e1 = 0;
  uint32_t w0 = 0, w1 = 0;
  for (int v = 0; v < wave; ++v) {
    w0 = p1_combine(w0, totals[2 * v]);
    w1 = p1_combine(w1, totals[2 * v + 1]);
  }
  const uint32_t carry0 = p1_combine(w0, e0) & 0xFFFFu, carry1 = p1_combine(w1, e1) & 0xFFFFu;
  if (!live)
    return;

  // 5. the carry in front of each parity's first reset, then 128 contiguous bytes
#pragma unroll
  for (int k = 0; k < 32; ++k) {
    const uint32_t lo = (px[k] + (uint32_t(2 * k) < f0 ? carry0 : 0u)) & 0xFFFFu;
    const uint32_t hi = ((px[k] >> 16) + (uint32_t(2 * k + 1) < f1 ? carry1 : 0u)) & 0xFFFFu;
    px[k] = lo | (hi << 16);
  }
  uint8_t* out = A.out_base + J.img_offset + uint64_t(R.row) * J.pitch + 2u * c0;
  const uint32_t pairs = min(32u, (width - c0) >> 1); // (width is even)
  const uintptr_t oa = reinterpret_cast<uintptr_t>(out);
  if (pairs == 32u && (oa & 15u) == 0u) {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      reinterpret_cast<uint4*>(out)[k] = make_uint4(px[4 * k], px[4 * k + 1], px[4 * k + 2], px[4 * k + 3]);
  } else if ((oa & 3u) == 0u) {
#pragma unroll
    for (int k = 0; k < 32; ++k)
      if (uint32_t(k) < pairs)
        reinterpret_cast<uint32_t*>(out)[k] = px[k];
  } else {
#pragma unroll
    for (int k = 0; k < 32; ++k)
      if (uint32_t(k) < pairs) {
        reinterpret_cast<uint16_t*>(out)[2 * k] = uint16_t(px[k]);
        reinterpret_cast<uint16_t*>(out)[2 * k + 1] = uint16_t(px[k] >> 16);
      }
  }
}

} // namespace

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
namespace {
struct P1Plan final : DecoderPlan {
  rsx_ctx* ctx = nullptr;
  std::vector<P1JobDev> jobs;
  JobStatus status;
  std::vector<uint32_t> job_rows; // rows of a job (0 when rejected)
  DeviceBuffer d_jobs, d_rows, d_row_status;
  std::vector<uint32_t> h_row_status;
  uint32_t total_rows = 0, max_words = 0;
  bool launched = false;
  int run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) override;
  int results(hipStream_t s, bool ran, int32_t* job_status, uint32_t* job_consumed) override;
  int row_status(hipStream_t s, int job, int32_t* statuses) override;
};
} // namespace

int phase_one_validate(int n_strips, const rsx_phase_one_strip* strips, size_t in_bytes,
                       const rsx_image& img) {
  // the constructor, PhaseOneDecompressor.cpp:43-84
  if (img.cpp != 1)
    return RSX_ERR_INVALID_ARG;
  if (img.dim_x <= 0 || img.dim_y <= 0 || img.dim_x % 2 != 0 || img.dim_x > P1_MAX_W ||
      img.dim_y > P1_MAX_H)
    return RSX_ERR_INVALID_ARG;
  if (img.pitch_bytes < uint32_t(img.dim_x) * 2u)
    return RSX_ERR_INVALID_ARG;
  // exactly one strip per row (prepareStrips, :60-84)
  if (!strips || n_strips != img.dim_y)
    return RSX_ERR_INVALID_ARG;
  std::vector<uint8_t> seen(size_t(img.dim_y), 0);
  for (int i = 0; i < n_strips; ++i) {
    const rsx_phase_one_strip& s = strips[i];
    if (s.n >= uint32_t(img.dim_y) || seen[s.n])
      return RSX_ERR_INVALID_ARG;
    seen[s.n] = 1;
    // (and inside the input: computeSripes cuts them out of raw_data, IiqDecoder.cpp:101-111)
    if (s.offset > in_bytes || s.bytes > in_bytes - s.offset)
      return RSX_ERR_INVALID_ARG;
  }
  return RSX_OK;
}

int phase_one_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_phase_one_job* jobs,
                          std::unique_ptr<DecoderPlan>* out) {
  auto p = std::make_unique<P1Plan>();
  p->ctx = ctx;
  p->status.host.assign(n_jobs, RSX_OK);
  p->job_rows.assign(n_jobs, 0);
  p->jobs.resize(n_jobs);
  std::vector<P1RowDev> rows;
  for (int i = 0; i < n_jobs; ++i) {
    const rsx_phase_one_job& j = jobs[i];
    P1JobDev& J = p->jobs[i];
    std::memset(&J, 0, sizeof J);
    int st = phase_one_validate(j.n_strips, j.strips, size_t(j.in_bytes), j.img);
    if (st == RSX_OK && (j.img_offset % 2 != 0 || j.img.pitch_bytes % 2 != 0))
      st = RSX_ERR_INVALID_ARG;
    if (st == RSX_OK && j.in_bytes >= (1ull << 32))
      st = RSX_ERR_UNSUPPORTED; // (strip sizes are 32-bit on the device)
    p->status.host[i] = st;
    if (st != RSX_OK)
      continue;
    J.img_offset = j.img_offset;
    J.pitch = j.img.pitch_bytes;
    J.width = uint32_t(j.img.dim_x);
    J.row_base = p->total_rows;
    const uint32_t words = p1_row_words(J.width);
    p->max_words = std::max(p->max_words, words);
    const size_t r0 = rows.size();
    rows.resize(r0 + size_t(j.img.dim_y));
    for (int k = 0; k < j.n_strips; ++k) {
      const rsx_phase_one_strip& s = j.strips[k];
      rows[r0 + s.n] = P1RowDev{j.in_offset + s.offset, uint32_t(s.bytes), uint32_t(i), s.n, words};
    }
    p->job_rows[i] = uint32_t(j.img.dim_y);
    p->total_rows += uint32_t(j.img.dim_y);
  }
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int st;
  if ((st = upload(ctx, p->d_jobs, p->jobs)) || (st = upload(ctx, p->d_rows, rows)) ||
      (st = p->d_row_status.ensure(size_t(p->total_rows) * 4 + 16)) || (st = p->status.init()))
    return st;
  *out = std::move(p);
  return RSX_OK;
}

int P1Plan::run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) {
  if (total_rows == 0)
    return RSX_OK; // (every job was rejected by the host)
  if (timer)
    timer->begin(s);
  P1Args A{};
  A.in_base = static_cast<const uint8_t*>(in_dev);
  A.out_base = static_cast<uint8_t*>(out_dev);
  A.rows = static_cast<const P1RowDev*>(d_rows.ptr);
  A.jobs = static_cast<const P1JobDev*>(d_jobs.ptr);
  A.row_status = static_cast<uint32_t*>(d_row_status.ptr);
  A.job_status = static_cast<uint32_t*>(status.dev.ptr);
  if (int st = status.reset(ctx, s))
    return st;
  const size_t lds = (size_t(P1_LDS_HEAD) + max_words) * 4;
  hipLaunchKernelGGL(p1_row_kernel, dim3(total_rows), dim3(P1_THREADS), lds, s, A);
  if (timer)
    timer->mark("p1_row_kernel");
  RSX_HIP_CHECK(ctx, hipGetLastError());
  launched = true;
  return RSX_OK;
}

int P1Plan::results(hipStream_t s, bool ran, int32_t* job_status, uint32_t* job_consumed) {
  if (job_consumed)
    std::fill(job_consumed, job_consumed + jobs.size(), 0u);
  return status.fold(ctx, s, ran && total_rows != 0, 0xFFu, FoldOrder::LAST_FAILING, job_status);
}

int P1Plan::row_status(hipStream_t s, int job, int32_t* statuses) {
  if (job < 0 || size_t(job) >= jobs.size() || !launched || job_rows[job] == 0)
    return RSX_ERR_INVALID_ARG;
  return fetch_words(ctx, s, d_row_status, jobs[job].row_base, job_rows[job], h_row_status, statuses);
}

} // namespace rsx
