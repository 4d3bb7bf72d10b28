// OlympusDecompressor (compressed ORF) on gfx950: include/rsx.h section 3v, DESIGN.md 4.20.
//
// Two kernels a run, one launch each over all jobs (frames) of a plan.
//
// olympus_parse_kernel: one wavefront (a workgroup of 64) per job walks the job's bits.  There is
// no marker and no alignment between rows, and a symbol's length depends on the symbols before it
// in its row, so the walk is serial; it needs no pixel (rsx_olympus_core.h).  The wave runs it
// uniformly, so that the chain -- position, carries, shifts, counts of leading zeros, compares and
// branches -- stays on the scalar unit.  The lanes carry what is not the chain:
//   * the byte window: OL_WIN_REGS registers a lane, 64 big-endian words each, from the next word
//     the walk loads; a refill of the reader's cache comes out of them by readlane.  All lanes reload the window
//     with coalesced loads when a batch's worst case (64 symbols of 31 bits) may outrun it;
//   * the differences: symbol i of a batch goes into lane i of a register (a compare and a select), and a
//     batch of up to 64 leaves as one 16-bit store a lane, into the job's image at (row, col).
// A reader failure sets the job's status and ends the walk.
//
// olympus_recon_kernel: one wavefront per (job, Bayer plane) turns differences into pixels in
// place.  Cell (i, j) of a plane needs (i, j-1), (i-1, j) and (i-1, j-1): a band of 64 plane rows
// is in flight, lane l on row 64 band + l and l columns behind lane l-1.  L stays in a register, U
// is the lane above's last value (one wave shift a step) and NW is the lane's own U of the step
// before.  Lane 0 reads its U from the row the band before left in LDS.  Bands follow one another
// in the same wavefront: no flag, no spin wait, nothing that depends on another workgroup being
// resident.  Global traffic runs along rows: tiles of 64 rows x 64 plane columns go through a ring
// of two tiles in LDS, loaded before the steps that need them and flushed when every lane is past
// them.  A job whose walk failed is skipped.
//
// No scratch; registers and LDS are what tests/test_olympus_build.py holds.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "rsx_olympus.h"
#include "rsx_olympus_core.h"
#include "rsx_ljpeg_dev.h"
#include "rsx_plan_host.h"

namespace rsx {

using namespace rsx_olympus;

namespace {

constexpr int OL_THREADS = 64;
constexpr int OL_WIN_REGS = 4;                 // window registers a lane
constexpr int OL_WIN_WORDS = 64 * OL_WIN_REGS; // words of the stream in the window
constexpr int OL_BATCH = 64;                   // symbols between two looks at the window
// words a batch loads at most: 64 symbols of 31 bits, and one for the cache's level
constexpr int OL_BATCH_WORDS = (OL_BATCH * 31 + 31) / 32 + 2;

constexpr int OL_BAND = 64;                // plane rows in flight
constexpr int OL_TILE = 64;                // plane columns of a tile
constexpr int OL_RING = 2 * OL_TILE;       // columns of a row in LDS
constexpr int OL_MAX_PW = MAX_X / 2;       // plane width at the limit

struct OlJobDev {
  uint64_t in_off;  // the bit stream (behind the 7 bytes), from the run's input base
  uint64_t out_off; // the image's first pixel, from the run's output base
  uint64_t size;    // bytes of the bit stream
  uint32_t pitch;
  uint32_t job;
  int32_t dim_x, dim_y;
};

struct OlArgs {
  const uint8_t* in_base;
  uint8_t* out_base;
  const OlJobDev* jobs;
  uint32_t* job_status; // per job of the plan: STATUS_NONE, or the walk's status
};

// bytes 4 k .. 4 k + 3 of the stream as a big-endian word; bytes behind the stream read as zero
__device__ __forceinline__ uint32_t ol_global_word(const uint8_t* p, uint64_t size, uint64_t k) {
  const uint64_t at = 4ull * k;
  if (at + 4 <= size) {
    uint32_t v;
    __builtin_memcpy(&v, p + at, 4);
    return __builtin_bswap32(v);
  }
  uint32_t w = 0;
  for (uint32_t b = 0; b < 4; ++b)
    w = w << 8 | (at + b < size ? uint32_t(p[at + b]) : 0u);
  return w;
}

__device__ __forceinline__ uint32_t ol_uni(uint32_t v) {
  return uint32_t(__builtin_amdgcn_readfirstlane(int32_t(v)));
}

// The walk's reader: rsx_olympus::Bits with the stream's words out of the lanes' registers, the
// word count in 32 bits (a frame at the limits takes 7.9e7 words) and the over-read rule as a
// sticky flag -- 4 k > size + 8 is monotone in k, and the words behind the stream read as zero, so
// the walk may finish its batch before it looks at the flag.
struct OlBits {
  uint32_t win[OL_WIN_REGS]; // lane l of register r: word k0 + 64 r + l
  uint32_t k0;
  uint32_t k;       // words loaded
  uint32_t k_limit; // the last word a fill may load: (size + 8) / 4, below 2^31
  uint64_t buf;     // the cache, left-aligned
  int32_t level;
  uint32_t failed; // bit 31: a fill loaded a word behind k_limit
  __device__ __forceinline__ void fill() {
    if (level >= 32)
      return;
    failed |= k_limit - k; // (both below 2^31; plain integers keep the flag on the scalar unit)
    const uint32_t j = k - k0;
    const int32_t l = int32_t(j & 63u);
    uint32_t v = uint32_t(__builtin_amdgcn_readlane(int32_t(win[0]), l));
#pragma unroll
    for (int r = 1; r < OL_WIN_REGS; ++r) {
      const uint32_t t = uint32_t(__builtin_amdgcn_readlane(int32_t(win[r]), l));
      v = (j >> 6) == uint32_t(r) ? t : v;
    }
    buf |= uint64_t(v) << (32 - level);
    level += 32;
    ++k;
  }
  __device__ __forceinline__ uint32_t peek32() const { return uint32_t(buf >> 32); }
  __device__ __forceinline__ void skip(int32_t n) {
    buf <<= n;
    level -= n;
  }
};

__global__ void __launch_bounds__(OL_THREADS) olympus_parse_kernel(OlArgs A) {
  const OlJobDev J = A.jobs[blockIdx.x];
  const int lane = int(threadIdx.x);
  const uint8_t* bytes = A.in_base + J.in_off;
  uint8_t* out = A.out_base + J.out_off;
  const int32_t w = int32_t(ol_uni(uint32_t(J.dim_x))), h = int32_t(ol_uni(uint32_t(J.dim_y)));

  OlBits B;
  const uint64_t last = (J.size + 8u) / 4u;
  B.k_limit = last > 0x7FFFFFFFull ? 0x7FFFFFFFu : uint32_t(last);
  B.k0 = 0;
  B.k = 0;
  B.buf = 0;
  B.level = 0;
  B.failed = 0;
  bool have_window = false;
  int32_t status = RSX_OK;

  for (int32_t row = 0; row < h && status == RSX_OK; ++row) {
    Carry s0 = {0, 0, 0}, s1 = {0, 0, 0};
    uint8_t* orow = out + size_t(row) * J.pitch;
    for (int32_t col0 = 0; col0 < w; col0 += OL_BATCH) {
      const int32_t n = w - col0 < OL_BATCH ? w - col0 : OL_BATCH; // (even)
      // the window: from the next word the walk loads, when a batch may outrun what is left
      if (!have_window || B.k - B.k0 + uint32_t(OL_BATCH_WORDS) > uint32_t(OL_WIN_WORDS)) {
        B.k0 = B.k;
#pragma unroll
        for (int r = 0; r < OL_WIN_REGS; ++r)
          B.win[r] = ol_global_word(bytes, J.size, uint64_t(B.k0) + uint64_t(64 * r + lane));
        have_window = true;
      }
      int32_t vdiff = 0;
      for (int32_t i = 0; i < n; i += 2) {
        // (pairs: the two column parities keep their carries in their own registers)
        int32_t d;
        B.fill();
        B.skip(symbol(s0, B.peek32(), &d));
        vdiff = lane == i ? d : vdiff;
        B.fill();
        B.skip(symbol(s1, B.peek32(), &d));
        vdiff = lane == i + 1 ? d : vdiff;
      }
      if (int32_t(B.failed) < 0) {
        // (the batch is not written: the image behind a failure is unspecified)
        status = RSX_ERR_INPUT_OVERFLOW;
        break;
      }
      if (lane < n)
        reinterpret_cast<uint16_t*>(orow)[col0 + lane] = uint16_t(vdiff);
    }
  }
  if (lane == 0)
    A.job_status[J.job] = uint32_t(status);
}

// wave_shr:1 -- lane l gets lane l-1's value, lane 0 keeps `self`
__device__ __forceinline__ int32_t ol_from_lane_above(int32_t v) {
  return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xF, 0xF, false);
}

__global__ void __launch_bounds__(OL_THREADS) olympus_recon_kernel(OlArgs A) {
  __shared__ uint16_t ring[OL_BAND * OL_RING]; // 64 rows x two tiles of columns
  __shared__ uint16_t prev_row[OL_MAX_PW];     // the last row of the band before

  const OlJobDev J = A.jobs[blockIdx.x >> 2];
  if (A.job_status[J.job] != uint32_t(RSX_OK))
    return;
  const int plane = int(blockIdx.x & 3u);
  const int pr = plane >> 1, pc = plane & 1;
  const int lane = int(threadIdx.x);
  const int32_t pw = J.dim_x / 2, ph = J.dim_y / 2;
  uint8_t* img = A.out_base + J.out_off;
  const int32_t n_tiles = (pw + OL_TILE - 1) / OL_TILE;

  for (int32_t i0 = 0; i0 < ph; i0 += OL_BAND) {
    const int32_t rows = ph - i0 < OL_BAND ? ph - i0 : OL_BAND;
    const int32_t i = i0 + lane;
    const bool live = lane < rows;
    int32_t left = 0, up_prev = 0, cur = 0;
    // tile `c` of the band between the image and the ring, along rows: lane = column
    auto tile_io = [&](int32_t c, bool load) {
      const int32_t j = c * OL_TILE + lane;
      if (j >= pw)
        return;
      for (int32_t r = 0; r < rows; ++r) {
        uint16_t* g = reinterpret_cast<uint16_t*>(img + size_t(2 * (i0 + r) + pr) * J.pitch) +
                      (2 * j + pc);
        uint16_t* s = &ring[r * OL_RING + (j & (OL_RING - 1))];
        if (load)
          *s = *g;
        else
          *g = *s;
      }
    };
    for (int32_t c = 0; c <= n_tiles; ++c) {
      if (c >= 2)
        tile_io(c - 2, false); // (every lane is past tile c-2: lane 63 stands at column 64 (c-1))
      if (c < n_tiles)
        tile_io(c, true);
      __syncthreads();
      for (int32_t t = c * OL_TILE; t < (c + 1) * OL_TILE; ++t) {
        const int32_t j = t - lane;
        // U: the lane above finished (i-1, j) in the step before; lane 0 takes it from the band
        // before.  NW is this lane's U of the step before.
        int32_t up = ol_from_lane_above(cur);
        if (lane == 0)
          up = (i0 != 0 && t < pw) ? int32_t(prev_row[t]) : 0;
        if (live && j >= 0 && j < pw) {
          uint16_t* cell = &ring[lane * OL_RING + (j & (OL_RING - 1))];
          const int32_t v = (pred(i, j, left, up, up_prev) + int32_t(*cell)) & 0xFFFF;
          *cell = uint16_t(v);
          if (lane == rows - 1)
            prev_row[j] = uint16_t(v); // (lane 0 read column j of the band before 63 steps ago)
          left = v;
          cur = v;
        }
        up_prev = up;
      }
      __syncthreads();
    }
    tile_io(n_tiles - 1, false);
    __syncthreads();
  }
}

} // namespace

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
namespace {
struct OlympusPlan final : DecoderPlan {
  rsx_ctx* ctx = nullptr;
  JobStatus status;
  DeviceBuffer d_jobs;
  uint32_t n_dev = 0; // jobs that go to the device
  bool launched = false;
  int run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) override;
  int results(hipStream_t s, bool ran, int32_t* job_status, uint32_t* job_consumed) override;
  int row_status(hipStream_t s, int job, int32_t* statuses) override;
};
} // namespace

int olympus_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_olympus_job* jobs,
                        std::unique_ptr<DecoderPlan>* out) {
  auto p = std::make_unique<OlympusPlan>();
  p->ctx = ctx;
  p->status.host.assign(n_jobs, RSX_OK);
  std::vector<OlJobDev> dev;
  for (int i = 0; i < n_jobs; ++i) {
    const rsx_olympus_job& j = jobs[i];
    int st = validate(j.in_bytes, &j.img);
    if (st == RSX_OK && (j.img_offset % 2 != 0 || j.img.pitch_bytes % 2 != 0))
      st = RSX_ERR_INVALID_ARG;
    p->status.host[i] = st;
    if (st != RSX_OK)
      continue;
    OlJobDev D;
    std::memset(&D, 0, sizeof D);
    D.in_off = j.in_offset + SKIP;
    D.out_off = j.img_offset;
    D.size = j.in_bytes - SKIP;
    D.pitch = j.img.pitch_bytes;
    D.job = uint32_t(i);
    D.dim_x = j.img.dim_x;
    D.dim_y = j.img.dim_y;
    dev.push_back(D);
  }
  p->n_dev = uint32_t(dev.size());
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int st;
  if ((st = upload(ctx, p->d_jobs, dev)) || (st = p->status.init()))
    return st;
  *out = std::move(p);
  return RSX_OK;
}

int OlympusPlan::run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) {
  if (n_dev == 0)
    return RSX_OK; // (every job was rejected by the host)
  if (timer)
    timer->begin(s);
  OlArgs A{};
  A.in_base = static_cast<const uint8_t*>(in_dev);
  A.out_base = static_cast<uint8_t*>(out_dev);
  A.jobs = static_cast<const OlJobDev*>(d_jobs.ptr);
  A.job_status = static_cast<uint32_t*>(status.dev.ptr);
  if (int st = status.reset(ctx, s))
    return st;
  hipLaunchKernelGGL(olympus_parse_kernel, dim3(n_dev), dim3(OL_THREADS), 0, s, A);
  if (timer)
    timer->mark("olympus_parse_kernel");
  hipLaunchKernelGGL(olympus_recon_kernel, dim3(4 * n_dev), dim3(OL_THREADS), 0, s, A);
  if (timer)
    timer->mark("olympus_recon_kernel");
  RSX_HIP_CHECK(ctx, hipGetLastError());
  launched = true;
  return RSX_OK;
}

// The status of the lowest-numbered failing job, or RSX_OK.
int OlympusPlan::results(hipStream_t s, bool ran, int32_t* job_status, uint32_t* job_consumed) {
  if (job_consumed)
    std::fill(job_consumed, job_consumed + status.host.size(), 0u);
  return status.fold(ctx, s, ran && n_dev != 0, ~0u, FoldOrder::LOWEST_FAILING, job_status);
}

// One status a job: what results() gave for it.
int OlympusPlan::row_status(hipStream_t, int job, int32_t* statuses) {
  if (job < 0 || size_t(job) >= status.host.size() || !statuses)
    return RSX_ERR_INVALID_ARG;
  int st = status.host[job];
  if (st == RSX_OK) {
    if (!launched || !status.fetched || status.words[job] == STATUS_NONE)
      return RSX_ERR_INVALID_ARG; // (before a run and its results)
    st = int(status.words[job]);
  }
  statuses[0] = st;
  return RSX_OK;
}

} // namespace rsx
