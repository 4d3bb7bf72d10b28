// rstest's image hash and rawspeed-identify's sums on gfx950: include/rsx.h section 4g, DESIGN.md
// 4.26.
//
// MD5 of a row is one serial chain, but the rows of an image are independent and so are the
// images of a plan.  Two launches serve every job of a plan:
//   image_hash_rows_kernel    a lane a row, 64 consecutive rows of one job a wavefront, a wavefront
//                             a workgroup.  The work list is flat: a wavefront finds its job by
//                             search in the plan's start table, so the job count is bounded by no
//                             grid axis.  A lane holds the state and two blocks of sixteen words in
//                             registers: the next block is loaded in front of the 64 steps of the
//                             current one.  Rows whose base and pitch lie on the 16-byte grid take
//                             four 16-byte loads a block; the others 4-byte or 2-byte loads.  The
//                             rest of the row and the padding are made in the words.  The sums of
//                             the bytes and of the 16-bit samples run along (one instruction a word
//                             each).  A lane stores its digest as 16 bytes; lane 0 stores the
//                             wavefront's two sums into the plan's scratch.  (A variant that
//                             stages the blocks through LDS with coalesced loads was no faster
//                             and stays behind RSX_IMAGE_HASH_KERNEL=lds.)
//   image_hash_finish_kernel  a lane a job: the MD5 of the job's digests (64 bytes a block, one
//                             padding block), the wavefronts' sums added in order, the 32-byte
//                             result.  For a tall image this chain of dim_y / 4 blocks on one lane
//                             is the larger part of the time (profiles/image_hash/README.md).
// Nothing is added with atomics: a run's results do not depend on the order of anything.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "rsx_image_hash.h"
#include "rsx_image_hash_core.h"
#include "rsx_ljpeg_dev.h"
#include "rsx_plan_host.h"

namespace rsx {

using namespace rsx_imghash;

namespace {

struct HashJobDev {
  uint64_t img_off, lines_off, result_off;
  uint32_t row_bytes, pitch, dim_y, sample_bytes;
  uint32_t first_wave, n_waves; // of the plan's flat list of wavefronts
};

struct HashSums {
  uint64_t bytes, halves;
};

struct HashArgs {
  const uint8_t* in_base;
  uint8_t* out_base;
  const HashJobDev* jobs;
  const uint32_t* starts; // first_wave of every job, and the total behind them
  HashSums* partials;     // a pair a wavefront
  uint32_t n_jobs;
};

template <class T>
__device__ __forceinline__ T load_as(const uint8_t* p) {
  return *reinterpret_cast<const T*>(p);
}

// a whole block; ALIGN: what the row's base and the pitch are multiples of (16, 4 or 2)
template <int ALIGN>
__device__ __forceinline__ void load_block(const uint8_t* p, uint32_t w[16]) {
  if constexpr (ALIGN == 16) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint4 v = load_as<uint4>(p + 16 * k);
      w[4 * k] = v.x;
      w[4 * k + 1] = v.y;
      w[4 * k + 2] = v.z;
      w[4 * k + 3] = v.w;
    }
  } else if constexpr (ALIGN == 4) {
#pragma unroll
    for (int i = 0; i < 16; ++i)
      w[i] = load_as<uint32_t>(p + 4 * i);
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i)
      w[i] = uint32_t(load_as<uint16_t>(p + 4 * i)) | uint32_t(load_as<uint16_t>(p + 4 * i + 2)) << 16;
  }
}

// The n < 64 bytes behind the last whole block (n is a multiple of 2), zeros above them; no byte
// past p + n is read.  Once a row, so 2-byte loads whatever the grid, and without a branch per
// word (a branch each made the loads wait for one another): a half that lies past the end loads
// the row's last two bytes instead and is dropped.
__device__ __forceinline__ void load_tail(const uint8_t* p, uint32_t n, uint32_t w[16]) {
  if (n == 0) {
#pragma unroll
    for (int i = 0; i < 16; ++i)
      w[i] = 0u;
    return;
  }
  uint32_t half[32];
#pragma unroll
  for (int k = 0; k < 32; ++k) {
    const uint32_t at = 2u * uint32_t(k);
    half[k] = load_as<uint16_t>(p + (at < n ? at : n - 2u));
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint32_t lo = 4u * uint32_t(i);
    w[i] = (lo < n ? half[2 * i] : 0u) | (lo + 2u < n ? half[2 * i + 1] << 16 : 0u);
  }
}

__device__ __forceinline__ void add_block(const uint32_t w[16], uint64_t& bytes, uint64_t& halves) {
  uint32_t bs = 0, hs = 0; // (at most 16 x 1020 and 16 x 131070)
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    bs = add_bytes(bs, w[i]);
    hs = add_halves(hs, w[i]);
  }
  bytes += bs;
  halves += hs;
}

// The row at p: every lane of the wavefront has the same row_bytes, so the loop is uniform.  The
// sums of a block are taken where its words arrive, in front of the next block's loads: the wait
// for the words then stands there, and the 64 steps run with the next loads in flight.  The rest
// of the row is loaded behind the loop (once a row; inside the loop its 32 uniform offsets would
// be kept in scalar registers across the steps).
template <int ALIGN>
__device__ __forceinline__ void hash_row_lane(const uint8_t* p, uint32_t row_bytes, uint32_t s[4],
                                              uint64_t& bytes, uint64_t& halves) {
  uint32_t cur[16], nxt[16];
  init_state(s);
  bytes = halves = 0;
  const uint32_t blocks = row_bytes >> 6, rest = row_bytes & 63u;
  if (blocks)
    load_block<ALIGN>(p, nxt);
  for (uint32_t b = 0; b < blocks; ++b) {
#pragma unroll
    for (int i = 0; i < 16; ++i)
      cur[i] = nxt[i];
    add_block(cur, bytes, halves);
    if (b + 1u < blocks)
      load_block<ALIGN>(p + (size_t(b) + 1u) * 64u, nxt);
    compress(s, cur);
  }
  load_tail(p + size_t(blocks) * 64u, rest, cur);
  add_block(cur, bytes, halves);
  finish(s, cur, row_bytes);
}

// The same row with its whole blocks staged through LDS (16-byte grid only): the variant that lost,
// kept behind RSX_IMAGE_HASH_KERNEL=lds.  A wavefront's 64 rows are 64 cache lines to every direct
// load instruction; here a load instruction takes 64 contiguous bytes of 16 rows (four lanes a
// row), a quarter of the lines, and the lanes exchange through LDS: lane L writes the chunk (row
// 16 k + L / 4, bytes 16 (L % 4) ..) of load k and reads the four chunks of its own row.  Rows are
// 80 bytes apart in LDS, so neither the 16-byte writes nor the reads meet in a bank.  One wavefront
// a workgroup: the barriers order the wavefront's own LDS traffic.  `first` is row 0 of the
// wavefront's rows, `last_row` the last one that exists.  Measured 3 to 6 % slower than the direct
// loads from 1 to 64 frames of 8192 x 5464.
constexpr int STAGE_PITCH = 80;

__device__ __forceinline__ void stage_load(const uint8_t* first, uint32_t pitch, uint32_t last_row,
                                           size_t at, uint4 v[4]) {
  const uint32_t lane = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t r = min(16u * uint32_t(k) + (lane >> 2), last_row);
    v[k] = load_as<uint4>(first + uint64_t(r) * pitch + at + 16u * (lane & 3u));
  }
}

__device__ __forceinline__ void hash_row_lane_staged(const uint8_t* first, uint32_t pitch,
                                                     uint32_t last_row, const uint8_t* p,
                                                     uint32_t row_bytes, uint8_t* lds, uint32_t s[4],
                                                     uint64_t& bytes, uint64_t& halves) {
  const uint32_t lane = threadIdx.x;
  uint32_t cur[16];
  uint4 nxt[4];
  init_state(s);
  bytes = halves = 0;
  const uint32_t blocks = row_bytes >> 6, rest = row_bytes & 63u;
  if (blocks)
    stage_load(first, pitch, last_row, 0, nxt);
  for (uint32_t b = 0; b < blocks; ++b) {
    __syncthreads(); // (the reads of the block before are done)
#pragma unroll
    for (int k = 0; k < 4; ++k)
      *reinterpret_cast<uint4*>(lds + (16u * uint32_t(k) + (lane >> 2)) * STAGE_PITCH +
                                16u * (lane & 3u)) = nxt[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint4 v = *reinterpret_cast<const uint4*>(lds + lane * STAGE_PITCH + 16 * k);
      cur[4 * k] = v.x;
      cur[4 * k + 1] = v.y;
      cur[4 * k + 2] = v.z;
      cur[4 * k + 3] = v.w;
    }
    add_block(cur, bytes, halves);
    if (b + 1u < blocks)
      stage_load(first, pitch, last_row, (size_t(b) + 1u) * 64u, nxt);
    compress(s, cur);
  }
  load_tail(p + size_t(blocks) * 64u, rest, cur);
  add_block(cur, bytes, halves);
  finish(s, cur, row_bytes);
}

template <bool STAGED>
__global__ __launch_bounds__(ROWS_PER_WAVE) void image_hash_rows_kernel(HashArgs A) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[STAGED ? ROWS_PER_WAVE * STAGE_PITCH : 16];
  const uint32_t wave = blockIdx.x;
  uint32_t lo = 0, hi = A.n_jobs - 1u;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1u) >> 1;
    if (A.starts[mid] <= wave)
      lo = mid;
    else
      hi = mid - 1u;
  }
  const HashJobDev& J = A.jobs[lo];
  const uint32_t row = (wave - J.first_wave) * uint32_t(ROWS_PER_WAVE) + threadIdx.x;
  const bool live = row < J.dim_y;
  // (a lane behind the last row takes the last row along: same loads, nothing stored or added)
  const uint8_t* base = A.in_base + J.img_off;
  const uint8_t* p = base + uint64_t(live ? row : J.dim_y - 1u) * J.pitch;
  const uint32_t grid = uint32_t(reinterpret_cast<uintptr_t>(base)) | J.pitch;
  uint32_t s[4];
  uint64_t bytes, halves;
  if (STAGED && (grid & 15u) == 0) {
    const uint32_t row0 = (wave - J.first_wave) * uint32_t(ROWS_PER_WAVE);
    hash_row_lane_staged(base + uint64_t(row0) * J.pitch, J.pitch, J.dim_y - 1u - row0, p,
                         J.row_bytes, lds, s, bytes, halves);
  } else if ((grid & 15u) == 0)
    hash_row_lane<16>(p, J.row_bytes, s, bytes, halves);
  else if ((grid & 3u) == 0)
    hash_row_lane<4>(p, J.row_bytes, s, bytes, halves);
  else
    hash_row_lane<2>(p, J.row_bytes, s, bytes, halves);
  if (live)
    *reinterpret_cast<uint4*>(A.out_base + J.lines_off + uint64_t(row) * 16u) =
        make_uint4(s[0], s[1], s[2], s[3]);
  if (!live)
    bytes = halves = 0;
  if (J.sample_bytes != 2u)
    halves = 0; // (identify's F32 sample sum has no one answer: rsx.h)
#pragma unroll
  for (int off = ROWS_PER_WAVE / 2; off > 0; off >>= 1) {
    bytes += __shfl_down(bytes, off, ROWS_PER_WAVE);
    halves += __shfl_down(halves, off, ROWS_PER_WAVE);
  }
  if (threadIdx.x == 0)
    A.partials[wave] = HashSums{bytes, halves};
}

__global__ __launch_bounds__(64) void image_hash_finish_kernel(HashArgs A) {
  const uint32_t j = blockIdx.x * 64u + threadIdx.x;
  if (j >= A.n_jobs)
    return;
  const HashJobDev J = A.jobs[j];
  const uint8_t* lines = A.out_base + J.lines_off;
  uint32_t s[4], w[16];
  init_state(s);
  const uint32_t blocks = J.dim_y >> 2, rest = J.dim_y & 3u;
  for (uint32_t b = 0; b < blocks; ++b) {
    load_block<16>(lines + size_t(b) * 64u, w);
    compress(s, w);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (uint32_t(k) < rest)
      v = load_as<uint4>(lines + size_t(blocks) * 64u + 16 * k);
    w[4 * k] = v.x;
    w[4 * k + 1] = v.y;
    w[4 * k + 2] = v.z;
    w[4 * k + 3] = v.w;
  }
  finish(s, w, uint64_t(J.dim_y) * 16u);
  uint64_t bytes = 0, halves = 0;
  for (uint32_t k = 0; k < J.n_waves; ++k) {
    const HashSums t = A.partials[J.first_wave + k];
    bytes += t.bytes;
    halves += t.halves;
  }
  uint64_t* out = reinterpret_cast<uint64_t*>(A.out_base + J.result_off);
  out[0] = uint64_t(s[0]) | uint64_t(s[1]) << 32;
  out[1] = uint64_t(s[2]) | uint64_t(s[3]) << 32;
  out[2] = bytes;
  out[3] = halves;
}

struct ImageHashPlan final : DecoderPlan {
  rsx_ctx* ctx = nullptr;
  std::vector<int32_t> host;    // validation result per job
  std::vector<HashJobDev> jobs; // the jobs that go to the device
  std::vector<uint32_t> starts;
  DeviceBuffer d_jobs, d_starts, d_partials;
  uint64_t total_waves = 0;
  bool has_f32 = false;
  bool staged = false; // the row kernel with the blocks staged through LDS

  void add(const rsx_image_hash_job& j) {
    HashJobDev D;
    std::memset(&D, 0, sizeof D);
    D.img_off = j.img_offset;
    D.lines_off = j.lines_offset;
    D.result_off = j.result_offset;
    D.row_bytes = uint32_t(j.img.dim_x) * uint32_t(j.img.cpp) * uint32_t(j.sample_bytes);
    D.pitch = j.img.pitch_bytes;
    D.dim_y = uint32_t(j.img.dim_y);
    D.sample_bytes = uint32_t(j.sample_bytes);
    D.first_wave = uint32_t(total_waves);
    D.n_waves = (D.dim_y + uint32_t(ROWS_PER_WAVE) - 1u) / uint32_t(ROWS_PER_WAVE);
    total_waves += D.n_waves;
    has_f32 = has_f32 || j.sample_bytes == 4;
    jobs.push_back(D);
  }
  int finish() {
    if (total_waves > 0x7FFFFFFFull)
      return RSX_ERR_UNSUPPORTED; // (a wavefront is a workgroup of the launch's grid)
    starts.reserve(jobs.size() + 1);
    for (const HashJobDev& D : jobs)
      starts.push_back(D.first_wave);
    starts.push_back(uint32_t(total_waves));
    RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    // The direct kernel ships: the staged one was no faster at any plan size measured
    // (profiles/image_hash/README.md).  RSX_IMAGE_HASH_KERNEL=lds, read here, selects it.
    if (const char* which = getenv("RSX_IMAGE_HASH_KERNEL"))
      staged = !std::strcmp(which, "lds");
    if (int st = upload(ctx, d_jobs, jobs))
      return st;
    if (int st = upload(ctx, d_starts, starts))
      return st;
    return d_partials.ensure(size_t(total_waves) * sizeof(HashSums) + 16);
  }
  int run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) override {
    if (jobs.empty())
      return RSX_OK; // (every job was refused by the host)
    // the samples must lie on their own grid, the digests on the 16-byte one
    if (reinterpret_cast<uintptr_t>(in_dev) % (has_f32 ? 4u : 2u) != 0 ||
        reinterpret_cast<uintptr_t>(out_dev) % 16u != 0)
      return RSX_ERR_INVALID_ARG;
    HashArgs A{};
    A.in_base = static_cast<const uint8_t*>(in_dev);
    A.out_base = static_cast<uint8_t*>(out_dev);
    A.jobs = static_cast<const HashJobDev*>(d_jobs.ptr);
    A.starts = static_cast<const uint32_t*>(d_starts.ptr);
    A.partials = static_cast<HashSums*>(d_partials.ptr);
    A.n_jobs = uint32_t(jobs.size());
    if (timer)
      timer->begin(s);
    if (staged)
      hipLaunchKernelGGL(image_hash_rows_kernel<true>, dim3(uint32_t(total_waves)),
                         dim3(ROWS_PER_WAVE), 0, s, A);
    else
      hipLaunchKernelGGL(image_hash_rows_kernel<false>, dim3(uint32_t(total_waves)),
                         dim3(ROWS_PER_WAVE), 0, s, A);
    if (timer)
      timer->mark("image_hash_rows_kernel");
    hipLaunchKernelGGL(image_hash_finish_kernel, dim3((A.n_jobs + 63u) / 64u), dim3(64), 0, s, A);
    if (timer)
      timer->mark("image_hash_finish_kernel");
    RSX_HIP_CHECK(ctx, hipGetLastError());
    return RSX_OK;
  }
  int results(hipStream_t, bool, int32_t* job_status, uint32_t* job_consumed) override {
    if (job_consumed)
      std::fill(job_consumed, job_consumed + host.size(), 0u);
    return fold_jobs(host.size(), FoldOrder::LAST_FAILING, job_status,
                     [&](size_t i) { return int(host[i]); });
  }
};

} // namespace

int image_hash_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_image_hash_job* jobs,
                           std::unique_ptr<DecoderPlan>* out) {
  auto p = std::make_unique<ImageHashPlan>();
  p->ctx = ctx;
  p->host.assign(n_jobs, RSX_OK);
  for (int i = 0; i < n_jobs; ++i) {
    const rsx_image_hash_job& j = jobs[i];
    int st = validate(&j.img, j.sample_bytes);
    if (st == RSX_OK && (j.lines_offset % 16u != 0 || j.result_offset % 8u != 0 ||
                         j.img_offset % uint64_t(j.sample_bytes) != 0))
      st = RSX_ERR_INVALID_ARG;
    p->host[i] = st;
    if (st == RSX_OK)
      p->add(j);
  }
  if (int st = p->finish())
    return st;
  *out = std::move(p);
  return RSX_OK;
}

} // namespace rsx
