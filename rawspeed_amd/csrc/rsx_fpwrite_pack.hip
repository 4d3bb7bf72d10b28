// rsx_fpwrite_pack.hip -- the writers of F32 images for gfx950 (include/rsx.h section 7d,
// DESIGN.md 4.28): the inverse of rsx_unpack_f32 (copyPixels and decodePackedFP<Pump, Binary16 |
// Binary24>) with the exact narrowing of rsx_fp_narrow.h, and the width class of windows.
//
// Pack: as in rsx_encode_pack.hip a lane owns 16 output bytes and gathers the samples that cover
// them (pack_chunk of rsx_fpwrite_core.h); a workgroup of 256 lanes owns 4096 consecutive output
// bytes of one job and finds its job by search in the plan's start table.  A lane that meets
// samples without a narrow pattern adds their number to its job's counter: a sum, so the order of
// the lanes does not show.  The counters are cleared on the run's stream in front of the launch.
//
// Fit: a window is cut into pieces of 4096 samples; up to 1024 workgroups a window take every
// n-th piece (a lane loads 16 bytes at once where the window's rows lie on that grid), fold the classes of their samples through LDS and atomicMax the result into the
// window's word (a maximum: order does not show either).  All windows share one launch.
#include <hip/hip_runtime.h>

#include <memory>
#include <vector>

#include "rsx_fpwrite.h"
#include "rsx_fpwrite_core.h"
#include "rsx_ljpeg_dev.h"
#include "rsx_plan_host.h"

namespace rsx {

using namespace rsx_fpwrite;

namespace {

// the job of workgroup `block`: the last one whose first workgroup is not behind it
__device__ __forceinline__ uint32_t job_of_block(const uint32_t* starts, uint32_t n_jobs,
                                                 uint32_t block) {
  uint32_t lo = 0, hi = n_jobs - 1u;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1u) >> 1;
    if (starts[mid] <= block)
      lo = mid;
    else
      hi = mid - 1u;
  }
  return lo;
}

struct PackArgs {
  const uint8_t* in_base;
  uint8_t* out_base;
  const PackGeom* jobs;
  const uint32_t* starts; // first_block of every job, and the total behind them
  unsigned long long* inexact; // one counter a job of the plan
  uint32_t n_jobs;
};

__global__ __launch_bounds__(PACK_THREADS) void fpwrite_pack_kernel(PackArgs A) {
  const uint32_t block = blockIdx.x;
  const PackGeom g = A.jobs[job_of_block(A.starts, A.n_jobs, block)];
  const uint64_t k = uint64_t(block - g.first_block) * PACK_THREADS + threadIdx.x;
  const uint64_t at = k * PACK_LANE_BYTES;
  if (at >= g.out_bytes)
    return;
  uint32_t w[4];
  const uint32_t bad = pack_chunk(A.in_base, g, k, w);
  if (bad)
    atomicAdd(&A.inexact[g.job], static_cast<unsigned long long>(bad));
  uint8_t* dst = A.out_base + g.out_off + at;
  const uint64_t left = g.out_bytes - at; // a multiple of 4
  const uintptr_t a = reinterpret_cast<uintptr_t>(dst);
  if (left >= 16u && (a & 15u) == 0) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    u32x4 t;
    t.x = w[0], t.y = w[1], t.z = w[2], t.w = w[3];
    __builtin_nontemporal_store(t, reinterpret_cast<u32x4*>(dst));
  } else if ((a & 3u) == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (uint64_t(4 * i) < left)
        reinterpret_cast<uint32_t*>(dst)[i] = w[i];
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (uint64_t(i) < left)
        dst[i] = uint8_t(w[i >> 2] >> (8 * (i & 3)));
  }
}

struct FitArgs {
  const uint8_t* in_base;
  uint32_t* out; // one word a window, cleared in front of the launch
  const FitGeom* jobs;
  const uint32_t* starts;
  uint32_t n_jobs;
};

__global__ __launch_bounds__(FIT_THREADS) void fpwrite_fit_kernel(FitArgs A) {
  __shared__ uint32_t group_cls;
  const uint32_t block = blockIdx.x;
  const uint32_t job = job_of_block(A.starts, A.n_jobs, block);
  const FitGeom g = A.jobs[job];
  if (threadIdx.x == 0)
    group_cls = 0;
  __syncthreads();
  uint32_t cls = 0;
  // rows of whole 16-byte groups on the 16-byte grid: a lane loads four samples at once
  const bool quads = g.w % 4u == 0 && g.img_pitch % 16u == 0 &&
                     (reinterpret_cast<uintptr_t>(A.in_base) + g.img_off) % 16u == 0;
  if (quads) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    constexpr uint32_t PIECE = FIT_BLOCK_SAMPLES / 4;
    const uint64_t n = g.samples >> 2;
    const uint32_t wq = g.w >> 2;
    for (uint64_t base = uint64_t(block - g.first_block) * PIECE; base < n;
         base += uint64_t(g.n_blocks) * PIECE) {
#pragma unroll
      for (int j = 0; j < FIT_LANE_SAMPLES / 4; ++j) {
        const uint64_t q = base + uint64_t(j) * FIT_THREADS + threadIdx.x;
        if (q < n) {
          uint64_t r = 0;
          if (q >= wq)
            r = q <= 0xFFFFFFFFull ? uint64_t(uint32_t(q) / wq) : q / wq;
          const u32x4 v = *reinterpret_cast<const u32x4*>(A.in_base + g.img_off + r * g.img_pitch +
                                                         (q - r * wq) * 16u);
          const uint32_t a = fp_fit_class(v.x), b = fp_fit_class(v.y);
          const uint32_t c = fp_fit_class(v.z), d = fp_fit_class(v.w);
          const uint32_t ab = a > b ? a : b, cd = c > d ? c : d;
          const uint32_t m = ab > cd ? ab : cd;
          cls = m > cls ? m : cls;
        }
      }
    }
  } else {
    for (uint64_t base = uint64_t(block - g.first_block) * FIT_BLOCK_SAMPLES; base < g.samples;
         base += uint64_t(g.n_blocks) * FIT_BLOCK_SAMPLES) {
#pragma unroll 4
      for (int j = 0; j < FIT_LANE_SAMPLES; ++j) {
        const uint64_t i = base + uint64_t(j) * FIT_THREADS + threadIdx.x;
        if (i < g.samples) {
          const uint32_t c = fit_sample_class(A.in_base, g, i);
          cls = c > cls ? c : cls;
        }
      }
    }
  }
  if (cls)
    atomicMax(&group_cls, cls);
  __syncthreads();
  if (threadIdx.x == 0 && group_cls)
    atomicMax(&A.out[job], group_cls);
}

struct FpPackPlan final : DecoderPlan {
  rsx_ctx* ctx = nullptr;
  std::vector<int32_t> host;      // validation result per job
  std::vector<uint64_t> written;  // roundUp(crop_h pitch, 4) per job (0 for a refused one)
  std::vector<uint64_t> stream;   // crop_h pitch per job
  std::vector<PackGeom> jobs;     // the jobs that go to the device
  std::vector<uint32_t> starts;
  std::vector<unsigned long long> counts; // of the last fetch, one a job of the plan
  DeviceBuffer d_jobs, d_starts, d_counts;
  uint64_t total_blocks = 0;
  bool fetched = false;

  int finish() {
    for (const PackGeom& g : jobs)
      starts.push_back(g.first_block);
    starts.push_back(uint32_t(total_blocks));
    counts.assign(host.size(), 0ull);
    RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (int st = upload(ctx, d_jobs, jobs))
      return st;
    if (int st = upload(ctx, d_starts, starts))
      return st;
    return d_counts.ensure(counts.size() * sizeof(unsigned long long) + 16);
  }
  int run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) override {
    fetched = false;
    if (jobs.empty())
      return RSX_OK; // (every job was refused by the host)
    if (reinterpret_cast<uintptr_t>(in_dev) % 4u != 0)
      return RSX_ERR_INVALID_ARG; // the samples lie on their grid
    RSX_HIP_CHECK(ctx, hipMemsetAsync(d_counts.ptr, 0, counts.size() * sizeof(unsigned long long), s));
    PackArgs A{};
    A.in_base = static_cast<const uint8_t*>(in_dev);
    A.out_base = static_cast<uint8_t*>(out_dev);
    A.jobs = static_cast<const PackGeom*>(d_jobs.ptr);
    A.starts = static_cast<const uint32_t*>(d_starts.ptr);
    A.inexact = static_cast<unsigned long long*>(d_counts.ptr);
    A.n_jobs = uint32_t(jobs.size());
    if (timer)
      timer->begin(s);
    hipLaunchKernelGGL(fpwrite_pack_kernel, dim3(uint32_t(total_blocks)), dim3(PACK_THREADS), 0, s, A);
    if (timer)
      timer->mark("fpwrite_pack_kernel");
    RSX_HIP_CHECK(ctx, hipGetLastError());
    return RSX_OK;
  }
  int status_of(size_t i) const {
    return host[i] != RSX_OK ? int(host[i]) : fetched && counts[i] ? RSX_ERR_VALUE_RANGE : RSX_OK;
  }
  int results(hipStream_t s, bool ran, int32_t* job_status, uint32_t* job_consumed) override {
    if (ran && !jobs.empty() && !fetched) {
      RSX_HIP_CHECK(ctx, hipMemcpyAsync(counts.data(), d_counts.ptr,
                                        counts.size() * sizeof(unsigned long long),
                                        hipMemcpyDeviceToHost, s));
      RSX_HIP_CHECK(ctx, hipStreamSynchronize(s));
      fetched = true;
    }
    if (job_consumed)
      for (size_t i = 0; i < host.size(); ++i)
        job_consumed[i] = status_of(i) == RSX_OK ? uint32_t(written[i]) : 0u;
    return fold_jobs(host.size(), FoldOrder::LAST_FAILING, job_status,
                     [&](size_t i) { return status_of(i); });
  }
  int fpwrite_pack_result(int job, rsx_fpwrite_pack_result* out) override {
    if (job < 0 || size_t(job) >= host.size() || !out)
      return RSX_ERR_INVALID_ARG;
    const int st = status_of(size_t(job));
    out->bytes_written = st == RSX_OK ? written[job] : 0;
    out->stream_bytes = host[job] == RSX_OK ? stream[job] : 0;
    out->inexact = host[job] == RSX_OK && fetched ? counts[job] : 0;
    return st;
  }
};

struct FpFitPlan final : DecoderPlan {
  rsx_ctx* ctx = nullptr;
  std::vector<FitGeom> jobs;
  std::vector<uint32_t> starts;
  DeviceBuffer d_jobs, d_starts;
  uint32_t total_blocks = 0;

  int run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) override {
    if (reinterpret_cast<uintptr_t>(in_dev) % 4u != 0 || reinterpret_cast<uintptr_t>(out_dev) % 4u != 0)
      return RSX_ERR_INVALID_ARG;
    RSX_HIP_CHECK(ctx, hipMemsetAsync(out_dev, 0, jobs.size() * 4u, s));
    FitArgs A{};
    A.in_base = static_cast<const uint8_t*>(in_dev);
    A.out = static_cast<uint32_t*>(out_dev);
    A.jobs = static_cast<const FitGeom*>(d_jobs.ptr);
    A.starts = static_cast<const uint32_t*>(d_starts.ptr);
    A.n_jobs = uint32_t(jobs.size());
    if (timer)
      timer->begin(s);
    hipLaunchKernelGGL(fpwrite_fit_kernel, dim3(total_blocks), dim3(FIT_THREADS), 0, s, A);
    if (timer)
      timer->mark("fpwrite_fit_kernel");
    RSX_HIP_CHECK(ctx, hipGetLastError());
    return RSX_OK;
  }
  int results(hipStream_t, bool, int32_t* job_status, uint32_t* job_consumed) override {
    if (job_status)
      job_status[0] = RSX_OK;
    if (job_consumed)
      job_consumed[0] = 0;
    return RSX_OK;
  }
};

} // namespace

int fpwrite_pack_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_fpwrite_pack_job* jobs,
                             std::unique_ptr<DecoderPlan>* out) {
  auto p = std::make_unique<FpPackPlan>();
  p->ctx = ctx;
  p->host.assign(n_jobs, RSX_OK);
  p->written.assign(n_jobs, 0);
  p->stream.assign(n_jobs, 0);
  for (int i = 0; i < n_jobs; ++i) {
    const rsx_fpwrite_pack_job& j = jobs[i];
    int st = validate_pack(&j.desc, &j.img, j.out_cap);
    if (st == RSX_OK && j.img_offset % 4u != 0)
      st = RSX_ERR_INVALID_ARG;
    p->host[i] = st;
    if (st != RSX_OK)
      continue;
    PackGeom g;
    pack_geom(j.desc, j.img, j.img_offset, j.out_offset, &g);
    g.first_block = uint32_t(p->total_blocks);
    g.job = uint32_t(i);
    p->total_blocks += (g.out_bytes + PACK_BLOCK_BYTES - 1u) / PACK_BLOCK_BYTES;
    if (p->total_blocks > 0x7FFFFFFFull)
      return RSX_ERR_UNSUPPORTED; // (a launch's grid)
    p->written[i] = g.out_bytes;
    p->stream[i] = g.stream_bytes;
    p->jobs.push_back(g);
  }
  if (int st = p->finish())
    return st;
  *out = std::move(p);
  return RSX_OK;
}

int fpwrite_fit_plan_create(rsx_ctx* ctx, int n_jobs, const FpFitJob* jobs,
                            std::unique_ptr<DecoderPlan>* out) {
  if (n_jobs != 1)
    return RSX_ERR_INVALID_ARG;
  const FpFitJob& j = jobs[0];
  if (int st = validate_fit(&j.img, j.n_windows, j.windows))
    return st;
  auto p = std::make_unique<FpFitPlan>();
  p->ctx = ctx;
  uint64_t total = 0;
  for (int i = 0; i < j.n_windows; ++i) {
    FitGeom g;
    fit_geom(j.img, j.windows[i], &g);
    g.first_block = uint32_t(total);
    total += g.n_blocks;
    if (total > 0x7FFFFFFFull)
      return RSX_ERR_UNSUPPORTED; // (a launch's grid)
    p->jobs.push_back(g);
    p->starts.push_back(g.first_block);
  }
  p->starts.push_back(uint32_t(total));
  p->total_blocks = uint32_t(total);
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (int st = upload(ctx, p->d_jobs, p->jobs))
    return st;
  if (int st = upload(ctx, p->d_starts, p->starts))
    return st;
  *out = std::move(p);
  return RSX_OK;
}

} // namespace rsx
