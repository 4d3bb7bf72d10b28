// rsx_encode_pack.hip -- packed-integer writer for gfx950: the mirror of rsx_unpack.hip, the
// inverse of UncompressedDecompressor::decodePackedInt, what BitVacuumer{LSB,MSB,MSB16,MSB32}
// write (include/rsx.h section 7a).
//
// A lane owns 16 output bytes and gathers the samples that cover them (pack_chunk of
// rsx_encode_core.h: the closed form of SURVEY.md A.1 the other way round; MSB16 and MSB32 are its
// byte permutation).  A workgroup of 256 lanes owns 4096 consecutive output bytes of one job; the
// jobs of a plan share one launch, a workgroup finds its job by search in the plan's start table.
// Neighbouring lanes read neighbouring samples, so a wavefront's loads fall into consecutive cache
// lines; the store is one 16-byte store where the address allows.  No atomics, no LDS.
#include <hip/hip_runtime.h>

#include <memory>
#include <vector>

#include "rsx_encode.h"
#include "rsx_encode_core.h"
#include "rsx_ljpeg_dev.h"
#include "rsx_plan_host.h"

namespace rsx {

using namespace rsx_encode;

namespace {

struct PackArgs {
  const uint8_t* in_base;
  uint8_t* out_base;
  const PackGeom* jobs;
  const uint32_t* starts; // first_block of every job, and the total behind them
  uint32_t n_jobs;
};

__global__ __launch_bounds__(PACK_THREADS) void encode_pack_kernel(PackArgs A) {
  const uint32_t block = blockIdx.x;
  uint32_t lo = 0, hi = A.n_jobs - 1u;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1u) >> 1;
    if (A.starts[mid] <= block)
      lo = mid;
    else
      hi = mid - 1u;
  }
  const PackGeom g = A.jobs[lo];
  const uint64_t k = uint64_t(block - g.first_block) * PACK_THREADS + threadIdx.x;
  const uint64_t at = k * PACK_LANE_BYTES;
  if (at >= g.out_bytes)
    return;
  uint32_t w[4];
  pack_chunk(A.in_base, g, k, w);
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

struct EncodePackPlan final : DecoderPlan {
  rsx_ctx* ctx = nullptr;
  std::vector<int32_t> host;      // validation result per job
  std::vector<uint64_t> written;  // bytes_written per job (0 for a refused one)
  std::vector<PackGeom> jobs;     // the jobs that go to the device
  std::vector<uint32_t> starts;
  DeviceBuffer d_jobs, d_starts;
  uint64_t total_blocks = 0;

  int finish() {
    if (total_blocks > 0x7FFFFFFFull)
      return RSX_ERR_UNSUPPORTED; // (a launch's grid)
    for (const PackGeom& g : jobs)
      starts.push_back(g.first_block);
    starts.push_back(uint32_t(total_blocks));
    RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (int st = upload(ctx, d_jobs, jobs))
      return st;
    return upload(ctx, d_starts, starts);
  }
  int run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) override {
    if (jobs.empty())
      return RSX_OK; // (every job was refused by the host)
    if (reinterpret_cast<uintptr_t>(in_dev) % 2u != 0)
      return RSX_ERR_INVALID_ARG; // the samples lie on their grid
    PackArgs A{};
    A.in_base = static_cast<const uint8_t*>(in_dev);
    A.out_base = static_cast<uint8_t*>(out_dev);
    A.jobs = static_cast<const PackGeom*>(d_jobs.ptr);
    A.starts = static_cast<const uint32_t*>(d_starts.ptr);
    A.n_jobs = uint32_t(jobs.size());
    if (timer)
      timer->begin(s);
    hipLaunchKernelGGL(encode_pack_kernel, dim3(uint32_t(total_blocks)), dim3(PACK_THREADS), 0, s, A);
    if (timer)
      timer->mark("encode_pack_kernel");
    RSX_HIP_CHECK(ctx, hipGetLastError());
    return RSX_OK;
  }
  int results(hipStream_t, bool, int32_t* job_status, uint32_t* job_consumed) override {
    if (job_consumed)
      for (size_t i = 0; i < host.size(); ++i)
        job_consumed[i] = uint32_t(written[i]);
    return fold_jobs(host.size(), FoldOrder::LAST_FAILING, job_status,
                     [&](size_t i) { return int(host[i]); });
  }
};

} // namespace

int encode_pack_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_encode_pack_job* jobs,
                            std::unique_ptr<DecoderPlan>* out) {
  auto p = std::make_unique<EncodePackPlan>();
  p->ctx = ctx;
  p->host.assign(n_jobs, RSX_OK);
  p->written.assign(n_jobs, 0);
  for (int i = 0; i < n_jobs; ++i) {
    const rsx_encode_pack_job& j = jobs[i];
    int st = validate_pack(&j.desc, &j.img, j.out_cap);
    if (st == RSX_OK && j.img_offset % 2u != 0)
      st = RSX_ERR_INVALID_ARG;
    p->host[i] = st;
    if (st != RSX_OK)
      continue;
    PackGeom g;
    pack_geom(j.desc, j.img, j.img_offset, j.out_offset, &g);
    g.first_block = uint32_t(p->total_blocks);
    p->total_blocks += (g.out_bytes + PACK_BLOCK_BYTES - 1u) / PACK_BLOCK_BYTES;
    if (p->total_blocks > 0x7FFFFFFFull)
      return RSX_ERR_UNSUPPORTED;
    p->written[i] = g.out_bytes;
    p->jobs.push_back(g);
  }
  if (int st = p->finish())
    return st;
  *out = std::move(p);
  return RSX_OK;
}

} // namespace rsx
