// DngDecoder's work behind the tile decode on the device (include/rsx.h section 4d): OpcodeList1
// (common/DngOpcodes.cpp) and the LinearizationTable look-up (RawImageData::sixteenBitLookup ->
// RawImageDataU16::doLookup, common/RawImageDataU16.cpp:488-519).
//
// What the reference does: every opcode is a single-threaded loop over its area, one full pass an
// opcode, and the look-up another pass over the image.  Every one of them reads and writes only
// the sample it stands on, so the list and the look-up are ONE pass.  The parse, the verdicts and
// the tables are host work (rsx_dng_post_core.h, shared with a host build).
//
//   dng_post_kernel<F32>   a lane owns 8 adjacent uint16 samples of an uncropped row (4 of an F32
//                          image) -- one 16-byte load and one 16-byte store where the address
//                          allows, else single samples -- and walks the job's opcode records in
//                          list order: the rectangle, the row phase (uniform along a row), the
//                          column phase kept by counting from one division a lane and opcode (none
//                          for pitches 1 and 2), the plane window, the operation.  Row deltas are
//                          one load a lane; column deltas, MapTable entries (128 KiB a table) and
//                          the dithering table (256 KiB, base | delta << 16) are gathers from
//                          global memory.  The generator of the look-up is jumped to the lane's
//                          first sample with one multiplication mod m (the argument is in the
//                          core header).  FixBadPixelsConstant: a workgroup that met hits takes
//                          one slice of the job's hit buffer with one atomic add and stores its
//                          entries (opcode number, row, column), as rsx_panasonic_v4.hip does;
//                          the host sorts them.  Samples no opcode stood on and that the look-up
//                          does not cover are not written, nor is the pitch padding.
// No scratch; 16 bytes of LDS (the workgroup's hit count and slice).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "rsx_internal.h"
#include "rsx_ljpeg_dev.h"
#include "rsx_plan_host.h"
#include "rsx_dng_post.h"
#include "rsx_dng_post_core.h"

namespace rsx {

namespace {

using namespace rsx_dngpost;

constexpr int DP_THREADS = 256;

struct DpArgs {
  uint8_t* out_base;
  const JobDev* jobs;
  const OpDev* ops;
  const uint16_t* tables;
  const int32_t* deltas;
  const uint32_t* luts;
  const uint32_t* pw;
  uint64_t* hits;
  unsigned long long* counts;
};

template <bool F32>
__global__ void __launch_bounds__(DP_THREADS) dng_post_kernel(DpArgs A) {
  constexpr uint32_t N = F32 ? 4u : 8u;
  __shared__ uint32_t wg_count;
  __shared__ unsigned long long wg_slice;
  const JobDev& J = A.jobs[blockIdx.y];
  if ((J.is_f32 != 0u) != F32)
    return; // (uniform: the other launch takes this job)
  const uint32_t lanes = J.h * J.vpr;
  if (blockIdx.x * DP_THREADS >= lanes)
    return; // (uniform)
  const uint32_t id = blockIdx.x * DP_THREADS + threadIdx.x;
  const bool active = id < lanes;
  const bool collect = !F32 && J.has_bad != 0u; // (uniform)
  if (collect && threadIdx.x == 0)
    wg_count = 0;
  uint32_t row = 0, s0 = 0, n = 0, touched = 0;
  uint32_t px[N];
  uint64_t hits[2] = {0, 0};
  uint8_t* p = nullptr;
  bool whole = false;
  if (active) {
    row = id / J.vpr;
    const uint32_t v = id - row * J.vpr;
    s0 = N * v;
    n = min(N, J.ws - s0);
    p = A.out_base + J.img_offset + uint64_t(row) * J.pitch + 16u * v;
    // (a job with nothing to do, in a plan whose grid another job sized)
    if (J.n_ops != 0u || J.lut_on != 0u) {
      whole = n == N && (reinterpret_cast<uintptr_t>(p) & 15u) == 0u;
      if (whole) {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
        if (F32) {
#pragma unroll
          for (uint32_t k = 0; k < 4; ++k)
            px[k] = w[k];
        } else {
#pragma unroll
          for (uint32_t k = 0; k < 4; ++k) {
            px[(2 * k) % N] = w[k] & 0xFFFFu;
            px[(2 * k + 1) % N] = w[k] >> 16;
          }
        }
      } else {
#pragma unroll
        for (uint32_t i = 0; i < N; ++i) {
          if (F32)
            px[i] = i < n ? reinterpret_cast<const uint32_t*>(p)[i] : 0u;
          else
            px[i] = i < n ? uint32_t(reinterpret_cast<const uint16_t*>(p)[i]) : 0u;
        }
      }
      touched = lane<F32>(J, A.ops, A.tables, A.deltas, A.luts, A.pw, row, s0, n, px, hits);
    }
  }
  if (touched != 0u) {
    if (whole) {
      if (F32)
        *reinterpret_cast<uint4*>(p) = make_uint4(px[0], px[1], px[2], px[3]);
      else
        *reinterpret_cast<uint4*>(p) =
            make_uint4(px[0] | px[1 % N] << 16, px[2 % N] | px[3 % N] << 16,
                       px[4 % N] | px[5 % N] << 16, px[6 % N] | px[7 % N] << 16);
    } else {
#pragma unroll
      for (uint32_t i = 0; i < N; ++i)
        if (i < n && (touched >> i & 1u)) {
          if (F32)
            reinterpret_cast<uint32_t*>(p)[i] = px[i];
          else
            reinterpret_cast<uint16_t*>(p)[i] = uint16_t(px[i]);
        }
    }
  }
  if (!collect)
    return;
  // the hits: a place in the workgroup's slice for every lane, one atomic on the job's counter
  // for a workgroup that met any
  __syncthreads();
  const uint32_t mine = uint32_t(__popcll(hits[0]) + __popcll(hits[1]));
  uint32_t at = 0;
  if (mine)
    at = atomicAdd(&wg_count, mine);
  __syncthreads();
  if (threadIdx.x == 0 && wg_count != 0u)
    wg_slice = atomicAdd(A.counts + J.job, (unsigned long long)wg_count);
  __syncthreads();
  if (!mine)
    return;
  uint64_t idx = wg_slice + at;
  uint64_t* list = A.hits + J.bad_base;
  for (uint32_t half = 0; half < 2; ++half) {
    uint64_t m = hits[half];
    while (m) {
      const uint32_t bit = uint32_t(__ffsll((long long)m)) - 1u;
      m &= m - 1u;
      const uint32_t o = half * 8u + (bit >> 3);
      const OpDev& op = A.ops[J.op0 + o];
      // (the counter goes on counting past the capacity; only entries inside it are stored)
      if (idx < J.bad_cap)
        list[idx] = hit_entry(o, row - op.y0, s0 + (bit & 7u) - op.x0);
      ++idx;
    }
  }
}

struct DpPlan final : DecoderPlan {
  rsx_ctx* ctx = nullptr;
  size_t n_jobs = 0;
  std::vector<Parsed> parsed;
  std::vector<JobDev> jobs;
  std::vector<unsigned long long> h_counts;
  std::vector<std::vector<uint32_t>> bad; // per job, composed by results()
  std::vector<uint8_t> overflow;          // the job's hits went past its capacity
  DeviceBuffer d_jobs, d_ops, d_tables, d_deltas, d_luts, d_pw, d_hits, d_counts;
  uint32_t max_blocks = 0;
  bool any_u16 = false, any_f32 = false, any_bad = false, have_results = false;
  int run(const void*, void* out_dev, hipStream_t s, KernelTimer* timer) override {
    have_results = false;
    if (max_blocks == 0)
      return RSX_OK; // (no job has anything to do)
    DpArgs A{};
    A.out_base = static_cast<uint8_t*>(out_dev);
    A.jobs = static_cast<const JobDev*>(d_jobs.ptr);
    A.ops = static_cast<const OpDev*>(d_ops.ptr);
    A.tables = static_cast<const uint16_t*>(d_tables.ptr);
    A.deltas = static_cast<const int32_t*>(d_deltas.ptr);
    A.luts = static_cast<const uint32_t*>(d_luts.ptr);
    A.pw = static_cast<const uint32_t*>(d_pw.ptr);
    A.hits = static_cast<uint64_t*>(d_hits.ptr);
    A.counts = static_cast<unsigned long long*>(d_counts.ptr);
    if (timer)
      timer->begin(s);
    if (any_bad)
      RSX_HIP_CHECK(ctx, hipMemsetAsync(d_counts.ptr, 0, n_jobs * sizeof(unsigned long long), s));
    if (any_u16)
      hipLaunchKernelGGL(dng_post_kernel<false>, dim3(max_blocks, uint32_t(n_jobs)),
                         dim3(DP_THREADS), 0, s, A);
    if (any_f32)
      hipLaunchKernelGGL(dng_post_kernel<true>, dim3(max_blocks, uint32_t(n_jobs)),
                         dim3(DP_THREADS), 0, s, A);
    if (timer)
      timer->mark("dng_post_kernel");
    RSX_HIP_CHECK(ctx, hipGetLastError());
    return RSX_OK;
  }
  int results(hipStream_t s, bool ran, int32_t* job_status, uint32_t* job_consumed) override {
    // (nothing in the pixels can fail, and a refused job fails the plan's creation; a hit list
    // past its capacity shows in bad_pixels(), the image is complete)
    if (job_consumed)
      std::fill(job_consumed, job_consumed + n_jobs, 0u);
    int rc = RSX_OK;
    std::fill(h_counts.begin(), h_counts.end(), 0ull);
    if (ran && any_bad && max_blocks != 0) {
      RSX_HIP_CHECK(ctx, hipMemcpyAsync(h_counts.data(), d_counts.ptr,
                                        n_jobs * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
      RSX_HIP_CHECK(ctx, hipStreamSynchronize(s));
    }
    for (size_t i = 0; i < n_jobs; ++i) {
      std::vector<uint64_t> hits;
      overflow[i] = h_counts[i] > jobs[i].bad_cap ? 1 : 0;
      if (ran && h_counts[i] != 0 && !overflow[i]) {
        hits.resize(size_t(h_counts[i]));
        RSX_HIP_CHECK(ctx, hipMemcpyAsync(hits.data(),
                                          static_cast<const uint64_t*>(d_hits.ptr) + jobs[i].bad_base,
                                          hits.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        RSX_HIP_CHECK(ctx, hipStreamSynchronize(s));
      }
      compose_bad(parsed[i], hits, &bad[i]);
      if (job_status)
        job_status[i] = overflow[i] ? int32_t(RSX_ERR_UNSUPPORTED) : int32_t(RSX_OK);
      if (overflow[i])
        rc = RSX_ERR_UNSUPPORTED;
    }
    have_results = ran;
    return rc;
  }
  int bad_pixels(int job, uint32_t* out, uint32_t cap, uint64_t* n_bad) override {
    if (n_bad)
      *n_bad = 0;
    if (job < 0 || size_t(job) >= n_jobs || !have_results)
      return RSX_ERR_INVALID_ARG;
    const uint64_t n = overflow[size_t(job)] ? fixed_count(parsed[size_t(job)]) + h_counts[size_t(job)]
                                             : bad[size_t(job)].size();
    if (n_bad)
      *n_bad = n;
    if (overflow[size_t(job)] || n > cap)
      return RSX_ERR_UNSUPPORTED;
    if (n)
      std::memcpy(out, bad[size_t(job)].data(), size_t(n) * sizeof(uint32_t));
    return RSX_OK;
  }
  int dng_post_result(int job, rsx_dng_post_result* out) override {
    if (job < 0 || size_t(job) >= n_jobs || !out)
      return RSX_ERR_INVALID_ARG;
    const Parsed& P = parsed[size_t(job)];
    fill_result(P, have_results ? (overflow[size_t(job)] ? fixed_count(P) + h_counts[size_t(job)]
                                                         : bad[size_t(job)].size())
                                : fixed_count(P),
                out);
    return RSX_OK;
  }
};

} // namespace

int dng_post_validate(const rsx_dng_post_desc* desc, const rsx_image* img,
                      rsx_dng_post_result* result, uint32_t* bad, uint32_t bad_cap) {
  if (!bad && bad_cap != 0)
    return RSX_ERR_INVALID_ARG;
  return rsx_dngpost::validate(desc, img, result, bad, bad_cap);
}

int dng_post_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_dng_post_job* jobs,
                         std::unique_ptr<DecoderPlan>* out) {
  if (n_jobs > 65535)
    return RSX_ERR_UNSUPPORTED; // (a grid's second dimension)
  auto p = std::make_unique<DpPlan>();
  p->ctx = ctx;
  p->n_jobs = size_t(n_jobs);
  p->parsed.resize(size_t(n_jobs));
  p->jobs.resize(size_t(n_jobs));
  p->h_counts.assign(size_t(n_jobs), 0ull);
  p->bad.resize(size_t(n_jobs));
  p->overflow.assign(size_t(n_jobs), 0);
  std::vector<OpDev> ops;
  std::vector<uint16_t> tables;
  std::vector<int32_t> deltas;
  std::vector<uint32_t> luts;
  uint64_t hit_entries = 0;
  uint32_t max_vpr = 1;
  for (int i = 0; i < n_jobs; ++i) {
    const rsx_dng_post_job& j = jobs[i];
    Parsed& P = p->parsed[size_t(i)];
    if (int st = parse(&j.desc, &j.img, &P))
      return st;
    const uint64_t bpc = j.desc.is_f32 ? 4u : 2u;
    if (j.img_offset % bpc != 0)
      return RSX_ERR_INVALID_ARG;
    JobDev& J = p->jobs[size_t(i)];
    fill_job(&j.desc, &j.img, P, &J);
    J.img_offset = j.img_offset;
    J.job = uint32_t(i);
    const uint64_t lanes = uint64_t(J.h) * J.vpr;
    if (lanes >= (1ull << 31))
      return RSX_ERR_UNSUPPORTED; // (lane numbers are 32-bit on the device)
    if (tables.size() + P.tables.size() >= (1ull << 32) || luts.size() + 65536ull >= (1ull << 32) ||
        deltas.size() + P.deltas.size() >= (1ull << 32))
      return RSX_ERR_UNSUPPORTED;
    J.op0 = uint32_t(ops.size());
    for (OpDev op : P.ops) {
      op.data_off += uint32_t(op.kind == OP_TABLE ? tables.size() : deltas.size());
      ops.push_back(op);
    }
    tables.insert(tables.end(), P.tables.begin(), P.tables.end());
    deltas.insert(deltas.end(), P.deltas.begin(), P.deltas.end());
    if (J.lut_on) {
      J.lut_off = uint32_t(luts.size());
      luts.insert(luts.end(), P.lut.begin(), P.lut.end());
      max_vpr = std::max(max_vpr, J.vpr);
    }
    if (J.has_bad) {
      uint64_t n_const = 0;
      for (const OpDev& op : P.ops)
        n_const += op.kind == OP_BAD_CONSTANT ? uint64_t(op.y1 - op.y0) * (op.x1 - op.x0) : 0u;
      J.bad_cap = uint32_t(std::min<uint64_t>(j.bad_cap, n_const));
      J.bad_base = hit_entries;
      hit_entries += J.bad_cap;
      p->any_bad = true;
    }
    if (J.n_ops != 0 || J.lut_on) {
      p->max_blocks = std::max(p->max_blocks, uint32_t((lanes + DP_THREADS - 1) / DP_THREADS));
      (J.is_f32 ? p->any_f32 : p->any_u16) = true;
    }
  }
  if (ops.size() > (1u << 20))
    return RSX_ERR_UNSUPPORTED;
  const std::vector<uint32_t> pw = dither_powers8(max_vpr);
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int st;
  if ((st = upload(ctx, p->d_jobs, p->jobs)) || (st = upload(ctx, p->d_ops, ops)) ||
      (st = upload(ctx, p->d_tables, tables)) || (st = upload(ctx, p->d_deltas, deltas)) ||
      (st = upload(ctx, p->d_luts, luts)) || (st = upload(ctx, p->d_pw, pw)) ||
      (st = p->d_hits.ensure(size_t(hit_entries) * 8 + 16)) ||
      (st = p->d_counts.ensure(p->jobs.size() * sizeof(unsigned long long) + 16)))
    return st;
  *out = std::move(p);
  return RSX_OK;
}

} // namespace rsx
