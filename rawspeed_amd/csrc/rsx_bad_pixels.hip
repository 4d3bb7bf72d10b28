// RawImageData::fixBadPixels on the device (include/rsx.h section 5).
//
// What the reference does (common/RawImage.cpp:211-323): one thread ORs the positions into a bit
// map, then row bands of the map are scanned in blocks of 32 pixels and every marked pixel walks,
// one pixel at a time, to the nearest unmarked pixel in four directions -- a dark RW2 frame or a
// DNG whose masked border equals the FixBadPixelsConstant value costs the pixel count times the
// extent of the bad region.  The stage reads only unmarked pixels and writes only marked ones, so
// every marked pixel is independent of every other.  The arithmetic and the word-wise search are
// rsx_bad_pixels_core.h, shared with the host build.
//
//   bp_init_kernel     one lane per 64-bit word of a job's ROW MAP (the reference's map, byte for
//                      byte): the word of map_in, or 0; the job's counters and flag are reset.
//                      Plain stores on the launch stream -- no memset is trusted to have run.
//   bp_zero_kernel     jobs whose bad pixels are the zero pixels of the image (Panasonic V4): a
//                      wavefront reads 64 pixels of a row, one per lane, and its ballot is the word.
//   bp_mark_kernel     one lane per position: one atomicOr on the row map; a position outside the
//                      image raises the job's flag, which makes the two kernels behind no-ops.
//   bp_columns_kernel  the COLUMN MAP by bit-matrix transpose: a wavefront owns 64 columns and 64
//                      rows, reads the 64 row-map words, one per lane, and for every row that
//                      holds a bit (a ballot) the word is broadcast and each lane takes the bit
//                      of its column into the word it stores; a clear block costs one load a
//                      lane.  The set bits are counted on the way (n_bad).  The map holds no duplicates and
//                      the caller's earlier bits, which a second atomicOr per position would not.
//   bp_fix_kernel      walks the row map, not the list: a wavefront loads 64 consecutive words,
//                      one per lane, and for every word with a bit set (a ballot) the word is
//                      broadcast and lane t takes bit t -- a dense word is fixed by 64 lanes, a
//                      clear stretch costs one load.  The scan's rule (pixels below fix_end only)
//                      is a mask on the word.  Every store is a plain vector store of one sample.
// No LDS, no scratch (tests/test_bad_pixels_build.py holds the numbers).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "rsx_internal.h"
#include "rsx_ljpeg_dev.h"
#include "rsx_plan_host.h"
#include "rsx_bad_pixels.h"
#include "rsx_bad_pixels_core.h"

namespace rsx {

namespace {

using namespace rsx_bp;

constexpr uint32_t BP_THREADS = 256, BP_WAVES = BP_THREADS / 64, BP_ZERO_WORDS = 8;

struct JobDev {
  uint64_t img_offset;
  uint64_t in_offset;
  uint64_t row_off;   // the job's row map: word index into the plan's maps
  uint64_t col_off;   // the job's column map
  uint64_t mapin_off; // the job's map_in: word index into the plan's copies (has_map_in)
  uint32_t n_positions;
  uint32_t n_words;   // h * wpr
  uint32_t has_map_in;
  uint32_t mark_zero;
  uint32_t active;    // the reference would make a map
  uint32_t reserved;
  Geo g;
};

struct JobOut {
  unsigned long long n_bad, n_fixed;
  uint32_t flag; // a position outside the image
  uint32_t reserved;
};

struct BpArgs {
  const uint8_t* in_base;
  uint8_t* out_base;
  const JobDev* jobs;
  JobOut* outs;
  uint64_t* maps;
  const uint64_t* mapin;
};

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    v += __shfl_xor(v, o, 64);
  return v;
}

__global__ void __launch_bounds__(BP_THREADS) bp_init_kernel(BpArgs A) {
  const JobDev& J = A.jobs[blockIdx.y];
  const uint32_t id = blockIdx.x * BP_THREADS + threadIdx.x;
  if (id == 0u) {
    JobOut& o = A.outs[blockIdx.y];
    o.n_bad = 0ull;
    o.n_fixed = 0ull;
    o.flag = 0u;
    o.reserved = 0u;
  }
  if (!J.active || J.mark_zero || id >= J.n_words)
    return;
  A.maps[J.row_off + id] = J.has_map_in ? A.mapin[J.mapin_off + id] : 0ull;
}

__global__ void __launch_bounds__(BP_THREADS) bp_zero_kernel(BpArgs A) {
  const JobDev& J = A.jobs[blockIdx.y];
  if (!J.mark_zero)
    return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t first = (blockIdx.x * BP_WAVES + (threadIdx.x >> 6)) * BP_ZERO_WORDS;
  const uint8_t* img = A.out_base + J.img_offset;
  for (uint32_t k = 0; k < BP_ZERO_WORDS; ++k) {
    const uint32_t wi = first + k;
    if (wi >= J.n_words)
      return; // (the same for every lane of the wavefront)
    const uint32_t y = wi / J.g.wpr, x = (wi - y * J.g.wpr) * 64u + lane;
    bool zero = false;
    if (x < J.g.w)
      zero = *reinterpret_cast<const uint16_t*>(img + size_t(y) * J.g.pitch + 2u * size_t(x)) == 0u;
    const uint64_t word = __ballot(zero);
    if (lane == 0u)
      A.maps[J.row_off + wi] = word;
  }
}

__global__ void __launch_bounds__(BP_THREADS) bp_mark_kernel(BpArgs A) {
  const JobDev& J = A.jobs[blockIdx.y];
  const uint32_t id = blockIdx.x * BP_THREADS + threadIdx.x;
  if (id >= J.n_positions)
    return;
  const uint32_t p = reinterpret_cast<const uint32_t*>(A.in_base + J.in_offset)[id];
  const uint32_t x = p & 0xFFFFu, y = p >> 16;
  if (x >= J.g.w || y >= J.g.h) {
    atomicOr(&A.outs[blockIdx.y].flag, 1u);
    return;
  }
  atomicOr(reinterpret_cast<unsigned long long*>(A.maps + J.row_off + size_t(y) * J.g.wpr + (x >> 6)),
           1ull << (x & 63u));
}

// grid (ceil(w / 64), wpc, job), one wavefront a workgroup
__global__ void __launch_bounds__(64) bp_columns_kernel(BpArgs A) {
  const JobDev& J = A.jobs[blockIdx.z];
  const uint32_t xw = blockIdx.x, yw = blockIdx.y, t = threadIdx.x;
  if (!J.active || xw * 64u >= J.g.w || yw >= J.g.wpc || A.outs[blockIdx.z].flag != 0u)
    return;
  const uint32_t x = xw * 64u + t;
  // column_word() with the rows spread over the lanes: lane t loads the word of row 64 yw + t, and
  // only the rows that hold a bit (a ballot) are broadcast and looked at
  const uint32_t y = yw * 64u + t;
  const uint64_t mine = y < J.g.h ? A.maps[J.row_off + size_t(y) * J.g.wpr + xw] : 0ull;
  uint64_t live = __ballot(mine != 0ull);
  uint64_t word = 0ull;
  while (live) {
    const uint32_t r = uint32_t(ctz64(live));
    live &= live - 1ull;
    word |= (__shfl(mine, int(r), 64) >> t & 1ull) << r;
  }
  if (x >= J.g.w)
    word = 0ull;
  else
    A.maps[J.col_off + size_t(x) * J.g.wpc + yw] = word;
  const uint32_t n = wave_sum(uint32_t(popc64(word)));
  if (t == 0u && n != 0u)
    atomicAdd(&A.outs[blockIdx.z].n_bad, (unsigned long long)n);
}

template <bool F32>
__global__ void __launch_bounds__(BP_THREADS) bp_fix_kernel(BpArgs A) {
  const JobDev& J = A.jobs[blockIdx.y];
  if (!J.active || (J.g.is_f32 != 0u) != F32 || A.outs[blockIdx.y].flag != 0u)
    return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t first = (blockIdx.x * BP_WAVES + (threadIdx.x >> 6)) * 64u;
  if (first >= J.n_words)
    return;
  const Geo g = J.g;
  const uint64_t* rowmap = A.maps + J.row_off;
  const uint64_t* colmap = A.maps + J.col_off;
  uint8_t* img = A.out_base + J.img_offset;
  const uint32_t end = min(g.fix_end, g.w);
  uint64_t mine = 0;
  {
    const uint32_t wi = first + lane;
    if (wi < J.n_words) {
      const uint32_t x0 = (wi % g.wpr) * 64u;
      mine = rowmap[wi];
      if (x0 >= end)
        mine = 0ull;
      else if (end - x0 < 64u)
        mine &= (1ull << (end - x0)) - 1ull;
    }
  }
  uint64_t live = __ballot(mine != 0ull);
  uint32_t fixed = 0;
  while (live) {
    const uint32_t src = uint32_t(ctz64(live));
    live &= live - 1ull;
    const uint64_t word = __shfl(mine, int(src), 64);
    if (word >> lane & 1ull) {
      const uint32_t wi = first + src, y = wi / g.wpr, x = (wi - y * g.wpr) * 64u + lane;
      ++fixed;
      if (F32)
        *reinterpret_cast<uint32_t*>(img + size_t(y) * g.pitch + 4u * size_t(x)) =
            fix_f32(g, rowmap, colmap, img, x, y);
      else
        *reinterpret_cast<uint16_t*>(img + size_t(y) * g.pitch + 2u * size_t(x)) =
            fix_u16(g, rowmap, colmap, img, x, y);
    }
  }
  const uint32_t n = wave_sum(fixed);
  if (lane == 0u && n != 0u)
    atomicAdd(&A.outs[blockIdx.y].n_fixed, (unsigned long long)n);
}

struct BpPlan final : DecoderPlan {
  rsx_ctx* ctx = nullptr;
  size_t n_jobs = 0;
  std::vector<JobDev> jobs;
  std::vector<JobOut> h_out;
  DeviceBuffer d_jobs, d_outs, d_maps, d_mapin;
  uint32_t word_blocks = 0, zero_blocks = 0, mark_blocks = 0, fix_blocks = 0, col_x = 0, col_y = 0;
  bool any_u16 = false, any_f32 = false, have_results = false;
  int run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) override {
    have_results = false;
    BpArgs A{};
    A.in_base = static_cast<const uint8_t*>(in_dev);
    A.out_base = static_cast<uint8_t*>(out_dev);
    A.jobs = static_cast<const JobDev*>(d_jobs.ptr);
    A.outs = static_cast<JobOut*>(d_outs.ptr);
    A.maps = static_cast<uint64_t*>(d_maps.ptr);
    A.mapin = static_cast<const uint64_t*>(d_mapin.ptr);
    if (mark_blocks != 0 && !in_dev)
      return RSX_ERR_INVALID_ARG;
    const uint32_t nj = uint32_t(n_jobs);
    if (timer)
      timer->begin(s);
    hipLaunchKernelGGL(bp_init_kernel, dim3(std::max(word_blocks, 1u), nj), dim3(BP_THREADS), 0, s, A);
    if (timer)
      timer->mark("bp_init_kernel");
    if (zero_blocks) {
      hipLaunchKernelGGL(bp_zero_kernel, dim3(zero_blocks, nj), dim3(BP_THREADS), 0, s, A);
      if (timer)
        timer->mark("bp_zero_kernel");
    }
    if (mark_blocks) {
      hipLaunchKernelGGL(bp_mark_kernel, dim3(mark_blocks, nj), dim3(BP_THREADS), 0, s, A);
      if (timer)
        timer->mark("bp_mark_kernel");
    }
    if (fix_blocks) {
      hipLaunchKernelGGL(bp_columns_kernel, dim3(col_x, col_y, nj), dim3(64), 0, s, A);
      if (timer)
        timer->mark("bp_columns_kernel");
      if (any_u16)
        hipLaunchKernelGGL(bp_fix_kernel<false>, dim3(fix_blocks, nj), dim3(BP_THREADS), 0, s, A);
      if (any_f32)
        hipLaunchKernelGGL(bp_fix_kernel<true>, dim3(fix_blocks, nj), dim3(BP_THREADS), 0, s, A);
      if (timer)
        timer->mark("bp_fix_kernel");
    }
    RSX_HIP_CHECK(ctx, hipGetLastError());
    return RSX_OK;
  }
  int results(hipStream_t s, bool ran, int32_t* job_status, uint32_t* job_consumed) override {
    if (job_consumed)
      std::fill(job_consumed, job_consumed + n_jobs, 0u);
    std::memset(h_out.data(), 0, h_out.size() * sizeof(JobOut));
    if (ran) {
      RSX_HIP_CHECK(ctx, hipMemcpyAsync(h_out.data(), d_outs.ptr, n_jobs * sizeof(JobOut),
                                        hipMemcpyDeviceToHost, s));
      RSX_HIP_CHECK(ctx, hipStreamSynchronize(s));
    }
    have_results = ran;
    return fold_jobs(n_jobs, FoldOrder::LAST_FAILING, job_status, [&](size_t i) {
      return h_out[i].flag ? int(RSX_ERR_INVALID_ARG) : int(RSX_OK);
    });
  }
  int bad_pixels_result(int job, rsx_bad_pixels_result* out) override {
    if (job < 0 || size_t(job) >= n_jobs || !out || !have_results)
      return RSX_ERR_INVALID_ARG;
    std::memset(out, 0, sizeof *out);
    const JobOut& o = h_out[size_t(job)];
    if (o.flag)
      return RSX_OK;
    out->n_bad = o.n_bad;
    out->n_fixed = o.n_fixed;
    out->map_made = jobs[size_t(job)].active ? 1 : 0;
    return RSX_OK;
  }
  int bad_pixels_map(int job, uint8_t* out, hipStream_t s) override {
    if (job < 0 || size_t(job) >= n_jobs || !out || !jobs[size_t(job)].active)
      return RSX_ERR_INVALID_ARG;
    const JobDev& J = jobs[size_t(job)];
    RSX_HIP_CHECK(ctx, hipMemcpyAsync(out, static_cast<const uint64_t*>(d_maps.ptr) + J.row_off,
                                      size_t(J.n_words) * 8u, hipMemcpyDeviceToHost, s));
    RSX_HIP_CHECK(ctx, hipStreamSynchronize(s));
    return RSX_OK;
  }
};

int plan_create(rsx_ctx* ctx, int n_jobs, const rsx_bad_pixels_job* jobs, bool mark_zero,
                std::unique_ptr<DecoderPlan>* out) {
  if (n_jobs > 65535)
    return RSX_ERR_UNSUPPORTED; // (a grid's second dimension)
  auto p = std::make_unique<BpPlan>();
  p->ctx = ctx;
  p->n_jobs = size_t(n_jobs);
  p->jobs.resize(size_t(n_jobs));
  p->h_out.resize(size_t(n_jobs));
  uint64_t map_words = 0, mapin_words = 0;
  std::vector<const uint8_t*> mapins;
  for (int i = 0; i < n_jobs; ++i) {
    const rsx_bad_pixels_job& j = jobs[i];
    const bool f32 = j.is_f32 != 0;
    if (int st = validate_image(&j.img, f32))
      return st;
    if (mark_zero && f32)
      return RSX_ERR_INVALID_ARG;
    const uint32_t w = uint32_t(j.img.dim_x), h = uint32_t(j.img.dim_y);
    if (j.map_in || j.map_pitch != 0) {
      if (j.map_pitch != map_pitch(w))
        return RSX_ERR_INVALID_ARG;
      if (j.map_in)
        if (int st = validate_map(j.map_in, j.map_pitch, w, h))
          return st;
    }
    if (j.img_offset % (f32 ? 4u : 2u) != 0 || j.in_offset % 4u != 0)
      return RSX_ERR_INVALID_ARG;
    JobDev& J = p->jobs[size_t(i)];
    std::memset(&J, 0, sizeof J);
    J.g = make_geo(w, h, j.img.pitch_bytes, j.img.is_cfa != 0, f32);
    J.img_offset = j.img_offset;
    J.in_offset = j.in_offset;
    J.n_positions = j.n_positions;
    J.n_words = h * J.g.wpr;
    J.has_map_in = j.map_in ? 1u : 0u;
    J.mark_zero = mark_zero ? 1u : 0u;
    J.active = (j.n_positions != 0 || j.map_in || mark_zero) ? 1u : 0u;
    mapins.push_back(j.map_in);
    if (!J.active)
      continue;
    J.row_off = map_words;
    map_words += J.n_words;
    J.col_off = map_words;
    map_words += uint64_t(w) * J.g.wpc;
    if (J.has_map_in) {
      J.mapin_off = mapin_words;
      mapin_words += J.n_words;
    }
    p->word_blocks = std::max(p->word_blocks, (J.n_words + BP_THREADS - 1) / BP_THREADS);
    if (mark_zero) {
      const uint32_t per = BP_WAVES * BP_ZERO_WORDS;
      p->zero_blocks = std::max(p->zero_blocks, (J.n_words + per - 1) / per);
    }
    if (J.n_positions)
      p->mark_blocks = std::max(p->mark_blocks, (J.n_positions - 1u) / BP_THREADS + 1u);
    p->fix_blocks = std::max(p->fix_blocks, (J.n_words + BP_THREADS - 1) / BP_THREADS);
    p->col_x = std::max(p->col_x, (w + 63u) / 64u);
    p->col_y = std::max(p->col_y, J.g.wpc);
    (f32 ? p->any_f32 : p->any_u16) = true;
  }
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int st;
  if ((st = upload(ctx, p->d_jobs, p->jobs)) ||
      (st = p->d_outs.ensure(p->jobs.size() * sizeof(JobOut) + 16)) ||
      (st = p->d_maps.ensure(size_t(map_words) * 8 + 16)) ||
      (st = p->d_mapin.ensure(size_t(mapin_words) * 8 + 16)))
    return st;
  for (size_t i = 0; i < p->jobs.size(); ++i)
    if (p->jobs[i].has_map_in && p->jobs[i].active)
      RSX_HIP_CHECK(ctx, hipMemcpy(static_cast<uint64_t*>(p->d_mapin.ptr) + p->jobs[i].mapin_off,
                                   mapins[i], size_t(p->jobs[i].n_words) * 8u, hipMemcpyHostToDevice));
  *out = std::move(p);
  return RSX_OK;
}

} // namespace

int bad_pixels_validate(const rsx_bad_pixels_desc* desc, const rsx_image* img) {
  return rsx_bp::validate(desc, img);
}

int bad_pixels_validate_image(const rsx_image* img, bool is_f32) {
  return rsx_bp::validate_image(img, is_f32);
}

uint32_t bad_pixels_map_pitch(uint32_t dim_x) { return rsx_bp::map_pitch(dim_x); }

int bad_pixels_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_bad_pixels_job* jobs,
                           std::unique_ptr<DecoderPlan>* out) {
  return plan_create(ctx, n_jobs, jobs, false, out);
}

int bad_pixels_zero_plan_create(rsx_ctx* ctx, const rsx_image* img,
                                std::unique_ptr<DecoderPlan>* out) {
  rsx_bad_pixels_job job;
  std::memset(&job, 0, sizeof job);
  job.img = *img;
  job.img.data = nullptr;
  return plan_create(ctx, 1, &job, true, out);
}

} // namespace rsx
