// RafDecoder::applyCorrections' 45 degree rotation on gfx950: include/rsx.h section 3y, DESIGN.md
// 4.23.
//
// The reference clears the rotated image and scatters the crop into it.  The map is a restriction
// of a bijection of the integer plane (rsx_fuji_rotate_core.h), so the device GATHERS: ONE launch
// over all jobs of a plan writes every sample of every R x (R - 1) image, the moved pixels and the
// zero corners alike, and there is no clear in front of it.  A workgroup takes a tile of FR_TW x
// FR_TH destination samples, a lane FR_LANE adjacent samples of one row, stored as 16 bytes where
// the address allows.
//
// Along a destination row the source walks a diagonal (normal layout: one source row per sample;
// alt: one per two samples), so a lane's loads land on different source rows.  Two kernels:
//
// fuji_rotate_kernel      the direct gather: every sample is one 2-byte load from the source.  A
//                         tile's loads fall into a diamond of about FR_TW + FR_TH source rows, which
//                         the tile's own rows share out of the cache.
// fuji_rotate_lds_kernel  the tile's source bounding box (the diamond's: at most 95 x 49 samples in
//                         either layout) goes into LDS by rows, 32 lanes along a source row, out of
//                         the crop as zeros; the gather then reads LDS and needs no bounds check.
//
// RSX_FUJI_ROTATE_KERNEL=direct|lds picks one at plan creation, for comparison; DESIGN.md 4.23 has
// what each costs and why the default is what it is.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "rsx_fuji_rotate.h"
#include "rsx_fuji_rotate_core.h"
#include "rsx_ljpeg_dev.h"
#include "rsx_plan_host.h"

namespace rsx {

using namespace rsx_fujirot;

namespace {

constexpr int FR_THREADS = 256;
constexpr int FR_LANE = 8;                      // samples a lane stores: 16 bytes
constexpr int FR_TW = 64, FR_TH = 32;           // the tile: 8 lanes across, 32 rows
constexpr int FR_LDS = 96 * 50;                 // samples of the largest bounding box, with slack
static_assert((FR_TW / FR_LANE) * FR_TH == FR_THREADS, "one lane per 8 samples of the tile");
static_assert((FR_TW + FR_TH - 1) * ((FR_TW + FR_TH) / 2 + 2) <= FR_LDS, "the diamond's box");

struct FrJobDev {
  uint64_t in_off, out_off;
  uint32_t src_pitch, dst_pitch;
  int32_t cx, cy, W, H, alt, R;
  uint32_t tiles_x, tiles; // tiles across, tiles in all
};

struct FrArgs {
  const uint8_t* in_base;
  uint8_t* out_base;
  const FrJobDev* jobs;
};

// v[0 .. 8) to the samples [w0, w0 + 8) of a row that has R: 16 bytes at once where they are all
// there and the address is on the grid
__device__ __forceinline__ void fr_store(uint8_t* row, int32_t w0, int32_t R, const uint16_t* v) {
  uint8_t* p = row + 2u * uint32_t(w0);
  if (w0 + FR_LANE <= R && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
    uint4 q;
    q.x = uint32_t(v[0]) | uint32_t(v[1]) << 16;
    q.y = uint32_t(v[2]) | uint32_t(v[3]) << 16;
    q.z = uint32_t(v[4]) | uint32_t(v[5]) << 16;
    q.w = uint32_t(v[6]) | uint32_t(v[7]) << 16;
    *reinterpret_cast<uint4*>(p) = q;
    return;
  }
#pragma unroll
  for (int k = 0; k < FR_LANE; ++k)
    if (w0 + k < R)
      reinterpret_cast<uint16_t*>(p)[k] = v[k];
}

__global__ __launch_bounds__(FR_THREADS) void fuji_rotate_kernel(FrArgs A) {
  const FrJobDev& J = A.jobs[blockIdx.y];
  if (blockIdx.x >= J.tiles)
    return;
  const int32_t w0 = int32_t(blockIdx.x % J.tiles_x) * FR_TW + FR_LANE * int32_t(threadIdx.x & 7u);
  const int32_t h = int32_t(blockIdx.x / J.tiles_x) * FR_TH + int32_t(threadIdx.x >> 3);
  if (h >= J.R - 1 || w0 >= J.R)
    return;
  const uint8_t* src = A.in_base + J.in_off;
  uint16_t v[FR_LANE];
#pragma unroll
  for (int k = 0; k < FR_LANE; ++k)
    v[k] = gather(src, J.src_pitch, J.cx, J.cy, J.W, J.H, J.alt, h, w0 + k);
  fr_store(A.out_base + J.out_off + uint64_t(h) * J.dst_pitch, w0, J.R, v);
}

__global__ __launch_bounds__(FR_THREADS) void fuji_rotate_lds_kernel(FrArgs A) {
  __shared__ uint16_t box[FR_LDS];
  const FrJobDev& J = A.jobs[blockIdx.y];
  if (blockIdx.x >= J.tiles)
    return;
  const int32_t tw0 = int32_t(blockIdx.x % J.tiles_x) * FR_TW;
  const int32_t th0 = int32_t(blockIdx.x / J.tiles_x) * FR_TH;
  // x grows with w and falls with h; y grows with both, in either layout
  int32_t x0, x1, y0, y1, t;
  inverse(J.W, J.alt, th0 + FR_TH - 1, tw0, &x0, &t);
  inverse(J.W, J.alt, th0, tw0 + FR_TW - 1, &x1, &t);
  inverse(J.W, J.alt, th0, tw0, &t, &y0);
  inverse(J.W, J.alt, th0 + FR_TH - 1, tw0 + FR_TW - 1, &t, &y1);
  const int32_t bw = x1 - x0 + 1, bh = y1 - y0 + 1;
  const bool fits = bw * bh <= FR_LDS; // (always: the static_assert above)
  const uint8_t* src = A.in_base + J.in_off;
  if (fits) {
    const int32_t g = int32_t(threadIdx.x >> 5), l = int32_t(threadIdx.x & 31u);
    for (int32_t r = g; r < bh; r += FR_THREADS / 32) {
      const int32_t y = y0 + r;
      const bool row_in = y >= 0 && y < J.H;
      const uint8_t* srow = src + uint64_t(row_in ? J.cy + y : 0) * J.src_pitch;
      for (int32_t c = l; c < bw; c += 32) {
        const int32_t x = x0 + c;
        uint16_t v = 0;
        if (row_in && x >= 0 && x < J.W)
          v = reinterpret_cast<const uint16_t*>(srow)[J.cx + x];
        box[r * bw + c] = v;
      }
    }
  }
  __syncthreads();
  const int32_t w0 = tw0 + FR_LANE * int32_t(threadIdx.x & 7u);
  const int32_t h = th0 + int32_t(threadIdx.x >> 3);
  if (h >= J.R - 1 || w0 >= J.R)
    return;
  uint16_t v[FR_LANE];
#pragma unroll
  for (int k = 0; k < FR_LANE; ++k) {
    if (fits) {
      int32_t x, y;
      inverse(J.W, J.alt, h, w0 + k, &x, &y);
      v[k] = box[(y - y0) * bw + (x - x0)];
    } else {
      v[k] = gather(src, J.src_pitch, J.cx, J.cy, J.W, J.H, J.alt, h, w0 + k);
    }
  }
  fr_store(A.out_base + J.out_off + uint64_t(h) * J.dst_pitch, w0, J.R, v);
}

struct FujiRotatePlan final : DecoderPlan {
  rsx_ctx* ctx = nullptr;
  std::vector<int32_t> host; // validation result per job
  std::vector<FrJobDev> jobs; // the jobs that go to the device
  DeviceBuffer d_jobs;
  uint32_t max_tiles = 0;
  bool lds = false;
  int run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) override;
  int results(hipStream_t, bool, int32_t* job_status, uint32_t* job_consumed) override {
    if (job_consumed)
      std::fill(job_consumed, job_consumed + host.size(), 0u);
    return fold_jobs(host.size(), FoldOrder::LAST_FAILING, job_status,
                     [&](size_t i) { return int(host[i]); });
  }
};

} // namespace

int fuji_rotate_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_raf_rotate_job* jobs,
                            std::unique_ptr<DecoderPlan>* out) {
  auto p = std::make_unique<FujiRotatePlan>();
  p->ctx = ctx;
  p->host.assign(n_jobs, RSX_OK);
  const char* which = getenv("RSX_FUJI_ROTATE_KERNEL");
  p->lds = which && std::strcmp(which, "lds") == 0;
  for (int i = 0; i < n_jobs; ++i) {
    const rsx_raf_rotate_job& j = jobs[i];
    rsx_image src = j.in, dst = j.img;
    src.data = dst.data = nullptr; // (.data ignored: the overlap is the caller's to avoid)
    int st = validate(&j.desc, &src, &dst);
    if (st == RSX_OK && (j.in_offset % 2 != 0 || j.img_offset % 2 != 0))
      st = RSX_ERR_INVALID_ARG;
    p->host[i] = st;
    if (st != RSX_OK)
      continue;
    FrJobDev D;
    std::memset(&D, 0, sizeof D);
    D.in_off = j.in_offset;
    D.out_off = j.img_offset;
    D.src_pitch = src.pitch_bytes;
    D.dst_pitch = dst.pitch_bytes;
    D.cx = j.desc.crop_x;
    D.cy = j.desc.crop_y;
    D.W = j.desc.size_x;
    D.H = j.desc.size_y;
    D.alt = j.desc.alt_layout ? 1 : 0;
    D.R = dst.dim_x;
    D.tiles_x = uint32_t(D.R + FR_TW - 1) / FR_TW;
    D.tiles = D.tiles_x * (uint32_t(D.R - 1 + FR_TH - 1) / FR_TH); // (at most 1024 x 2048)
    p->max_tiles = std::max(p->max_tiles, D.tiles);
    p->jobs.push_back(D);
  }
  if (p->jobs.size() > 65535u)
    return RSX_ERR_UNSUPPORTED; // (a job is a row of the launch's grid)
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (int st = upload(ctx, p->d_jobs, p->jobs))
    return st;
  *out = std::move(p);
  return RSX_OK;
}

int FujiRotatePlan::run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) {
  if (jobs.empty())
    return RSX_OK; // (every job was refused by the host)
  FrArgs A{};
  A.in_base = static_cast<const uint8_t*>(in_dev);
  A.out_base = static_cast<uint8_t*>(out_dev);
  A.jobs = static_cast<const FrJobDev*>(d_jobs.ptr);
  if (timer)
    timer->begin(s);
  const dim3 grid(max_tiles, uint32_t(jobs.size())), block(FR_THREADS);
  if (lds) {
    hipLaunchKernelGGL(fuji_rotate_lds_kernel, grid, block, 0, s, A);
    if (timer)
      timer->mark("fuji_rotate_lds_kernel");
  } else {
    hipLaunchKernelGGL(fuji_rotate_kernel, grid, block, 0, s, A);
    if (timer)
      timer->mark("fuji_rotate_kernel");
  }
  RSX_HIP_CHECK(ctx, hipGetLastError());
  return RSX_OK;
}

} // namespace rsx
