// rsx_fpwrite_deflate.hip -- deflate tiles of F32 DNGs for gfx950 (compression 8; include/rsx.h
// section 7d): the inverse of rsx_dng_deflate.hip.  Everything a stream holds is
// computed by rsx_deflate_core.h, the same statements the host build runs, so the device stream is
// the host stream byte for byte and the same from run to run; nothing depends on the order in
// which lanes finish.  Four launches a run, all tiles of the plan in each:
//   planes  a lane a byte: the narrow sample's byte plane with the forward predictor applied, into
//           the plan's plane scratch; a lane that meets an inexact sample ORs the tile's flag.
//   block   a lane a block of RSX_FPWRITE_BLOCK bytes: the greedy parse, the block's tables and the
//           dynamic form from bit 0 of the block's own scratch, and the Adler partial sums.
//   scan    a lane a tile: stored or dynamic for every block, the blocks' bit positions, Adler-32,
//           the stream's length and the tile's verdict.
//   emit    a lane a byte of the stream: gathered from the blocks' scratch (or, for a stored block,
//           from the planes) at its bit position; every byte is written once, whole, so no scratch
//           needs clearing and no word is shared between lanes.
// The block kernel is the long one and runs one lane a block: the parse and the tree are serial as
// written; the cut into blocks is where its parallelism comes from.
#include <hip/hip_runtime.h>

#include <memory>
#include <vector>

#include "rsx_deflate_core.h"
#include "rsx_fpwrite.h"
#include "rsx_ljpeg_dev.h"
#include "rsx_plan_host.h"

namespace rsx {

using namespace rsx_deflate;

namespace {

constexpr int EMIT_THREADS = 256;
constexpr int BLOCK_THREADS = 64;

struct DflArgs {
  const uint8_t* in_base;
  uint8_t* out_base;
  const TileGeom* tiles;
  const uint32_t* group_starts; // first_group of every tile, and the total behind them
  const uint32_t* block_starts; // first_block of every tile, and the total behind them
  uint8_t* planes;
  BlockWork* works;
  BlockInfo* info;
  TileInfo* tinfo;
  uint32_t* flags; // bit 0: the tile holds an inexact sample
  uint32_t n_tiles;
  uint32_t n_blocks;
};

__device__ __forceinline__ uint32_t last_not_above(const uint32_t* starts, uint32_t n, uint32_t v) {
  uint32_t lo = 0, hi = n - 1u;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1u) >> 1;
    if (starts[mid] <= v)
      lo = mid;
    else
      hi = mid - 1u;
  }
  return lo;
}

__global__ __launch_bounds__(EMIT_THREADS) void fpwrite_deflate_planes_kernel(DflArgs A) {
  const uint32_t t = last_not_above(A.group_starts, A.n_tiles, blockIdx.x);
  const TileGeom g = A.tiles[t];
  const uint64_t i = uint64_t(blockIdx.x - g.first_group) * EMIT_THREADS + threadIdx.x;
  if (i >= g.n_bytes)
    return;
  bool inexact = false;
  A.planes[g.plane_off + i] = plane_byte(A.in_base, g, uint32_t(i), &inexact);
  if (inexact)
    atomicOr(&A.flags[t], 1u);
}

__global__ __launch_bounds__(BLOCK_THREADS) void fpwrite_deflate_block_kernel(DflArgs A) {
  const uint32_t b = blockIdx.x * BLOCK_THREADS + threadIdx.x;
  if (b >= A.n_blocks)
    return;
  const uint32_t t = last_not_above(A.block_starts, A.n_tiles, b);
  const TileGeom& g = A.tiles[t];
  const uint32_t k = b - g.first_block;
  const uint32_t n = k + 1u < g.n_blocks ? BLOCK : g.n_bytes - k * BLOCK;
  compress_block(A.planes + g.plane_off, g.n_bytes, k * BLOCK, n, k + 1u == g.n_blocks, &A.works[b]);
}

__global__ __launch_bounds__(BLOCK_THREADS) void fpwrite_deflate_scan_kernel(DflArgs A) {
  const uint32_t t = blockIdx.x * BLOCK_THREADS + threadIdx.x;
  if (t >= A.n_tiles)
    return;
  scan_tile(A.tiles[t], A.works, (A.flags[t] & 1u) != 0, A.info, &A.tinfo[t]);
}

__global__ __launch_bounds__(EMIT_THREADS) void fpwrite_deflate_emit_kernel(DflArgs A) {
  const uint32_t t = last_not_above(A.group_starts, A.n_tiles, blockIdx.x);
  const TileGeom& g = A.tiles[t];
  const TileInfo ti = A.tinfo[t];
  const uint64_t j = uint64_t(blockIdx.x - g.first_group) * EMIT_THREADS + threadIdx.x;
  if (ti.status != RSX_OK || j >= ti.bytes) // (bytes <= out_cap where the status is RSX_OK)
    return;
  A.out_base[g.out_off + j] = stream_byte(g, ti, A.works, A.info, A.planes + g.plane_off, j);
}

struct FpDeflatePlan final : DecoderPlan {
  rsx_ctx* ctx = nullptr;
  std::vector<int32_t> host;    // validation result per job
  std::vector<int32_t> dev_of;  // job -> index among the tiles that go to the device, or -1
  std::vector<TileGeom> tiles;
  std::vector<uint32_t> group_starts, block_starts;
  std::vector<TileInfo> tinfo;  // of the last fetch
  DeviceBuffer d_tiles, d_groups, d_blocks, d_planes, d_works, d_info, d_tinfo, d_flags;
  uint64_t total_groups = 0, total_blocks = 0, plane_bytes = 0;
  bool fetched = false;

  int finish() {
    for (const TileGeom& g : tiles) {
      group_starts.push_back(g.first_group);
      block_starts.push_back(g.first_block);
    }
    group_starts.push_back(uint32_t(total_groups));
    block_starts.push_back(uint32_t(total_blocks));
    tinfo.resize(tiles.size());
    RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (int st = upload(ctx, d_tiles, tiles))
      return st;
    if (int st = upload(ctx, d_groups, group_starts))
      return st;
    if (int st = upload(ctx, d_blocks, block_starts))
      return st;
    if (int st = d_planes.ensure(size_t(plane_bytes) + 16))
      return st;
    if (int st = d_works.ensure(size_t(total_blocks) * sizeof(BlockWork) + 16))
      return st;
    if (int st = d_info.ensure(size_t(total_blocks) * sizeof(BlockInfo) + 16))
      return st;
    if (int st = d_tinfo.ensure(tiles.size() * sizeof(TileInfo) + 16))
      return st;
    return d_flags.ensure(tiles.size() * 4 + 16);
  }
  int run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) override {
    fetched = false;
    if (tiles.empty())
      return RSX_OK; // (every job was refused by the host)
    if (reinterpret_cast<uintptr_t>(in_dev) % 4u != 0)
      return RSX_ERR_INVALID_ARG; // the samples lie on their grid
    RSX_HIP_CHECK(ctx, hipMemsetAsync(d_flags.ptr, 0, tiles.size() * 4, s));
    DflArgs A{};
    A.in_base = static_cast<const uint8_t*>(in_dev);
    A.out_base = static_cast<uint8_t*>(out_dev);
    A.tiles = static_cast<const TileGeom*>(d_tiles.ptr);
    A.group_starts = static_cast<const uint32_t*>(d_groups.ptr);
    A.block_starts = static_cast<const uint32_t*>(d_blocks.ptr);
    A.planes = static_cast<uint8_t*>(d_planes.ptr);
    A.works = static_cast<BlockWork*>(d_works.ptr);
    A.info = static_cast<BlockInfo*>(d_info.ptr);
    A.tinfo = static_cast<TileInfo*>(d_tinfo.ptr);
    A.flags = static_cast<uint32_t*>(d_flags.ptr);
    A.n_tiles = uint32_t(tiles.size());
    A.n_blocks = uint32_t(total_blocks);
    const uint32_t block_groups = uint32_t((total_blocks + BLOCK_THREADS - 1) / BLOCK_THREADS);
    const uint32_t tile_groups = uint32_t((tiles.size() + BLOCK_THREADS - 1) / BLOCK_THREADS);
    if (timer)
      timer->begin(s);
    hipLaunchKernelGGL(fpwrite_deflate_planes_kernel, dim3(uint32_t(total_groups)), dim3(EMIT_THREADS),
                       0, s, A);
    if (timer)
      timer->mark("fpwrite_deflate_planes_kernel");
    hipLaunchKernelGGL(fpwrite_deflate_block_kernel, dim3(block_groups), dim3(BLOCK_THREADS), 0, s, A);
    if (timer)
      timer->mark("fpwrite_deflate_block_kernel");
    hipLaunchKernelGGL(fpwrite_deflate_scan_kernel, dim3(tile_groups), dim3(BLOCK_THREADS), 0, s, A);
    if (timer)
      timer->mark("fpwrite_deflate_scan_kernel");
    hipLaunchKernelGGL(fpwrite_deflate_emit_kernel, dim3(uint32_t(total_groups)), dim3(EMIT_THREADS),
                       0, s, A);
    if (timer)
      timer->mark("fpwrite_deflate_emit_kernel");
    RSX_HIP_CHECK(ctx, hipGetLastError());
    return RSX_OK;
  }
  int status_of(size_t i) const {
    if (host[i] != RSX_OK || !fetched)
      return int(host[i]);
    return tinfo[size_t(dev_of[i])].status;
  }
  int results(hipStream_t s, bool ran, int32_t* job_status, uint32_t* job_consumed) override {
    if (ran && !tiles.empty() && !fetched) {
      RSX_HIP_CHECK(ctx, hipMemcpyAsync(tinfo.data(), d_tinfo.ptr, tinfo.size() * sizeof(TileInfo),
                                        hipMemcpyDeviceToHost, s));
      RSX_HIP_CHECK(ctx, hipStreamSynchronize(s));
      fetched = true;
    }
    if (job_consumed)
      for (size_t i = 0; i < host.size(); ++i)
        job_consumed[i] = host[i] == RSX_OK && fetched ? uint32_t(tinfo[size_t(dev_of[i])].bytes) : 0u;
    return fold_jobs(host.size(), FoldOrder::LAST_FAILING, job_status,
                     [&](size_t i) { return status_of(i); });
  }
  int fpwrite_deflate_result(int job, rsx_fpwrite_deflate_result* out) override {
    if (job < 0 || size_t(job) >= host.size() || !out)
      return RSX_ERR_INVALID_ARG;
    *out = rsx_fpwrite_deflate_result{};
    out->status = status_of(size_t(job));
    if (host[job] == RSX_OK && fetched) {
      const TileInfo& t = tinfo[size_t(dev_of[job])];
      out->adler = t.adler, out->bytes = t.bytes, out->blocks = t.blocks;
      out->stored_blocks = t.stored_blocks;
    }
    return out->status;
  }
};

} // namespace

int fpwrite_deflate_validate(const rsx_dng_deflate_desc& d, uint32_t tile_w, uint32_t tile_h,
                             uint32_t off_x, uint32_t off_y, uint32_t width, uint32_t height,
                             const rsx_image& img) {
  return validate_tile(d, tile_w, tile_h, off_x, off_y, width, height, img);
}

int fpwrite_deflate_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_fpwrite_deflate_job* jobs,
                                std::unique_ptr<DecoderPlan>* out) {
  auto p = std::make_unique<FpDeflatePlan>();
  p->ctx = ctx;
  p->host.assign(n_jobs, RSX_OK);
  p->dev_of.assign(n_jobs, -1);
  for (int i = 0; i < n_jobs; ++i) {
    const rsx_fpwrite_deflate_job& j = jobs[i];
    int st = fpwrite_deflate_validate(j.desc, j.tile_w, j.tile_h, j.off_x, j.off_y, j.width, j.height,
                                      j.img);
    if (st == RSX_OK && j.img_offset % 4u != 0)
      st = RSX_ERR_INVALID_ARG;
    p->host[i] = st;
    if (st != RSX_OK)
      continue;
    TileGeom g;
    tile_geom(j.desc, j.tile_w, j.tile_h, j.off_x, j.off_y, j.width, j.height, j.img, j.img_offset,
              j.out_offset, j.out_cap, &g);
    g.plane_off = p->plane_bytes;
    g.first_block = uint32_t(p->total_blocks);
    g.first_group = uint32_t(p->total_groups);
    p->plane_bytes += (uint64_t(g.n_bytes) + 15u) & ~uint64_t(15);
    p->total_blocks += g.n_blocks;
    p->total_groups += (bound_of(g.n_bytes) + EMIT_THREADS - 1) / EMIT_THREADS;
    if (p->total_groups > 0x7FFFFFFFull || p->total_blocks > 0x7FFFFFFFull)
      return RSX_ERR_UNSUPPORTED; // (a launch's grid)
    p->dev_of[i] = int32_t(p->tiles.size());
    p->tiles.push_back(g);
  }
  if (int st = p->finish())
    return st;
  *out = std::move(p);
  return RSX_OK;
}

} // namespace rsx
