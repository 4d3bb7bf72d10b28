// Lossy-JPEG DNG tiles (compression 0x884c): AbstractDngDecompressor's decompressThread<0x884c>
// -> JpegDecompressor::decode (decompressors/JpegDecompressor.cpp:128-170), include/rsx.h
// section 4e.  The arithmetic is rsx_jpeg_core.h, which also runs on the host.
//
// The host reads every tile's header while the plan is made: the tables, the geometry and the
// entropy segments (the scan, or its restart intervals: the RSTn markers are looked for there).
// Two kernels, gfx950, no MFMA.
//
// jpeg_blocks_kernel: ONE WAVE (a workgroup of 64) per entropy segment.  The tile's Huffman
//   look-ups (a 9-bit look-ahead table and the long-code arrays per component) and quantisers are
//   in LDS, and so is a window of 8 KiB of the segment's bytes, reloaded by all lanes when the walk
//   has used half of it.  Lane 0 walks the bits through a 64-bit buffer and leaves the
//   coefficients of eight blocks in LDS; all 64 lanes then dequantise and transform them, 8 blocks
//   x 8 columns and 8 blocks x 8 rows (jpeg_idct_islow), and store the samples, 8 bytes a lane,
//   into the component planes in the plan's scratch (whole MCUs).  A refusal goes into the tile's
//   status word with an atomic max; nothing is read back in between.
// jpeg_finish_kernel: a lane owns the eight output samples of one 16-byte unit of an image row
//   (sample by sample where the window's edge cuts it).  It reads the planes, upsamples with
//   libjpeg-turbo's triangle filters, converts YCbCr to RGB and widens to 16 bits; only inside the
//   tile's window, and only where the tile's status is RSX_OK.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "rsx_dng_jpeg.h"
#include "rsx_internal.h"
#include "rsx_jpeg_core.h"
#include "rsx_ljpeg_dev.h"
#include "rsx_plan_host.h"

namespace rsx {
namespace {

using rsx_jpeg::Segment;
using rsx_jpeg::Tables;
using rsx_jpeg::Tile;

constexpr uint64_t JPEG_MAX_SCRATCH = uint64_t(1) << 30; // what the other tile codecs accept
constexpr uint32_t WIN = 8192;       // bytes of a segment in LDS
constexpr uint32_t WIN_KEEP = 4096;  // reload when fewer are left: eight blocks never take more
constexpr uint32_t FIN_LANES = 128;  // a workgroup of the finish kernel: 128 units of a row

struct JpArgs {
  const uint8_t* in_base;
  uint8_t* out_base;
  uint8_t* planes;
  const Tile* tiles;
  const Segment* segs;
  const Tables* tables;
  uint32_t* status; // per tile: RSX_OK or the largest refusal of its segments
};

// bytes of the tile: out of the LDS window where it holds them
struct WinSrc {
  const uint8_t* g;
  const uint8_t* win;
  uint32_t base; // the window's first byte (may lie before the tile: modulo 2^32)
  __device__ __forceinline__ uint32_t at(uint32_t i) const {
    const uint32_t d = i - base;
    return d < WIN ? win[d] : g[i];
  }
};

__global__ void __launch_bounds__(64) jpeg_blocks_kernel(JpArgs A) {
  __shared__ Tables LT;
  __shared__ uint4 win4[WIN / 16];
  __shared__ int16_t coef[rsx_jpeg::BATCH * 64];
  __shared__ int32_t ws[rsx_jpeg::BATCH * 64];
  __shared__ uint8_t order[64];
  const uint32_t lane = threadIdx.x;
  order[lane] = uint8_t(rsx_jpeg::natural_order(lane));
  const Segment S = A.segs[blockIdx.x];
  const Tile T = A.tiles[S.tile];
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(A.tables + T.tables);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&LT);
    for (uint32_t i = lane; i < sizeof(Tables) / 4u; i += 64u)
      dst[i] = src[i];
  }
  const uint8_t* const tile_in = A.in_base + T.in_off;
  WinSrc src{tile_in, reinterpret_cast<const uint8_t*>(win4), 0u};
  rsx_jpeg::Bits<WinSrc> B;
  B.init(&src, S.start, S.end);
  const uint32_t per_mcu = T.ncomp == 1 ? 1u : uint32_t(T.hs) * T.vs + 2u;
  const uint32_t nb = S.n_mcus * per_mcu; // (fits: an MCU count times at most 6)
  int32_t pred0 = 0, pred1 = 0, pred2 = 0;
  int st = RSX_OK;
  bool overshoot = false, have_win = false;
  for (uint32_t b0 = 0; b0 < nb; b0 += rsx_jpeg::BATCH) {
    const uint32_t pos = uint32_t(__builtin_amdgcn_readfirstlane(int(B.pos)));
    if (!have_win || pos - src.base > WIN - WIN_KEEP) {
      // the window from the 16-byte unit of the input that holds byte `pos`
      have_win = true;
      src.base = pos - uint32_t(reinterpret_cast<uintptr_t>(tile_in + pos) & 15u);
      __syncthreads(); // (lane 0 is done with the old window)
      for (uint32_t u = lane; u < WIN / 16u; u += 64u) {
        const uint32_t first = src.base + 16u * u; // modulo 2^32 in front of the tile
        uint4 v = make_uint4(0, 0, 0, 0);
        if (first < T.in_bytes && T.in_bytes - first >= 16u) {
          v = *reinterpret_cast<const uint4*>(tile_in + first);
        } else {
          uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
          for (uint32_t k = 0; k < 16u; ++k) {
            const uint32_t i = first + k;
            if (i < T.in_bytes)
              w[k >> 2] |= uint32_t(tile_in[i]) << (8u * (k & 3u));
          }
          v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        win4[u] = v;
      }
    }
    for (uint32_t i = lane; i < rsx_jpeg::BATCH * 32u; i += 64u)
      reinterpret_cast<uint32_t*>(coef)[i] = 0u;
    __syncthreads();
    const uint32_t nbk = std::min(rsx_jpeg::BATCH, nb - b0);
    if (lane == 0) {
      for (uint32_t k = 0; k < nbk && st == RSX_OK; ++k) {
        const uint32_t comp = rsx_jpeg::block_comp(T, b0 + k);
        int32_t p = comp == 0 ? pred0 : comp == 1 ? pred1 : pred2;
        st = rsx_jpeg::decode_block(B, comp == 0 ? LT.dc[0] : comp == 1 ? LT.dc[1] : LT.dc[2],
                                    comp == 0 ? LT.ac[0] : comp == 1 ? LT.ac[1] : LT.ac[2], order,
                                    &p, coef + k * 64u);
        if (comp == 0)
          pred0 = p;
        else if (comp == 1)
          pred1 = p;
        else
          pred2 = p;
      }
    }
    __syncthreads();
    if (__builtin_amdgcn_readfirstlane(st) != RSX_OK)
      break; // (the segment is refused: the tile writes nothing)
    const uint32_t blk = lane >> 3, sub = lane & 7u;
    uint32_t comp = 0;
    uint64_t at = 0;
    if (blk < nbk) {
      rsx_jpeg::block_place(T, S, b0 + blk, &comp, &at);
      if (!rsx_jpeg::idct_column(coef + blk * 64u, LT.q[comp], sub, ws + blk * 64u))
        overshoot = true;
    }
    __syncthreads();
    if (blk < nbk) {
      union {
        uint8_t b[8];
        uint2 v;
      } o;
      rsx_jpeg::idct_row(ws + blk * 64u, sub, o.b);
      const uint32_t pw = comp == 0 ? T.plane_w[0] : comp == 1 ? T.plane_w[1] : T.plane_w[2];
      *reinterpret_cast<uint2*>(A.planes + at + uint64_t(sub) * pw) = o.v;
    }
  }
  int verdict = __builtin_amdgcn_readfirstlane(st);
  if (__any(overshoot) && verdict < RSX_ERR_UNSUPPORTED)
    verdict = RSX_ERR_UNSUPPORTED;
  if (lane == 0 && verdict != RSX_OK)
    atomicMax(&A.status[S.tile], uint32_t(verdict));
}

// grid: (units of a row / FIN_LANES, rows, tiles), each the largest of the plan
__global__ void __launch_bounds__(FIN_LANES) jpeg_finish_kernel(JpArgs A) {
  const Tile T = A.tiles[blockIdx.z];
  const uint32_t y = blockIdx.y;
  if (y >= T.copy_h || A.status[blockIdx.z] != uint32_t(RSX_OK))
    return; // (a tile that is not whole writes nothing)
  uint8_t* const rowp = A.out_base + T.img_off + uint64_t(T.off_y + y) * T.pitch;
  const uint32_t nc = T.ncomp;
  // samples [w0, w1) of the row are the window's; sample s lies in the 16-byte unit (s + a) >> 3
  const int32_t a = int32_t((reinterpret_cast<uintptr_t>(rowp) >> 1) & 7u);
  const int32_t w0 = int32_t(T.off_x * nc), w1 = w0 + int32_t(T.copy_w * nc);
  const int32_t unit = ((w0 + a) >> 3) + int32_t(blockIdx.x * FIN_LANES + threadIdx.x);
  const int32_t s_lo = unit * 8 - a;
  const int32_t lo = std::max(s_lo, w0), hi = std::min(s_lo + 8, w1);
  if (lo >= hi)
    return;
  uint32_t v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k)
    v[k] = 0;
  if (nc == 1) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int32_t s = s_lo + k;
      if (s >= lo && s < hi) {
        uint32_t px[3];
        rsx_jpeg::pixel_at(A.planes, T, uint32_t(s - w0), y, px);
        v[k] = px[0];
      }
    }
  } else {
    const int32_t p_lo = (lo - w0) / 3, p_hi = (hi - 1 - w0) / 3;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int32_t p = p_lo + j;
      if (p > p_hi)
        break;
      uint32_t px[3];
      rsx_jpeg::pixel_at(A.planes, T, uint32_t(p), y, px);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int32_t k = w0 + 3 * p + c - s_lo;
#pragma unroll
        for (int kk = 0; kk < 8; ++kk)
          if (kk == k)
            v[kk] = px[c];
      }
    }
  }
  uint16_t* const dst = reinterpret_cast<uint16_t*>(rowp) + s_lo;
  if (hi - lo == 8) {
    *reinterpret_cast<uint4*>(dst) = make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16),
                                                v[4] | (v[5] << 16), v[6] | (v[7] << 16));
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (s_lo + k >= lo && s_lo + k < hi)
        dst[k] = uint16_t(v[k]);
  }
}

struct JpegPlan final : DecoderPlan {
  rsx_ctx* ctx = nullptr;
  std::vector<int32_t> job_host_status;          // a job that is no job at all
  std::vector<uint32_t> job_first;               // its first tile; n_jobs + 1 entries
  std::vector<std::vector<JpegWindow>> windows;  // per job
  std::vector<int32_t> tile_final;               // per tile, after results
  DeviceBuffer d_tiles, d_segs, d_tables, d_status, d_planes;
  std::vector<uint32_t> h_status;
  uint32_t n_tiles = 0, n_segs = 0, max_units = 0, max_rows = 0;
  int run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) override;
  int results(hipStream_t s, bool ran, int32_t* job_status, uint32_t* job_consumed) override;
  int row_status(hipStream_t, int job, int32_t* out) override {
    if (job < 0 || size_t(job) + 1 >= job_first.size() || !out || tile_final.size() != n_tiles)
      return RSX_ERR_INVALID_ARG;
    std::copy(tile_final.begin() + job_first[job], tile_final.begin() + job_first[job + 1], out);
    return RSX_OK;
  }
};

} // namespace

const std::vector<JpegWindow>& dng_jpeg_plan_windows(const DecoderPlan* plan, int job) {
  return static_cast<const JpegPlan*>(plan)->windows[size_t(job)];
}

int dng_jpeg_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_dng_jpeg_job* jobs,
                         std::unique_ptr<DecoderPlan>* out) {
  auto p = std::make_unique<JpegPlan>();
  p->ctx = ctx;
  p->job_host_status.assign(n_jobs, RSX_OK);
  p->windows.resize(n_jobs);
  std::vector<Tile> tiles;
  std::vector<Segment> segs;
  std::vector<Tables> tables;
  uint64_t scratch = 0;
  for (int i = 0; i < n_jobs; ++i) {
    const rsx_dng_jpeg_job& j = jobs[i];
    p->job_first.push_back(uint32_t(tiles.size()));
    if (j.n_tiles < 1 || !j.tiles || !j.in_offsets || j.img_offset % 2 != 0) {
      p->job_host_status[i] = RSX_ERR_INVALID_ARG;
      continue;
    }
    for (int t = 0; t < j.n_tiles; ++t) {
      const rsx_dng_jpeg_tile& jt = j.tiles[t];
      rsx_jpeg::Header H;
      Tile T = Tile();
      int st = rsx_jpeg::validate_tile(jt.in, jt.in_bytes, jt.off_x, jt.off_y, j.img, &H);
      const size_t seg0 = segs.size();
      if (st == RSX_OK)
        st = rsx_jpeg::scan_segments(jt.in, jt.in_bytes, H,
                                     [&](uint32_t, uint32_t first, uint32_t n, uint32_t a, uint32_t b) {
                                       segs.push_back(Segment{uint32_t(tiles.size()), first, n, a, b});
                                     });
      if (st == RSX_OK) {
        const uint64_t end = rsx_jpeg::fill_tile(H, jt.off_x, jt.off_y, j.img, scratch, &T);
        if (end > JPEG_MAX_SCRATCH)
          return RSX_ERR_UNSUPPORTED;
        scratch = end;
        T.in_off = j.in_offsets[t];
        T.in_bytes = uint32_t(jt.in_bytes);
        T.img_off = j.img_offset;
        Tables tb;
        std::memset(&tb, 0, sizeof tb);
        rsx_jpeg::fill_tables(H, &tb);
        // (the tiles of a file share their tables: the one in front is usually the same)
        if (tables.empty() || std::memcmp(&tables.back(), &tb, sizeof tb) != 0)
          tables.push_back(tb);
        T.tables = uint32_t(tables.size() - 1);
        const uint32_t units = (T.copy_w * T.ncomp + 7u) / 8u + 1u;
        p->max_units = std::max(p->max_units, units);
        p->max_rows = std::max(p->max_rows, T.copy_h);
      } else {
        segs.resize(seg0);
      }
      p->windows[i].push_back(JpegWindow{T.off_x, T.off_y, T.copy_w, T.copy_h, T.ncomp, st});
      tiles.push_back(T);
    }
  }
  p->job_first.push_back(uint32_t(tiles.size()));
  p->n_tiles = uint32_t(tiles.size());
  p->n_segs = uint32_t(segs.size());
  if (p->max_rows > 65535u || p->n_tiles > 65535u)
    return RSX_ERR_UNSUPPORTED; // (the finish kernel's grid)
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int st;
  if ((st = upload(ctx, p->d_tiles, tiles)) || (st = upload(ctx, p->d_segs, segs)) ||
      (st = upload(ctx, p->d_tables, tables)) || (st = p->d_status.ensure(tiles.size() * 4 + 16)) ||
      (st = p->d_planes.ensure(size_t(scratch) + 16)))
    return st;
  p->h_status.assign(tiles.size(), 0u);
  *out = std::move(p);
  return RSX_OK;
}

namespace {

int JpegPlan::run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) {
  tile_final.clear();
  if (n_segs == 0)
    return RSX_OK; // (every tile was refused by the host)
  if ((reinterpret_cast<uintptr_t>(out_dev) & 1u) != 0)
    return RSX_ERR_INVALID_ARG;
  if (timer)
    timer->begin(s);
  JpArgs A{};
  A.in_base = static_cast<const uint8_t*>(in_dev);
  A.out_base = static_cast<uint8_t*>(out_dev);
  A.planes = static_cast<uint8_t*>(d_planes.ptr);
  A.tiles = static_cast<const Tile*>(d_tiles.ptr);
  A.segs = static_cast<const Segment*>(d_segs.ptr);
  A.tables = static_cast<const Tables*>(d_tables.ptr);
  A.status = static_cast<uint32_t*>(d_status.ptr);
  RSX_HIP_CHECK(ctx, hipMemsetAsync(d_status.ptr, 0, size_t(n_tiles) * 4, s));
  hipLaunchKernelGGL(jpeg_blocks_kernel, dim3(n_segs), dim3(64), 0, s, A);
  if (timer)
    timer->mark("jpeg_blocks_kernel");
  RSX_HIP_CHECK(ctx, hipGetLastError());
  hipLaunchKernelGGL(jpeg_finish_kernel, dim3((max_units + FIN_LANES - 1) / FIN_LANES, max_rows, n_tiles),
                     dim3(FIN_LANES), 0, s, A);
  if (timer)
    timer->mark("jpeg_finish_kernel");
  RSX_HIP_CHECK(ctx, hipGetLastError());
  return RSX_OK;
}

int JpegPlan::results(hipStream_t s, bool ran, int32_t* job_status, uint32_t* job_consumed) {
  const size_t n_jobs = job_host_status.size();
  if (job_consumed)
    std::fill(job_consumed, job_consumed + n_jobs, 0u);
  if (ran && n_segs != 0)
    if (int st = fetch_words(ctx, s, d_status, 0, h_status.size(), h_status.data()))
      return st;
  tile_final.assign(n_tiles, RSX_OK);
  // a job's tiles fold into RSX_ERR_TILE_ERRORS, or RSX_ERR_DEVICE if one of them says so
  return fold_jobs(n_jobs, FoldOrder::LAST_FAILING, job_status, [&](size_t i) {
    int st = job_host_status[i];
    for (uint32_t t = job_first[i]; t < job_first[i + 1]; ++t) {
      int ts = windows[i][t - job_first[i]].host_status;
      if (ts == RSX_OK && ran) {
        const uint32_t v = h_status[t];
        ts = v <= uint32_t(RSX_ERR_VALUE_RANGE) ? int(v) : RSX_ERR_DEVICE;
      }
      tile_final[t] = ts;
      if (ts != RSX_OK)
        st = ts == RSX_ERR_DEVICE ? RSX_ERR_DEVICE : RSX_ERR_TILE_ERRORS;
    }
    return st;
  });
}

} // namespace
} // namespace rsx
