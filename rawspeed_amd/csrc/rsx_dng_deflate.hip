// Deflate-compressed floating-point DNG tiles (compression 8): AbstractDngDecompressor's
// decompressThread<8> (AbstractDngDecompressor.cpp:134-155) -> DeflateDecompressor::decode
// (decompressors/DeflateDecompressor.cpp:49-176), include/rsx.h section 4b.
//
// Two kernels, gfx950.
//
// dfl_inflate_kernel: zlib's uncompress() of one tile stream by ONE WAVE (a workgroup of 64).  The
//   decoder is rsx_inflate_core.h, which also runs on the host.  The stream's state -- a 64-bit
//   LSB-first bit buffer, the positions, the symbol just decoded -- is the same in all lanes and
//   lives in scalar registers.  The input comes in windows of 256 bytes, a dword a lane, the next
//   window loaded while this one is read; a word is taken from its lane with v_readlane.  The
//   tables (zlib's shape: a root table of 9 resp. 6 bits and sub-tables) and the last 32 KiB of
//   output are in LDS, 40 112 bytes a wave, so four waves share a CU.  Matches and stored blocks
//   are copied by all lanes; the window goes to the plan's scratch in 16-byte stores, and the
//   Adler-32 is summed over what is flushed.  Per job: a verdict and the stream's length.
// dfl_row_kernel: one wave per tile row below `height`, only where the inflate gave exactly
//   dstLen bytes.  The stride-predFactor byte prefix sum mod 256 over the whole row: a lane sums
//   a piece of PF * K bytes, the pieces' totals (PF bytes, packed in dwords, added bytewise) go
//   through a wave scan, chunk after chunk with a carry; in place in the scratch.  Then the byte
//   planes are gathered, most significant first, widened (widen_fp) and stored as floats.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "rsx_dng_deflate.h"
#include "rsx_fp_widen.h"
#include "rsx_inflate_core.h"
#include "rsx_internal.h"
#include "rsx_ljpeg_dev.h"
#include "rsx_plan_host.h"

namespace rsx {
namespace {

constexpr uint64_t DFL_MAX_SCRATCH = uint64_t(1) << 30; // what the LJPEG pipeline accepts

struct DflJobDev {
  uint64_t in_off, img_off, scratch_off;
  uint32_t in_bytes, dst_len; // dst_len 0: refused by the host
  uint32_t tile_w, tile_h, off_x, off_y, width, height; // samples
  uint32_t pitch, bytesps, pf, pad;
};
struct DflRowDev {
  uint32_t job, row;
};
struct DflArgs {
  const uint8_t* in_base;
  uint8_t* out_base;
  uint8_t* scratch;
  const DflJobDev* jobs;
  const DflRowDev* rows;
  uint32_t* status; // per job: verdict, bytes consumed
};

// The wave of rsx_inflate_core.h on the device.
struct DevWave {
  static constexpr uint32_t N = 64;
  uint32_t lane = 0, skip = 0;
  const uint8_t* in = nullptr;
  const uint32_t* base = nullptr; // `in`, down to a 4-byte boundary
  uint32_t n_words = 0;           // the words from `base` that hold input
  uint32_t cur = 0, nxt = 0;      // this lane's word of the window at cur_base, and of the next
  uint32_t cur_base = 0xFFFF0000u;
  __device__ __forceinline__ uint32_t uni(uint32_t x) const { return __builtin_amdgcn_readfirstlane(x); }
  __device__ __forceinline__ void sync() const {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  __device__ __forceinline__ uint64_t ballot(bool p) const { return __ballot(p); }
  __device__ __forceinline__ uint64_t lt_mask() const { return (uint64_t(1) << lane) - 1u; }
  __device__ __forceinline__ uint64_t reduce_add(uint64_t x) const {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const uint32_t lo = __shfl_xor(uint32_t(x), d), hi = __shfl_xor(uint32_t(x >> 32), d);
      x += (uint64_t(hi) << 32) | lo;
    }
    return x;
  }
  __device__ __forceinline__ uint32_t load(uint32_t wb) const {
    const uint32_t i = wb + lane;
    return i < n_words ? base[i] : 0u;
  }
  __device__ __forceinline__ uint32_t word(uint32_t i) {
    i = uni(i);
    const uint32_t wb = i & ~63u;
    if (wb != cur_base) {
      cur = wb == cur_base + 64u ? nxt : load(wb);
      nxt = load(wb + 64u);
      cur_base = wb;
    }
    return uint32_t(__builtin_amdgcn_readlane(int(cur), int(i & 63u)));
  }
  __device__ __forceinline__ uint8_t byte(uint64_t i) const { return in[i]; }
  __device__ __forceinline__ void store16(uint8_t* dst, const rsx_inflate::U4& v) const {
    *reinterpret_cast<uint4*>(dst) = make_uint4(v.x, v.y, v.z, v.w);
  }
};

__global__ void __launch_bounds__(64) dfl_inflate_kernel(DflArgs A) {
  __shared__ rsx_inflate::Shared S;
  const DflJobDev J = A.jobs[blockIdx.x];
  if (J.dst_len == 0u)
    return;
  DevWave w;
  w.lane = threadIdx.x;
  w.in = A.in_base + J.in_off;
  w.skip = uint32_t(reinterpret_cast<uintptr_t>(w.in) & 3u);
  w.base = reinterpret_cast<const uint32_t*>(w.in - w.skip);
  w.n_words = J.in_bytes ? uint32_t((uint64_t(w.skip) + J.in_bytes + 3u) >> 2) : 0u;
  uint32_t produced = 0, consumed = 0;
  const int v = rsx_inflate::inflate_stream(w, S, J.in_bytes, A.scratch + J.scratch_off, J.dst_len,
                                            &produced, &consumed);
  if (threadIdx.x == 0) {
    A.status[2u * blockIdx.x] = uint32_t(v);
    A.status[2u * blockIdx.x + 1u] = consumed;
  }
}

// bytewise a + b mod 256 of four packed bytes
__device__ __forceinline__ uint32_t dfl_add8(uint32_t a, uint32_t b) {
  return ((a & 0x7F7F7F7Fu) + (b & 0x7F7F7F7Fu)) ^ ((a ^ b) & 0x80808080u);
}

// One tile row: rowp[i] += rowp[i - PF] for PF <= i < row_bytes, in place; then the samples.
template <int PF>
__device__ __forceinline__ void dfl_row(const DflArgs& A, const DflJobDev& J, const uint32_t row) {
  constexpr int K = 16 / PF > 0 ? 16 / PF : 1;
  constexpr int S = PF * K;         // bytes a lane sums by itself: a multiple of PF
  constexpr int NQ = (PF + 3) / 4;  // dwords that hold PF running sums
  const uint32_t lane = threadIdx.x;
  const uint32_t row_bytes = J.bytesps * J.tile_w;
  uint8_t* const rowp = A.scratch + J.scratch_off + uint64_t(row) * row_bytes;
  uint32_t carry[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q)
    carry[q] = 0;
  for (uint64_t base = 0; base < row_bytes; base += 64u * S) { // (64-bit: rows up to 4 GiB)
    const uint64_t start = base + lane * S;
    uint32_t b[S];
#pragma unroll
    for (int i = 0; i < S; ++i)
      b[i] = start + i < row_bytes ? rowp[start + i] : 0u;
#pragma unroll
    for (int i = PF; i < S; ++i)
      b[i] = (b[i] + b[i - PF]) & 255u;
    uint32_t t[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      t[q] = 0;
#pragma unroll
    for (int r = 0; r < PF; ++r)
      t[r >> 2] |= b[S - PF + r] << (8 * (r & 3));
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const uint32_t u = __shfl_up(t[q], d);
        if (lane >= uint32_t(d))
          t[q] = dfl_add8(t[q], u);
      }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const uint32_t before = __shfl_up(t[q], 1), all = __shfl(t[q], 63);
      t[q] = dfl_add8(lane ? before : 0u, carry[q]);
      carry[q] = dfl_add8(carry[q], all);
    }
#pragma unroll
    for (int i = 0; i < S; ++i) {
      const int r = i % PF;
      const uint32_t v = (b[i] + (t[r >> 2] >> (8 * (r & 3)))) & 255u;
      if (start + i < row_bytes)
        rowp[start + i] = uint8_t(v);
    }
  }
  __syncthreads(); // (the lanes read each other's bytes from here on)
  uint8_t* const orow = A.out_base + J.img_off + uint64_t(J.off_y + row) * J.pitch + uint64_t(J.off_x) * 4u;
  for (uint32_t col = lane * 4u; col < J.width; col += 256u) {
    uint32_t v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      uint32_t x = 0;
      if (col + k < J.width) {
#pragma unroll
        for (int p = 0; p < 4; ++p)
          if (uint32_t(p) < J.bytesps)
            x = (x << 8) | rowp[col + k + uint64_t(p) * J.tile_w];
        x = J.bytesps == 2u ? widen_fp<10, 5>(x) : J.bytesps == 3u ? widen_fp<16, 7>(x) : x;
      }
      v[k] = x;
    }
    uint8_t* dst = orow + uint64_t(col) * 4u;
    if (col + 4u <= J.width && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0u) {
      *reinterpret_cast<uint4*>(dst) = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (col + k < J.width)
          reinterpret_cast<uint32_t*>(dst)[k] = v[k];
    }
  }
}

__global__ void __launch_bounds__(64) dfl_row_kernel(DflArgs A) {
  const DflRowDev R = A.rows[blockIdx.x];
  if (A.status[2u * R.job] != uint32_t(rsx_inflate::V_OK))
    return; // (a tile that is not whole writes nothing)
  const DflJobDev J = A.jobs[R.job];
  switch (J.pf) { // predFactor x cpp: {1, 2, 4} x {1 .. 4}
  case 1: dfl_row<1>(A, J, R.row); break;
  case 2: dfl_row<2>(A, J, R.row); break;
  case 3: dfl_row<3>(A, J, R.row); break;
  case 4: dfl_row<4>(A, J, R.row); break;
  case 6: dfl_row<6>(A, J, R.row); break;
  case 8: dfl_row<8>(A, J, R.row); break;
  case 12: dfl_row<12>(A, J, R.row); break;
  default: dfl_row<16>(A, J, R.row); break;
  }
}

struct DflPlan final : DecoderPlan {
  rsx_ctx* ctx = nullptr;
  std::vector<DflJobDev> jobs;
  JobStatus status; // two words a job: the verdict, the input bytes consumed
  DeviceBuffer d_jobs, d_rows, d_scratch;
  uint32_t total_rows = 0, live = 0;
  int run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) override;
  int results(hipStream_t s, bool ran, int32_t* job_status, uint32_t* job_consumed) override;
};

} // namespace

int dng_deflate_validate(const rsx_dng_deflate_desc& d, uint32_t tile_w, uint32_t tile_h, uint32_t off_x,
                         uint32_t off_y, uint32_t width, uint32_t height, uint64_t in_bytes,
                         const rsx_image& img) {
  // DngDecoder admits 16, 24 and 32 bits for sample format 3; the constructor's predictor switch
  if (d.bps != 16 && d.bps != 24 && d.bps != 32)
    return RSX_ERR_INVALID_ARG;
  if (d.predictor != 3 && d.predictor != 34894 && d.predictor != 34895)
    return RSX_ERR_INVALID_ARG;
  // an F32 image: rows of 4-byte samples
  if (img.cpp < 1 || img.cpp > 4 || img.dim_x <= 0 || img.dim_y <= 0 || img.pitch_bytes % 4u != 0)
    return RSX_ERR_INVALID_ARG;
  if (tile_w == 0 || tile_h == 0 || width == 0 || height == 0 || width > tile_w || height > tile_h)
    return RSX_ERR_INVALID_ARG;
  if (uint64_t(off_x) + width > uint64_t(img.dim_x) * uint32_t(img.cpp) ||
      uint64_t(off_y) + height > uint64_t(img.dim_y))
    return RSX_ERR_INVALID_ARG;
  if (uint64_t(img.pitch_bytes) < uint64_t(img.dim_x) * uint32_t(img.cpp) * 4u)
    return RSX_ERR_INVALID_ARG;
  if (in_bytes >= (uint64_t(1) << 32) ||
      uint64_t(d.bps / 8) * tile_w * uint64_t(tile_h) >= (uint64_t(1) << 32))
    return RSX_ERR_UNSUPPORTED;
  return RSX_OK;
}

int dng_deflate_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_dng_deflate_job* jobs,
                            std::unique_ptr<DecoderPlan>* out) {
  auto p = std::make_unique<DflPlan>();
  p->ctx = ctx;
  p->status.host.assign(n_jobs, RSX_OK);
  p->jobs.resize(n_jobs);
  std::vector<DflRowDev> rows;
  uint64_t scratch = 0;
  for (int i = 0; i < n_jobs; ++i) {
    const rsx_dng_deflate_job& j = jobs[i];
    DflJobDev& J = p->jobs[i];
    std::memset(&J, 0, sizeof J);
    int st = dng_deflate_validate(j.desc, j.tile_w, j.tile_h, j.off_x, j.off_y, j.width, j.height,
                                  j.in_bytes, j.img);
    if (st == RSX_OK && j.img_offset % 4 != 0)
      st = RSX_ERR_INVALID_ARG;
    p->status.host[i] = st;
    if (st != RSX_OK)
      continue;
    J.in_off = j.in_offset;
    J.img_off = j.img_offset;
    J.scratch_off = scratch;
    J.in_bytes = uint32_t(j.in_bytes);
    J.bytesps = uint32_t(j.desc.bps / 8);
    J.dst_len = J.bytesps * j.tile_w * j.tile_h;
    J.tile_w = j.tile_w;
    J.tile_h = j.tile_h;
    J.off_x = j.off_x;
    J.off_y = j.off_y;
    J.width = j.width;
    J.height = j.height;
    J.pitch = j.img.pitch_bytes;
    J.pf = (j.desc.predictor == 3 ? 1u : j.desc.predictor == 34894 ? 2u : 4u) * uint32_t(j.img.cpp);
    scratch += (uint64_t(J.dst_len) + 15u) & ~uint64_t(15);
    if (scratch > DFL_MAX_SCRATCH)
      return RSX_ERR_UNSUPPORTED;
    for (uint32_t y = 0; y < J.height; ++y)
      rows.push_back(DflRowDev{uint32_t(i), y});
    p->total_rows += J.height;
    ++p->live;
  }
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int st;
  if ((st = upload(ctx, p->d_jobs, p->jobs)) || (st = upload(ctx, p->d_rows, rows)) ||
      (st = p->status.init(2)) || (st = p->d_scratch.ensure(size_t(scratch) + 16)))
    return st;
  *out = std::move(p);
  return RSX_OK;
}

namespace {

int DflPlan::run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) {
  if (live == 0)
    return RSX_OK; // (every job was refused by the host)
  if ((reinterpret_cast<uintptr_t>(out_dev) & 3u) != 0)
    return RSX_ERR_INVALID_ARG;
  if (timer)
    timer->begin(s);
  DflArgs A{};
  A.in_base = static_cast<const uint8_t*>(in_dev);
  A.out_base = static_cast<uint8_t*>(out_dev);
  A.scratch = static_cast<uint8_t*>(d_scratch.ptr);
  A.jobs = static_cast<const DflJobDev*>(d_jobs.ptr);
  A.rows = static_cast<const DflRowDev*>(d_rows.ptr);
  A.status = static_cast<uint32_t*>(status.dev.ptr);
  if (int st = status.reset(ctx, s))
    return st;
  hipLaunchKernelGGL(dfl_inflate_kernel, dim3(uint32_t(jobs.size())), dim3(64), 0, s, A);
  if (timer)
    timer->mark("dfl_inflate_kernel");
  RSX_HIP_CHECK(ctx, hipGetLastError());
  hipLaunchKernelGGL(dfl_row_kernel, dim3(total_rows), dim3(64), 0, s, A);
  if (timer)
    timer->mark("dfl_row_kernel");
  RSX_HIP_CHECK(ctx, hipGetLastError());
  return RSX_OK;
}

int DflPlan::results(hipStream_t s, bool ran, int32_t* job_status, uint32_t* job_consumed) {
  if (job_consumed)
    std::fill(job_consumed, job_consumed + jobs.size(), 0u);
  if (ran && live != 0)
    if (int st = status.fetch(ctx, s))
      return st;
  return fold_jobs(jobs.size(), FoldOrder::LAST_FAILING, job_status, [&](size_t i) {
    int st = status.host[i];
    if (st == RSX_OK && ran) {
      // libz's Z_OK with exactly dstLen bytes; Z_OK with fewer (the reference then reads
      // indeterminate bytes: the CPU gets the tile); everything libz rejects
      const uint32_t v = status.words[2 * i];
      st = v == uint32_t(rsx_inflate::V_OK)      ? RSX_OK
           : v == uint32_t(rsx_inflate::V_SHORT) ? RSX_ERR_UNSUPPORTED
           : v == uint32_t(rsx_inflate::V_FAIL)  ? RSX_ERR_IO
                                                 : RSX_ERR_DEVICE;
      if (job_consumed && v != uint32_t(rsx_inflate::V_FAIL) && st != RSX_ERR_DEVICE)
        job_consumed[i] = status.words[2 * i + 1];
    }
    return st;
  });
}

} // namespace
} // namespace rsx
