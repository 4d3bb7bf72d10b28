// PanasonicV5Decompressor, PanasonicV6Decompressor and PanasonicV7Decompressor on the device
// (include/rsx.h section 3j).
//
// What the reference does: the image is a sequence of 16-byte packets, each read as one 128-bit
// little-endian number (bit 0 = the LSB of byte 0).  Packet p holds the pixels [p n, (p + 1) n)
// in row-major order; dim_x % n == 0, so a packet never straddles a row.
//   V7 (PanasonicV7Decompressor.cpp:67-74), 14 bits, n = 9: pixel i = bits [14 i, 14 i + 14);
//     packet p at byte 16 p.
//   V5 (PanasonicV5Decompressor.cpp:190-207), 12 bits n = 10 / 14 bits n = 9: pixel i = bits
//     [bps i, bps i + bps).  The input is cut into blocks of 0x4000 bytes = 1024 packets, and a
//     block is rotated before it is read (:149-188): its bytes [0x1FF8, 0x4000) come first.
//     Packet q of a block starts at byte (16 q + 0x1FF8) mod 0x4000 of the block -- 8-byte
//     aligned, and packet 512 wraps: its low half is the block's last 8 bytes, its high half
//     the block's first 8.
//   V6 (PanasonicV6Decompressor.cpp:88-133, 176-220), 14 bits n = 11 / 12 bits n = 14: from the
//     TOP of the packet down: two first pixels of bps bits, then per triple of pixels a 2-bit
//     scale and three fields of 10 (8) bits; 4 (0) unused bits at the bottom.  Serial over the
//     packet's pixels with state per column parity; packet p at byte 16 p.
// No packet depends on another, and nothing in the data can fail.
//
//   panasonic_kernel<VER, BPS>   one workgroup of 256 lanes per item (a run of consecutive
//       packets of one job: 1024 for n = 9, 768 for n = 10 and 11, 512 for n = 14, so that an
//       item's values take at most 20 KiB of LDS); one lane per packet, 4, 3 or 2 packets a lane:
//       1. every lane issues the loads of its packets: one 16-byte load each when the input is
//          16-byte aligned (V5: two 8-byte loads), dwords shifted together else;
//       2. a lane decodes each of its packets into n values and writes them into the item's
//          pixel run in LDS (dword stores, the odd value of an odd n as a half); ONE barrier;
//       3. the workgroup writes the run out along the 16-byte grid of the OUTPUT: each lane
//          takes aligned 16-byte pieces of the rows the run covers -- five LDS dwords shifted
//          by the piece's parity in the run, one 16-byte store -- and the pieces cut by a row's
//          end, by the run's ends or by the image's left edge (rows that do not start on the
//          grid) go out as single values.  Nothing outside the image rectangle is written.
// Bit-exact against the model tests/rw2_files.py, which tests/test_panasonic_model.py holds
// against the reference's whole-file decode.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "rsx_internal.h"
#include "rsx_ljpeg_dev.h"
#include "rsx_plan_host.h"
#include "rsx_panasonic.h"
#include "rsx_panasonic_dev.h"

namespace rsx {

namespace {

constexpr int PN_LAYOUTS = 5;

// pixels a packet: bitsPerPacket / bps for V5 and V7, BlockDsc::PixelsPerBlock for V6
__host__ __device__ constexpr int pn_pixels(int ver, int bps) {
  return ver == 6 ? (bps == 14 ? 11 : 14) : (bps == 14 ? 9 : 10);
}
// packets a lane takes: an item's values fill at most 20 KiB of LDS (8 workgroups a CU)
__host__ __device__ constexpr int pn_passes(int n) { return n == 9 ? 4 : (n == 14 ? 2 : 3); }
// 0..4: V5/12, V5/14, V6/12, V6/14, V7/14
constexpr int pn_layout(int ver, int bps) {
  return ver == 5 ? (bps == 12 ? 0 : 1) : (ver == 6 ? (bps == 12 ? 2 : 3) : 4);
}

struct PnItem {
  uint32_t job, first, count, pad; // packets [first, first + count) of the job
};

struct PnArgs {
  const uint8_t* in_base;
  uint8_t* out_base;
  const PnItem* items; // (of the launch's layout)
  const PnJobDev* jobs;
};

// the 16 bytes of packet p of a job; `aligned`: the job's input lies on the 16-byte grid (V5: 8)
template <int VER>
__device__ __forceinline__ void pn_load(const uint8_t* in, uint32_t p, bool aligned, uint32_t (&w)[4]) {
  if constexpr (VER == 5) {
    const uint8_t* blk = in + uint64_t(p >> 10) * PN_V5_BLOCK;
    const uint32_t q = 16u * (p & 1023u);
    pn_load8(blk + ((q + PN_V5_SPLIT) & (PN_V5_BLOCK - 1)), aligned, w[0], w[1]);
    pn_load8(blk + ((q + PN_V5_SPLIT + 8u) & (PN_V5_BLOCK - 1)), aligned, w[2], w[3]);
  } else {
    const uint8_t* src = in + 16ull * p;
    if (aligned) {
      const uint4 v = *reinterpret_cast<const uint4*>(src);
      w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    } else {
      pn_load8(src, false, w[0], w[1]);
      pn_load8(src + 8, false, w[2], w[3]);
    }
  }
}

// V5 and V7: pixel i = bits [BPS i, BPS i + BPS)
template <int BPS, int N, int I = 0>
__device__ __forceinline__ void pn_plain(const uint32_t (&w)[4], uint32_t (&px)[N]) {
  if constexpr (I < N) {
    px[I] = pn_bits<BPS * I, BPS>(w);
    pn_plain<BPS, N, I + 1>(w, px);
  }
}

// V6: entry K of pana_cs6_page_decoder's pixelbuffer (fillBuffer, :88-133), which nextpixel()
// hands out in the order 0, 1, 2, ..: 0 and 1 are the first pixels from the packet's top, then
// per triple a 2-bit scale and three FB-bit fields, each below the one before
template <int BPS, int K> __device__ __forceinline__ uint32_t pn_v6_entry(const uint32_t (&w)[4]) {
  constexpr int FB = BPS == 14 ? 10 : 8;
  if constexpr (K < 2) {
    return pn_bits<128 - BPS * (K + 1), BPS>(w);
  } else {
    constexpr int t = (K - 2) / 4, m = (K - 2) % 4;
    constexpr int top = 128 - 2 * BPS - t * (3 * FB + 2);
    if constexpr (m == 0)
      return pn_bits<top - 2, 2>(w);
    else
      return pn_bits<top - 2 - m * FB, FB>(w);
  }
}

// V6's state (decompressBlock, :185-219).  Per column parity: `seen` = oddeven[] != 0 (a
// non-zero field was met while it was 0), `nz` = nonzero[] -- which both branches leave equal
// to the pixel's value e.  The value stored is e - 15 (0 below 15: the `else` of the final
// test is only reached there, fields this narrow cannot push e past SpixCompare + 15 or past
// 16 bits -- 14 bits: at most 16383 + 5 * 2044, 12 bits: 4095 + 6 * 508; a scale of 16 adds
// nothing, since then pixel_base == PixelbaseCompare).
struct PnV6State {
  uint32_t seen[2], nz[2], shift, base;
};

template <int BPS, int N, int PIX = 0, int K = 0>
__device__ __forceinline__ void pn_v6(const uint32_t (&w)[4], PnV6State& S, uint32_t (&px)[N]) {
  if constexpr (PIX < N) {
    constexpr uint32_t ZERO = BPS == 14 ? 0x200u : 0x80u, CMP = BPS == 14 ? 0x2000u : 0x800u;
    constexpr uint32_t SPIX = BPS == 14 ? 0xFFFFu : 0x3FFFu;
    constexpr bool scale = PIX % 3 == 2;
    constexpr int p = PIX & 1;
    if constexpr (scale) {
      const uint32_t b = pn_v6_entry<BPS, K>(w);
      S.shift = b == 3u ? 4u : b;
      S.base = ZERO << S.shift;
    }
    const uint32_t f = pn_v6_entry<BPS, K + (scale ? 1 : 0)>(w);
    const uint32_t add = (S.base < CMP && S.nz[p] > S.base) ? S.nz[p] - S.base : 0u;
    const uint32_t later = (f << S.shift) + add; // (PIX < 2: never taken, seen is 0)
    const uint32_t first = f ? f : S.nz[p];
    const uint32_t e = S.seen[p] ? later : first;
    S.seen[p] |= f;
    S.nz[p] = e;
    px[PIX] = e >= 15u ? ((e - 15u) & SPIX) : 0u;
    pn_v6<BPS, N, PIX + 1, K + (scale ? 2 : 1)>(w, S, px);
  }
}

template <int VER, int BPS, int N>
__device__ __forceinline__ void pn_decode(const uint32_t (&w)[4], uint32_t (&px)[N]) {
  if constexpr (VER == 6) {
    PnV6State S{{0u, 0u}, {0u, 0u}, 0u, 0u};
    pn_v6<BPS, N>(w, S, px);
  } else {
    pn_plain<BPS, N>(w, px);
  }
}

// the lane's N values into the pass's run at value index o = t N: dwords, and for an odd N the
// value left over as a half (the first one where o is odd, the last one where it is even)
template <int N>
__device__ __forceinline__ void pn_stage(uint32_t* stage, uint32_t t, const uint32_t (&px)[N]) {
  const uint32_t o = t * uint32_t(N);
  if constexpr (N % 2 == 0) {
#pragma unroll
    for (int k = 0; k < N / 2; ++k)
      stage[(o >> 1) + k] = px[2 * k] | (px[2 * k + 1] << 16);
  } else {
    const bool odd = (t & 1u) != 0u;
    const uint32_t d0 = (o + 1u) >> 1;
#pragma unroll
    for (int k = 0; k < N / 2; ++k) {
      const uint32_t lo = odd ? px[2 * k + 1] : px[2 * k];
      const uint32_t hi = odd ? px[2 * k + 2] : px[2 * k + 1];
      stage[d0 + k] = lo | (hi << 16);
    }
    reinterpret_cast<uint16_t*>(stage)[odd ? o : o + uint32_t(N - 1)] = uint16_t(odd ? px[0] : px[N - 1]);
  }
}

template <int VER, int BPS>
__global__ void __launch_bounds__(PN_THREADS) panasonic_kernel(PnArgs A) {
  constexpr int N = pn_pixels(VER, BPS);
  constexpr int PN_PASSES = pn_passes(N);
  // the item's run, and one dword more: the fifth dword of the run's last piece
  __shared__ uint32_t stage[PN_THREADS * PN_PASSES * N / 2 + 4];
  static_assert(sizeof(stage) <= 20 * 1024, "8 workgroups a CU");
  const PnItem I = A.items[blockIdx.x];
  const PnJobDev J = A.jobs[I.job];
  const uint32_t tid = threadIdx.x;
  const uint8_t* in = A.in_base + J.in_off;
  const bool aligned = (reinterpret_cast<uintptr_t>(in) & (VER == 5 ? 7u : 15u)) == 0u;

  // 1. the loads of the lane's packets go out first
  uint32_t w[PN_PASSES][4];
#pragma unroll
  for (int k = 0; k < PN_PASSES; ++k) {
    const uint32_t t = tid + uint32_t(k) * PN_THREADS;
    w[k][0] = w[k][1] = w[k][2] = w[k][3] = 0u;
    if (t < I.count)
      pn_load<VER>(in, I.first + t, aligned, w[k]);
  }
  // 2. decode into the item's run
#pragma unroll
  for (int k = 0; k < PN_PASSES; ++k) {
    const uint32_t t = tid + uint32_t(k) * PN_THREADS;
    if (t < I.count) {
      uint32_t px[N];
      pn_decode<VER, BPS, N>(w[k], px);
      pn_stage<N>(stage, t, px);
    }
  }
  __syncthreads();
  // 3. the run out along the output's grid
  pn_store(stage, A.out_base + J.img_offset, J, I.first * uint32_t(N), I.count * uint32_t(N));
}

typedef void (*PnKernel)(PnArgs);
const PnKernel PN_KERNELS[PN_LAYOUTS] = {panasonic_kernel<5, 12>, panasonic_kernel<5, 14>,
                                         panasonic_kernel<6, 12>, panasonic_kernel<6, 14>,
                                         panasonic_kernel<7, 14>};

} // namespace

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
namespace {
struct PanasonicPlan final : DecoderPlan {
  rsx_ctx* ctx = nullptr;
  std::vector<PnJobDev> jobs;
  std::vector<int32_t> host_status; // validation result per job
  std::vector<uint32_t> consumed;   // input bytes a job takes (peekStream)
  DeviceBuffer d_jobs, d_items;
  uint32_t first[PN_LAYOUTS + 1] = {}; // the items of layout l: [first[l], first[l + 1])
  int run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) override;
  int results(hipStream_t s, bool ran, int32_t* job_status, uint32_t* job_consumed) override;
};
} // namespace

int panasonic_validate(const rsx_panasonic_desc* desc, const rsx_image& img, size_t in_bytes,
                       uint64_t* consumed) {
  if (consumed)
    *consumed = 0;
  if (!desc)
    return RSX_ERR_INVALID_ARG;
  // Rw2Decoder::decodeRawInternal (decoders/Rw2Decoder.cpp:138-175): the versions with a
  // decompressor here, and the bit depths it builds V6 and V7 with
  if (desc->version != 5 && desc->version != 6 && desc->version != 7)
    return RSX_ERR_INVALID_ARG; // (4: section 3j; others: "Version %i is unsupported")
  if (desc->version == 6 && desc->bps != 12 && desc->bps != 14)
    return RSX_ERR_INVALID_ARG; // :155-157
  if (desc->version == 7 && desc->bps != 14)
    return RSX_ERR_INVALID_ARG; // :165-167
  // the constructors (V5 :74-108, V6 :141-169, V7 :44-60), in their order
  if (img.cpp != 1)
    return RSX_ERR_INVALID_ARG; // "Unexpected component count / data type"
  if (desc->bps != 12 && desc->bps != 14)
    return RSX_ERR_INVALID_ARG; // "Unsupported bps"
  const int n = pn_pixels(desc->version, desc->bps);
  if (img.dim_x <= 0 || img.dim_y <= 0 || img.dim_x % n != 0)
    return RSX_ERR_INVALID_ARG; // "Unexpected image dimensions found"
  if (img.pitch_bytes < uint64_t(img.dim_x) * 2u)
    return RSX_ERR_INVALID_ARG;
  const uint64_t packets = uint64_t(img.dim_x) * uint64_t(img.dim_y) / uint64_t(n);
  // V5: whole blocks of 0x4000 bytes, the last one padded; V6, V7: the packets
  const uint64_t unit = desc->version == 5 ? PN_V5_BLOCK : 16u;
  const uint64_t units = desc->version == 5 ? (packets + PN_V5_PACKETS - 1) / PN_V5_PACKETS : packets;
  const uint64_t need = units * unit;
  if (need > 0xFFFFFFFFull)
    return RSX_ERR_UNSUPPORTED; // (job_consumed has 32 bits)
  if (consumed)
    *consumed = need;
  if (uint64_t(in_bytes) / unit < units)
    return RSX_ERR_INVALID_ARG; // "Insufficient count of input blocks for a given image"
  return RSX_OK;
}

int panasonic_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_panasonic_job* jobs,
                          std::unique_ptr<DecoderPlan>* out) {
  auto p = std::make_unique<PanasonicPlan>();
  p->ctx = ctx;
  p->host_status.assign(n_jobs, RSX_OK);
  p->consumed.assign(n_jobs, 0);
  p->jobs.resize(n_jobs);
  std::vector<PnItem> items[PN_LAYOUTS];
  for (int i = 0; i < n_jobs; ++i) {
    const rsx_panasonic_job& j = jobs[i];
    PnJobDev& J = p->jobs[i];
    std::memset(&J, 0, sizeof J);
    uint64_t need = 0;
    int st = panasonic_validate(&j.desc, j.img, size_t(j.in_bytes), &need);
    if (st == RSX_OK) // (also for a job the alignment check below turns down)
      p->consumed[i] = uint32_t(need);
    if (st == RSX_OK && (j.img_offset % 2 != 0 || j.img.pitch_bytes % 2 != 0))
      st = RSX_ERR_INVALID_ARG;
    p->host_status[i] = st;
    if (st != RSX_OK)
      continue;
    J.in_off = j.in_offset;
    J.img_offset = j.img_offset;
    J.pitch = j.img.pitch_bytes;
    J.width = uint32_t(j.img.dim_x);
    const int n = pn_pixels(j.desc.version, j.desc.bps);
    const uint32_t packets = uint32_t(uint64_t(j.img.dim_x) * uint64_t(j.img.dim_y) / uint64_t(n));
    std::vector<PnItem>& its = items[pn_layout(j.desc.version, j.desc.bps)];
    const uint32_t per = uint32_t(PN_THREADS * pn_passes(n)); // packets an item
    for (uint32_t f = 0; f < packets; f += per)
      its.push_back(PnItem{uint32_t(i), f, std::min(per, packets - f), 0});
  }
  std::vector<PnItem> all;
  for (int l = 0; l < PN_LAYOUTS; ++l) {
    p->first[l] = uint32_t(all.size());
    all.insert(all.end(), items[l].begin(), items[l].end());
  }
  p->first[PN_LAYOUTS] = uint32_t(all.size());
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int st;
  if ((st = upload(ctx, p->d_jobs, p->jobs)) || (st = upload(ctx, p->d_items, all)))
    return st;
  *out = std::move(p);
  return RSX_OK;
}

int PanasonicPlan::run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) {
  if (first[PN_LAYOUTS] == 0)
    return RSX_OK; // (every job was rejected by the host)
  PnArgs A{};
  A.in_base = static_cast<const uint8_t*>(in_dev);
  A.out_base = static_cast<uint8_t*>(out_dev);
  A.jobs = static_cast<const PnJobDev*>(d_jobs.ptr);
  if (timer)
    timer->begin(s);
  // one launch per layout the plan holds (they write disjoint images)
  for (int l = 0; l < PN_LAYOUTS; ++l) {
    const uint32_t n = first[l + 1] - first[l];
    if (n == 0)
      continue;
    A.items = static_cast<const PnItem*>(d_items.ptr) + first[l];
    hipLaunchKernelGGL(PN_KERNELS[l], dim3(n), dim3(PN_THREADS), 0, s, A);
  }
  if (timer)
    timer->mark("panasonic_kernel");
  RSX_HIP_CHECK(ctx, hipGetLastError());
  return RSX_OK;
}

int PanasonicPlan::results(hipStream_t s, bool ran, int32_t* job_status, uint32_t* job_consumed) {
  if (job_consumed)
    std::copy(consumed.begin(), consumed.end(), job_consumed);
  if (ran && first[PN_LAYOUTS] != 0)
    RSX_HIP_CHECK(ctx, hipStreamSynchronize(s));
  return fold_jobs(jobs.size(), FoldOrder::LAST_FAILING, job_status,
                   [&](size_t i) { return int(host_status[i]); });
}

} // namespace rsx
