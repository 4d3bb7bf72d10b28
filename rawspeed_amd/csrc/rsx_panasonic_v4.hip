// PanasonicV4Decompressor on the device (include/rsx.h section 3l).
//
// What the reference does (decompressors/PanasonicV4Decompressor.cpp): the input is cut into
// blocks of 0x4000 bytes = 1024 packets of 16 bytes (section_split_offset 0: the last block may
// be partial), and a block is rotated before it is read (ProxyStream, :129-171): its bytes
// [split, 0x4000) come first.  getBits walks from the top of the rotated block's packet q =
// its bytes [16 q, 16 q + 16), one 128-bit little-endian number, from bit 128 down; a packet
// holds 14 pixels of one row and always takes exactly its 128 bits (processPixelPacket,
// :173-218): per pixel 8 bits, in front of the pixels 2, 5, 8 and 11 a 2-bit scale, and per
// column parity ONE 4-bit field, behind the first non-zero 8-bit field of the parity or, where
// there was none, behind the parity's last pixel (12 resp. 13).  So a field's position is the
// one it has without the 4-bit fields, lowered by 4 k for the k = 0, 1, 2 of them read before.
// Per parity: pred, nonz; the stored pixel is uint16(pred), and pred stays in 0 .. 16287.
// With zero_is_bad every pixel with pred == 0 goes into mRaw->mBadPixelPositions as
// row << 16 | col.  No packet depends on another, and nothing in the data can fail.
//
//   panasonic_v4_kernel   one workgroup of 256 lanes per item = 512 consecutive packets of one
//       job (14 KiB of pixels in LDS); one lane per packet, two packets a lane:
//       1. every lane issues the loads of its packets: one 16-byte load each; split 0x1FF8:
//          packet q of a block starts at its byte (16 q + 0x1FF8) mod 0x4000 -- 8-byte aligned,
//          and packet 512 wraps (two 8-byte halves); an input off the grid: dwords shifted
//          together;
//       2. a lane decodes its packets from registers: every field is a 16-bit (10-bit) window
//          at a constant position, shifted by 8 - 4 k; pred and nonz per parity are scalars.
//          It notes its zero pixels in a 14-bit mask and writes the pixels into the item's run
//          in LDS; the zero counts are summed per wave; ONE barrier;
//       3. the workgroup writes the run out along the 16-byte grid of the OUTPUT (pn_store);
//       4. only a workgroup that met zeros (zero_is_bad): one atomic add on the job's counter
//          takes its slice of the job's list -- issued in front of step 3's stores, read behind
//          them --, a second barrier hands the slice's start round, and the lanes write their
//          entries while they lie inside bad_cap.  The counter goes on counting past bad_cap.
// The counters are cleared on the run's stream in front of every launch; the host sorts a
// job's list after the download (rsx_plan_results).
// Bit-exact against the model tests/rw2_v4_files.py, which tests/test_panasonic_v4_model.py
// holds against the reference's whole-file decode.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "rsx_internal.h"
#include "rsx_ljpeg_dev.h"
#include "rsx_plan_host.h"
#include "rsx_panasonic_dev.h"
#include "rsx_panasonic_v4.h"

namespace rsx {

namespace {

constexpr int P4_N = 14;     // PixelsPerPacket
constexpr int P4_PASSES = 2; // packets a lane
constexpr int P4_WAVES = PN_THREADS / 64;
constexpr uint32_t P4_PER_ITEM = uint32_t(PN_THREADS * P4_PASSES);
// the item's run, and one dword more (the fifth dword of the run's last piece)
constexpr uint32_t P4_STAGE = P4_PER_ITEM * P4_N / 2 + 4;
constexpr uint32_t P4_FLAG_SPLIT = 1u, P4_FLAG_ZERO = 2u;

struct P4JobDev {
  PnJobDev g;
  uint64_t bad_base; // the job's first entry in the plan's list buffer
  uint32_t bad_cap;  // entries the job's list holds
  uint32_t flags;    // P4_FLAG_SPLIT: section_split_offset 0x1FF8 (else 0); P4_FLAG_ZERO: zero_is_bad
};

struct P4Item {
  uint32_t job, first, count, pad; // packets [first, first + count) of the job
};

struct P4Args {
  const uint8_t* in_base;
  uint8_t* out_base;
  const P4Item* items;
  const P4JobDev* jobs;
  uint32_t* counts; // [job]: zero pixels met (cleared in front of every launch)
  uint32_t* lists;
};

typedef uint32_t p4_u32x4_a8 __attribute__((ext_vector_type(4), aligned(8)));

// the 16 bytes of packet p of a job; `aligned`: the job's input lies on the 16-byte grid (the
// 8-byte grid with a split)
__device__ __forceinline__ void p4_load(const uint8_t* in, uint32_t p, bool split, bool aligned,
                                        uint32_t (&w)[4]) {
  if (split) {
    const uint8_t* blk = in + uint64_t(p >> 10) * PN_V5_BLOCK;
    const uint32_t a = (16u * (p & 1023u) + PN_V5_SPLIT) & (PN_V5_BLOCK - 1);
    if (aligned && a != PN_V5_BLOCK - 8u) {
      const p4_u32x4_a8 v = *reinterpret_cast<const p4_u32x4_a8*>(blk + a);
      w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    } else {
      pn_load8(blk + a, aligned, w[0], w[1]);
      pn_load8(blk + ((a + 8u) & (PN_V5_BLOCK - 1)), aligned, w[2], w[3]);
    }
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

// processPixelPacket's state (:178-186); s8 = 8 - 4 k for the k 4-bit fields read so far
struct P4State {
  int32_t pred[2];
  uint32_t nonz[2], sh, s8, zeros;
};

// pixel P of the packet (:188-217).  T = the bits in front of its 8-bit field without the 4-bit
// fields; the window holds the field for every k, and the 4-bit field behind it for k <= 1 (a
// parity that has not read its own yet)
template <int P = 0>
__device__ __forceinline__ void p4_pixels(const uint32_t (&w)[4], P4State& S, uint32_t (&px)[P4_N]) {
  if constexpr (P < P4_N) {
    constexpr int c = P & 1;
    constexpr int T = 8 * P + 2 * ((P + 1) / 3);
    if constexpr (P % 3 == 2) {
      const uint32_t b = (pn_bits<128 - T - 8, 10>(w) >> S.s8) & 3u;
      S.sh = b == 3u ? 4u : b; // extractHighBits(4U, b, 3) = 4 >> (3 - b)
    }
    const uint32_t win = pn_bits<128 - T - 16, 16>(w);
    const uint32_t f = (win >> S.s8) & 0xFFu;
    const uint32_t f4 = (win >> ((S.s8 - 4u) & 31u)) & 0xFu; // (read only while s8 >= 4)
    const bool seen = S.nonz[c] != 0u;
    // nonz[c]: j = f
    int32_t t = S.pred[c] - int32_t(0x80u << S.sh);
    if (t < 0 || S.sh == 4u)
      t &= int32_t((1u << S.sh) - 1u);
    t += int32_t(f << S.sh);
    const int32_t later = f ? t : S.pred[c];
    // else: nonz[c] = f, and the 4-bit field for a non-zero f or behind the parity's last pixel
    const bool take = f != 0u || P > 11;
    const int32_t first = take ? int32_t((f << 4) | f4) : S.pred[c];
    S.pred[c] = seen ? later : first;
    S.s8 -= (!seen && take) ? 4u : 0u;
    S.nonz[c] = seen ? S.nonz[c] : f;
    px[P] = uint32_t(S.pred[c]) & 0xFFFFu;
    S.zeros |= uint32_t(S.pred[c] == 0) << P;
    p4_pixels<P + 1>(w, S, px);
  }
}

__global__ void __launch_bounds__(PN_THREADS) panasonic_v4_kernel(P4Args A) {
  // the run; behind it the waves' zero counts and the start of the workgroup's slice
  __shared__ uint32_t stage[P4_STAGE + P4_WAVES + 1];
  static_assert(sizeof(stage) <= 20 * 1024, "8 workgroups a CU");
  const P4Item I = A.items[blockIdx.x];
  const P4JobDev J = A.jobs[I.job];
  const uint32_t tid = threadIdx.x;
  const uint8_t* in = A.in_base + J.g.in_off;
  const bool split = (J.flags & P4_FLAG_SPLIT) != 0u;
  const bool collect = (J.flags & P4_FLAG_ZERO) != 0u;
  const bool aligned = (reinterpret_cast<uintptr_t>(in) & (split ? 7u : 15u)) == 0u;

  // 1. the loads of the lane's packets go out first
  uint32_t w[P4_PASSES][4];
#pragma unroll
  for (int k = 0; k < P4_PASSES; ++k) {
    const uint32_t t = tid + uint32_t(k) * PN_THREADS;
    w[k][0] = w[k][1] = w[k][2] = w[k][3] = 0u;
    if (t < I.count)
      p4_load(in, I.first + t, split, aligned, w[k]);
  }
  // 2. decode into the item's run
  uint32_t zm[P4_PASSES];
#pragma unroll
  for (int k = 0; k < P4_PASSES; ++k) {
    const uint32_t t = tid + uint32_t(k) * PN_THREADS;
    zm[k] = 0u;
    if (t < I.count) {
      uint32_t px[P4_N];
      P4State S{{0, 0}, {0u, 0u}, 0u, 8u, 0u};
      p4_pixels(w[k], S, px);
      zm[k] = S.zeros;
#pragma unroll
      for (int i = 0; i < P4_N / 2; ++i)
        stage[t * uint32_t(P4_N / 2) + i] = px[2 * i] | (px[2 * i + 1] << 16);
    }
  }
  // the lane's zeros, and the count of the lanes below it in its wave (waves without a zero skip the scan)
  uint32_t cnt = 0u, incl = 0u;
  if (collect) {
    cnt = uint32_t(__popc(zm[0]) + __popc(zm[1]));
    if (__ballot(cnt != 0u) != 0ull) {
      const uint32_t lane = tid & 63u;
      incl = cnt;
#pragma unroll
      for (uint32_t d = 1; d < 64u; d *= 2u) {
        const uint32_t v = uint32_t(__shfl_up(int(incl), d, 64));
        incl += lane >= d ? v : 0u;
      }
    }
    if ((tid & 63u) == 63u)
      stage[P4_STAGE + (tid >> 6)] = incl;
  }
  __syncthreads();
  // 4a. a workgroup that met zeros takes its slice of the job's list (uniform over the
  // workgroup: the flag and the waves' counts).  The atomic goes out in front of the stores of
  // step 3: every workgroup of a job adds to one address, and the answer takes its time
  uint32_t below = 0u, total = 0u, slice = 0u;
  if (collect) {
#pragma unroll
    for (uint32_t v = 0; v < uint32_t(P4_WAVES); ++v) {
      const uint32_t c = stage[P4_STAGE + v];
      below += v < (tid >> 6) ? c : 0u;
      total += c;
    }
    if (total != 0u && tid == 0u)
      slice = atomicAdd(A.counts + I.job, total);
  }
  // 3. the run out along the output's grid
  pn_store(stage, A.out_base + J.g.img_offset, J.g, I.first * uint32_t(P4_N), I.count * uint32_t(P4_N));
  // 4b. the entries
  if (total == 0u)
    return;
  if (tid == 0u)
    stage[P4_STAGE + P4_WAVES] = slice;
  __syncthreads();
  uint32_t idx = stage[P4_STAGE + P4_WAVES] + below + incl - cnt;
  uint32_t* list = A.lists + J.bad_base;
#pragma unroll
  for (int k = 0; k < P4_PASSES; ++k) {
    // (a packet's pixels lie in one row: width % 14 == 0)
    const uint32_t P0 = (I.first + tid + uint32_t(k) * PN_THREADS) * uint32_t(P4_N);
    const uint32_t row = P0 / J.g.width, col = P0 - row * J.g.width;
    for (uint32_t m = zm[k]; m != 0u; m &= m - 1u, ++idx)
      if (idx < J.bad_cap)
        list[idx] = (row << 16) | (col + uint32_t(__ffs(int(m)) - 1));
  }
}

} // namespace

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
namespace {
struct P4Plan final : DecoderPlan {
  rsx_ctx* ctx = nullptr;
  std::vector<P4JobDev> jobs;
  std::vector<int32_t> host_status; // validation result per job
  std::vector<uint32_t> consumed;   // input bytes a job takes (peekStream)
  DeviceBuffer d_jobs, d_items, d_counts, d_lists;
  std::vector<uint32_t> h_counts;            // of the last run, after results
  std::vector<std::vector<uint32_t>> h_lists; // ... and the jobs' sorted lists
  uint32_t n_items = 0;
  bool have_lists = false;
  int run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) override;
  int results(hipStream_t s, bool ran, int32_t* job_status, uint32_t* job_consumed) override;
  int bad_pixels(int job, uint32_t* out, uint32_t cap, uint64_t* n_bad) override;
};
} // namespace

int panasonic_v4_validate(const rsx_panasonic_v4_desc* desc, const rsx_image& img, size_t in_bytes,
                          uint64_t* consumed) {
  if (consumed)
    *consumed = 0;
  if (!desc)
    return RSX_ERR_INVALID_ARG;
  // the constructor (PanasonicV4Decompressor.cpp:49-86), in its order
  if (img.cpp != 1)
    return RSX_ERR_INVALID_ARG; // "Unexpected component count / data type"
  if (img.dim_x <= 0 || img.dim_y <= 0 || img.dim_x % P4_N != 0)
    return RSX_ERR_INVALID_ARG; // "Unexpected image dimensions found"
  if (img.pitch_bytes < uint64_t(img.dim_x) * 2u)
    return RSX_ERR_INVALID_ARG;
  if (desc->section_split_offset > PN_V5_BLOCK)
    return RSX_ERR_INVALID_ARG; // "Bad section_split_offset"
  const uint64_t total = uint64_t(img.dim_x) * uint64_t(img.dim_y) / uint64_t(P4_N) * 16u;
  const uint64_t need = desc->section_split_offset == 0
                            ? total
                            : (total + PN_V5_BLOCK - 1) / PN_V5_BLOCK * PN_V5_BLOCK;
  if (need > 0xFFFFFFFFull)
    return RSX_ERR_INVALID_ARG; // "Raw dimensions require input buffer larger than supported"
  if (consumed)
    *consumed = need;
  if (uint64_t(in_bytes) < need)
    return RSX_ERR_IO; // input_.peekStream(bufSize)
  // what Rw2Decoder passes (decoders/Rw2Decoder.cpp:116-120, :140-146); nothing else is tested
  if (desc->section_split_offset != 0 && desc->section_split_offset != PN_V5_SPLIT)
    return RSX_ERR_UNSUPPORTED;
  return RSX_OK;
}

int panasonic_v4_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_panasonic_v4_job* jobs,
                             std::unique_ptr<DecoderPlan>* out) {
  auto p = std::make_unique<P4Plan>();
  p->ctx = ctx;
  p->host_status.assign(n_jobs, RSX_OK);
  p->consumed.assign(n_jobs, 0);
  p->jobs.resize(n_jobs);
  p->h_counts.assign(n_jobs, 0);
  p->h_lists.resize(n_jobs);
  std::vector<P4Item> items;
  uint64_t entries = 0;
  for (int i = 0; i < n_jobs; ++i) {
    const rsx_panasonic_v4_job& j = jobs[i];
    P4JobDev& J = p->jobs[i];
    std::memset(&J, 0, sizeof J);
    uint64_t need = 0;
    int st = panasonic_v4_validate(&j.desc, j.img, size_t(j.in_bytes), &need);
    if (st == RSX_OK) // (also for a job the alignment check below turns down)
      p->consumed[i] = uint32_t(need);
    if (st == RSX_OK && (j.img_offset % 2 != 0 || j.img.pitch_bytes % 2 != 0))
      st = RSX_ERR_INVALID_ARG;
    p->host_status[i] = st;
    if (st != RSX_OK)
      continue;
    const uint64_t area = uint64_t(j.img.dim_x) * uint64_t(j.img.dim_y); // (< 2^32: need fits 32 bits)
    J.g.in_off = j.in_offset;
    J.g.img_offset = j.img_offset;
    J.g.pitch = j.img.pitch_bytes;
    J.g.width = uint32_t(j.img.dim_x);
    J.flags = (j.desc.section_split_offset ? P4_FLAG_SPLIT : 0u) | (j.desc.zero_is_bad ? P4_FLAG_ZERO : 0u);
    // (an image has no more zero pixels than pixels: a larger capacity needs no memory)
    J.bad_cap = j.desc.zero_is_bad ? uint32_t(std::min<uint64_t>(j.bad_cap, area)) : 0u;
    J.bad_base = entries;
    entries += J.bad_cap;
    const uint32_t packets = uint32_t(area / uint64_t(P4_N));
    for (uint32_t f = 0; f < packets; f += P4_PER_ITEM)
      items.push_back(P4Item{uint32_t(i), f, std::min(P4_PER_ITEM, packets - f), 0});
  }
  p->n_items = uint32_t(items.size());
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int st;
  if ((st = upload(ctx, p->d_jobs, p->jobs)) || (st = upload(ctx, p->d_items, items)) ||
      (st = p->d_counts.ensure(size_t(n_jobs) * 4 + 16)) ||
      (st = p->d_lists.ensure(size_t(entries) * 4 + 16)))
    return st;
  *out = std::move(p);
  return RSX_OK;
}

int P4Plan::run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) {
  have_lists = false;
  if (n_items == 0)
    return RSX_OK; // (every job was rejected by the host)
  P4Args A{};
  A.in_base = static_cast<const uint8_t*>(in_dev);
  A.out_base = static_cast<uint8_t*>(out_dev);
  A.items = static_cast<const P4Item*>(d_items.ptr);
  A.jobs = static_cast<const P4JobDev*>(d_jobs.ptr);
  A.counts = static_cast<uint32_t*>(d_counts.ptr);
  A.lists = static_cast<uint32_t*>(d_lists.ptr);
  // every run counts from zero: cleared on the stream of the kernel that adds to them
  RSX_HIP_CHECK(ctx, hipMemsetAsync(d_counts.ptr, 0, jobs.size() * 4, s));
  if (timer)
    timer->begin(s);
  hipLaunchKernelGGL(panasonic_v4_kernel, dim3(n_items), dim3(PN_THREADS), 0, s, A);
  if (timer)
    timer->mark("panasonic_v4_kernel");
  RSX_HIP_CHECK(ctx, hipGetLastError());
  return RSX_OK;
}

int P4Plan::results(hipStream_t s, bool ran, int32_t* job_status, uint32_t* job_consumed) {
  if (job_consumed)
    std::copy(consumed.begin(), consumed.end(), job_consumed);
  std::fill(h_counts.begin(), h_counts.end(), 0u);
  for (std::vector<uint32_t>& l : h_lists)
    l.clear();
  if (ran && n_items != 0) {
    if (int st = fetch_words(ctx, s, d_counts, 0, h_counts.size(), h_counts.data()))
      return st;
    // the lists that fit, in the reference's single-thread order
    for (size_t i = 0; i < jobs.size(); ++i) {
      if (host_status[i] != RSX_OK || h_counts[i] == 0 || h_counts[i] > jobs[i].bad_cap)
        continue;
      h_lists[i].resize(h_counts[i]);
      RSX_HIP_CHECK(ctx, hipMemcpyAsync(h_lists[i].data(),
                                        static_cast<const uint32_t*>(d_lists.ptr) + jobs[i].bad_base,
                                        size_t(h_counts[i]) * 4, hipMemcpyDeviceToHost, s));
    }
    RSX_HIP_CHECK(ctx, hipStreamSynchronize(s));
    for (std::vector<uint32_t>& l : h_lists)
      std::sort(l.begin(), l.end());
    have_lists = true;
  }
  return fold_jobs(jobs.size(), FoldOrder::LAST_FAILING, job_status, [&](size_t i) {
    // (the image is complete; the list did not fit)
    return host_status[i] == RSX_OK && h_counts[i] > jobs[i].bad_cap ? int(RSX_ERR_UNSUPPORTED)
                                                                     : int(host_status[i]);
  });
}

int P4Plan::bad_pixels(int job, uint32_t* out, uint32_t cap, uint64_t* n_bad) {
  if (n_bad)
    *n_bad = 0;
  if (job < 0 || size_t(job) >= jobs.size() || !have_lists || host_status[job] != RSX_OK)
    return RSX_ERR_INVALID_ARG;
  const uint32_t n = h_counts[job];
  if (n_bad)
    *n_bad = n;
  if (n > jobs[job].bad_cap || n > cap)
    return RSX_ERR_UNSUPPORTED;
  if (n != 0 && !out)
    return RSX_ERR_INVALID_ARG;
  std::copy(h_lists[job].begin(), h_lists[job].end(), out);
  return RSX_OK;
}

} // namespace rsx
