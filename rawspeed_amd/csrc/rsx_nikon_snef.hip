// NefDecoder::DecodeNikonSNef on the device (include/rsx.h section 3m).
//
// What the reference does (decoders/NefDecoder.cpp:707-792): row y of a W-pixel image is exactly
// the bytes [3 W y, 3 W (y + 1)); its first three bytes seed the dither generator.  A group of
// six bytes is four 12-bit fields, LSB first: y1, y2, cb, cr -- two pixels that share one chroma
// sample.  The second pixel takes the mean of its group's chroma and the next group's (in
// binary32, exact; the last group of a row has no neighbour), 2048 comes off all four, and
//   e0 = y + 1.370705 cr,  e1 = (y - 0.337633 cb) - 0.698001 cr,  e2 = y + 1.732446 cb
// are evaluated in binary64 with every product and every sum rounded (the reference's build has
// no FMA), truncated, clamped to 12 bits and stored through the dithering TableLookUp
// (setWithLookUp, common/RawImage.h:335-353), one generator step per sample in output order;
// red and blue then lose the white balance again: min(32767, (inv_wb t + 512) >> 10).
// Nothing depends on another group, save the generator (rsx_dither_dev.h: the state in front of
// sample n is the seed times 15700^n mod m) and the neighbour's chroma, which a lane reads.
//
//   nikon_snef_kernel  one workgroup of 256 lanes per item (up to 1024 runs of one job); a run
//                      is four groups of one row (the last run of a row: what is left): 24
//                      bytes in, 48 bytes out.  A lane has two runs in flight, an item takes two
//                      such rounds:
//                      1. every lane issues the loads of its runs -- the 30 bytes of the run
//                         and of the next group's chroma, as the dwords that hold them (input
//                         rows start at any byte; no dword without a byte of the job is
//                         touched) -- and of the rows' seed bytes;
//                      2. in the first round the job's table -> LDS, meanwhile (4096 x u32
//                         base | delta << 16: TableLookUp's own layout);
//                      3. a lane jumps the generator to its first sample (24 run), decodes its
//                         groups in order and stores three 16-byte vectors where the image
//                         lies on the 16-byte grid (dwords, or halves, otherwise).
// This translation unit is compiled without floating-point contraction: a fused e1 differs
// from the reference for 34 chroma pairs (tests/test_snef_model.py plants them;
// tests/test_snef_build.py looks for v_fma_f64).
// Registers: 61 VGPRs, no scratch, 16 KiB of LDS: 8 waves a SIMD, 8 workgroups a CU
// (tests/test_snef_build.py holds the kernel to 64 VGPRs; four runs in flight took 76).
// Bit-exact against the model tests/snef_files.py, which tests/test_snef_model.py holds against
// the reference's whole-file decode.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "rsx_dither_dev.h"
#include "rsx_internal.h"
#include "rsx_ljpeg_dev.h"
#include "rsx_plan_host.h"
#include "rsx_nikon_snef.h"

#pragma clang fp contract(off)

namespace rsx {

namespace {

constexpr int SN_THREADS = 256;
constexpr int SN_PER_LANE = 2;                               // runs a lane has in flight
constexpr int SN_ROUNDS = 2;                                 // rounds of them an item
constexpr uint32_t SN_RUN = 4;                               // groups a run
constexpr uint32_t SN_ITEM_RUNS = SN_THREADS * SN_PER_LANE * SN_ROUNDS; // runs an item (at most)
constexpr int32_t SN_MAX_W = 3680, SN_MAX_H = 2456;          // NefDecoder.cpp:389-391
constexpr uint32_t SN_MAX_RUNS = (SN_MAX_W / 2 + SN_RUN - 1) / SN_RUN; // runs a row (at most)
constexpr uint32_t SN_LUT = 4096;                            // table entries: v = 0 .. 4095
// int(1024.0F / wb) for the wb NefDecoder.cpp:682-687 lets through: wb <= 10.0F gives
// int(102.4F) = 102; wb >= float(13421568.0 / 429496627.0) = 0.03124953 gives
// int(32768.492F) = 32768, and 32768 * 65535 + 512 = 2147451904 still fits an int
constexpr int32_t SN_INV_WB_MIN = 102, SN_INV_WB_MAX = 32768;

struct SnJobDev {
  uint64_t in_off;     // first byte of row 0 in the plan's input
  uint64_t img_offset; // first byte of the image in the plan's output
  uint32_t pitch, width;
  uint32_t groups;     // groups a row: width / 2
  uint32_t rpr;        // runs a row: ceil(groups / 4)
  uint32_t in_len;     // bytes the job reads: 3 width height
  uint32_t table;      // first entry of the job's table in tables[]
  uint32_t inv_wb_r, inv_wb_b;
};

struct SnItem {
  uint32_t job, first, count, pad; // runs [first, first + count) of the job, row-major
};

struct SnArgs {
  const uint8_t* in_base;
  uint8_t* out_base;
  const SnItem* items;
  const SnJobDev* jobs;
  const uint32_t* tables; // [job's table][v]: base | delta << 16
  const uint32_t* pow24;  // [run]: 15700^(24 run) mod m
};

typedef uint32_t sn_u32x4 __attribute__((ext_vector_type(4), aligned(4)));

// The 32 bytes at `p` (any byte address), of which the caller uses the first 30 at most: the
// dwords that hold them, shifted together.  Only dwords that start in front of `end` (the end
// of the job's input) are loaded, so each holds a byte of the job; far enough from the end
// they are two 16-byte loads (dword-aligned) and the ninth dword when the shift needs it.
__device__ __forceinline__ void sn_load(const uint8_t* p, const uint8_t* end, uint32_t (&w)[8]) {
  // (pointer arithmetic, not an integer round trip: the loads stay global ones)
  const uint32_t s = uint32_t(reinterpret_cast<uintptr_t>(p) & 3u);
  const uint32_t* d = reinterpret_cast<const uint32_t*>(p - s);
  const uintptr_t lim = reinterpret_cast<uintptr_t>(end);
  uint32_t x[9];
  if (reinterpret_cast<uintptr_t>(d) + 36u <= lim) {
    const sn_u32x4 v0 = *reinterpret_cast<const sn_u32x4*>(d);
    const sn_u32x4 v1 = *reinterpret_cast<const sn_u32x4*>(d + 4);
    x[0] = v0.x, x[1] = v0.y, x[2] = v0.z, x[3] = v0.w;
    x[4] = v1.x, x[5] = v1.y, x[6] = v1.z, x[7] = v1.w;
    x[8] = s == 3u ? d[8] : 0u;
  } else {
#pragma unroll
    for (int k = 0; k < 9; ++k)
      x[k] = reinterpret_cast<uintptr_t>(d + k) < lim && (k < 8 || s == 3u) ? d[k] : 0u;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k)
    w[k] = __builtin_amdgcn_alignbyte(x[k + 1], x[k], s);
}

// the 12-bit field F of the run (bits 12 F of its bytes; F is a constant after unrolling)
template <int F> __device__ __forceinline__ int32_t sn_field(const uint32_t (&w)[8]) {
  constexpr int q = 12 * F, lo = q >> 5, s = q & 31;
  if constexpr (s <= 20)
    return int32_t((w[lo] >> s) & 0xFFFu);
  else
    return int32_t(__builtin_amdgcn_alignbit(w[lo + 1], w[lo], s) & 0xFFFu);
}

__device__ __forceinline__ uint32_t sn_clamp12(int32_t v) { return uint32_t(min(max(v, 0), 4095)); }

// One pixel: the three table look-ups in output order and the white balance taken off red and
// blue.  cb and cr are whole or half numbers; every operation below rounds on its own.
__device__ __forceinline__ void sn_pixel(double y, double cb, double cr, const uint32_t* lut,
                                         uint32_t& r, uint32_t inv_r, uint32_t inv_b,
                                         uint32_t (&t)[3]) {
  const double pr = 1.370705 * cr;
  const double pg1 = 0.337633 * cb;
  const double pg2 = 0.698001 * cr;
  const double pb = 1.732446 * cb;
  const uint32_t v0 = sn_clamp12(int32_t(y + pr));
  const uint32_t v1 = sn_clamp12(int32_t((y - pg1) - pg2));
  const uint32_t v2 = sn_clamp12(int32_t(y + pb));
  const uint32_t t0 = dither_lookup(lut[v0], r);
  const uint32_t t1 = dither_lookup(lut[v1], r);
  const uint32_t t2 = dither_lookup(lut[v2], r);
  t[0] = min(32767u, (inv_r * t0 + 512u) >> 10);
  t[1] = t1;
  t[2] = min(32767u, (inv_b * t2 + 512u) >> 10);
}

// Group G of a run: six samples, two a word.  `last`: the row's last group (no neighbour).
template <int G>
__device__ __forceinline__ void sn_group(const uint32_t (&w)[8], bool last, const uint32_t* lut,
                                         uint32_t& r, uint32_t inv_r, uint32_t inv_b,
                                         uint32_t (&o)[3]) {
  const int32_t y1 = sn_field<4 * G>(w), y2 = sn_field<4 * G + 1>(w);
  const int32_t cb = sn_field<4 * G + 2>(w), cr = sn_field<4 * G + 3>(w);
  const int32_t cbn = sn_field<4 * G + 6>(w), crn = sn_field<4 * G + 7>(w);
  const double dcb = double(cb - 2048), dcr = double(cr - 2048);
  // (float(next) + float(this)) * 0.5F - 2048: a multiple of 1/2 below 2^12, exact either way
  const double dcb2 = last ? dcb : double(cbn + cb - 4096) * 0.5;
  const double dcr2 = last ? dcr : double(crn + cr - 4096) * 0.5;
  uint32_t p[3], q[3];
  sn_pixel(double(y1), dcb, dcr, lut, r, inv_r, inv_b, p);
  sn_pixel(double(y2), dcb2, dcr2, lut, r, inv_r, inv_b, q);
  o[0] = p[0] | (p[1] << 16);
  o[1] = p[2] | (q[0] << 16);
  o[2] = q[1] | (q[2] << 16);
}

__global__ void __launch_bounds__(SN_THREADS, 8) nikon_snef_kernel(SnArgs A) {
  __shared__ uint32_t lut[SN_LUT];
  const SnItem I = A.items[blockIdx.x];
  const SnJobDev J = A.jobs[I.job];
  const int tid = threadIdx.x;
  const uint8_t* in = A.in_base + J.in_off;
  const uint8_t* end = in + J.in_len;
  uint8_t* out = A.out_base + J.img_offset;
  const bool out16 = ((reinterpret_cast<uintptr_t>(out) | J.pitch) & 15u) == 0u;
  const bool out4 = ((reinterpret_cast<uintptr_t>(out) | J.pitch) & 3u) == 0u;

#pragma unroll 1
  for (uint32_t base = 0; base < I.count; base += SN_THREADS * SN_PER_LANE) {
    // 1. the loads of the lane's runs (and seeds) go out first
    uint32_t w[SN_PER_LANE][8];
    uint32_t row[SN_PER_LANE], run[SN_PER_LANE], seed[SN_PER_LANE], pw[SN_PER_LANE];
#pragma unroll
    for (int k = 0; k < SN_PER_LANE; ++k) {
      const uint32_t t = base + uint32_t(tid) + uint32_t(k) * SN_THREADS;
      row[k] = run[k] = seed[k] = pw[k] = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        w[k][j] = 0;
      if (t < I.count) {
        const uint32_t u = I.first + t;
        row[k] = u / J.rpr;
        run[k] = u - row[k] * J.rpr;
        const uint8_t* r0 = in + row[k] * (3u * J.width);
        sn_load(r0 + 6u * SN_RUN * run[k], end, w[k]);
        seed[k] = uint32_t(r0[0]) | (uint32_t(r0[1]) << 8) | (uint32_t(r0[2]) << 16);
        pw[k] = A.pow24[run[k]];
      }
    }
    // 2. the table -> LDS while the first ones are in flight
    if (base == 0) {
      const uint4* src = reinterpret_cast<const uint4*>(A.tables + J.table);
      for (uint32_t k = tid; k < SN_LUT / 4; k += SN_THREADS)
        reinterpret_cast<uint4*>(lut)[k] = src[k];
      __syncthreads();
    }

    // 3. decode the groups in order, store 48 bytes a run
#pragma unroll
    for (int k = 0; k < SN_PER_LANE; ++k) {
      const uint32_t t = base + uint32_t(tid) + uint32_t(k) * SN_THREADS;
      if (t >= I.count)
        continue;
      const uint32_t g0 = SN_RUN * run[k];           // the run's first group
      const uint32_t n = min(SN_RUN, J.groups - g0); // its groups
      uint32_t r = dither_jump(seed[k], pw[k]);
      uint32_t o[3 * SN_RUN];
#pragma unroll
      for (int j = 0; j < int(3 * SN_RUN); ++j)
        o[j] = 0;
#define SN_G(g)                                                                                \
  if (uint32_t(g) < n) {                                                                       \
    uint32_t og[3];                                                                            \
    sn_group<g>(w[k], g0 + uint32_t(g) + 1u == J.groups, lut, r, J.inv_wb_r, J.inv_wb_b, og); \
    o[3 * g] = og[0], o[3 * g + 1] = og[1], o[3 * g + 2] = og[2];                              \
  }
      SN_G(0) SN_G(1) SN_G(2) SN_G(3)
#undef SN_G
      uint8_t* dst = out + uint64_t(row[k]) * J.pitch + 12u * g0;
      const uint32_t nw = 3u * n; // words of the run that belong to the row
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        if (out16 && 4u * uint32_t(q) + 4u <= nw) {
          reinterpret_cast<uint4*>(dst)[q] =
              make_uint4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
          continue;
        }
#pragma unroll
        for (int j = 4 * q; j < 4 * q + 4; ++j) {
          if (uint32_t(j) >= nw)
            continue;
          if (out4) {
            reinterpret_cast<uint32_t*>(dst)[j] = o[j];
          } else {
            reinterpret_cast<uint16_t*>(dst)[2 * j] = uint16_t(o[j]);
            reinterpret_cast<uint16_t*>(dst)[2 * j + 1] = uint16_t(o[j] >> 16);
          }
        }
      }
    }
  }
}

// the device form of a table: [v] = base | delta << 16
void sn_lut(const rsx_nikon_snef_desc& d, uint32_t* out) {
  for (uint32_t v = 0; v < SN_LUT; ++v)
    out[v] = uint32_t(d.table[2 * v]) | (uint32_t(d.table[2 * v + 1]) << 16);
}

} // namespace

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
namespace {
struct NikonSnefPlan final : DecoderPlan {
  rsx_ctx* ctx = nullptr;
  std::vector<SnJobDev> jobs;
  std::vector<int32_t> host_status; // validation result per job
  std::vector<uint32_t> consumed;   // input bytes a job reads (3 w h when validated)
  std::vector<uint32_t> h_tables;   // device form of every job's table
  DeviceBuffer d_jobs, d_items, d_tables, d_pow;
  uint32_t n_items = 0;
  int run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) override;
  int results(hipStream_t s, bool ran, int32_t* job_status, uint32_t* job_consumed) override;
};
} // namespace

int nikon_snef_validate(const rsx_nikon_snef_desc* desc, const rsx_image& img, size_t in_bytes) {
  if (!desc || !desc->table)
    return RSX_ERR_INVALID_ARG;
  // DecodeSNefUncompressed, NefDecoder.cpp:389-396 (cpp 3)
  if (img.cpp != 3)
    return RSX_ERR_INVALID_ARG;
  if (img.dim_x <= 0 || img.dim_y <= 0 || img.dim_x % 2 != 0 || img.dim_x > SN_MAX_W ||
      img.dim_y > SN_MAX_H)
    return RSX_ERR_INVALID_ARG; // "Unexpected image dimensions found"
  if (img.pitch_bytes < uint32_t(img.dim_x) * 6u)
    return RSX_ERR_INVALID_ARG;
  // DecodeNikonSNef, :666-667
  if (img.dim_x < 6)
    return RSX_ERR_IO; // "got a %i wide sNEF, aborting"
  // :682-687 "Whitebalance has bad values", in terms of what :693-694 make of them
  for (const int32_t inv : {desc->inv_wb_r, desc->inv_wb_b})
    if (inv < SN_INV_WB_MIN || inv > SN_INV_WB_MAX)
      return RSX_ERR_INVALID_ARG;
  // input.peekData(3 w h), :711 (bytes behind them are not read)
  if (in_bytes < size_t(img.dim_x) * size_t(img.dim_y) * 3u)
    return RSX_ERR_IO;
  return RSX_OK;
}

int nikon_snef_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_nikon_snef_job* jobs,
                           std::unique_ptr<DecoderPlan>* out) {
  auto p = std::make_unique<NikonSnefPlan>();
  p->ctx = ctx;
  p->host_status.assign(n_jobs, RSX_OK);
  p->consumed.assign(n_jobs, 0);
  p->jobs.resize(n_jobs);
  std::vector<SnItem> items;
  for (int i = 0; i < n_jobs; ++i) {
    const rsx_nikon_snef_job& j = jobs[i];
    SnJobDev& J = p->jobs[i];
    std::memset(&J, 0, sizeof J);
    int st = nikon_snef_validate(&j.desc, j.img, size_t(j.in_bytes));
    if (st == RSX_OK) // (also for a job the alignment check below turns down)
      p->consumed[i] = uint32_t(j.img.dim_x) * uint32_t(j.img.dim_y) * 3u;
    if (st == RSX_OK && (j.img_offset % 2 != 0 || j.img.pitch_bytes % 2 != 0))
      st = RSX_ERR_INVALID_ARG;
    p->host_status[i] = st;
    if (st != RSX_OK)
      continue;
    J.in_off = j.in_offset;
    J.img_offset = j.img_offset;
    J.pitch = j.img.pitch_bytes;
    J.width = uint32_t(j.img.dim_x);
    J.groups = J.width / 2u;
    J.rpr = (J.groups + SN_RUN - 1u) / SN_RUN;
    J.in_len = p->consumed[i];
    J.inv_wb_r = uint32_t(j.desc.inv_wb_r);
    J.inv_wb_b = uint32_t(j.desc.inv_wb_b);
    J.table = uint32_t(p->h_tables.size());
    p->h_tables.resize(p->h_tables.size() + SN_LUT);
    sn_lut(j.desc, p->h_tables.data() + J.table);
    const uint32_t runs = J.rpr * uint32_t(j.img.dim_y);
    for (uint32_t f = 0; f < runs; f += SN_ITEM_RUNS)
      items.push_back(SnItem{uint32_t(i), f, std::min(SN_ITEM_RUNS, runs - f), 0});
  }
  p->n_items = uint32_t(items.size());
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const std::vector<uint32_t> pw = dither_powers(6u * SN_RUN, SN_MAX_RUNS); // 15700^(24 run) mod m
  int st;
  // (no pad behind d_pow: the kernel reads it one word at an index, pow24[run])
  if ((st = upload(ctx, p->d_jobs, p->jobs)) || (st = upload(ctx, p->d_items, items)) ||
      (st = upload(ctx, p->d_tables, p->h_tables)) || (st = upload(ctx, p->d_pow, pw, 0)))
    return st;
  *out = std::move(p);
  return RSX_OK;
}

int nikon_snef_plan_set_table(DecoderPlan* plan, int job, const rsx_nikon_snef_desc* desc, hipStream_t s) {
  NikonSnefPlan* p = dynamic_cast<NikonSnefPlan*>(plan);
  if (!p || job < 0 || size_t(job) >= p->jobs.size() || !desc || !desc->table ||
      p->host_status[job] != RSX_OK)
    return RSX_ERR_INVALID_ARG;
  rsx_ctx* ctx = p->ctx;
  // (h_tables is not touched again before the stream has passed the copy: every run ends in
  // the plan's results, which wait for the stream)
  uint32_t* t = p->h_tables.data() + p->jobs[job].table;
  sn_lut(*desc, t);
  RSX_HIP_CHECK(ctx, hipMemcpyAsync(static_cast<uint32_t*>(p->d_tables.ptr) + p->jobs[job].table, t,
                                    SN_LUT * 4, hipMemcpyHostToDevice, s));
  return RSX_OK;
}

int NikonSnefPlan::run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) {
  if (n_items == 0)
    return RSX_OK; // (every job was rejected by the host)
  SnArgs A{};
  A.in_base = static_cast<const uint8_t*>(in_dev);
  A.out_base = static_cast<uint8_t*>(out_dev);
  A.items = static_cast<const SnItem*>(d_items.ptr);
  A.jobs = static_cast<const SnJobDev*>(d_jobs.ptr);
  A.tables = static_cast<const uint32_t*>(d_tables.ptr);
  A.pow24 = static_cast<const uint32_t*>(d_pow.ptr);
  if (timer)
    timer->begin(s);
  hipLaunchKernelGGL(nikon_snef_kernel, dim3(n_items), dim3(SN_THREADS), 0, s, A);
  if (timer)
    timer->mark("nikon_snef_kernel");
  RSX_HIP_CHECK(ctx, hipGetLastError());
  return RSX_OK;
}

int NikonSnefPlan::results(hipStream_t s, bool ran, int32_t* job_status, uint32_t* job_consumed) {
  if (job_consumed)
    std::copy(consumed.begin(), consumed.end(), job_consumed);
  if (ran && n_items != 0)
    RSX_HIP_CHECK(ctx, hipStreamSynchronize(s));
  return fold_jobs(jobs.size(), FoldOrder::LAST_FAILING, job_status,
                   [&](size_t i) { return int(host_status[i]); });
}

} // namespace rsx
