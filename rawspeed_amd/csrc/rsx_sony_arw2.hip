// SonyArw2Decompressor on the device (include/rsx.h section 3i).
//
// What the reference does (decompressors/SonyArw2Decompressor.cpp:56-110): row y of a w-pixel
// image is exactly the bytes [y w, (y + 1) w), read LSB-first.  The row's first 24 bits seed
// the dither generator.  The row then splits into 16-byte blocks of 16 pixels each; block b
// holds the columns 32 (b >> 1) + (b & 1) + 2 i, i = 0..15:
//   bits 0-10 max, 11-21 min, 22-25 imax, 26-29 imin, then fourteen 7-bit fields at 30 + 7 k;
//   pixel imax is max, pixel imin is min, the others take the next field in order:
//   p = min(0x7ff, (field << sh) + min), sh the smallest of 0..4 with (0x80 << sh) > max - min
//   or sh == 4; imax == imin fails the row.  The value stored is setWithLookUp(p << 1)
//   (common/RawImage.h:335-353): as it is, through a plain table, or through the dither
//   table, which steps the generator r' = 15700 (r & 65535) + (r >> 16) once per pixel in
//   decode order.
// Nothing in a block depends on another block, save the generator -- and that is a lag-1
// multiply-with-carry, r_n = r_0 15700^n mod m, m = 15700 * 2^16 - 1 (rsx_dither_dev.h, shared
// with rsx_nikon_snef.hip; tests/test_dither_jump_model.py checks it): the state in front of
// block b is one multiplication mod m away from the seed.
//
//   arw2_kernel   one workgroup of 256 lanes per item (whole rows of one job, at most 1024
//                 blocks); one lane per 16-byte block, up to 4 blocks a lane:
//                 1. every lane issues the loads of its blocks (one 16-byte load each when the
//                    input is 16-byte aligned, five dwords shifted together otherwise) and the
//                    row's seed bytes;
//                 2. the job's table -> LDS, meanwhile (2048 x u32 base | delta << 16, only
//                    even values p << 1 <= 4094 can be looked up; a plain table is the same
//                    with delta 0, which adds (0 + 1024) >> 12 = 0);
//                 3. a lane decodes its block into 16 values (the generator state jumped to
//                    16 b once, then 16 plain steps), swaps half of them with the lane of the
//                    block's partner (b ^ 1: the other column parity of the same 32 columns,
//                    a DPP swap of neighbouring lanes) and stores 32 contiguous output bytes;
//                 4. a row with a block of imax == imin is marked in LDS; one lane per row
//                    writes the row's status.
// Bit-exact against the reference's whole-file decode (tests/test_gpu_sony_arw2.py) and
// against the model tests/arw2_files.py, which tests/test_arw2_model.py holds against the
// reference.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "rsx_dither_dev.h"
#include "rsx_internal.h"
#include "rsx_ljpeg_dev.h"
#include "rsx_plan_host.h"
#include "rsx_sony_arw2.h"

namespace rsx {

namespace {

constexpr int A2_THREADS = 256;
constexpr int A2_PER_LANE = 4;                          // blocks a lane (at most)
constexpr uint32_t A2_ITEM_BLOCKS = A2_THREADS * A2_PER_LANE; // blocks an item (at most)
constexpr int32_t A2_MAX_W = 9600, A2_MAX_H = 6376;      // SonyArw2Decompressor.cpp:47-50
constexpr uint32_t A2_MAX_BLOCKS = A2_MAX_W / 16;        // blocks a row (at most)
constexpr uint32_t A2_LUT = 2048;                        // table entries: p = 0 .. 0x7ff
constexpr uint32_t A2_NO_TABLE = 0xFFFFFFFFu;

struct A2JobDev {
  uint64_t in_off;     // first byte of row 0 in the plan's input
  uint64_t img_offset; // first byte of the image in the plan's output
  uint32_t pitch, width;
  uint32_t bpr;        // blocks a row: width / 16 (even)
  uint32_t row_base;   // first entry of the job in row_status[]
  uint32_t table;      // first entry of the job's table in tables[], A2_NO_TABLE: none
  uint32_t pad;
};

struct A2Item {
  uint32_t job, row0, nrows, pad;
};

struct A2Args {
  const uint8_t* in_base;
  uint8_t* out_base;
  const A2Item* items;
  const A2JobDev* jobs;
  const uint32_t* tables; // [job's table][p]: base | delta << 16
  const uint32_t* pow16;  // [b]: 15700^(16 b) mod m
  uint32_t* row_status;   // [row of the plan]: rsx_status
  uint32_t* job_status;   // [job]: first failing row << 8 | status, STATUS_NONE = fine
};

// the 16 bytes of a block at any byte address: 16-byte aligned -> one load; else the five
// dwords that hold them (all five hold bytes of the block: no dword reaches past its last byte)
__device__ __forceinline__ void a2_load(const uint8_t* p, bool aligned, uint32_t (&w)[4]) {
  if (aligned) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    return;
  }
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  const uint32_t* d = reinterpret_cast<const uint32_t*>(a & ~uintptr_t(3));
  const uint32_t s = uint32_t(a & 3u);
  const uint32_t d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3];
  const uint32_t d4 = s ? d[4] : 0u;
  w[0] = __builtin_amdgcn_alignbyte(d1, d0, s);
  w[1] = __builtin_amdgcn_alignbyte(d2, d1, s);
  w[2] = __builtin_amdgcn_alignbyte(d3, d2, s);
  w[3] = __builtin_amdgcn_alignbyte(d4, d3, s);
}

// the 7-bit field k (bits 30 + 7 k of the block; k is a constant after unrolling)
template <int K> __device__ __forceinline__ uint32_t a2_field(const uint32_t (&w)[4]) {
  constexpr int q = 30 + 7 * K, lo = q >> 5, s = q & 31;
  if constexpr (s <= 25)
    return (w[lo] >> s) & 0x7Fu;
  else
    return __builtin_amdgcn_alignbit(w[lo + 1], w[lo], s) & 0x7Fu;
}

// One block: 16 values in decode order, two a word (value 2 j in the low half of pk[j]).
// `r`: the generator's state in front of the block.  Returns imax == imin.
template <bool LUT>
__device__ __forceinline__ bool a2_block(const uint32_t (&w)[4], uint32_t r, const uint32_t* lut,
                                         uint32_t (&pk)[8]) {
  const uint32_t mx = w[0] & 0x7FFu, mn = (w[0] >> 11) & 0x7FFu;
  const uint32_t imax = (w[0] >> 22) & 15u, imin = (w[0] >> 26) & 15u;
  const int32_t diff = int32_t(mx) - int32_t(mn);
  const uint32_t sh = uint32_t(diff >= 0x80) + uint32_t(diff >= 0x100) + uint32_t(diff >= 0x200) +
                      uint32_t(diff >= 0x400);
  uint32_t f[14];
#define A2_F(k) f[k] = a2_field<k>(w)
  A2_F(0); A2_F(1); A2_F(2); A2_F(3); A2_F(4); A2_F(5); A2_F(6);
  A2_F(7); A2_F(8); A2_F(9); A2_F(10); A2_F(11); A2_F(12); A2_F(13);
#undef A2_F
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    // pixel i takes field i - (fields skipped for imax / imin in front of it)
    const uint32_t d = uint32_t(uint32_t(i) > imax) + uint32_t(uint32_t(i) > imin);
    const uint32_t f0 = i < 14 ? f[i < 14 ? i : 0] : 0u;
    const uint32_t f1 = (i >= 1 && i - 1 < 14) ? f[(i >= 1 && i - 1 < 14) ? i - 1 : 0] : 0u;
    const uint32_t f2 = (i >= 2 && i - 2 < 14) ? f[(i >= 2 && i - 2 < 14) ? i - 2 : 0] : 0u;
    const uint32_t fi = d == 0u ? f0 : (d == 1u ? f1 : f2);
    uint32_t p = min(0x7FFu, (fi << sh) + mn);
    p = uint32_t(i) == imin ? mn : p;
    p = uint32_t(i) == imax ? mx : p;
    uint32_t v;
    if constexpr (LUT) {
      v = dither_lookup(lut[p], r);
    } else {
      v = p << 1;
    }
    if (i & 1)
      pk[i >> 1] |= v << 16;
    else
      pk[i >> 1] = v;
  }
  return imax == imin;
}

template <bool LUT> __device__ __forceinline__ void a2_item(const A2Args& A, const A2Item& I, const A2JobDev& J,
                                                            uint32_t* lut, uint32_t* bad) {
  const int tid = threadIdx.x;
  const uint32_t n = I.nrows * J.bpr;
  const uint8_t* in = A.in_base + J.in_off;
  const bool in_aligned = ((reinterpret_cast<uintptr_t>(in) | J.width) & 15u) == 0u;

  // 1. the loads of the lane's blocks (and seeds) go out first
  uint32_t w[A2_PER_LANE][4];
  uint32_t row[A2_PER_LANE], blk[A2_PER_LANE], seed[A2_PER_LANE], pw[A2_PER_LANE];
#pragma unroll
  for (int k = 0; k < A2_PER_LANE; ++k) {
    const uint32_t t = uint32_t(tid) + uint32_t(k) * A2_THREADS;
    row[k] = blk[k] = seed[k] = pw[k] = 0;
    if (t < n) {
      row[k] = I.row0 + t / J.bpr;
      blk[k] = t - (row[k] - I.row0) * J.bpr;
      const uint8_t* r0 = in + uint64_t(row[k]) * J.width;
      a2_load(r0 + 16u * blk[k], in_aligned, w[k]);
      if constexpr (LUT) {
        seed[k] = uint32_t(r0[0]) | (uint32_t(r0[1]) << 8) | (uint32_t(r0[2]) << 16);
        pw[k] = A.pow16[blk[k]];
      }
    }
  }
  // 2. the table -> LDS while they are in flight
  if constexpr (LUT) {
    const uint4* src = reinterpret_cast<const uint4*>(A.tables + J.table);
    for (uint32_t k = tid; k < A2_LUT / 4; k += A2_THREADS)
      reinterpret_cast<uint4*>(lut)[k] = src[k];
  }
  __syncthreads();

  // 3. decode, swap with the partner block, store 32 bytes
  uint8_t* out = A.out_base + J.img_offset;
  const bool out16 = ((reinterpret_cast<uintptr_t>(out) | J.pitch) & 15u) == 0u;
  const bool out4 = ((reinterpret_cast<uintptr_t>(out) | J.pitch) & 3u) == 0u;
#pragma unroll
  for (int k = 0; k < A2_PER_LANE; ++k) {
    const uint32_t t = uint32_t(tid) + uint32_t(k) * A2_THREADS;
    if (t >= n) // (n is even, so both lanes of a block pair take the same side)
      continue;
    uint32_t r = 0;
    if constexpr (LUT)
      r = dither_jump(seed[k], pw[k]);
    uint32_t pk[8];
    if (a2_block<LUT>(w[k], r, lut, pk))
      atomicOr(&bad[(row[k] - I.row0) >> 5], 1u << ((row[k] - I.row0) & 31u));
    // block b even: columns 0, 2, .. 30 of the pair (its values 0..7 -> the first 16 columns),
    // b odd: columns 1, 3, .. 31.  The even lane keeps values 0..7 and gets the partner's
    // 0..7; the odd lane keeps 8..15 and gets the partner's 8..15.
    const bool odd = (blk[k] & 1u) != 0u;
    uint32_t mine[4], other[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t send = odd ? pk[j] : pk[4 + j];
      // (the partner is the neighbouring lane: DPP quad_perm [1, 0, 3, 2])
      const uint32_t got = uint32_t(__builtin_amdgcn_update_dpp(0, int(send), 0xB1, 0xF, 0xF, false));
      mine[j] = odd ? pk[4 + j] : pk[j];
      other[j] = got;
    }
    uint32_t o[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t ev = odd ? other[j] : mine[j]; // the even columns' two values
      const uint32_t od = odd ? mine[j] : other[j]; // the odd columns' two values
      o[2 * j] = (ev & 0xFFFFu) | (od << 16);
      o[2 * j + 1] = (ev >> 16) | (od & 0xFFFF0000u);
    }
    uint8_t* dst = out + uint64_t(row[k]) * J.pitch + 32u * blk[k];
    if (out16) {
      reinterpret_cast<uint4*>(dst)[0] = make_uint4(o[0], o[1], o[2], o[3]);
      reinterpret_cast<uint4*>(dst)[1] = make_uint4(o[4], o[5], o[6], o[7]);
    } else if (out4) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        reinterpret_cast<uint32_t*>(dst)[j] = o[j];
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        reinterpret_cast<uint16_t*>(dst)[2 * j] = uint16_t(o[j]);
        reinterpret_cast<uint16_t*>(dst)[2 * j + 1] = uint16_t(o[j] >> 16);
      }
    }
  }
}

__global__ void __launch_bounds__(A2_THREADS) arw2_kernel(A2Args A) {
  __shared__ uint32_t lut[A2_LUT];
  __shared__ uint32_t bad[A2_ITEM_BLOCKS / 2 / 32]; // a bit per row (rows have >= 2 blocks)
  const A2Item I = A.items[blockIdx.x];
  const A2JobDev J = A.jobs[I.job];
  for (int k = threadIdx.x; k < int(A2_ITEM_BLOCKS / 2 / 32); k += A2_THREADS)
    bad[k] = 0;
  // (the barrier inside a2_item orders these stores before any atomicOr)
  if (J.table != A2_NO_TABLE)
    a2_item<true>(A, I, J, lut, bad);
  else
    a2_item<false>(A, I, J, lut, bad);
  __syncthreads();
  // 4. the rows' statuses: imax == imin anywhere in a row fails it
  for (uint32_t r = threadIdx.x; r < I.nrows; r += A2_THREADS) {
    const bool b = (bad[r >> 5] >> (r & 31u)) & 1u;
    A.row_status[J.row_base + I.row0 + r] = b ? uint32_t(RSX_ERR_INVALID_ARG) : uint32_t(RSX_OK);
    if (b)
      atomicMin(&A.job_status[I.job], ((I.row0 + r) << 8) | uint32_t(RSX_ERR_TILE_ERRORS));
  }
}

// the device form of a table: [p] = base | delta << 16 (a plain table: delta 0)
void a2_lut(const rsx_sony_arw2_desc& d, uint32_t* out) {
  for (uint32_t p = 0; p < A2_LUT; ++p)
    out[p] = d.table_mode == RSX_ARW2_TABLE_DITHER
                 ? uint32_t(d.table[4 * p]) | (uint32_t(d.table[4 * p + 1]) << 16)
                 : uint32_t(d.table[2 * p]);
}

} // namespace

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
namespace {
struct Arw2Plan final : DecoderPlan {
  rsx_ctx* ctx = nullptr;
  std::vector<A2JobDev> jobs;
  JobStatus status;
  std::vector<uint32_t> consumed; // input bytes a job reads (w * h when validated)
  std::vector<uint32_t> job_rows; // rows of a job (0 when rejected)
  std::vector<int32_t> job_mode;  // table mode per job
  std::vector<uint32_t> h_tables; // device form of every job's table
  DeviceBuffer d_jobs, d_items, d_tables, d_pow, d_row_status;
  std::vector<uint32_t> h_row_status;
  uint32_t n_items = 0, total_rows = 0;
  bool launched = false;
  int run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) override;
  int results(hipStream_t s, bool ran, int32_t* job_status, uint32_t* job_consumed) override;
  int row_status(hipStream_t s, int job, int32_t* statuses) override;
};
} // namespace

int sony_arw2_validate(const rsx_sony_arw2_desc* desc, const rsx_image& img, size_t in_bytes) {
  // the table SonyArw2Decompressor finds in mRaw (none, plain or dithering)
  if (!desc)
    return RSX_ERR_INVALID_ARG;
  if (desc->table_mode != RSX_ARW2_TABLE_NONE && desc->table_mode != RSX_ARW2_TABLE_PLAIN &&
      desc->table_mode != RSX_ARW2_TABLE_DITHER)
    return RSX_ERR_INVALID_ARG;
  if (desc->table_mode != RSX_ARW2_TABLE_NONE && !desc->table)
    return RSX_ERR_INVALID_ARG;
  // the constructor, SonyArw2Decompressor.cpp:40-54, in its order
  if (img.cpp != 1)
    return RSX_ERR_INVALID_ARG;
  if (img.dim_x <= 0 || img.dim_y <= 0 || img.dim_x % 32 != 0 || img.dim_x > A2_MAX_W ||
      img.dim_y > A2_MAX_H)
    return RSX_ERR_INVALID_ARG;
  if (img.pitch_bytes < uint32_t(img.dim_x) * 2u)
    return RSX_ERR_INVALID_ARG;
  // input.peekStream(w * h): one byte per pixel (bytes behind them are not read)
  if (in_bytes < size_t(img.dim_x) * size_t(img.dim_y))
    return RSX_ERR_IO;
  return RSX_OK;
}

int sony_arw2_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_sony_arw2_job* jobs,
                          std::unique_ptr<DecoderPlan>* out) {
  auto p = std::make_unique<Arw2Plan>();
  p->ctx = ctx;
  p->status.host.assign(n_jobs, RSX_OK);
  p->consumed.assign(n_jobs, 0);
  p->job_rows.assign(n_jobs, 0);
  p->job_mode.assign(n_jobs, RSX_ARW2_TABLE_NONE);
  p->jobs.resize(n_jobs);
  std::vector<A2Item> items;
  for (int i = 0; i < n_jobs; ++i) {
    const rsx_sony_arw2_job& j = jobs[i];
    A2JobDev& J = p->jobs[i];
    std::memset(&J, 0, sizeof J);
    J.table = A2_NO_TABLE;
    int st = sony_arw2_validate(&j.desc, j.img, size_t(j.in_bytes));
    if (st == RSX_OK) // (also for a job the alignment check below turns down)
      p->consumed[i] = uint32_t(j.img.dim_x) * uint32_t(j.img.dim_y);
    if (st == RSX_OK && (j.img_offset % 2 != 0 || j.img.pitch_bytes % 2 != 0))
      st = RSX_ERR_INVALID_ARG;
    p->status.host[i] = st;
    if (st != RSX_OK)
      continue;
    J.in_off = j.in_offset;
    J.img_offset = j.img_offset;
    J.pitch = j.img.pitch_bytes;
    J.width = uint32_t(j.img.dim_x);
    J.bpr = J.width / 16u;
    J.row_base = p->total_rows;
    p->job_mode[i] = j.desc.table_mode;
    if (j.desc.table_mode != RSX_ARW2_TABLE_NONE) {
      J.table = uint32_t(p->h_tables.size());
      p->h_tables.resize(p->h_tables.size() + A2_LUT);
      a2_lut(j.desc, p->h_tables.data() + J.table);
    }
    const uint32_t h = uint32_t(j.img.dim_y);
    const uint32_t per = std::max(1u, A2_ITEM_BLOCKS / J.bpr); // rows an item
    for (uint32_t r = 0; r < h; r += per)
      items.push_back(A2Item{uint32_t(i), r, std::min(per, h - r), 0});
    p->job_rows[i] = h;
    p->total_rows += h;
  }
  p->n_items = uint32_t(items.size());
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const std::vector<uint32_t> pw = dither_powers(16, A2_MAX_BLOCKS); // 15700^(16 b) mod m
  int st;
  // (no pad behind d_pow: the kernel reads it one word at an index, pow16[block])
  if ((st = upload(ctx, p->d_jobs, p->jobs)) || (st = upload(ctx, p->d_items, items)) ||
      (st = upload(ctx, p->d_tables, p->h_tables)) || (st = upload(ctx, p->d_pow, pw, 0)) ||
      (st = p->d_row_status.ensure(size_t(p->total_rows) * 4 + 16)) || (st = p->status.init()))
    return st;
  *out = std::move(p);
  return RSX_OK;
}

int sony_arw2_plan_set_table(DecoderPlan* plan, int job, const rsx_sony_arw2_desc* desc, hipStream_t s) {
  Arw2Plan* p = dynamic_cast<Arw2Plan*>(plan);
  if (!p || job < 0 || size_t(job) >= p->jobs.size() || !desc || p->status.host[job] != RSX_OK ||
      desc->table_mode != p->job_mode[job])
    return RSX_ERR_INVALID_ARG;
  rsx_ctx* ctx = p->ctx;
  if (desc->table_mode == RSX_ARW2_TABLE_NONE)
    return RSX_OK;
  if (!desc->table)
    return RSX_ERR_INVALID_ARG;
  // (h_tables is not touched again before the stream has passed the copy: every run ends in
  // the plan's results, which wait for the stream)
  uint32_t* t = p->h_tables.data() + p->jobs[job].table;
  a2_lut(*desc, t);
  RSX_HIP_CHECK(ctx, hipMemcpyAsync(static_cast<uint32_t*>(p->d_tables.ptr) + p->jobs[job].table, t,
                                    A2_LUT * 4, hipMemcpyHostToDevice, s));
  return RSX_OK;
}

int Arw2Plan::run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) {
  if (n_items == 0)
    return RSX_OK; // (every job was rejected by the host)
  A2Args A{};
  A.in_base = static_cast<const uint8_t*>(in_dev);
  A.out_base = static_cast<uint8_t*>(out_dev);
  A.items = static_cast<const A2Item*>(d_items.ptr);
  A.jobs = static_cast<const A2JobDev*>(d_jobs.ptr);
  A.tables = static_cast<const uint32_t*>(d_tables.ptr);
  A.pow16 = static_cast<const uint32_t*>(d_pow.ptr);
  A.row_status = static_cast<uint32_t*>(d_row_status.ptr);
  A.job_status = static_cast<uint32_t*>(status.dev.ptr);
  if (int st = status.reset(ctx, s))
    return st;
  if (timer)
    timer->begin(s);
  hipLaunchKernelGGL(arw2_kernel, dim3(n_items), dim3(A2_THREADS), 0, s, A);
  if (timer)
    timer->mark("arw2_kernel");
  RSX_HIP_CHECK(ctx, hipGetLastError());
  launched = true;
  return RSX_OK;
}

int Arw2Plan::results(hipStream_t s, bool ran, int32_t* job_status, uint32_t* job_consumed) {
  if (job_consumed)
    std::copy(consumed.begin(), consumed.end(), job_consumed);
  return status.fold(ctx, s, ran && n_items != 0, 0xFFu, FoldOrder::LAST_FAILING, job_status);
}

int Arw2Plan::row_status(hipStream_t s, int job, int32_t* statuses) {
  if (job < 0 || size_t(job) >= jobs.size() || !launched || job_rows[job] == 0)
    return RSX_ERR_INVALID_ARG;
  return fetch_words(ctx, s, d_row_status, jobs[job].row_base, job_rows[job], h_row_status, statuses);
}

} // namespace rsx
