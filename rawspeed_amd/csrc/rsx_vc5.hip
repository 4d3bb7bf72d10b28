// VC5Decompressor (GoPro VC-5 DNG tiles) on the device (include/rsx.h section 4c).  The
// arithmetic -- code look-up, segment walks, filters, merge -- is rsx_vc5_core.h; this file is
// how it is spread over the machine.
//
//   vc5_lowpass_kernel  sixteen workgroups per low-pass band (4 bands an image): `precision`-bit MSB fields
//                       to int16_t.
//   vc5_band_kernel     one workgroup of 1024 lanes per high-pass band stream (36 an image), all
//                       jobs of a plan in one grid.  The book's table (18 KiB) goes to LDS, the
//                       band's storage is zeroed, then the stream is taken in windows of
//                       1024 segments x 128 bits (16 KiB of LDS and one padding word per segment,
//                       so that lanes 16 bytes apart read different banks):
//                       1. every lane parses its segment from entry offset 0 (lane 0 from where
//                          the window before truly ended): where does it leave the segment, how
//                          many coefficients did it meet (parse_count);
//                       2. every lane takes the exit of the lane in front of it as its entry and
//                          parses again if that changed, until a workgroup vote finds no change.
//                          Lane k is exact after k rounds whatever the stream, so this ends and
//                          is exact; streams re-synchronise within a few symbols, so it ends
//                          after two or three rounds;
//                       3. an exclusive scan of the counts gives every lane its first
//                          coefficient; the first lane that meets the band's end or an error
//                          is found; the lanes up to it walk once more and write the non-zero
//                          runs (parse_write), that lane gives the band's status.
//                       A failed band raises its job's flag.
//   vc5_level_kernel    one launch per level, 3 -> 1, all channels and jobs in one grid: a lane
//                       computes one 2x2 cell of the level's result, both passes in registers
//                       (the vertical pass of its three low-pass columns and its one high-pass
//                       column, then the horizontal pass); the intermediates never reach memory.
//   vc5_merge_kernel    a lane merges four 2x2 cells of a row pair: the log table in LDS, two
//                       16-byte stores; nothing is written when the job's flag is up.
// Registers and LDS (tests/test_vc5_build.py): no scratch anywhere; the band kernel is held to 128
// VGPRs (the 16 waves of a workgroup are four a SIMD) and 44 KiB of LDS and takes 59 and 42.4 KiB,
// so a CU has room for two workgroups -- a frame has 36 of them, a plan of eight frames 288 on
// 256 CUs -- the others within 64 VGPRs.  Workgroups of 512 and 256
// lanes and segments of 64, 256 and 512 bits were measured too (-DRSX_VC5_THREADS,
// -DRSX_VC5_SEG_BITS, scripts/exp_vc5_variants.py): DESIGN.md 4.13.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "rsx_internal.h"
#include "rsx_ljpeg_dev.h"
#include "rsx_plan_host.h"
#include "rsx_vc5.h"
#include "rsx_vc5_core.h"

namespace rsx {

namespace {

using namespace rsx_vc5;

#ifndef RSX_VC5_THREADS
#define RSX_VC5_THREADS 1024
#endif
constexpr uint32_t VC_THREADS = RSX_VC5_THREADS;          // lanes = segments of a window
constexpr uint32_t VC_WIN_BITS = VC_THREADS * SEG_BITS;   // 128 Kbit
constexpr uint32_t VC_WIN_WORDS = VC_WIN_BITS / 32;
constexpr uint32_t VC_WIN_LOAD = VC_WIN_WORDS + 4;        // a symbol behind the last segment
constexpr uint32_t VC_SEG_WORDS = SEG_BITS / 32;
constexpr uint32_t VC_WIN_LDS = VC_WIN_LOAD + VC_WIN_LOAD / VC_SEG_WORDS + 1;
constexpr uint32_t VC_LOG = 4096;
constexpr int VC_MIN_DIM = 34, VC_MAX_DIM = 65534;
constexpr uint32_t VC_TILE_X = 64, VC_TILE_Y = 4;         // cells of a level workgroup
constexpr uint32_t VC_MERGE_ROWS = 32;                    // cell rows of a merge workgroup

static_assert(sizeof(Code) == sizeof(rsx_vc5_code), "the core's Code is the ABI's");

struct VcBand { // a band stream (or a low-pass band)
  uint64_t in_off;  // first byte of the chunk in the plan's input
  uint64_t out_off; // first coefficient in the plan's band storage (a multiple of 8)
  uint32_t bytes, n; // chunk bytes; coefficients
  int32_t quant;
  uint32_t precision;
  uint32_t job, table; // the job; its book's table
  uint32_t slot, pad;  // where status and counters go: job * 40 + channel * 10 + subband
};

struct VcLevel { // one level of one channel
  uint64_t b0, b1, b2, b3, out; // first coefficient of each in the band storage
  uint32_t pitch0, w, h;
  int32_t shift, clamp;
  uint32_t pad;
};

struct VcItem {
  uint32_t index, tx, ty, pad; // level (or merge job) index; tile
};

struct VcMerge {
  uint64_t plane[4];
  uint64_t img_offset;
  uint32_t ppitch, pitch; // plane pitch (coefficients), image pitch (bytes)
  uint32_t w2, h2;        // cells
  uint32_t phase, table, job, pad;
};

struct VcArgs {
  const uint8_t* in_base;
  uint8_t* out_base;
  int16_t* store;           // band storage
  const VcBand* bands;
  const VcLevel* levels;
  const VcItem* items;
  const VcMerge* merges;
  const Table* tables;
  const uint16_t* logs;     // [table][4096]
  uint32_t* band_status;    // [slot]
  uint32_t* band_stats;     // [slot][2]: windows, rounds
  uint32_t* job_flag;       // [job]: != 0 when a band failed
};

// ---------------------------------------------------------------------------
// a. the low-pass band
// ---------------------------------------------------------------------------
constexpr uint32_t VC_LP_SPLIT = 16; // workgroups a low-pass band
__global__ void __launch_bounds__(256) vc5_lowpass_kernel(VcArgs A) {
  const VcBand B = A.bands[blockIdx.x / VC_LP_SPLIT];
  const uint32_t part = blockIdx.x % VC_LP_SPLIT;
  const uint8_t* in = A.in_base + B.in_off;
  int16_t* out = A.store + B.out_off;
  for (uint32_t i = part * 256u + threadIdx.x; i < B.n; i += 256u * VC_LP_SPLIT) {
    const uint64_t bit = uint64_t(i) * B.precision;
    const uint64_t at = bit >> 3;
    uint32_t v = 0;
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k) // (a field of at most 16 bits lies in three bytes)
      v = (v << 8) | (at + k < B.bytes ? uint32_t(in[at + k]) : 0u);
    v = (v >> (24u - uint32_t(bit & 7u) - B.precision)) & ((1u << B.precision) - 1u);
    out[i] = int16_t(uint16_t(v));
  }
  if (threadIdx.x == 0 && part == 0)
    A.band_status[B.slot] = B_OK;
}

// ---------------------------------------------------------------------------
// b. the high-pass band streams
// ---------------------------------------------------------------------------
struct LdsReader {
  const uint32_t* win; // big-endian words of the window, one padding word per segment
  __device__ __forceinline__ uint32_t word(uint32_t d) const { return win[d + d / VC_SEG_WORDS]; }
  __device__ __forceinline__ uint32_t peek27(uint32_t pos) const {
    const uint32_t d = pos >> 5;
    const uint64_t v = (uint64_t(word(d)) << 32) | word(d + 1);
    return uint32_t(v >> (37u - (pos & 31u))) & 0x07FFFFFFu;
  }
};

// inclusive sum over the workgroup (every lane calls it); *total = the sum over all lanes
__device__ __forceinline__ uint32_t vc_scan(uint32_t x, uint32_t* wave_sums, uint32_t* total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t v = x;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(v, d, 64);
    if (lane >= uint32_t(d))
      v += y;
  }
  if (lane == 63u)
    wave_sums[wave] = v;
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (uint32_t k = 0; k < VC_THREADS / 64; ++k) {
    const uint32_t s = wave_sums[k];
    before += k < wave ? s : 0u;
    all += s;
  }
  *total = all;
  return v + before;
}

__global__ void __launch_bounds__(VC_THREADS) vc5_band_kernel(VcArgs A) {
  __shared__ uint32_t s_l1[L1_SIZE];
  __shared__ uint32_t s_start[MAX_CODES];
  __shared__ uint32_t s_info[MAX_CODES];
  __shared__ uint32_t s_win[VC_WIN_LDS];
  __shared__ uint32_t s_exit[VC_THREADS];
  __shared__ uint32_t s_sums[VC_THREADS / 64];
  __shared__ uint32_t s_first;

  const VcBand B = A.bands[blockIdx.x];
  const uint32_t tid = threadIdx.x;
  {
    const Table* T = A.tables + B.table;
    for (uint32_t k = tid; k < L1_SIZE; k += VC_THREADS)
      s_l1[k] = T->l1[k];
    for (uint32_t k = tid; k < MAX_CODES; k += VC_THREADS) {
      s_start[k] = T->start[k];
      s_info[k] = T->info[k];
    }
  }
  int16_t* out = A.store + B.out_off;
  {
    uint4* z = reinterpret_cast<uint4*>(out); // (storage starts on 16 bytes and is padded to them)
    const uint32_t n16 = (B.n + 7u) / 8u;
    for (uint32_t k = tid; k < n16; k += VC_THREADS)
      z[k] = make_uint4(0, 0, 0, 0);
  }
  const TableRef t{s_l1, s_start, s_info};
  const LdsReader rd{s_win};
  // the chunk as aligned dwords: `skew` bytes of the first one lie in front of it
  const uint8_t* in = A.in_base + B.in_off;
  const uint32_t skew = uint32_t(reinterpret_cast<uintptr_t>(in) & 3u);
  const uint32_t* in32 = reinterpret_cast<const uint32_t*>(in - skew);
  const uint64_t in_words = (uint64_t(skew) + B.bytes + 3u) / 4u; // dwords that hold a byte of it
  const uint64_t limit = start_limit(B.bytes);
  const uint32_t seg0 = tid * SEG_BITS, seg1 = seg0 + SEG_BITS;

  uint32_t base = 0, carry = 0, windows = 0, rounds = 0, verdict = B_NONE;
  for (uint64_t w = 0;; ++w) {
    const uint64_t bit0 = w * VC_WIN_BITS;
    if (bit0 > limit + VC_WIN_BITS) { // (not reached: the limit ends every walk)
      verdict = B_OVERREAD;
      break;
    }
    __syncthreads(); // the window before is done with (and the table and the zeros are written)
    for (uint32_t d = tid; d < VC_WIN_LOAD; d += VC_THREADS) {
      const uint64_t q = w * VC_WIN_WORDS + d; // dword q of the chunk = bytes 4q .. 4q + 3
      const uint32_t a0 = q < in_words ? in32[q] : 0u;
      const uint32_t a1 = skew != 0u && q + 1 < in_words ? in32[q + 1] : 0u;
      uint32_t v = __builtin_amdgcn_alignbyte(a1, a0, skew);
      const uint64_t b = 4u * q;
      if (b + 4u > B.bytes) // bytes behind the chunk read as zeros
        v = b >= B.bytes ? 0u : v & ((1u << (8u * uint32_t(B.bytes - b))) - 1u);
      s_win[d + d / VC_SEG_WORDS] = __builtin_bswap32(v);
    }
    __syncthreads();
    ++windows;
    const int64_t dl = int64_t(limit) - int64_t(bit0);
    const int32_t lim = int32_t(dl < -1 ? -1 : (dl > (1 << 30) ? (1 << 30) : dl));

    uint32_t entry = tid == 0 ? carry : 0u;
    SegCount c = parse_count(rd, t, B.quant, seg0 + entry, seg1, lim);
    for (;;) {
      s_exit[tid] = c.exit;
      __syncthreads();
      const uint32_t e = tid == 0 ? carry : s_exit[tid - 1];
      const bool changed = e != entry;
      ++rounds;
      if (!__syncthreads_or(changed))
        break;
      if (changed) {
        entry = e;
        c = parse_count(rd, t, B.quant, seg0 + entry, seg1, lim);
      }
    }
    uint32_t total;
    const uint32_t p = base + vc_scan(c.ncoef, s_sums, &total) - c.ncoef;
    if (tid == 0)
      s_first = VC_THREADS;
    __syncthreads();
    if (c.term || p + c.ncoef >= B.n)
      atomicMin(&s_first, tid);
    __syncthreads();
    const uint32_t first = s_first;
    if (tid <= first) {
      const uint32_t v = parse_write(rd, t, B.quant, seg0 + entry, seg1, lim, p, B.n, out);
      if (tid == first) {
        A.band_status[B.slot] = v;
        if (v != B_OK)
          atomicOr(&A.job_flag[B.job], 1u);
      }
    }
    if (first < VC_THREADS) {
      verdict = B_OK; // (given by lane `first`)
      break;
    }
    base += total;
    carry = s_exit[VC_THREADS - 1];
  }
  if (tid == 0) {
    if (verdict == B_OVERREAD) {
      A.band_status[B.slot] = B_OVERREAD;
      atomicOr(&A.job_flag[B.job], 1u);
    }
    A.band_stats[2 * B.slot] = windows;
    A.band_stats[2 * B.slot + 1] = rounds;
  }
}

// ---------------------------------------------------------------------------
// c. one wavelet level
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) vc5_level_kernel(VcArgs A, uint32_t first_item) {
  const VcItem I = A.items[first_item + blockIdx.x];
  const VcLevel V = A.levels[I.index];
  const uint32_t c = I.tx * VC_TILE_X + (threadIdx.x & (VC_TILE_X - 1));
  const uint32_t r = I.ty * VC_TILE_Y + threadIdx.x / VC_TILE_X;
  if (c >= V.w || r >= V.h)
    return;
  const LevelView L{A.store + V.b0, A.store + V.b1, A.store + V.b2, A.store + V.b3,
                    V.pitch0, V.w, V.h, V.shift, V.clamp};
  int16_t v[4];
  level_cell(L, r, c, v);
  // (the result starts on 16 bytes and its pitch 2w is even: column 2c lies on a dword)
  uint32_t* o = reinterpret_cast<uint32_t*>(A.store + V.out + uint64_t(2u * r) * (2u * V.w) + 2u * c);
  o[0] = uint32_t(uint16_t(v[0])) | (uint32_t(uint16_t(v[1])) << 16);
  o[V.w] = uint32_t(uint16_t(v[2])) | (uint32_t(uint16_t(v[3])) << 16);
}

// ---------------------------------------------------------------------------
// d. the merge
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) vc5_merge_kernel(VcArgs A, uint32_t first_item) {
  __shared__ __attribute__((aligned(16))) uint16_t s_log[VC_LOG];
  const VcItem I = A.items[first_item + blockIdx.x];
  const VcMerge M = A.merges[I.index];
  if (A.job_flag[M.job] != 0u)
    return; // a band failed: the image stays as it was (uniform over the workgroup)
  {
    const uint4* src = reinterpret_cast<const uint4*>(A.logs + size_t(M.table) * VC_LOG);
    for (uint32_t k = threadIdx.x; k < VC_LOG / 8; k += 256)
      reinterpret_cast<uint4*>(s_log)[k] = src[k];
  }
  __syncthreads();
  uint8_t* img = A.out_base + M.img_offset;
  const bool out16 = ((reinterpret_cast<uintptr_t>(img) | M.pitch) & 15u) == 0u;
  const uint32_t c0 = 4u * (I.tx * 64u + (threadIdx.x & 63u)); // the lane's first cell
  if (c0 >= M.w2)
    return;
  const uint32_t nc = min(4u, M.w2 - c0);
  for (uint32_t r = I.ty * VC_MERGE_ROWS + (threadIdx.x >> 6);
       r < min(M.h2, (I.ty + 1) * VC_MERGE_ROWS); r += 4) {
    uint16_t px[4][4];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      const uint64_t i = uint64_t(r) * M.ppitch + min(c0 + k, M.w2 - 1u);
      merge_cell(A.store[M.plane[0] + i], A.store[M.plane[1] + i], A.store[M.plane[2] + i],
                 A.store[M.plane[3] + i], int(M.phase), s_log, px[k]);
    }
    uint8_t* row0 = img + uint64_t(2u * r) * M.pitch + 4u * c0;
    uint8_t* row1 = row0 + M.pitch;
    if (out16 && nc == 4u) {
      *reinterpret_cast<uint4*>(row0) =
          make_uint4(px[0][0] | (uint32_t(px[0][1]) << 16), px[1][0] | (uint32_t(px[1][1]) << 16),
                     px[2][0] | (uint32_t(px[2][1]) << 16), px[3][0] | (uint32_t(px[3][1]) << 16));
      *reinterpret_cast<uint4*>(row1) =
          make_uint4(px[0][2] | (uint32_t(px[0][3]) << 16), px[1][2] | (uint32_t(px[1][3]) << 16),
                     px[2][2] | (uint32_t(px[2][3]) << 16), px[3][2] | (uint32_t(px[3][3]) << 16));
    } else {
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k)
        if (k < nc) {
          reinterpret_cast<uint16_t*>(row0)[2 * k] = px[k][0];
          reinterpret_cast<uint16_t*>(row0)[2 * k + 1] = px[k][1];
          reinterpret_cast<uint16_t*>(row1)[2 * k] = px[k][2];
          reinterpret_cast<uint16_t*>(row1)[2 * k + 1] = px[k][3];
        }
    }
  }
}

} // namespace

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
namespace {
struct Vc5Plan final : DecoderPlan {
  rsx_ctx* ctx = nullptr;
  int n_jobs = 0;
  std::vector<int32_t> host_status; // validation result per job
  std::vector<uint32_t> consumed;   // input bytes a job's bands reach
  std::vector<uint32_t> h_status, h_stats;
  DeviceBuffer d_store, d_bands, d_levels, d_items, d_merges, d_tables, d_logs, d_status, d_stats,
      d_flags;
  uint32_t n_lp = 0, n_hp = 0;      // bands[0, n_lp) low-pass, [n_lp, n_lp + n_hp) high-pass
  uint32_t level_first[3] = {}, level_count[3] = {}; // items of level 3, 2, 1
  uint32_t merge_first = 0, merge_count = 0;
  int run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) override;
  int results(hipStream_t s, bool ran, int32_t* job_status, uint32_t* job_consumed) override;
};

uint64_t round8(uint64_t n) { return (n + 7u) & ~uint64_t(7); }
} // namespace

int vc5_validate(const rsx_vc5_desc* desc, const rsx_image& img, size_t in_bytes) {
  if (!desc || !desc->log_table || !desc->codes)
    return RSX_ERR_INVALID_ARG;
  // the constructor, VC5Decompressor.cpp:384-404
  if (img.cpp != 1)
    return RSX_ERR_INVALID_ARG; // "Unexpected component count / data type"
  if (img.dim_x <= 0 || img.dim_y <= 0 || img.dim_x % 2 != 0 || img.dim_y % 2 != 0 ||
      img.dim_x > VC_MAX_DIM || img.dim_y > VC_MAX_DIM)
    return RSX_ERR_INVALID_ARG; // (ImageWidth / ImageHeight are 16-bit tags)
  if (img.pitch_bytes < uint32_t(img.dim_x) * 2u)
    return RSX_ERR_INVALID_ARG;
  if (desc->phase != 0 && desc->phase != 1)
    return RSX_ERR_INVALID_ARG; // "Unexpected bayer phase"
  {
    std::unique_ptr<Table> T(new Table);
    if (!build_table(reinterpret_cast<const Code*>(desc->codes), desc->n_codes, T.get()))
      return RSX_ERR_INVALID_ARG;
  }
  if (img.dim_x < VC_MIN_DIM || img.dim_y < VC_MIN_DIM)
    return RSX_ERR_UNSUPPORTED; // a level of fewer than 3 rows or columns
  const uint64_t w3 = level_dim(uint32_t(img.dim_x), 3), h3 = level_dim(uint32_t(img.dim_y), 3);
  for (int c = 0; c < 4; ++c)
    for (int s = 0; s < 10; ++s) {
      const rsx_vc5_band& b = desc->bands[c][s];
      if (s == 0 && (b.precision < 8 || b.precision > 16))
        return RSX_ERR_INVALID_ARG; // "Invalid precision"
      if (b.offset > in_bytes || b.bytes > in_bytes - b.offset)
        return RSX_ERR_IO;
      if (s == 0 ? b.bytes < 8u * ((w3 * h3 * b.precision + 63u) / 64u) : b.bytes < 4u)
        return RSX_ERR_IO;
    }
  return RSX_OK;
}

int vc5_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_vc5_job* jobs,
                    std::unique_ptr<DecoderPlan>* out) {
  auto p = std::make_unique<Vc5Plan>();
  p->ctx = ctx;
  p->n_jobs = n_jobs;
  p->host_status.assign(n_jobs, RSX_OK);
  p->consumed.assign(n_jobs, 0);
  std::vector<VcBand> lp, hp;
  std::vector<VcLevel> levels;
  std::vector<VcMerge> merges;
  std::vector<VcItem> items[4]; // level 3, 2, 1, merge
  std::vector<Table> tables;
  std::vector<std::vector<uint8_t>> books; // the code words a table was made from
  std::vector<uint16_t> logs;
  uint64_t store = 0;
  for (int i = 0; i < n_jobs; ++i) {
    const rsx_vc5_job& j = jobs[i];
    int st = vc5_validate(&j.desc, j.img, size_t(j.in_bytes));
    if (st == RSX_OK && (j.img_offset % 2 != 0 || j.img.pitch_bytes % 2 != 0))
      st = RSX_ERR_INVALID_ARG;
    p->host_status[i] = st;
    if (st != RSX_OK)
      continue;
    // the book's table (jobs with the same words share one) and the log table
    const uint8_t* cb = reinterpret_cast<const uint8_t*>(j.desc.codes);
    std::vector<uint8_t> book(cb, cb + size_t(j.desc.n_codes) * sizeof(rsx_vc5_code));
    uint32_t table = 0;
    while (table < books.size() && books[table] != book)
      ++table;
    if (table == books.size()) {
      books.push_back(book);
      tables.emplace_back();
      build_table(reinterpret_cast<const Code*>(j.desc.codes), j.desc.n_codes, &tables.back());
    }
    uint32_t log = 0;
    while (log < logs.size() / VC_LOG &&
           std::memcmp(&logs[size_t(log) * VC_LOG], j.desc.log_table, VC_LOG * 2) != 0)
      ++log;
    if (log == logs.size() / VC_LOG)
      logs.insert(logs.end(), j.desc.log_table, j.desc.log_table + VC_LOG);

    uint32_t w[4], h[4];
    for (int k = 0; k < 4; ++k) {
      w[k] = level_dim(uint32_t(j.img.dim_x), k);
      h[k] = level_dim(uint32_t(j.img.dim_y), k);
    }
    VcMerge M{};
    uint64_t reach = 0;
    for (int c = 0; c < 4; ++c) {
      uint64_t band_at[4][4] = {}; // [level][band]
      auto take = [&](uint64_t n) {
        const uint64_t at = store;
        store += round8(n);
        return at;
      };
      for (int s = 0; s < 10; ++s) {
        const rsx_vc5_band& b = j.desc.bands[c][s];
        const int level = s == 0 ? 3 : 3 - (s - 1) / 3, band = s == 0 ? 0 : 1 + (s - 1) % 3;
        VcBand B{};
        B.in_off = j.in_offset + b.offset;
        B.bytes = b.bytes;
        B.n = w[level] * h[level];
        B.out_off = band_at[level][band] = take(B.n);
        B.quant = b.quant;
        B.precision = b.precision;
        B.job = uint32_t(i);
        B.table = table;
        B.slot = uint32_t(i) * 40u + uint32_t(c) * 10u + uint32_t(s);
        (s == 0 ? lp : hp).push_back(B);
        reach = std::max(reach, b.offset + b.bytes);
      }
      for (int level = 3; level >= 1; --level) {
        VcLevel V{};
        V.w = w[level], V.h = h[level];
        V.b0 = band_at[level][0];
        V.pitch0 = level == 3 ? w[3] : 2u * w[level + 1];
        V.b1 = band_at[level][1], V.b2 = band_at[level][2], V.b3 = band_at[level][3];
        V.out = take(uint64_t(2u * V.w) * (2u * V.h));
        V.shift = j.desc.prescale[c][level - 1] == 2 ? 2 : 0;
        V.clamp = level == 1;
        if (level > 1)
          band_at[level - 1][0] = V.out;
        else
          M.plane[c] = V.out;
        const uint32_t index = uint32_t(levels.size());
        levels.push_back(V);
        for (uint32_t ty = 0; ty < (V.h + VC_TILE_Y - 1) / VC_TILE_Y; ++ty)
          for (uint32_t tx = 0; tx < (V.w + VC_TILE_X - 1) / VC_TILE_X; ++tx)
            items[3 - level].push_back(VcItem{index, tx, ty, 0});
      }
    }
    p->consumed[i] = uint32_t(std::min<uint64_t>(reach, 0xFFFFFFFFu));
    M.img_offset = j.img_offset;
    M.ppitch = 2u * w[1];
    M.pitch = j.img.pitch_bytes;
    M.w2 = uint32_t(j.img.dim_x) / 2u, M.h2 = uint32_t(j.img.dim_y) / 2u;
    M.phase = uint32_t(j.desc.phase);
    M.table = log;
    M.job = uint32_t(i);
    const uint32_t index = uint32_t(merges.size());
    merges.push_back(M);
    for (uint32_t ty = 0; ty < (M.h2 + VC_MERGE_ROWS - 1) / VC_MERGE_ROWS; ++ty)
      for (uint32_t tx = 0; tx < (M.w2 + 255u) / 256u; ++tx)
        items[3].push_back(VcItem{index, tx, ty, 0});
  }
  p->n_lp = uint32_t(lp.size());
  p->n_hp = uint32_t(hp.size());
  std::vector<VcBand> bands(lp);
  bands.insert(bands.end(), hp.begin(), hp.end());
  std::vector<VcItem> all;
  for (int k = 0; k < 4; ++k) {
    (k < 3 ? p->level_first[k] : p->merge_first) = uint32_t(all.size());
    (k < 3 ? p->level_count[k] : p->merge_count) = uint32_t(items[k].size());
    all.insert(all.end(), items[k].begin(), items[k].end());
  }
  p->h_status.assign(size_t(n_jobs) * 40, STATUS_NONE);
  p->h_stats.assign(size_t(n_jobs) * 80, 0);
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int st;
  // (d_status and d_stats start as STATUS_NONE and zeros: bands of jobs the host turned down
  // keep these)
  if ((st = p->d_store.ensure(store * 2 + 16)) || (st = upload(ctx, p->d_bands, bands)) ||
      (st = upload(ctx, p->d_levels, levels)) || (st = upload(ctx, p->d_items, all)) ||
      (st = upload(ctx, p->d_merges, merges)) || (st = upload(ctx, p->d_tables, tables)) ||
      (st = upload(ctx, p->d_logs, logs)) || (st = upload(ctx, p->d_status, p->h_status)) ||
      (st = upload(ctx, p->d_stats, p->h_stats)) ||
      (st = p->d_flags.ensure(size_t(n_jobs) * 4 + 16)))
    return st;
  *out = std::move(p);
  return RSX_OK;
}

int Vc5Plan::run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) {
  if (n_hp == 0)
    return RSX_OK; // (every job was rejected by the host)
  VcArgs A{};
  A.in_base = static_cast<const uint8_t*>(in_dev);
  A.out_base = static_cast<uint8_t*>(out_dev);
  A.store = static_cast<int16_t*>(d_store.ptr);
  A.levels = static_cast<const VcLevel*>(d_levels.ptr);
  A.items = static_cast<const VcItem*>(d_items.ptr);
  A.merges = static_cast<const VcMerge*>(d_merges.ptr);
  A.tables = static_cast<const Table*>(d_tables.ptr);
  A.logs = static_cast<const uint16_t*>(d_logs.ptr);
  A.band_status = static_cast<uint32_t*>(d_status.ptr);
  A.band_stats = static_cast<uint32_t*>(d_stats.ptr);
  A.job_flag = static_cast<uint32_t*>(d_flags.ptr);
  RSX_HIP_CHECK(ctx, hipMemsetAsync(d_flags.ptr, 0, size_t(n_jobs) * 4, s));
  if (timer)
    timer->begin(s);
  A.bands = static_cast<const VcBand*>(d_bands.ptr);
  hipLaunchKernelGGL(vc5_lowpass_kernel, dim3(n_lp * VC_LP_SPLIT), dim3(256), 0, s, A);
  if (timer)
    timer->mark("vc5_lowpass_kernel");
  A.bands = static_cast<const VcBand*>(d_bands.ptr) + n_lp;
  hipLaunchKernelGGL(vc5_band_kernel, dim3(n_hp), dim3(VC_THREADS), 0, s, A);
  if (timer)
    timer->mark("vc5_band_kernel");
  static const char* const names[3] = {"vc5_level_kernel(3)", "vc5_level_kernel(2)",
                                       "vc5_level_kernel(1)"};
  for (int k = 0; k < 3; ++k) {
    hipLaunchKernelGGL(vc5_level_kernel, dim3(level_count[k]), dim3(256), 0, s, A, level_first[k]);
    if (timer)
      timer->mark(names[k]);
  }
  hipLaunchKernelGGL(vc5_merge_kernel, dim3(merge_count), dim3(256), 0, s, A, merge_first);
  if (timer)
    timer->mark("vc5_merge_kernel");
  RSX_HIP_CHECK(ctx, hipGetLastError());
  return RSX_OK;
}

int Vc5Plan::results(hipStream_t s, bool ran, int32_t* job_status, uint32_t* job_consumed) {
  if (job_consumed)
    std::copy(consumed.begin(), consumed.end(), job_consumed);
  const bool have = ran && n_hp != 0;
  if (have) {
    RSX_HIP_CHECK(ctx, hipMemcpyAsync(h_status.data(), d_status.ptr, h_status.size() * 4,
                                      hipMemcpyDeviceToHost, s));
    RSX_HIP_CHECK(ctx, hipMemcpyAsync(h_stats.data(), d_stats.ptr, h_stats.size() * 4,
                                      hipMemcpyDeviceToHost, s));
    RSX_HIP_CHECK(ctx, hipStreamSynchronize(s));
  }
  return fold_jobs(size_t(n_jobs), FoldOrder::LAST_FAILING, job_status, [&](size_t i) {
    int st = host_status[i];
    if (st == RSX_OK && have) // the first failing band in (channel, subband) order
      for (int b = 0; b < 40 && st == RSX_OK; ++b)
        st = h_status[i * 40 + b] == STATUS_NONE ? RSX_ERR_DEVICE : int(h_status[i * 40 + b]);
    return st;
  });
}

int vc5_plan_bands(DecoderPlan* plan, int job, int32_t* band_status, uint32_t* windows,
                   uint32_t* rounds) {
  Vc5Plan* p = dynamic_cast<Vc5Plan*>(plan);
  if (!p || job < 0 || job >= p->n_jobs)
    return RSX_ERR_INVALID_ARG;
  for (int b = 0; b < 40; ++b) {
    const size_t slot = size_t(job) * 40 + b;
    if (band_status)
      band_status[b] = p->host_status[job] != RSX_OK ? p->host_status[job] : int32_t(p->h_status[slot]);
    if (windows)
      windows[b] = p->h_stats[2 * slot];
    if (rounds)
      rounds[b] = p->h_stats[2 * slot + 1];
  }
  return RSX_OK;
}

} // namespace rsx
