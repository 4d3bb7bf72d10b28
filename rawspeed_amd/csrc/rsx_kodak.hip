// KodakDecompressor (Kodak DCR, compression 65000) on gfx950: include/rsx.h section 3w,
// DESIGN.md 4.21.
//
// A segment's size is a closed form of the sum of its 4-bit lengths (rsx_kodak_core.h), and every
// segment size is even, so "the segment behind the one that starts here" is a function of the
// even offset alone.  The segments' starts -- the only serial part of the format -- come out of
// maps over HALF-OFFSETS (offset / 2), each entry the half-offset of the successor or KD_PAST
// where the segment would read past the stream's end.  KD_PAST absorbs.  A run is, over all jobs
// (frames) of a plan at once:
//
// kodak_succ_kernel       F (a full segment's successor) and T (the tail segment's) for every
//                         half-offset.  F needs the sum of the 256 nibbles behind the offset: a
//                         sliding window, so a workgroup sums its tile of bytes plus a halo of 128
//                         in LDS and takes differences; no device-wide prefix sum is needed.
// kodak_row_map_kernel    R = T o F^n, the successor of a ROW, by n + 1 gathers a half-offset; a
//                         gather lands within 305 entries of where it started, so they stay in
//                         the cache.  Also zeroes the row starts.
// kodak_row_double_kernel level j: row y with bit j set goes through R^(2^j), and R^(2^(j+1)) =
//                         R^(2^j) o R^(2^j) is made for the next level (ping-pong between two
//                         buffers); ceil(log2(rows + 1)) launches give the start of every row.
//                         (kodak_row_walk_kernel: the same starts by one lane a frame and one
//                         dependent load a row, for comparison; RSX_KODAK_ROW_WALK=1 selects it.)
// kodak_seg_kernel        one thread a row: the starts of the row's segments, F^k of its start.
// kodak_decode_kernel     one wavefront a segment, four pixels a lane: the segment's bytes into
//                         LDS, a wave prefix sum of the lengths, every field cut from the two units
//                         it can straddle and extended, the two predictors as two wave scans, the
//                         range check, the table, one 8-byte store a lane.  A segment whose
//                         successor is KD_PAST is the one the reference's reader fails in; verdicts
//                         meet in one atomicMin over 2 segment + kind a job.
//
// Nothing walks the frame segment by segment, and nothing is guessed.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "rsx_kodak.h"
#include "rsx_kodak_core.h"
#include "rsx_ljpeg_dev.h"
#include "rsx_plan_host.h"

namespace rsx {

using namespace rsx_kodak;

namespace {

constexpr int KD_THREADS = 256;
constexpr uint32_t KD_PAST = 0xFFFFFFFFu;
constexpr int KD_HALO = SEGMENT / 4;            // half-offsets of a full segment's lengths (64)
constexpr int KD_TILE = 4 * KD_THREADS - KD_HALO; // half-offsets a workgroup of kodak_succ makes
constexpr int KD_SEG_WAVES = KD_THREADS / 64;   // segments a workgroup of kodak_decode takes
// bytes of a segment at most: segment_bound(256) = 610, rounded up to words
constexpr int KD_SEG_WORDS = 154;
static_assert(KD_SEG_WORDS * 4 >= 128 + 2 + 4 * 120, "a full segment with every length 15");

struct KdJobDev {
  uint64_t in_off;  // the stream, from the run's input base
  uint64_t out_off; // the image's first pixel, from the run's output base
  uint64_t f_off, t_off, r_off; // the job's three maps (m entries each) in maps[]
  uint64_t row_off; // its dim_y + 1 row starts in rows[]
  uint64_t seg_off; // its n_segs + 1 segment starts in segs[]
  uint32_t in_bytes; // bytes of the stream that can be read
  uint32_t m;        // map entries: in_bytes / 2 + 1
  uint32_t pitch;
  uint32_t job;
  int32_t dim_x, dim_y;
  uint32_t n_full, tail; // segments of 256 pixels a row, pixels of the tail segment (or 0)
  uint32_t row_segs, n_segs;
  int32_t bps, mode;
  uint32_t table; // first entry of the job's table in tables[]
  uint32_t reserved;
};

struct KdArgs {
  const uint8_t* in_base;
  uint8_t* out_base;
  const KdJobDev* jobs;
  uint32_t* maps;
  uint32_t* rows;
  uint32_t* segs;
  const uint16_t* tables; // [job's table][value]: what a pixel of that value becomes
  uint32_t* job_status;   // per job of the plan: STATUS_NONE, or the least 2 segment + kind
};

__device__ __forceinline__ int32_t kd_wave_scan(int32_t v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int32_t u = __shfl_up(v, d);
    v += lane >= d ? u : 0;
  }
  return v; // inclusive
}

__device__ __forceinline__ uint32_t kd_hop(const uint32_t* map, uint32_t p) {
  return p == KD_PAST ? KD_PAST : map[p];
}

// the successor of the segment of `len` pixels at half-offset idx, whose lengths sum to `sum`
__device__ __forceinline__ uint32_t kd_successor(uint32_t idx, uint32_t len, uint32_t sum,
                                                 uint32_t in_bytes) {
  const uint32_t end = 2u * idx + segment_bytes(len, sum); // (below 2^27)
  return end > in_bytes ? KD_PAST : end / 2u;
}

__global__ void __launch_bounds__(KD_THREADS) kodak_succ_kernel(KdArgs A) {
  __shared__ uint32_t pre[4 * KD_THREADS + 1]; // nibble sums in front of byte pair i of the tile
  __shared__ uint32_t wave_sum[KD_THREADS / 64];
  const KdJobDev J = A.jobs[blockIdx.y];
  const uint32_t tile0 = blockIdx.x * uint32_t(KD_TILE);
  if (tile0 >= J.m)
    return;
  const uint8_t* in = A.in_base + J.in_off;
  const int t = int(threadIdx.x), lane = t & 63, wave = t >> 6;
  // four byte pairs a thread; bytes behind the stream count as zero (a segment that would take
  // them is KD_PAST whatever they are)
  const uint32_t b0 = 2u * (tile0 + 4u * uint32_t(t));
  uint32_t s[4];
  if (b0 + 8u <= J.in_bytes) {
    uint32_t w[2];
    __builtin_memcpy(w, in + b0, 8);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t h = (w[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
      s[k] = (h & 15u) + ((h >> 4) & 15u) + ((h >> 8) & 15u) + (h >> 12);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t a = b0 + 2u * uint32_t(k);
      s[k] = (a < J.in_bytes ? nibble_sum(in[a]) : 0u) +
             (a + 1u < J.in_bytes ? nibble_sum(in[a + 1u]) : 0u);
    }
  }
  const uint32_t tot = s[0] + s[1] + s[2] + s[3];
  const uint32_t incl = uint32_t(kd_wave_scan(int32_t(tot), lane));
  if (lane == 63)
    wave_sum[wave] = incl;
  __syncthreads();
  uint32_t ex = incl - tot;
  for (int w = 0; w < wave; ++w)
    ex += wave_sum[w];
  pre[4 * t] = ex;
  pre[4 * t + 1] = ex + s[0];
  pre[4 * t + 2] = ex + s[0] + s[1];
  pre[4 * t + 3] = ex + s[0] + s[1] + s[2];
  if (t == KD_THREADS - 1)
    pre[4 * KD_THREADS] = ex + tot;
  __syncthreads();
  uint32_t* F = A.maps + J.f_off;
  uint32_t* T = A.maps + J.t_off;
  const uint32_t tail_pairs = J.tail / 4u; // (at most 63: inside the halo)
  for (int i = t; i < KD_TILE; i += KD_THREADS) {
    const uint32_t idx = tile0 + uint32_t(i);
    if (idx >= J.m)
      break;
    if (J.n_full)
      F[idx] = 2u * idx + uint32_t(SEGMENT) / 2u > J.in_bytes
                   ? KD_PAST
                   : kd_successor(idx, uint32_t(SEGMENT), pre[i + KD_HALO] - pre[i], J.in_bytes);
    if (J.tail)
      T[idx] = 2u * idx + J.tail / 2u > J.in_bytes
                   ? KD_PAST
                   : kd_successor(idx, J.tail, pre[i + tail_pairs] - pre[i], J.in_bytes);
  }
}

// thread g of a job: g < m is half-offset g, then come the job's dim_y + 1 rows
__global__ void __launch_bounds__(KD_THREADS) kodak_row_map_kernel(KdArgs A) {
  const KdJobDev J = A.jobs[blockIdx.y];
  const uint32_t g = blockIdx.x * uint32_t(KD_THREADS) + threadIdx.x;
  if (g < J.m) {
    const uint32_t* F = A.maps + J.f_off;
    uint32_t p = g;
    for (uint32_t k = 0; k < J.n_full && p != KD_PAST; ++k)
      p = F[p];
    if (J.tail)
      p = kd_hop(A.maps + J.t_off, p);
    A.maps[J.r_off + g] = p;
  } else if (g - J.m <= uint32_t(J.dim_y)) {
    A.rows[J.row_off + (g - J.m)] = 0;
  }
}

// Level `level`: G = R^(2^level) lies in the job's r map (level even) or t map (odd).
__global__ void __launch_bounds__(KD_THREADS) kodak_row_double_kernel(KdArgs A, uint32_t level) {
  const KdJobDev J = A.jobs[blockIdx.y];
  const uint32_t H = uint32_t(J.dim_y);
  if ((1u << level) > H)
    return; // (no row of this job has the bit)
  const uint32_t g = blockIdx.x * uint32_t(KD_THREADS) + threadIdx.x;
  const uint32_t* G = A.maps + ((level & 1u) ? J.t_off : J.r_off);
  if (g < J.m) {
    if ((2u << level) <= H) // (the next level has work)
      A.maps[((level & 1u) ? J.r_off : J.t_off) + g] = kd_hop(G, G[g]);
  } else if (g - J.m <= H) {
    const uint32_t y = g - J.m;
    if ((y >> level) & 1u)
      A.rows[J.row_off + y] = kd_hop(G, A.rows[J.row_off + y]);
  }
}

// The row starts by one dependent load a row, for comparison.
__global__ void __launch_bounds__(64) kodak_row_walk_kernel(KdArgs A) {
  const KdJobDev J = A.jobs[blockIdx.x];
  if (threadIdx.x != 0)
    return;
  const uint32_t* R = A.maps + J.r_off;
  uint32_t p = 0;
  for (int32_t y = 0; y <= J.dim_y; ++y) {
    A.rows[J.row_off + uint32_t(y)] = p;
    p = kd_hop(R, p);
  }
}

__global__ void __launch_bounds__(KD_THREADS) kodak_seg_kernel(KdArgs A) {
  const KdJobDev J = A.jobs[blockIdx.y];
  const uint32_t y = blockIdx.x * uint32_t(KD_THREADS) + threadIdx.x;
  if (y > uint32_t(J.dim_y))
    return;
  uint32_t p = A.rows[J.row_off + y];
  uint32_t* seg = A.segs + J.seg_off + uint64_t(y) * J.row_segs;
  if (y == uint32_t(J.dim_y)) {
    seg[0] = p; // (behind the last segment)
    return;
  }
  const uint32_t* F = A.maps + J.f_off;
  for (uint32_t k = 0; k < J.row_segs; ++k) {
    seg[k] = p;
    if (k + 1u < J.row_segs)
      p = kd_hop(F, p); // (every segment but a row's last is a full one)
  }
}

__global__ void __launch_bounds__(KD_THREADS) kodak_decode_kernel(KdArgs A) {
  __shared__ uint32_t bytes_w[KD_SEG_WAVES][KD_SEG_WORDS];
  const KdJobDev J = A.jobs[blockIdx.y];
  const int t = int(threadIdx.x), lane = t & 63, wave = t >> 6;
  const uint32_t s = blockIdx.x * uint32_t(KD_SEG_WAVES) + uint32_t(wave);
  if (blockIdx.x * uint32_t(KD_SEG_WAVES) >= J.n_segs)
    return;
  uint32_t start = KD_PAST, next = KD_PAST;
  if (s < J.n_segs) {
    start = A.segs[J.seg_off + s];
    next = A.segs[J.seg_off + s + 1u];
  }
  // start == KD_PAST: an earlier segment failed.  next == KD_PAST: this one reads past the end.
  const bool io_fail = start != KD_PAST && next == KD_PAST;
  const bool live = start != KD_PAST && next != KD_PAST;
  uint32_t size = live ? 2u * (next - start) : 0u;
  size = size < uint32_t(4 * KD_SEG_WORDS) ? size : uint32_t(4 * KD_SEG_WORDS);
  const uint8_t* in = A.in_base + J.in_off + 2ull * start;
  uint8_t* seg_bytes = reinterpret_cast<uint8_t*>(bytes_w[wave]);
  // (start + size is the successor: inside the stream)
  for (uint32_t i = 4u * uint32_t(lane); i < size; i += 256u) {
    if (i + 4u <= size) {
      uint32_t w;
      __builtin_memcpy(&w, in + i, 4);
      bytes_w[wave][i >> 2] = w;
    } else {
      seg_bytes[i] = in[i]; // (a segment's size is even)
      seg_bytes[i + 1u] = in[i + 1u];
    }
  }
  __syncthreads();
  if (io_fail && lane == 0)
    atomicMin(&A.job_status[J.job], 2u * s);
  if (!live)
    return;
  const uint32_t k = s % J.row_segs, y = s / J.row_segs;
  const uint32_t len = k < J.n_full ? uint32_t(SEGMENT) : J.tail;
  const bool active = 4u * uint32_t(lane) < len;
  // the lane's four lengths
  uint32_t n[4] = {0, 0, 0, 0};
  if (active) {
    const uint32_t b0 = seg_bytes[2 * lane], b1 = seg_bytes[2 * lane + 1];
    n[0] = b0 & 15u;
    n[1] = b0 >> 4;
    n[2] = b1 & 15u;
    n[3] = b1 >> 4;
  }
  const uint32_t tot = n[0] + n[1] + n[2] + n[3];
  uint32_t cum = uint32_t(kd_wave_scan(int32_t(tot), lane)) - tot;
  const uint8_t* area = seg_bytes + len / 2u;
  int32_t d[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    d[i] = extend(field_at(area, cum, n[i]), n[i]);
    cum += n[i];
  }
  // pred[0] runs over the even pixels, pred[1] over the odd ones
  const int32_t even = d[0] + d[2], odd = d[1] + d[3];
  const int32_t e0 = kd_wave_scan(even, lane) - even, o0 = kd_wave_scan(odd, lane) - odd;
  const int32_t v[4] = {e0 + d[0], o0 + d[1], e0 + even, o0 + odd};
  const bool bad = active && (out_of_range(v[0], J.bps) || out_of_range(v[1], J.bps) ||
                              out_of_range(v[2], J.bps) || out_of_range(v[3], J.bps));
  if (__ballot(bad) != 0ull) {
    if (lane == 0)
      atomicMin(&A.job_status[J.job], 2u * s + 1u);
    return;
  }
  if (!active)
    return;
  uint16_t px[4];
  if (J.mode == RSX_KODAK_TABLE_NONE) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      px[i] = uint16_t(v[i]);
  } else {
    const uint16_t* table = A.tables + J.table; // (2^bps entries, and v is below 2^bps)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      px[i] = table[v[i]];
  }
  uint8_t* row = A.out_base + J.out_off + uint64_t(y) * J.pitch;
  __builtin_memcpy(row + 2u * (k * uint32_t(SEGMENT) + 4u * uint32_t(lane)), px, 8);
}

// the device form of a table: [value] = what setWithLookUp stores with the generator at 0
void kd_lut(const rsx_kodak_desc& d, uint16_t* out) {
  const uint32_t n = 1u << d.bps;
  for (uint32_t v = 0; v < n; ++v)
    out[v] = d.table[d.table_mode == RSX_KODAK_TABLE_DITHER ? 2u * v : v];
}

uint32_t kd_blocks(uint64_t n, uint32_t per) { return uint32_t((n + per - 1) / per); }

} // namespace

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
namespace {
struct KodakPlan final : DecoderPlan {
  rsx_ctx* ctx = nullptr;
  std::vector<KdJobDev> jobs; // the jobs that go to the device
  std::vector<int> dev_of;    // per job of the plan: its index in `jobs`, or -1
  std::vector<int32_t> job_mode, job_bps;
  std::vector<uint16_t> h_tables;
  JobStatus status;
  DeviceBuffer d_jobs, d_maps, d_rows, d_segs, d_tables;
  uint32_t max_m = 0, max_rows = 0, max_segs = 0;
  bool row_walk = false;
  int run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) override;
  int results(hipStream_t s, bool ran, int32_t* job_status, uint32_t* job_consumed) override;
};
} // namespace

int kodak_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_kodak_job* jobs,
                      std::unique_ptr<DecoderPlan>* out) {
  auto p = std::make_unique<KodakPlan>();
  p->ctx = ctx;
  p->status.host.assign(n_jobs, RSX_OK);
  p->dev_of.assign(n_jobs, -1);
  p->job_mode.assign(n_jobs, RSX_KODAK_TABLE_NONE);
  p->job_bps.assign(n_jobs, 0);
  const char* walk = getenv("RSX_KODAK_ROW_WALK");
  p->row_walk = walk && walk[0] == '1';
  uint64_t maps = 0, rows = 0, segs = 0;
  for (int i = 0; i < n_jobs; ++i) {
    const rsx_kodak_job& j = jobs[i];
    int st = validate(&j.desc, &j.img, j.in_bytes);
    if (st == RSX_OK && (j.img_offset % 2 != 0 || j.img.pitch_bytes % 2 != 0))
      st = RSX_ERR_INVALID_ARG;
    p->status.host[i] = st;
    if (st != RSX_OK)
      continue;
    KdJobDev D;
    std::memset(&D, 0, sizeof D);
    D.in_off = j.in_offset;
    D.out_off = j.img_offset;
    // (at most 3.3e7: what an image of 4516 x 3012 can take)
    D.in_bytes = uint32_t(std::min<uint64_t>(j.in_bytes, image_bound(j.img.dim_x, j.img.dim_y)));
    D.m = D.in_bytes / 2u + 1u;
    D.pitch = j.img.pitch_bytes;
    D.job = uint32_t(i);
    D.dim_x = j.img.dim_x;
    D.dim_y = j.img.dim_y;
    D.n_full = uint32_t(D.dim_x) / uint32_t(SEGMENT);
    D.tail = uint32_t(D.dim_x) % uint32_t(SEGMENT);
    D.row_segs = D.n_full + (D.tail ? 1u : 0u);
    D.n_segs = D.row_segs * uint32_t(D.dim_y);
    D.bps = j.desc.bps;
    D.mode = j.desc.table_mode;
    D.f_off = maps;
    D.t_off = maps + D.m;
    D.r_off = maps + 2ull * D.m;
    maps += 3ull * D.m;
    D.row_off = rows;
    rows += uint64_t(D.dim_y) + 1u;
    D.seg_off = segs;
    segs += uint64_t(D.n_segs) + 1u;
    p->job_mode[i] = D.mode;
    p->job_bps[i] = D.bps;
    if (D.mode != RSX_KODAK_TABLE_NONE) {
      D.table = uint32_t(p->h_tables.size());
      p->h_tables.resize(p->h_tables.size() + (size_t(1) << D.bps));
      kd_lut(j.desc, p->h_tables.data() + D.table);
    }
    p->max_m = std::max(p->max_m, D.m);
    p->max_rows = std::max(p->max_rows, uint32_t(D.dim_y));
    p->max_segs = std::max(p->max_segs, D.n_segs);
    p->dev_of[i] = int(p->jobs.size());
    p->jobs.push_back(D);
  }
  if (p->jobs.size() > 65535u)
    return RSX_ERR_UNSUPPORTED; // (a job is a row of the launches' grids)
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int st;
  if ((st = upload(ctx, p->d_jobs, p->jobs)) || (st = upload(ctx, p->d_tables, p->h_tables)) ||
      (st = p->d_maps.ensure(maps * 4 + 16)) || (st = p->d_rows.ensure(rows * 4 + 16)) ||
      (st = p->d_segs.ensure(segs * 4 + 16)) || (st = p->status.init()))
    return st;
  *out = std::move(p);
  return RSX_OK;
}

int kodak_plan_set_table(DecoderPlan* plan, int job, const rsx_kodak_desc* desc, hipStream_t s) {
  KodakPlan* p = dynamic_cast<KodakPlan*>(plan);
  if (!p || job < 0 || size_t(job) >= p->dev_of.size() || !desc || p->dev_of[job] < 0 ||
      desc->table_mode != p->job_mode[job] || desc->bps != p->job_bps[job])
    return RSX_ERR_INVALID_ARG;
  rsx_ctx* ctx = p->ctx;
  if (desc->table_mode == RSX_KODAK_TABLE_NONE)
    return RSX_OK;
  if (!desc->table)
    return RSX_ERR_INVALID_ARG;
  // (h_tables is not touched again before the stream has passed the copy: every run ends in
  // the plan's results, which wait for the stream)
  const uint32_t at = p->jobs[p->dev_of[job]].table;
  kd_lut(*desc, p->h_tables.data() + at);
  RSX_HIP_CHECK(ctx, hipMemcpyAsync(static_cast<uint16_t*>(p->d_tables.ptr) + at,
                                    p->h_tables.data() + at, (size_t(1) << desc->bps) * 2,
                                    hipMemcpyHostToDevice, s));
  return RSX_OK;
}

int KodakPlan::run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) {
  if (jobs.empty())
    return RSX_OK; // (every job was rejected by the host)
  KdArgs A{};
  A.in_base = static_cast<const uint8_t*>(in_dev);
  A.out_base = static_cast<uint8_t*>(out_dev);
  A.jobs = static_cast<const KdJobDev*>(d_jobs.ptr);
  A.maps = static_cast<uint32_t*>(d_maps.ptr);
  A.rows = static_cast<uint32_t*>(d_rows.ptr);
  A.segs = static_cast<uint32_t*>(d_segs.ptr);
  A.tables = static_cast<const uint16_t*>(d_tables.ptr);
  A.job_status = static_cast<uint32_t*>(status.dev.ptr);
  if (int st = status.reset(ctx, s))
    return st;
  if (timer)
    timer->begin(s);
  const uint32_t n_dev = uint32_t(jobs.size());
  const dim3 block(KD_THREADS);
  const dim3 per_entry(kd_blocks(uint64_t(max_m) + max_rows + 1u, KD_THREADS), n_dev);
  hipLaunchKernelGGL(kodak_succ_kernel, dim3(kd_blocks(max_m, KD_TILE), n_dev), block, 0, s, A);
  if (timer)
    timer->mark("kodak_succ_kernel");
  hipLaunchKernelGGL(kodak_row_map_kernel, per_entry, block, 0, s, A);
  if (timer)
    timer->mark("kodak_row_map_kernel");
  if (row_walk) {
    hipLaunchKernelGGL(kodak_row_walk_kernel, dim3(n_dev), dim3(64), 0, s, A);
    if (timer)
      timer->mark("kodak_row_walk_kernel");
  } else {
    for (uint32_t level = 0; (1u << level) <= max_rows; ++level) {
      hipLaunchKernelGGL(kodak_row_double_kernel, per_entry, block, 0, s, A, level);
      if (timer)
        timer->mark("kodak_row_double_kernel");
    }
  }
  hipLaunchKernelGGL(kodak_seg_kernel, dim3(kd_blocks(uint64_t(max_rows) + 1u, KD_THREADS), n_dev),
                     block, 0, s, A);
  if (timer)
    timer->mark("kodak_seg_kernel");
  hipLaunchKernelGGL(kodak_decode_kernel, dim3(kd_blocks(max_segs, KD_SEG_WAVES), n_dev), block, 0,
                     s, A);
  if (timer)
    timer->mark("kodak_decode_kernel");
  RSX_HIP_CHECK(ctx, hipGetLastError());
  return RSX_OK;
}

// A job's word is the least 2 segment + kind of its failing segments: the segment the reference
// fails in, and there the read (kind 0) in front of the value (kind 1).
int KodakPlan::results(hipStream_t s, bool ran, int32_t* job_status, uint32_t* job_consumed) {
  if (job_consumed)
    std::fill(job_consumed, job_consumed + status.host.size(), 0u);
  const bool ran_with_work = ran && !jobs.empty();
  if (ran_with_work)
    if (int st = status.fetch(ctx, s))
      return st;
  return fold_jobs(status.host.size(), FoldOrder::LAST_FAILING, job_status, [&](size_t i) {
    if (status.host[i] != RSX_OK || !ran_with_work || status.words[i] == STATUS_NONE)
      return int(status.host[i]);
    return int((status.words[i] & 1u) ? RSX_ERR_VALUE_RANGE : RSX_ERR_IO);
  });
}

} // namespace rsx
