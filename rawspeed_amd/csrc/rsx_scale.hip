// RawImageData::scaleBlackWhite on the device (include/rsx.h section 6).
//
// What the reference does (common/RawImageDataU16.cpp:148-392, RawImageDataFloat.cpp:120-170): one
// thread scans a window for min and max, one thread fills four histograms of 65 536 cells from the
// black areas and walks them to their medians, then row bands scale every sample, each row with a
// dither generator of its own.  The arithmetic, the validation and everything between the
// reductions and the pass (resolve) are rsx_scale_core.h, shared with the host build.  A run is
// six launches on one stream and no host round trip:
//
//   sc_init_kernel      resets the job's reduction record and, where areas count, its 4 x 65 536
//                       32-bit counters in global scratch (they do not fit LDS).  Plain stores on
//                       the launch stream -- no memset is trusted to have run.
//   sc_estimate_kernel  a workgroup per window row and 2048 samples: wavefront min / max (or the
//                       key of the binary32 minimum and a NaN flag), one atomic a wavefront.
//   sc_hist_kernel      one lane per line of an area: a horizontal area counts ONE sample crop_x
//                       times, a vertical one ONE sample size times, so a line is two atomicAdds
//                       (the even and the odd columns' histograms).  32-bit counts, truncated to
//                       the reference's 16-bit cells in front of the walk.
//   sc_levels_kernel    a workgroup per job: per histogram the sums of 256 segments (a wavefront
//                       loads a segment as 16 bytes a lane, LDS adds), the segment the walk stops in, and a
//                       wavefront scan inside it; then lane 0 runs resolve() and leaves the levels
//                       and the pass's constants in the job's record.
//   sc_chain_kernel     SSE2 variant with dither: the eight 16-bit generators of a row are not
//                       linear (mulhi ^ mullo), so rows x 8 lanes walk their chains and leave a
//                       checkpoint every CHK_BLOCKS blocks of eight pixels.
//   sc_pass_kernel      every lane loads, scales and stores 16 bytes.  SSE2: a block of eight
//                       pixels, its generators CHK_BLOCKS / 2 steps on average from a checkpoint.
//                       Plain: eight samples on the 16-byte grid of the row, the generator one
//                       modular multiplication from the row's seed (Mwc<18000>::jump_settled).
//                       F32: four samples.  A run that is cut by the crop, or that does not lie
//                       on the 16-byte grid, is loaded and stored sample by sample, so nothing
//                       outside the pass's samples is written.  A job the record refuses or skips
//                       costs one load a lane.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "rsx_internal.h"
#include "rsx_ljpeg_dev.h"
#include "rsx_plan_host.h"
#include "rsx_scale.h"
#include "rsx_scale_core.h"

namespace rsx {

namespace {

using namespace rsx_sc;

constexpr uint32_t SC_THREADS = 256, SC_EST_SAMPLES = 8;

struct ScArgs {
  uint8_t* out_base;
  const Job* jobs;
  const rsx_scale_area* areas;
  Acc* accs;
  Rec* recs;
  uint32_t* hist;
  uint16_t* chk;
  const uint32_t* pw; // [k] = 18000^k mod m
  uint32_t est_xb, pass_xb; // workgroups a row of the widest job
};

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    v += __shfl_xor(v, o, 64);
  return v;
}

__global__ void __launch_bounds__(SC_THREADS) sc_init_kernel(ScArgs A) {
  const Job& J = A.jobs[blockIdx.y];
  const uint32_t id = blockIdx.x * SC_THREADS + threadIdx.x;
  if (id == 0u)
    acc_init(&A.accs[blockIdx.y]);
  if (J.use_areas && J.n_areas != 0u && J.totalpixels != 0 && id < HIST_CELLS)
    A.hist[J.hist_off + id] = 0u;
}

__global__ void __launch_bounds__(SC_THREADS) sc_estimate_kernel(ScArgs A) {
  const Job& J = A.jobs[blockIdx.y];
  if (!J.need_estimate)
    return;
  const int32_t r = J.er0 + int32_t(blockIdx.x / A.est_xb);
  const uint32_t xb = blockIdx.x % A.est_xb;
  if (r >= J.er1)
    return;
  const uint8_t* row = A.out_base + J.img_offset + size_t(J.off_y + r) * J.pitch;
  const int64_t s0 = int64_t(J.off_x) * J.cpp;
  int32_t mn = 65536, mx = 0;
  uint32_t key = 0xFFFFFFFFu, nan = 0;
  for (uint32_t k = 0; k < SC_EST_SAMPLES; ++k) {
    const int64_t c = int64_t(J.ec0) + (int64_t(xb) * SC_EST_SAMPLES + k) * SC_THREADS + threadIdx.x;
    if (c >= J.ec1)
      break;
    if (J.is_f32) {
      const uint32_t bits = reinterpret_cast<const uint32_t*>(row)[s0 + c];
      if ((bits & 0x7FFFFFFFu) > 0x7F800000u)
        nan = 1;
      else
        key = min(key, f_key(bits));
    } else {
      const int32_t p = reinterpret_cast<const uint16_t*>(row)[s0 + c];
      mn = min(mn, p);
      mx = max(mx, p);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = min(mn, __shfl_xor(mn, o, 64));
    mx = max(mx, __shfl_xor(mx, o, 64));
    key = min(key, uint32_t(__shfl_xor(int(key), o, 64)));
    nan |= uint32_t(__shfl_xor(int(nan), o, 64));
  }
  if ((threadIdx.x & 63u) == 0u) {
    Acc& a = A.accs[blockIdx.y];
    // an atomic only where the wavefront improves what it sees (a stale look costs an atomic,
    // never a result): every wavefront of the window on one address took 1.8 ms on 8192 x 5464
    if (J.is_f32) {
      if (key < __hip_atomic_load(&a.fmin_key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMin(&a.fmin_key, key);
      if (nan && !__hip_atomic_load(&a.nan, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicOr(&a.nan, 1u);
    } else {
      if (mn < __hip_atomic_load(&a.mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMin(&a.mn, mn);
      if (mx > __hip_atomic_load(&a.mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax(&a.mx, mx);
    }
  }
}

__global__ void __launch_bounds__(SC_THREADS) sc_hist_kernel(ScArgs A) {
  const Job& J = A.jobs[blockIdx.y];
  if (!J.use_areas || J.n_areas == 0u || J.totalpixels == 0)
    return;
  const uint32_t line = blockIdx.x * SC_THREADS + threadIdx.x;
  const uint8_t* img = A.out_base + J.img_offset;
  uint32_t* hist = A.hist + J.hist_off;
  for (uint32_t i = 0; i < J.n_areas; ++i) {
    const rsx_scale_area a = A.areas[J.area_first + i];
    const uint32_t size = a.size - (a.size & 1u);
    if (size == 0u)
      continue;
    uint32_t y, sample, n_even, n_odd;
    if (!a.is_vertical) {
      if (line >= size)
        continue;
      y = a.offset + line;
      sample = uint32_t(J.off_x);
      n_even = (uint32_t(J.crop_x) + ((J.off_x & 1) ? 0u : 1u)) / 2u;
      n_odd = uint32_t(J.crop_x) - n_even;
    } else {
      if (line >= uint32_t(J.crop_y))
        continue;
      y = uint32_t(J.off_y) + line;
      sample = a.offset;
      n_even = n_odd = size / 2u;
    }
    const uint32_t bin = reinterpret_cast<const uint16_t*>(img + size_t(y) * J.pitch)[sample];
    if (n_even)
      atomicAdd(&hist[(2u * (y & 1u)) * 65536u + bin], n_even);
    if (n_odd)
      atomicAdd(&hist[(2u * (y & 1u) + 1u) * 65536u + bin], n_odd);
  }
}

// grid (job), SC_THREADS lanes
__global__ void __launch_bounds__(SC_THREADS) sc_levels_kernel(ScArgs A) {
  const Job& J = A.jobs[blockIdx.x];
  __shared__ uint32_t seg[256];
  __shared__ int32_t med[4];
  __shared__ uint32_t stop_seg;
  __shared__ long long stop_before;
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  if (t < 4u)
    med[t] = 0;
  if (J.use_areas && J.n_areas != 0u && J.totalpixels != 0) {
    const long long total = J.totalpixels / 8;
    for (uint32_t h = 0; h < 4u; ++h) {
      const uint32_t* hist = A.hist + J.hist_off + size_t(h) * 65536u;
      __syncthreads();
      seg[t] = 0u;
      __syncthreads();
      // (LDS adds, not a shuffle chain a segment: the loads of the unrolled rounds are in flight
      // together, where 256 dependent rounds took 0.13 ms)
#pragma unroll 8
      for (uint32_t s = wave; s < 256u; s += SC_THREADS / 64u) {
        const uint4 c = reinterpret_cast<const uint4*>(hist + s * 256u)[lane];
        const uint32_t n = (c.x & 0xFFFFu) + (c.y & 0xFFFFu) + (c.z & 0xFFFFu) + (c.w & 0xFFFFu);
        if (n)
          atomicAdd(&seg[s], n);
      }
      __syncthreads();
      if (t == 0u) {
        // the first segment whose inclusive sum exceeds the total: the walk stops inside it
        long long acc = 0;
        uint32_t s = 0;
        for (; s < 256u; ++s) {
          if (acc + (long long)seg[s] > total)
            break;
          acc += seg[s];
        }
        stop_seg = s;
        stop_before = acc;
      }
      __syncthreads();
      if (wave == 0u) {
        int32_t v = 65535;
        if (stop_seg < 256u) {
          const uint4 c = reinterpret_cast<const uint4*>(hist + stop_seg * 256u)[lane];
          const uint32_t c0 = c.x & 0xFFFFu, c1 = c0 + (c.y & 0xFFFFu), c2 = c1 + (c.z & 0xFFFFu),
                         c3 = c2 + (c.w & 0xFFFFu);
          uint32_t incl = c3;
#pragma unroll
          for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(incl, o, 64);
            if (lane >= uint32_t(o))
              incl += up;
          }
          const long long before = stop_before + (long long)(incl - c3);
          const int k = before + c0 > total ? 0 : before + c1 > total ? 1 : before + c2 > total ? 2
                        : before + c3 > total ? 3 : 4;
          const uint64_t hit = __ballot(k < 4);
          const int first = __ffsll((unsigned long long)hit) - 1; // (hit != 0: the segment's sum exceeds)
          v = int32_t(stop_seg * 256u + uint32_t(first) * 4u) + __shfl(k, first, 64);
        }
        if (lane == 0u)
          med[h] = v;
      }
    }
  }
  __syncthreads();
  if (t == 0u) {
    // (into the record itself: a Rec of the lane's own would live in scratch, its levels are
    // indexed by the crop's parity)
    resolve(J, A.accs[blockIdx.x], med, &A.recs[blockIdx.x]);
  }
}

__global__ void __launch_bounds__(SC_THREADS) sc_chain_kernel(ScArgs A) {
  const Job& J = A.jobs[blockIdx.y];
  const Rec& R = A.recs[blockIdx.y];
  if (!J.may_sse2_dither || R.status != 0 || R.skipped || R.variant != VARIANT_SSE2)
    return;
  const uint32_t id = blockIdx.x * SC_THREADS + threadIdx.x, y = id >> 3, g = id & 7u;
  if (y >= uint32_t(J.crop_y))
    return;
  uint16_t* chk = A.chk + J.chk_off + size_t(y) * J.n_chk * 8u + g;
  uint32_t s = sse2_seed(J, y, g);
  for (uint32_t b = 0; b < J.n_blocks; ++b) {
    if (b % CHK_BLOCKS == 0u)
      chk[size_t(b / CHK_BLOCKS) * 8u] = uint16_t(s);
    s = sse2_step(s, g);
  }
}

__device__ __forceinline__ uint32_t get16(const uint4& v, int j) {
  const uint32_t w = (j >> 1) == 0 ? v.x : (j >> 1) == 1 ? v.y : (j >> 1) == 2 ? v.z : v.w;
  return (w >> (16 * (j & 1))) & 0xFFFFu;
}
__device__ __forceinline__ void put16(uint4& v, int j, uint32_t p) {
  uint32_t& w = (j >> 1) == 0 ? v.x : (j >> 1) == 1 ? v.y : (j >> 1) == 2 ? v.z : v.w;
  w = (j & 1) ? (w & 0xFFFFu) | (p << 16) : (w & 0xFFFF0000u) | p;
}

// 8 uint16 slots at p, those of `mask`: as 16 bytes where all are meant and p is on the grid
__device__ __forceinline__ uint4 load8(const uint8_t* p, uint32_t mask) {
  if (mask == 0xFFu && (reinterpret_cast<uintptr_t>(p) & 15u) == 0u)
    return *reinterpret_cast<const uint4*>(p);
  uint4 v = make_uint4(0, 0, 0, 0);
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (mask >> j & 1u)
      put16(v, j, reinterpret_cast<const uint16_t*>(p)[j]);
  return v;
}
__device__ __forceinline__ void store8(uint8_t* p, uint32_t mask, const uint4& v) {
  if (mask == 0xFFu && (reinterpret_cast<uintptr_t>(p) & 15u) == 0u) {
    *reinterpret_cast<uint4*>(p) = v;
    return;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (mask >> j & 1u)
      reinterpret_cast<uint16_t*>(p)[j] = uint16_t(get16(v, j));
}

__global__ void __launch_bounds__(SC_THREADS) sc_pass_kernel(ScArgs A) {
  const Job& J = A.jobs[blockIdx.y];
  const Rec& R = A.recs[blockIdx.y];
  if (R.status != 0 || R.skipped)
    return;
  const uint32_t y = blockIdx.x / A.pass_xb;
  const int64_t k = int64_t(blockIdx.x % A.pass_xb) * SC_THREADS + threadIdx.x;
  if (y >= uint32_t(J.crop_y))
    return;
  uint8_t* row = A.out_base + J.img_offset + size_t(uint32_t(J.off_y) + y) * J.pitch;
  const int64_t gw = int64_t(J.crop_x) * J.cpp;
  if (R.variant == VARIANT_SSE2) {
    if (k >= int64_t(J.n_blocks))
      return;
    uint8_t* p = row + 16u * size_t(k);
    uint4 v = load8(p, 0xFFu), s = make_uint4(0, 0, 0, 0);
    if (J.dither) {
      const uint32_t b = uint32_t(k), steps = b % CHK_BLOCKS + 1u;
      s = *reinterpret_cast<const uint4*>(A.chk + J.chk_off +
                                          (size_t(y) * J.n_chk + b / CHK_BLOCKS) * 8u);
      uint32_t g[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        g[j] = get16(s, j);
      for (uint32_t i = 0; i < steps; ++i) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          g[j] = sse2_step(g[j], uint32_t(j));
      }
#pragma unroll
      for (int j = 0; j < 8; ++j)
        put16(s, j, g[j]);
    }
    const uint32_t par = (uint32_t(J.off_y) + y) & 1u;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      put16(v, j, sse2_pixel(R, par, uint32_t(j), get16(v, j), get16(s, j)));
    store8(p, 0xFFu, v);
    return;
  }
  if (R.variant == VARIANT_F32) {
    uint8_t* a = row + size_t(J.off_x) * J.cpp * 4u;
    const int64_t lead = int64_t((reinterpret_cast<uintptr_t>(a) & 15u) >> 2), x0 = 4 * k - lead;
    if (x0 >= gw)
      return;
    float* p = reinterpret_cast<float*>(a) + x0;
    if (x0 >= 0 && x0 + 4 <= gw) {
      float4 v = *reinterpret_cast<const float4*>(p);
      const uint32_t q = 2u * (y & 1u) + (uint32_t(x0) & 1u);
      v.x = f32_sample(R, v.x, q);
      v.y = f32_sample(R, v.y, q ^ 1u);
      v.z = f32_sample(R, v.z, q);
      v.w = f32_sample(R, v.w, q ^ 1u);
      *reinterpret_cast<float4*>(p) = v;
    } else {
      for (int64_t x = max(x0, (int64_t)0); x < min(x0 + 4, gw); ++x)
        p[x - x0] = f32_sample(R, p[x - x0], 2u * (y & 1u) + (uint32_t(x) & 1u));
    }
    return;
  }
  // plain
  uint8_t* a = row + size_t(J.off_x) * J.cpp * 2u;
  const int64_t lead = int64_t((reinterpret_cast<uintptr_t>(a) & 15u) >> 1), x0 = 8 * k - lead;
  uint32_t wrapped = 0;
  if (x0 < gw) {
    const int64_t xs = max(x0, (int64_t)0), xe = min(x0 + 8, gw);
    const uint32_t mask = (0xFFu << uint32_t(xs - x0)) & (0xFFu >> uint32_t(x0 + 8 - xe));
    uint8_t* p = a + 2 * x0;
    uint4 v = load8(p, mask);
    const uint32_t par0 = 2u * (y & 1u) + (uint32_t(x0) & 1u);
    const int32_t sub0 = R.sub[par0], sub1 = R.sub[par0 ^ 1u], mul0 = R.mul[par0], mul1 = R.mul[par0 ^ 1u];
    uint32_t gen = 0;
    if (J.dither) {
      const uint32_t seed = plain_seed(J, y);
      gen = xs == 0 ? seed : xs == 1 ? Gen::step(seed) : Gen::jump_settled(seed, A.pw[xs - Gen::SETTLE]);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (mask >> j & 1u) {
        int32_t rnd = 0;
        if (J.dither) {
          gen = Gen::step(gen);
          rnd = plain_rand(R, gen);
        }
        bool w;
        put16(v, j, plain_sample((j & 1) ? sub1 : sub0, (j & 1) ? mul1 : mul0, get16(v, j), rnd, &w));
        wrapped += w ? 1u : 0u;
      }
    store8(p, mask, v);
  }
  const uint32_t n = wave_sum(wrapped);
  if ((threadIdx.x & 63u) == 0u && n != 0u)
    atomicAdd(&A.accs[blockIdx.y].n_wrapped, (unsigned long long)n);
}

struct ScPlan final : DecoderPlan {
  rsx_ctx* ctx = nullptr;
  size_t n_jobs = 0;
  std::vector<Job> jobs;
  std::vector<Rec> h_rec;
  std::vector<Acc> h_acc;
  DeviceBuffer d_jobs, d_areas, d_accs, d_recs, d_hist, d_chk, d_pw;
  uint32_t init_blocks = 1, est_xb = 0, est_rows = 0, hist_blocks = 0, chain_blocks = 0, pass_xb = 0,
           pass_rows = 0;
  bool have_results = false;
  int run(const void*, void* out_dev, hipStream_t s, KernelTimer* timer) override {
    have_results = false;
    ScArgs A{};
    A.out_base = static_cast<uint8_t*>(out_dev);
    A.jobs = static_cast<const Job*>(d_jobs.ptr);
    A.areas = static_cast<const rsx_scale_area*>(d_areas.ptr);
    A.accs = static_cast<Acc*>(d_accs.ptr);
    A.recs = static_cast<Rec*>(d_recs.ptr);
    A.hist = static_cast<uint32_t*>(d_hist.ptr);
    A.chk = static_cast<uint16_t*>(d_chk.ptr);
    A.pw = static_cast<const uint32_t*>(d_pw.ptr);
    A.est_xb = std::max(est_xb, 1u);
    A.pass_xb = std::max(pass_xb, 1u);
    if (reinterpret_cast<uintptr_t>(out_dev) % 4u != 0)
      return RSX_ERR_INVALID_ARG;
    const uint32_t nj = uint32_t(n_jobs);
    if (timer)
      timer->begin(s);
    hipLaunchKernelGGL(sc_init_kernel, dim3(init_blocks, nj), dim3(SC_THREADS), 0, s, A);
    if (timer)
      timer->mark("sc_init_kernel");
    if (est_xb && est_rows) {
      hipLaunchKernelGGL(sc_estimate_kernel, dim3(est_xb * est_rows, nj), dim3(SC_THREADS), 0, s, A);
      if (timer)
        timer->mark("sc_estimate_kernel");
    }
    if (hist_blocks) {
      hipLaunchKernelGGL(sc_hist_kernel, dim3(hist_blocks, nj), dim3(SC_THREADS), 0, s, A);
      if (timer)
        timer->mark("sc_hist_kernel");
    }
    hipLaunchKernelGGL(sc_levels_kernel, dim3(nj), dim3(SC_THREADS), 0, s, A);
    if (timer)
      timer->mark("sc_levels_kernel");
    if (chain_blocks) {
      hipLaunchKernelGGL(sc_chain_kernel, dim3(chain_blocks, nj), dim3(SC_THREADS), 0, s, A);
      if (timer)
        timer->mark("sc_chain_kernel");
    }
    if (pass_xb && pass_rows) {
      hipLaunchKernelGGL(sc_pass_kernel, dim3(pass_xb * pass_rows, nj), dim3(SC_THREADS), 0, s, A);
      if (timer)
        timer->mark("sc_pass_kernel");
    }
    RSX_HIP_CHECK(ctx, hipGetLastError());
    return RSX_OK;
  }
  int results(hipStream_t s, bool ran, int32_t* job_status, uint32_t* job_consumed) override {
    if (job_consumed)
      std::fill(job_consumed, job_consumed + n_jobs, 0u);
    std::memset(static_cast<void*>(h_rec.data()), 0, h_rec.size() * sizeof(Rec));
    std::memset(static_cast<void*>(h_acc.data()), 0, h_acc.size() * sizeof(Acc));
    if (ran) {
      RSX_HIP_CHECK(ctx, hipMemcpyAsync(h_rec.data(), d_recs.ptr, n_jobs * sizeof(Rec),
                                        hipMemcpyDeviceToHost, s));
      RSX_HIP_CHECK(ctx, hipMemcpyAsync(h_acc.data(), d_accs.ptr, n_jobs * sizeof(Acc),
                                        hipMemcpyDeviceToHost, s));
      RSX_HIP_CHECK(ctx, hipStreamSynchronize(s));
    }
    have_results = ran;
    return fold_jobs(n_jobs, FoldOrder::LAST_FAILING, job_status,
                     [&](size_t i) { return int(h_rec[i].status); });
  }
  int scale_result(int job, rsx_scale_result* out) override {
    if (job < 0 || size_t(job) >= n_jobs || !out || !have_results)
      return RSX_ERR_INVALID_ARG;
    std::memset(out, 0, sizeof *out);
    const Rec& R = h_rec[size_t(job)];
    if (R.status)
      return RSX_OK;
    out->black_level = R.black_level;
    out->white_point = R.white_point;
    for (int i = 0; i < 4; ++i)
      out->black_separate[i] = R.bs[i];
    out->estimated = R.estimated;
    out->skipped = R.skipped;
    out->variant = R.variant;
    out->n_wrapped = h_acc[size_t(job)].n_wrapped;
    return RSX_OK;
  }
};

} // namespace

int scale_validate(const rsx_scale_desc* desc, const rsx_image* img) {
  return rsx_sc::validate(desc, img);
}

int scale_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_scale_job* jobs,
                      std::unique_ptr<DecoderPlan>* out) {
  if (n_jobs > 65535)
    return RSX_ERR_UNSUPPORTED; // (a grid's second dimension)
  auto p = std::make_unique<ScPlan>();
  p->ctx = ctx;
  p->n_jobs = size_t(n_jobs);
  p->jobs.resize(size_t(n_jobs));
  p->h_rec.resize(size_t(n_jobs));
  p->h_acc.resize(size_t(n_jobs));
  std::vector<rsx_scale_area> areas;
  uint64_t hist_cells = 0, chk_states = 0;
  uint32_t max_gw = 0;
  for (int i = 0; i < n_jobs; ++i) {
    const rsx_scale_job& j = jobs[i];
    if (int st = validate(&j.desc, &j.img))
      return st;
    if (j.img_offset % (j.desc.is_f32 ? 4u : 2u) != 0)
      return RSX_ERR_INVALID_ARG;
    Job& J = p->jobs[size_t(i)];
    J = make_job(&j.desc, &j.img);
    J.img_offset = j.img_offset;
    J.area_first = uint32_t(areas.size());
    areas.insert(areas.end(), j.desc.areas, j.desc.areas + j.desc.n_areas);
    const uint32_t gw = uint32_t(J.crop_x) * uint32_t(J.cpp);
    max_gw = std::max(max_gw, gw);
    if (J.need_estimate && J.er1 > J.er0 && J.ec1 > J.ec0) {
      const uint32_t per = SC_THREADS * SC_EST_SAMPLES;
      p->est_xb = std::max(p->est_xb, (uint32_t(J.ec1 - J.ec0) + per - 1u) / per);
      p->est_rows = std::max(p->est_rows, uint32_t(J.er1 - J.er0));
    }
    if (J.use_areas && J.n_areas != 0 && J.totalpixels != 0) {
      J.hist_off = hist_cells;
      hist_cells += HIST_CELLS;
      p->init_blocks = HIST_CELLS / SC_THREADS;
      uint32_t lines = 0;
      for (uint32_t a = 0; a < J.n_areas; ++a)
        lines = std::max(lines, j.desc.areas[a].is_vertical ? uint32_t(J.crop_y) : j.desc.areas[a].size);
      p->hist_blocks = std::max(p->hist_blocks, (lines + SC_THREADS - 1u) / SC_THREADS);
    }
    if (J.may_sse2_dither && J.n_blocks != 0 && J.crop_y != 0) {
      J.chk_off = chk_states;
      chk_states += uint64_t(J.crop_y) * J.n_chk * 8u;
      p->chain_blocks = std::max(p->chain_blocks, (uint32_t(J.crop_y) * 8u + SC_THREADS - 1u) / SC_THREADS);
    }
    if (!J.empty_crop) {
      // lanes a row: the blocks of the SSE2 variant, or the 16-byte runs of the cropped samples
      // on the grid (one more where the row does not start on it)
      const uint32_t lanes = std::max(J.is_f32 ? 0u : J.n_blocks, gw / (J.is_f32 ? 4u : 8u) + 2u);
      p->pass_xb = std::max(p->pass_xb, (lanes + SC_THREADS - 1u) / SC_THREADS);
      p->pass_rows = std::max(p->pass_rows, uint32_t(J.crop_y));
    }
  }
  if (uint64_t(p->pass_xb) * p->pass_rows > 0x7FFFFFFFull || uint64_t(p->est_xb) * p->est_rows > 0x7FFFFFFFull)
    return RSX_ERR_UNSUPPORTED;
  const std::vector<uint32_t> pw = Gen::powers(1, max_gw + 1u);
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int st;
  if ((st = upload(ctx, p->d_jobs, p->jobs)) || (st = upload(ctx, p->d_areas, areas)) ||
      (st = p->d_accs.ensure(p->jobs.size() * sizeof(Acc) + 16)) ||
      (st = p->d_recs.ensure(p->jobs.size() * sizeof(Rec) + 16)) ||
      (st = p->d_hist.ensure(size_t(hist_cells) * 4 + 16)) ||
      (st = p->d_chk.ensure(size_t(chk_states) * 2 + 16)) || (st = upload(ctx, p->d_pw, pw)))
    return st;
  *out = std::move(p);
  return RSX_OK;
}

} // namespace rsx
