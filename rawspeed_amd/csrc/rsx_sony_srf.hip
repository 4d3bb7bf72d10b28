// ArwDecoder::SonyDecrypt and ArwDecoder::decodeSRF on gfx950: include/rsx.h section 3z, DESIGN.md
// 4.24.
//
// The reference walks its 127-word lagged generator one word at a time over the whole image.  The
// generator is linear over GF(2) (rsx_sony_srf_core.h), so ONE launch makes the stream in chunks
// of CHUNK words, a workgroup a chunk, none waiting for another:
//   1. x^(first word of the chunk) mod P by square-and-multiply: some 22 squarings of a 127-bit
//      polynomial in four 64-bit registers, the same in every lane;
//   2. lanes 0..126: one of the chunk's first 127 words each, the words of the job's table
//      w[0..252] (made by the host from the key, 1 KiB a job) under the polynomial's set bits;
//   3. the doubling identity in LDS: with K words known and 127 2^k <= K the next 63 2^k words
//      read only known ones, so the known part grows by a quarter to a half per barrier (eleven
//      barriers for 2048 words);
//   4. the pass over the chunk's bytes: input ^ stream, and for an SRF frame the widening of the
//      16-bit big-endian samples fused in: 16 bytes in, 16 bytes out per lane where the addresses
//      allow, else byte loads and 2-byte stores (a row of odd width starts in the middle of a word).
// Steps 1 to 3 are most of the kernel: a frame takes about ten times what a copy of its bytes takes
// (DESIGN.md 4.24).  A longer chunk would amortise steps 1 and 2 better but leave fewer workgroups
// than the device has slots for on a small buffer.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "rsx_ljpeg_dev.h"
#include "rsx_plan_host.h"
#include "rsx_sony_srf.h"
#include "rsx_sony_srf_core.h"

namespace rsx {

using namespace rsx_sony_srf;

namespace {

constexpr int SRF_THREADS = 256;

struct SrfJobDev {
  uint64_t in_off, out_off;
  uint32_t n_words;  // words of the stream (at most 2^32 - 1)
  uint32_t n_chunks;
  uint32_t table;    // first word of the job's w[0..252] in the plan's tables
  uint32_t widen;    // 0: the generator alone; 1: decodeSRF's rows
  uint32_t width;    // samples of an image row
  uint32_t pitch;    // bytes between image rows
};

struct SrfArgs {
  const uint8_t* in_base;
  uint8_t* out_base;
  const SrfJobDev* jobs;
  const uint32_t* tables;
};

__device__ __forceinline__ uint32_t srf_load_word(const uint8_t* p) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4); // (any alignment: byte loads)
  return v;
}

// decrypted word j of an SRF job: pixels 2 j and 2 j + 1 of the row stream
// (an image has at most 3360 x 2460 / 2 words: 32-bit divisions)
__device__ __forceinline__ void srf_store_pixels(const SrfJobDev& J, uint8_t* out, uint32_t j,
                                                 uint32_t pair) {
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const uint32_t q = 2u * j + uint32_t(k);
    const uint32_t y = q / J.width, x = q % J.width;
    *reinterpret_cast<uint16_t*>(out + uint64_t(y) * J.pitch + 2u * x) = uint16_t(pair >> (16 * k));
  }
}

__global__ __launch_bounds__(SRF_THREADS) void sony_srf_kernel(SrfArgs A) {
  __shared__ uint32_t table[TABLE + 3];
  __shared__ uint32_t s[PAD + CHUNK];
  const SrfJobDev& J = A.jobs[blockIdx.y];
  if (blockIdx.x >= J.n_chunks)
    return;
  const uint32_t tid = threadIdx.x;
  const uint64_t first = uint64_t(blockIdx.x) * CHUNK;
  const uint32_t count = uint32_t(min(uint64_t(CHUNK), uint64_t(J.n_words) - first));
  if (tid < uint32_t(TABLE))
    table[tid] = A.tables[J.table + tid];
  const Poly c = x_pow(first);
  __syncthreads();
  if (tid < uint32_t(PAD))
    s[tid] = jump_word(c, table, int(tid));
  __syncthreads();
  const uint32_t total = uint32_t(PAD) + count;
  for (uint32_t known = PAD; known < total;) {
    const int k = doubling_shift(known);
    const uint32_t step = min(63u << k, total - known);
    for (uint32_t t = known + tid; t < known + step; t += SRF_THREADS)
      s[t] = s[t - (127u << k)] ^ s[t - (63u << k)];
    known += step;
    __syncthreads();
  }
  const uint8_t* in = A.in_base + J.in_off + 4u * first;
  uint8_t* out = A.out_base + J.out_off;
  const uint32_t* stream = s + PAD;
  if (!J.widen) {
    out += 4u * first;
    const bool wide = ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15u) == 0;
    const uint32_t quads = wide ? count / 4u : 0u;
    for (uint32_t g = tid; g < quads; g += SRF_THREADS) {
      uint4 v = reinterpret_cast<const uint4*>(in)[g];
      v.x ^= stream[4u * g];
      v.y ^= stream[4u * g + 1u];
      v.z ^= stream[4u * g + 2u];
      v.w ^= stream[4u * g + 3u];
      reinterpret_cast<uint4*>(out)[g] = v;
    }
    for (uint32_t i = 4u * quads + tid; i < count; i += SRF_THREADS) {
      const uint32_t v = srf_load_word(in + 4u * i) ^ stream[i];
      __builtin_memcpy(out + 4u * i, &v, 4);
    }
    return;
  }
  const bool wide_in = (reinterpret_cast<uintptr_t>(in) & 15u) == 0;
  const uint32_t quads = wide_in ? count / 4u : 0u;
  for (uint32_t g = tid; g < quads; g += SRF_THREADS) {
    uint4 v = reinterpret_cast<const uint4*>(in)[g];
    v.x = widen_be16(v.x ^ stream[4u * g]);
    v.y = widen_be16(v.y ^ stream[4u * g + 1u]);
    v.z = widen_be16(v.z ^ stream[4u * g + 2u]);
    v.w = widen_be16(v.w ^ stream[4u * g + 3u]);
    const uint32_t j = uint32_t(first) + 4u * g; // the quad's first word: pixels 2 j .. 2 j + 7
    const uint32_t y = 2u * j / J.width, x = 2u * j % J.width;
    uint8_t* p = out + uint64_t(y) * J.pitch + 2u * x;
    if (x + 8u <= J.width && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
      *reinterpret_cast<uint4*>(p) = v;
    } else {
      srf_store_pixels(J, out, j, v.x);
      srf_store_pixels(J, out, j + 1u, v.y);
      srf_store_pixels(J, out, j + 2u, v.z);
      srf_store_pixels(J, out, j + 3u, v.w);
    }
  }
  for (uint32_t i = 4u * quads + tid; i < count; i += SRF_THREADS)
    srf_store_pixels(J, out, uint32_t(first) + i, widen_be16(srf_load_word(in + 4u * i) ^ stream[i]));
}

struct SonySrfPlan final : DecoderPlan {
  rsx_ctx* ctx = nullptr;
  std::vector<int32_t> host; // validation result per job
  std::vector<SrfJobDev> jobs; // the jobs that go to the device
  std::vector<uint32_t> h_tables;
  DeviceBuffer d_jobs, d_tables;
  uint32_t max_chunks = 0;
  void add(uint64_t in_off, uint64_t out_off, uint64_t n_words, uint32_t key, const rsx_image* img) {
    SrfJobDev D;
    std::memset(&D, 0, sizeof D);
    D.in_off = in_off;
    D.out_off = out_off;
    D.n_words = uint32_t(n_words);
    D.n_chunks = uint32_t((n_words + CHUNK - 1) / CHUNK);
    D.table = uint32_t(h_tables.size());
    h_tables.resize(h_tables.size() + TABLE);
    table_from_key(key, h_tables.data() + D.table, TABLE);
    if (img) {
      D.widen = 1;
      D.width = uint32_t(img->dim_x);
      D.pitch = img->pitch_bytes;
    }
    max_chunks = std::max(max_chunks, D.n_chunks);
    jobs.push_back(D);
  }
  int finish() {
    if (jobs.size() > 65535u)
      return RSX_ERR_UNSUPPORTED; // (a job is a row of the launch's grid)
    RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (int st = upload(ctx, d_jobs, jobs))
      return st;
    return upload(ctx, d_tables, h_tables);
  }
  int run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) override {
    if (jobs.empty() || max_chunks == 0)
      return RSX_OK; // (every job was refused by the host, or there is nothing to do)
    SrfArgs A{};
    A.in_base = static_cast<const uint8_t*>(in_dev);
    A.out_base = static_cast<uint8_t*>(out_dev);
    A.jobs = static_cast<const SrfJobDev*>(d_jobs.ptr);
    A.tables = static_cast<const uint32_t*>(d_tables.ptr);
    if (timer)
      timer->begin(s);
    hipLaunchKernelGGL(sony_srf_kernel, dim3(max_chunks, uint32_t(jobs.size())), dim3(SRF_THREADS),
                       0, s, A);
    if (timer)
      timer->mark("sony_srf_kernel");
    RSX_HIP_CHECK(ctx, hipGetLastError());
    return RSX_OK;
  }
  int results(hipStream_t, bool, int32_t* job_status, uint32_t* job_consumed) override {
    if (job_consumed)
      std::fill(job_consumed, job_consumed + host.size(), 0u);
    return fold_jobs(host.size(), FoldOrder::LAST_FAILING, job_status,
                     [&](size_t i) { return int(host[i]); });
  }
};

} // namespace

int sony_srf_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_sony_srf_job* jobs,
                         std::unique_ptr<DecoderPlan>* out) {
  auto p = std::make_unique<SonySrfPlan>();
  p->ctx = ctx;
  p->host.assign(n_jobs, RSX_OK);
  for (int i = 0; i < n_jobs; ++i) {
    const rsx_sony_srf_job& j = jobs[i];
    int st = validate(j.in_bytes, &j.img);
    if (st == RSX_OK && j.img_offset % 2 != 0)
      st = RSX_ERR_INVALID_ARG;
    p->host[i] = st;
    if (st == RSX_OK)
      p->add(j.in_offset, j.img_offset, uint64_t(j.img.dim_x) * uint64_t(j.img.dim_y) / 2u, j.key,
             &j.img);
  }
  if (int st = p->finish())
    return st;
  *out = std::move(p);
  return RSX_OK;
}

int sony_decrypt_plan_create(rsx_ctx* ctx, uint64_t n_words, uint32_t key,
                             std::unique_ptr<DecoderPlan>* out) {
  if (n_words > 0xFFFFFFFFull)
    return RSX_ERR_UNSUPPORTED;
  auto p = std::make_unique<SonySrfPlan>();
  p->ctx = ctx;
  p->host.assign(1, RSX_OK);
  p->add(0, 0, n_words, key, nullptr);
  if (int st = p->finish())
    return st;
  *out = std::move(p);
  return RSX_OK;
}

} // namespace rsx
