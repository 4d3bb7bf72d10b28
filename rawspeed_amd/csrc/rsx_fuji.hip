// FujiDecompressor (compressed RAF) on gfx950: include/rsx.h section 3u, DESIGN.md 4.19.
//
// One wavefront (a workgroup of 64) per strip; the strips of every job of a plan are one launch.
// The strip's state lives in LDS: the 18 line buffers (18 x 514 samples), the six gradient tables,
// the records of the pass at hand and a window of the strip's bytes, 28.7 KB in all, so five
// strips share a CU.  The chain through a strip's bits is serial (rsx_fuji::walk): the wave runs
// it uniformly, every lane the same reads and the same stores, so that it stays on the scalar
// unit; everything around it is spread over the lanes:
//   * in front of a pass, the records of both of its lines (rsx_fuji_core.h): prediction and
//     gradient of every even position -- final at once where X-Trans takes no bits -- and, for
//     the odd positions, what the line above decides;
//   * the byte window: FJ_WIN big-endian words from the word the walk stands at, refilled between
//     chunks of FJ_CHUNK iterations when less than a chunk's worst case is left (a zero run that
//     outlasts the window reads its words from memory);
//   * the helper columns behind a pass, and per line of the strip the copy-out of the six image
//     rows (16-byte stores where the image's base and pitch allow) and the rotation.
// A first failing sample ends the strip with its status; the rows of the lines before it are
// written.  No scratch; the registers are what tests/test_fuji_build.py holds.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "rsx_fuji.h"
#include "rsx_fuji_core.h"
#include "rsx_ljpeg_dev.h"
#include "rsx_plan_host.h"

namespace rsx {

using namespace rsx_fuji;

namespace {

constexpr int FJ_THREADS = 64;
constexpr int FJ_WIN = 512;  // words of a strip's bytes in LDS
constexpr int FJ_CHUNK = 32; // iterations of a pass between two looks at the window
// a chunk's worst case without an overlong zero run: 4 samples an iteration, each at most
// 47 zeros, a 1 and 16 bits
constexpr int FJ_CHUNK_WORDS = FJ_CHUNK * 4 * 2 + 2;

struct FjStripDev {
  uint64_t in_off;  // the strip's bytes, from the run's input base
  uint64_t out_off; // the strip's first pixel, from the run's output base
  uint32_t size;
  uint32_t pitch;
  uint32_t job, strip;
  int32_t width, total_lines, raw_type, raw_bits;
};

struct FjArgs {
  const uint8_t* in_base;
  uint8_t* out_base;
  const FjStripDev* strips;
  uint32_t* strip_status;
  uint32_t* job_status;
};

// bytes 4 k .. 4 k + 3 of the strip as a big-endian word; bytes behind the strip read as zero
__device__ __forceinline__ uint32_t fj_global_word(const uint8_t* p, uint32_t size, uint32_t k) {
  const uint64_t at = 4ull * k;
  if (at + 4 <= size) {
    uint32_t v;
    __builtin_memcpy(&v, p + at, 4);
    return __builtin_bswap32(v);
  }
  uint32_t w = 0;
  for (uint32_t b = 0; b < 4; ++b)
    w = w << 8 | (at + b < size ? uint32_t(p[at + b]) : 0u);
  return w;
}

struct FjSrc {
  const uint32_t* win; // LDS
  const uint8_t* bytes;
  uint32_t size;
  uint32_t k0; // the window holds words k0 .. k0 + FJ_WIN - 1
  __device__ __forceinline__ uint32_t word(uint32_t k) const {
    const uint32_t j = k - k0;
    return j < uint32_t(FJ_WIN) ? win[j] : fj_global_word(bytes, size, k);
  }
};

__global__ void __launch_bounds__(FJ_THREADS) fuji_strip_kernel(FjArgs A) {
  __shared__ __attribute__((aligned(16))) uint16_t lines[LTOTAL * STRIDE];
  __shared__ int32_t ge[TABLE_INTS], go[TABLE_INTS];
  __shared__ uint32_t ev[MAX_LW], od[2 * MAX_LW];
  __shared__ uint32_t win[FJ_WIN];
  __shared__ uint32_t s_k;
  __shared__ int32_t s_status;

  const FjStripDev S = A.strips[blockIdx.x];
  const int lane = int(threadIdx.x);
  if (S.size < 4u) {
    if (lane == 0) {
      A.strip_status[blockIdx.x] = RSX_ERR_IO;
      atomicMin(&A.job_status[S.job], S.strip << 8 | uint32_t(RSX_ERR_IO));
    }
    return;
  }
  Params P;
  params_init(&P, S.raw_type, S.raw_bits);
  const int32_t half = P.lw / 2;
  const uint8_t* bytes = A.in_base + S.in_off;
  uint8_t* out = A.out_base + S.out_off;
  const bool wide = ((reinterpret_cast<uintptr_t>(out) | S.pitch) & 15u) == 0u;

  for (int i = lane; i < LTOTAL * STRIDE / 2; i += FJ_THREADS)
    reinterpret_cast<uint32_t*>(lines)[i] = 0u;
  for (int i = lane; i < TABLE_INTS; i += FJ_THREADS)
    ge[i] = go[i] = (i & 1) ? 1 : P.max_diff;
  if (lane == 0) {
    s_k = 0u;
    s_status = RSX_OK;
  }
  FjSrc src{win, bytes, S.size, 0u};
  Bits<FjSrc> B;
  B.init(&src, S.size);
  bool have_window = false;
  __syncthreads();

  int32_t status = RSX_OK;
  for (int32_t line = 0; line < S.total_lines && status == RSX_OK; ++line) {
    for (int32_t row = 0; row < 6 && status == RSX_OK; ++row) {
      int32_t c[2];
      pass_lines(row, &c[0], &c[1]);
      // the records of both lines
      for (int32_t idx = lane; idx < 2 * half; idx += FJ_THREADS) {
        const int32_t comp = idx >= half, col = idx - comp * half;
        const uint16_t* above1 = lines + (c[comp] - 1) * STRIDE;
        const bool no_bits = P.xtrans && xtrans_no_bits(row, col, comp);
        const uint32_t rec = even_record(above1, above1 - STRIDE, col, no_bits);
        ev[comp * (MAX_LW / 2) + col] = rec;
        if (no_bits)
          lines[c[comp] * STRIDE + 1 + 2 * col] = uint16_t(rec & 0xFFFFu);
        uint32_t r0, r1;
        odd_record(above1, col, &r0, &r1);
        od[(comp * (MAX_LW / 2) + col) * 2] = r0;
        od[(comp * (MAX_LW / 2) + col) * 2 + 1] = r1;
      }
      __syncthreads();
      const int32_t t = (row % 3) * GRADS * 2;
      for (int32_t i0 = 0; i0 < half + 4 && status == RSX_OK; i0 += FJ_CHUNK) {
        // the window: from the word the walk stands at, when a chunk may outrun what is left
        const uint32_t k = s_k;
        if (!have_window || k - src.k0 + uint32_t(FJ_CHUNK_WORDS) > uint32_t(FJ_WIN)) {
          __syncthreads(); // (every lane has read s_k and has left the old window)
          for (int j = lane; j < FJ_WIN; j += FJ_THREADS)
            win[j] = fj_global_word(bytes, S.size, k + uint32_t(j));
          src.k0 = k;
          have_window = true;
          __syncthreads();
        }
        // (every lane alike: the same reads, and stores of the same values to the same places)
        const int32_t st = walk(B, P, lines + c[0] * STRIDE, lines + c[1] * STRIDE, i0,
                                imin(i0 + FJ_CHUNK, half + 4), ev, od, ge + t, go + t);
        if (lane == 0) {
          s_k = B.k;
          s_status = st;
        }
        __syncthreads();
        status = s_status;
      }
      if (status != RSX_OK)
        break;
      // the helper columns of the pass's two colours
      if (lane < 16) {
        const int32_t comp = lane >> 3;
        const int32_t kc = c[comp] < G0 ? 0 : c[comp] < B0 ? 1 : 2;
        const int32_t i = colour_first(kc) + 2 + (lane & 7);
        if (i < colour_first(kc) + colour_count(kc))
          extend_one(lines, i, P.lw);
      }
      __syncthreads();
    }
    if (status != RSX_OK)
      break;
    // the six image rows
    const int32_t groups = S.width / 8; // (raw_width and 768 are multiples of 24)
    for (int32_t idx = lane; idx < 6 * groups; idx += FJ_THREADS) {
      const int32_t r = idx / groups, x0 = (idx - r * groups) * 8;
      uint16_t v[8];
      for (int32_t j = 0; j < 8; ++j)
        v[j] = lines[out_index(P.xtrans != 0, r, x0 + j)];
      uint8_t* dst = out + size_t(6 * line + r) * S.pitch + size_t(x0) * 2;
      if (wide) {
        uint4 q;
        q.x = uint32_t(v[0]) | uint32_t(v[1]) << 16;
        q.y = uint32_t(v[2]) | uint32_t(v[3]) << 16;
        q.z = uint32_t(v[4]) | uint32_t(v[5]) << 16;
        q.w = uint32_t(v[6]) | uint32_t(v[7]) << 16;
        *reinterpret_cast<uint4*>(dst) = q;
      } else {
        for (int32_t j = 0; j < 8; ++j)
          reinterpret_cast<uint16_t*>(dst)[j] = v[j];
      }
    }
    if (line + 1 == S.total_lines)
      break;
    __syncthreads();
    // the last two lines of each colour become its first two
    constexpr int32_t LINE_WORDS = STRIDE / 2;
    for (int32_t kc = 0; kc < 3; ++kc) {
      const int32_t a = colour_first(kc), b = colour_count(kc);
      uint32_t* w = reinterpret_cast<uint32_t*>(lines);
      for (int32_t j = lane; j < 2 * LINE_WORDS; j += FJ_THREADS)
        w[a * LINE_WORDS + j] = w[(a + b - 2) * LINE_WORDS + j];
    }
    __syncthreads();
    if (lane < 3) {
      const int32_t a = colour_first(lane);
      lines[(a + 2) * STRIDE + P.lw + 1] = lines[(a + 1) * STRIDE + P.lw];
    }
    __syncthreads();
  }
  if (lane == 0) {
    A.strip_status[blockIdx.x] = uint32_t(status);
    if (status != RSX_OK)
      atomicMin(&A.job_status[S.job], S.strip << 8 | uint32_t(status));
  }
}

} // namespace

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
namespace {
struct FujiPlan final : DecoderPlan {
  rsx_ctx* ctx = nullptr;
  JobStatus status;
  std::vector<uint32_t> strip_base, n_strips; // per job, into the plan's strips
  DeviceBuffer d_strips, d_strip_status;
  std::vector<uint32_t> h_strip_status;
  uint32_t total_strips = 0;
  bool launched = false;
  int run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) override;
  int results(hipStream_t s, bool ran, int32_t* job_status, uint32_t* job_consumed) override;
  int row_status(hipStream_t s, int job, int32_t* statuses) override;
};
} // namespace

int fuji_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_fuji_job* jobs,
                     std::unique_ptr<DecoderPlan>* out) {
  auto p = std::make_unique<FujiPlan>();
  p->ctx = ctx;
  p->status.host.assign(n_jobs, RSX_OK);
  p->strip_base.assign(n_jobs, 0u);
  p->n_strips.assign(n_jobs, 0u);
  std::vector<FjStripDev> strips;
  for (int i = 0; i < n_jobs; ++i) {
    const rsx_fuji_job& j = jobs[i];
    int st = validate(&j.desc, &j.img);
    if (st == RSX_OK)
      st = check_strips(j.desc, j.in_bytes);
    if (st == RSX_OK && (j.img_offset % 2 != 0 || j.img.pitch_bytes % 2 != 0))
      st = RSX_ERR_INVALID_ARG;
    p->status.host[i] = st;
    p->strip_base[i] = uint32_t(strips.size());
    if (st != RSX_OK)
      continue;
    p->n_strips[i] = uint32_t(j.desc.n_strips);
    for (int32_t s = 0; s < j.desc.n_strips; ++s) {
      FjStripDev S;
      std::memset(&S, 0, sizeof S);
      S.in_off = j.in_offset + j.desc.strip_offset[s];
      S.out_off = j.img_offset + uint64_t(s) * BLOCK * 2;
      S.size = j.desc.strip_bytes[s];
      S.pitch = j.img.pitch_bytes;
      S.job = uint32_t(i);
      S.strip = uint32_t(s);
      S.width = strip_width(j.desc.raw_width, s);
      S.total_lines = j.desc.total_lines;
      S.raw_type = j.desc.raw_type;
      S.raw_bits = j.desc.raw_bits;
      strips.push_back(S);
    }
  }
  p->total_strips = uint32_t(strips.size());
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int st;
  if ((st = upload(ctx, p->d_strips, strips)) ||
      (st = p->d_strip_status.ensure(strips.size() * 4 + 16)) || (st = p->status.init()))
    return st;
  *out = std::move(p);
  return RSX_OK;
}

int FujiPlan::run(const void* in_dev, void* out_dev, hipStream_t s, KernelTimer* timer) {
  if (total_strips == 0)
    return RSX_OK; // (every job was rejected by the host)
  if (timer)
    timer->begin(s);
  FjArgs A{};
  A.in_base = static_cast<const uint8_t*>(in_dev);
  A.out_base = static_cast<uint8_t*>(out_dev);
  A.strips = static_cast<const FjStripDev*>(d_strips.ptr);
  A.strip_status = static_cast<uint32_t*>(d_strip_status.ptr);
  A.job_status = static_cast<uint32_t*>(status.dev.ptr);
  if (int st = status.reset(ctx, s))
    return st;
  hipLaunchKernelGGL(fuji_strip_kernel, dim3(total_strips), dim3(FJ_THREADS), 0, s, A);
  if (timer)
    timer->mark("fuji_strip_kernel");
  RSX_HIP_CHECK(ctx, hipGetLastError());
  launched = true;
  return RSX_OK;
}

int FujiPlan::results(hipStream_t s, bool ran, int32_t* job_status, uint32_t* job_consumed) {
  if (job_consumed)
    std::fill(job_consumed, job_consumed + status.host.size(), 0u);
  return status.fold(ctx, s, ran && total_strips != 0, 0xFFu, FoldOrder::LAST_FAILING, job_status);
}

int FujiPlan::row_status(hipStream_t s, int job, int32_t* statuses) {
  if (job < 0 || size_t(job) >= status.host.size() || !launched || n_strips[job] == 0 || !statuses)
    return RSX_ERR_INVALID_ARG;
  return fetch_words(ctx, s, d_strip_status, strip_base[job], n_strips[job], h_strip_status,
                     statuses);
}

} // namespace rsx
