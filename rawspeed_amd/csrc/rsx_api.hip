// rsx_api.hip -- the C-ABI entry points declared in include/rsx.h.
//
// Host glue only: validation, staging, plan bookkeeping, launches.  There is
// no CPU decode path anywhere in this library: without a GPU, context creation
// fails with RSX_ERR_DEVICE.
#include "rsx_device.h"
#include "rsx_internal.h"
#include "rsx_ljpeg.h"
#include "rsx_dng_deflate.h"
#include "rsx_ljpeg_dev.h"
#include "rsx_panasonic.h"
#include "rsx_panasonic_v4.h"
#include "rsx_phase_one.h"
#include "rsx_samsung_v0.h"
#include "rsx_fuji.h"
#include "rsx_fuji_core.h"
#include "rsx_olympus.h"
#include "rsx_olympus_core.h"
#include "rsx_kodak.h"
#include "rsx_kodak_core.h"
#include "rsx_crw.h"
#include "rsx_crw_core.h"
#include "rsx_fuji_rotate.h"
#include "rsx_fuji_rotate_core.h"
#include "rsx_sony_srf.h"
#include "rsx_sony_srf_core.h"
#include "rsx_image_hash.h"
#include "rsx_image_hash_core.h"
#include "rsx_samsung_v2.h"
#include "rsx_sony_arw2.h"
#include "rsx_nikon_snef.h"
#include "rsx_vc5.h"
#include "rsx_iiq_corr.h"
#include "rsx_dng_post.h"
#include "rsx_bad_pixels.h"
#include "rsx_scale.h"
#include "rsx_dng_jpeg.h"
#include "rsx_jpeg_core.h"
#include "rsx_encode.h"
#include "rsx_encode_core.h"
#include "rsx_fpwrite.h"
#include "rsx_fpwrite_core.h"
#include "rsx_dctwrite.h"
#include "rsx_dctwrite_core.h"
#include "rsx_deflate_core.h"

#include <algorithm>
#include <map>
#include <atomic>
#include <thread>
#include <cstring>
#include <memory>
#include <type_traits>

using namespace rsx;

// ---------------------------------------------------------------------------
// Plan
// ---------------------------------------------------------------------------
namespace {

enum PlanKind { PLAN_UNPACK, PLAN_SRAW, PLAN_DECODER };

struct UnpackLaunch {
  int mode = UNPACK_MODE_PACKED;
  int order = 0;
  int n_jobs = 0;
  uint32_t total_blocks = 0;
  DeviceBuffer d_jobs, d_block_start;
  std::vector<UnpackJobDev> jobs; // host copy (alignment flags patched per base)
  uintptr_t last_out_base = ~uintptr_t(0);
};

// in-run kernel time: launches a plan can time between two read-outs (rsx_stamp.h)
constexpr size_t TIMED_LAUNCHES = 64;

} // namespace

struct rsx_plan {
  rsx_ctx* ctx = nullptr;
  PlanKind kind = PLAN_UNPACK;
  int n_jobs = 0;
  std::vector<int32_t> job_status; // host-side validation result per job
  std::vector<UnpackLaunch> unpack;
  std::unique_ptr<DecoderPlan> dec; // PLAN_DECODER
  // PLAN_SRAW
  DeviceBuffer d_sraw_jobs, d_sraw_starts;
  int n_sraw = 0;
  uint32_t sraw_blocks = 0;
  bool sraw_versions[3] = {false, false, false};
  hipStream_t last_stream = nullptr;
  bool ran = false;
  // dominant-kernel timing: TIMED_LAUNCHES x STAMP_WORDS clock words the kernels fold their
  // entry and exit times into; `stamps_dirty` launches' worth has been handed out since the
  // buffer was last seeded, on `timed_streams`
  bool timing = false;
  DeviceBuffer d_stamps;
  size_t stamps_used = 0, stamps_dirty = 0;
  std::vector<hipStream_t> timed_streams;
  int wall_clock_khz = 0;
  // decoder plans: an event after every kernel of a timed run; the totals per kernel
  // name are folded in before the events are reused
  std::unique_ptr<KernelTimer> ktimer;
  bool ktimer_pending = false;
  std::vector<std::pair<const char*, double>> ktotals;
  int kruns = 0;
};

namespace {

int upload(rsx_ctx* ctx, DeviceBuffer& buf, const void* src, size_t bytes) {
  if (int st = buf.ensure(bytes ? bytes : 16))
    return st;
  if (bytes)
    RSX_HIP_CHECK(ctx, hipMemcpy(buf.ptr, src, bytes, hipMemcpyHostToDevice));
  return RSX_OK;
}

// The buffer is made by rsx_plan_set_timing(); once its TIMED_LAUNCHES sets of slots are
// handed out, further launches simply go untimed.
unsigned long long* next_stamps(rsx_plan* p, hipStream_t s) {
  if (!p->d_stamps.ptr || p->stamps_used == TIMED_LAUNCHES)
    return nullptr;
  if (std::find(p->timed_streams.begin(), p->timed_streams.end(), s) == p->timed_streams.end())
    p->timed_streams.push_back(s);
  unsigned long long* w =
      static_cast<unsigned long long*>(p->d_stamps.ptr) + p->stamps_used++ * STAMP_WORDS;
  p->stamps_dirty = std::max(p->stamps_dirty, p->stamps_used);
  return w;
}

// (first entry, last exit) = (~0, 0) in every slot handed out since the last seeding.  Waits
// for the timed launches first: never called between the steps of a timed loop.
int seed_stamps(rsx_plan* p, size_t launches) {
  rsx_ctx* ctx = p->ctx;
  for (hipStream_t s : p->timed_streams)
    RSX_HIP_CHECK(ctx, hipStreamSynchronize(s));
  p->timed_streams.clear();
  if (launches) {
    std::vector<unsigned long long> seed(launches * STAMP_WORDS, 0ull);
    for (size_t i = 0; i < seed.size(); i += 2)
      seed[i] = ~0ull;
    RSX_HIP_CHECK(ctx, hipMemcpy(p->d_stamps.ptr, seed.data(),
                                 seed.size() * sizeof(unsigned long long),
                                 hipMemcpyHostToDevice));
  }
  p->stamps_dirty = 0;
  return RSX_OK;
}

// add the durations of the last timed LJPEG run to the per-kernel totals
int fold_kernel_timer(rsx_plan* p) {
  if (!p->ktimer || !p->ktimer_pending)
    return RSX_OK;
  rsx_ctx* ctx = p->ctx;
  KernelTimer& t = *p->ktimer;
  p->ktimer_pending = false;
  if (t.n == 0)
    return RSX_OK;
  RSX_HIP_CHECK(ctx, hipEventSynchronize(t.ev[t.n]));
  for (int i = 0; i < t.n; ++i) {
    float ms = 0;
    RSX_HIP_CHECK(ctx, hipEventElapsedTime(&ms, t.ev[i], t.ev[i + 1]));
    bool found = false;
    for (auto& kv : p->ktotals)
      if (kv.first == t.name[i] || std::strcmp(kv.first, t.name[i]) == 0) {
        kv.second += ms;
        found = true;
        break;
      }
    if (!found)
      p->ktotals.emplace_back(t.name[i], double(ms));
  }
  ++p->kruns;
  return RSX_OK;
}

int flatten_unpack_job(const rsx_unpack_job& j, UnpackJobDev* out, int* order) {
  const rsx_unpack_desc& d = j.desc;
  if (int st = validate_unpack(d, j.img, size_t(j.in_bytes)))
    return st;
  if (j.img.pitch_bytes % 2 != 0)
    return RSX_ERR_INVALID_ARG;
  UnpackJobDev u{};
  u.in_offset = j.in_offset;
  u.stream_bytes = uint64_t(d.crop_h) * uint64_t(d.input_pitch_bytes);
  u.in_pitch = uint32_t(d.input_pitch_bytes);
  u.out_pitch = j.img.pitch_bytes;
  // h = min(h + oy, dim.y); rows [oy, h)  (UncompressedDecompressor.cpp:209-210)
  const int64_t rows_avail = int64_t(j.img.dim_y) - d.crop_y;
  u.n_rows = uint32_t(std::min<int64_t>(d.crop_h, rows_avail));
  u.cols = uint32_t(d.crop_w) * uint32_t(j.img.cpp);
  u.bps = uint32_t(d.bits_per_pixel);
  uint64_t out_off = j.img_offset + uint64_t(d.crop_y) * j.img.pitch_bytes;
  // Only the 16-bit LSB copyPixels path honours offset.x (:257-264); the
  // packed paths write from column 0 (:196) -- replicated.
  if (d.bit_order == RSX_ORDER_LSB && d.bits_per_pixel == 16)
    out_off += uint64_t(d.crop_x) * uint64_t(j.img.cpp) * 2;
  u.out_offset = out_off;
  unpack_blocks_for(&u);
  u.out_aligned = 0; // resolved at run time (needs the output base pointer)
  *out = u;
  *order = d.bit_order;
  return RSX_OK;
}

} // namespace

// ---------------------------------------------------------------------------
// Misc
// ---------------------------------------------------------------------------
// The lane pool is capped (RSX_MAX_LANES: every lane owns a stream, staging for a whole
// image and a cached plan with its scratch): a caller beyond the cap waits for a lane to
// come back instead of growing the pool with the thread count of the host program.
rsx_ctx::HostLane* rsx_ctx::acquire_lane(const std::vector<uint8_t>* want_key) {
  std::unique_lock<std::mutex> g(lanes_mu);
  while (true) {
    if (!lanes_free.empty()) {
      // (a lane whose cached plan was made from the same jobs, if there is one: the bands of
      // a split DNG call come back in any order)
      size_t pick = lanes_free.size() - 1;
      if (want_key)
        for (size_t k = 0; k < lanes_free.size(); ++k)
          if (lanes_free[k]->holds_plan(*want_key)) {
            pick = k;
            break;
          }
      HostLane* l = lanes_free[pick];
      lanes_free.erase(lanes_free.begin() + long(pick));
      return l;
    }
    if (lanes_all.size() < size_t(RSX_MAX_LANES))
      break;
    lanes_cv.wait(g);
  }
  auto l = std::make_unique<HostLane>();
  if (hipStreamCreateWithFlags(&l->stream, hipStreamNonBlocking) != hipSuccess)
    return nullptr;
  lanes_all.push_back(std::move(l));
  return lanes_all.back().get();
}

void rsx_ctx::release_lane(HostLane* l) {
  {
    std::lock_guard<std::mutex> g(lanes_mu);
    lanes_free.push_back(l);
  }
  lanes_cv.notify_one();
}

namespace {
struct LaneGuard {
  rsx_ctx* ctx;
  rsx_ctx::HostLane* lane;
  explicit LaneGuard(rsx_ctx* c, const std::vector<uint8_t>* want_key = nullptr)
      : ctx(c), lane(c->acquire_lane(want_key)) {}
  LaneGuard(const LaneGuard&) = delete;
  ~LaneGuard() {
    if (lane)
      ctx->release_lane(lane);
  }
};
} // namespace

static void set_error(rsx_ctx* ctx, const std::string& msg) {
  std::lock_guard<std::mutex> g(ctx->err_mu);
  ctx->last_error = msg;
}

// ---------------------------------------------------------------------------------------
// Downloads into the CALLER's memory (round 6; DESIGN 7 "the undelivered sixteen bytes").
//
// The caller's image is pageable.  A device-to-host copy into it is carried out by the
// runtime on the caller's pages (pinned for the copy); for a rectangle whose start, pitch or
// width is off the 16-byte grid that is a byte-granular copy kernel (16 x 16 lanes, a byte
// each), and ONE such copy left one 16-lane row segment of one workgroup undelivered in a
// few images of several hundred (round 5: 3-sample pixels, tiles of unequal heights; status
// OK, the caller's fill showing through; never reproduced outside the library, never on a
// copy that lies on the grid).  The rule since round 6, at EVERY download of the library:
//   * what lies on the 16-byte grid in the caller's memory AND on the device (start, pitch,
//     width) is copied straight into the image -- the path every frame of every benchmark
//     and test has taken since round 1;
//   * everything else goes through page-locked staging of the lane (hipHostMalloc): the
//     device side of such a copy is widened to the grid, so the runtime only ever sees
//     aligned copies into memory it pinned itself, and the host moves the bytes the caller
//     owns into the image.  A rectangle that merely starts or ends off the grid (an odd
//     width, a tile in the middle of a 3-sample image) is split: its aligned body goes
//     straight, the < 16 bytes a row on either side are staged as 16-byte columns.
// Nothing is written outside the rectangles (the reference's contract: row padding and other
// tiles' pixels are never touched, LJpegDecompressor.cpp:264-268,
// AbstractDngDecompressor.cpp:112-131).
// ---------------------------------------------------------------------------------------
namespace {

struct DownRect {
  uint8_t* host;      // first byte of the rectangle in the caller's image
  size_t host_pitch;
  const uint8_t* dev; // first byte of the rectangle on the device
  size_t dev_pitch;
  size_t bytes, rows; // width in bytes, rows
};

constexpr size_t PIN_HALF = size_t(8) << 20; // a half of the lane's staging

// a piece that goes through the staging: rows of `width` device bytes from `dev` (every
// dev_pitch; on the 16-byte grid) or, `linear`, the contiguous device range that holds them;
// of row y the host takes `take` bytes from offset `skip` (+ y * dev_pitch when linear)
struct StagedPiece {
  const uint8_t* dev;
  size_t dev_pitch, width, rows;
  bool linear;
  uint8_t* host;
  size_t host_pitch, skip, take;
};

int ensure_pin(rsx_ctx* ctx, rsx_ctx::HostLane* L) {
  if (!L->h_pin) {
    void* p = nullptr;
    if (hipHostMalloc(&p, 2 * PIN_HALF, hipHostMallocDefault) != hipSuccess || !p) {
      (void)hipGetLastError();
      return RSX_ERR_NOMEM;
    }
    L->h_pin = static_cast<uint8_t*>(p);
    L->h_pin_bytes = 2 * PIN_HALF;
  }
  for (hipEvent_t& e : L->ev_pin)
    if (!e)
      RSX_HIP_CHECK(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return RSX_OK;
}

inline bool on_grid(uintptr_t v) { return (v & 15u) == 0; }

// Queues the copies of `n` rectangles on `s` and returns when every byte is in the caller's
// memory (the stream is synchronised).  The device rows must be final on `s`.
int download_rects(rsx_ctx* ctx, rsx_ctx::HostLane* L, hipStream_t s, const DownRect* rects,
                   size_t n) {
  std::vector<StagedPiece> staged;
  hipError_t err = hipSuccess;
  auto direct = [&](uint8_t* host, size_t hp, const uint8_t* dev, size_t dp, size_t bytes,
                    size_t rows) {
    if (err != hipSuccess || bytes == 0 || rows == 0)
      return;
    if (rows == 1 || (bytes == hp && bytes == dp))
      err = hipMemcpyAsync(host, dev, rows == 1 ? bytes : bytes * rows, hipMemcpyDeviceToHost, s);
    else
      err = hipMemcpy2DAsync(host, hp, dev, dp, bytes, rows, hipMemcpyDeviceToHost, s);
  };
  // Several rectangles in one call (tiles of unequal heights side by side, a tile set with a
  // failed tile: what does not merge into one rectangle) share the pages of their rows.  Copied
  // straight, each would have the runtime pin its own, overlapping range of the caller's pages
  // -- the one constellation in which bytes were ever lost (profiles/r06/host_path_defect.md).
  // They all go through the staging; ONE rectangle's body goes straight.
  size_t n_live = 0;
  for (size_t i = 0; i < n; ++i)
    n_live += rects[i].bytes != 0 && rects[i].rows != 0;
  const bool all_staged = n_live >= 2;
  for (size_t i = 0; i < n; ++i) {
    const DownRect& r = rects[i];
    if (r.bytes == 0 || r.rows == 0)
      continue;
    const uintptr_t ha = reinterpret_cast<uintptr_t>(r.host), da = reinterpret_cast<uintptr_t>(r.dev);
    const bool pitches = (r.rows == 1) || (on_grid(r.host_pitch) && on_grid(r.dev_pitch));
    if (all_staged) {
      const size_t mis = da & 15u;
      if (on_grid(r.dev_pitch) || r.rows == 1)
        staged.push_back({r.dev - mis, r.dev_pitch, (mis + r.bytes + 15) & ~size_t(15), r.rows, false,
                          r.host, r.host_pitch, mis, r.bytes});
      else
        staged.push_back({r.dev, r.dev_pitch, r.bytes, r.rows, true, r.host, r.host_pitch, 0, r.bytes});
      continue;
    }
    if (pitches && on_grid(ha) && on_grid(da) && on_grid(r.bytes)) {
      direct(r.host, r.host_pitch, r.dev, r.dev_pitch, r.bytes, r.rows);
      continue;
    }
    if (pitches && (ha & 15u) == (da & 15u)) {
      // [head < 16][body on the grid][tail < 16]
      const size_t mis = ha & 15u;
      const size_t head = std::min(r.bytes, (16u - mis) & 15u);
      const size_t body = (r.bytes - head) & ~size_t(15);
      const size_t tail = r.bytes - head - body;
      if (head)
        staged.push_back({r.dev - mis, r.dev_pitch, 16, r.rows, false, r.host, r.host_pitch, mis, head});
      direct(r.host + head, r.host_pitch, r.dev + head, r.dev_pitch, body, r.rows);
      if (tail)
        staged.push_back({r.dev + head + body, r.dev_pitch, 16, r.rows, false,
                          r.host + head + body, r.host_pitch, 0, tail});
      continue;
    }
    // the host and the device disagree about the grid (a compact device rectangle for a
    // cropped host one), or a pitch is off it: everything through the staging
    const size_t mis = da & 15u;
    if (on_grid(r.dev_pitch) || r.rows == 1)
      staged.push_back({r.dev - mis, r.dev_pitch, (mis + r.bytes + 15) & ~size_t(15), r.rows, false,
                        r.host, r.host_pitch, mis, r.bytes});
    else
      staged.push_back({r.dev, r.dev_pitch, r.bytes, r.rows, true, r.host, r.host_pitch, 0, r.bytes});
  }
  if (err == hipSuccess && !staged.empty()) {
    if (int e = ensure_pin(ctx, L)) {
      (void)hipStreamSynchronize(s);
      return e;
    }
    // chunks = (piece, row range) that fit a half; copy of chunk c + 1 under the scatter of chunk c
    struct Chunk {
      size_t piece, y0, y1, lin_lo; // lin_lo: first device byte of a linear chunk, relative to piece.dev
    };
    std::vector<Chunk> chunks;
    for (size_t k = 0; k < staged.size(); ++k) {
      const StagedPiece& p = staged[k];
      const size_t per_row = p.linear ? p.dev_pitch : p.width;
      const size_t rows_per = std::max<size_t>(1, (PIN_HALF - 64) / std::max<size_t>(per_row, 1));
      for (size_t y = 0; y < p.rows; y += rows_per)
        chunks.push_back({k, y, std::min(p.rows, y + rows_per), 0});
    }
    auto issue = [&](size_t c) {
      Chunk& ch = chunks[c];
      const StagedPiece& p = staged[ch.piece];
      uint8_t* half = L->h_pin + (c & 1u) * PIN_HALF;
      if (!p.linear) {
        const size_t rows = ch.y1 - ch.y0;
        if (p.width > PIN_HALF - 64) { // (a single row wider than a half: cannot happen for images of < 8 MB a row)
          err = hipErrorInvalidValue;
          return;
        }
        err = rows == 1 || p.width == p.dev_pitch
                  ? hipMemcpyAsync(half, p.dev + ch.y0 * p.dev_pitch, p.width * rows, hipMemcpyDeviceToHost, s)
                  : hipMemcpy2DAsync(half, p.width, p.dev + ch.y0 * p.dev_pitch, p.dev_pitch, p.width,
                                     rows, hipMemcpyDeviceToHost, s);
      } else {
        // the device bytes of rows y0 .. y1 - 1, from the 16-byte boundary in front of them to
        // the one behind (the lane's device buffers start on the grid and end with slack)
        const uintptr_t d0 = reinterpret_cast<uintptr_t>(p.dev) + ch.y0 * p.dev_pitch;
        const uintptr_t d1 = reinterpret_cast<uintptr_t>(p.dev) + (ch.y1 - 1) * p.dev_pitch + p.take;
        const uintptr_t lo = d0 & ~uintptr_t(15), hi = (d1 + 15) & ~uintptr_t(15);
        ch.lin_lo = size_t(d0 - lo);
        if (hi - lo > PIN_HALF) {
          err = hipErrorInvalidValue;
          return;
        }
        err = hipMemcpyAsync(half, reinterpret_cast<const void*>(lo), size_t(hi - lo),
                             hipMemcpyDeviceToHost, s);
      }
      if (err == hipSuccess)
        err = hipEventRecord(L->ev_pin[c & 1u], s);
    };
    for (size_t c = 0; c < chunks.size() && c < 2 && err == hipSuccess; ++c)
      issue(c);
    for (size_t c = 0; c < chunks.size() && err == hipSuccess; ++c) {
      err = hipEventSynchronize(L->ev_pin[c & 1u]);
      if (err != hipSuccess)
        break;
      const Chunk& ch = chunks[c];
      const StagedPiece& p = staged[ch.piece];
      const uint8_t* half = L->h_pin + (c & 1u) * PIN_HALF;
      for (size_t y = ch.y0; y < ch.y1; ++y) {
        const uint8_t* src = p.linear ? half + ch.lin_lo + (y - ch.y0) * p.dev_pitch
                                      : half + (y - ch.y0) * p.width + p.skip;
        std::memcpy(p.host + y * p.host_pitch, src, p.take);
      }
      if (c + 2 < chunks.size())
        issue(c + 2);
    }
  }
  // (on every way out: the caller's image may be freed the moment the call returns)
  const hipError_t es = hipStreamSynchronize(s);
  if (err == hipSuccess)
    err = es;
  if (err != hipSuccess) {
    set_error(ctx, std::string("download: ") + hipGetErrorString(err));
    return RSX_ERR_DEVICE;
  }
  return RSX_OK;
}

} // namespace

extern "C" int rsx_abi_version(void) { return RSX_ABI_VERSION; }

extern "C" const char* rsx_status_string(int status) {
  switch (status) {
  case RSX_OK: return "RSX_OK";
  case RSX_ERR_INVALID_ARG: return "RSX_ERR_INVALID_ARG";
  case RSX_ERR_IO: return "RSX_ERR_IO";
  case RSX_ERR_BAD_HUFFMAN_CODE: return "RSX_ERR_BAD_HUFFMAN_CODE";
  case RSX_ERR_RESTART_MARKER: return "RSX_ERR_RESTART_MARKER";
  case RSX_ERR_INPUT_OVERFLOW: return "RSX_ERR_INPUT_OVERFLOW";
  case RSX_ERR_DEVICE: return "RSX_ERR_DEVICE";
  case RSX_ERR_UNSUPPORTED: return "RSX_ERR_UNSUPPORTED";
  case RSX_ERR_NOMEM: return "RSX_ERR_NOMEM";
  case RSX_ERR_TILE_ERRORS: return "RSX_ERR_TILE_ERRORS";
  case RSX_ERR_VALUE_RANGE: return "RSX_ERR_VALUE_RANGE";
  default: return "RSX_ERR_UNKNOWN";
  }
}

extern "C" int rsx_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess)
    return 0;
  return n;
}

extern "C" int rsx_ctx_create(int device, rsx_ctx** out_ctx) {
  if (!out_ctx)
    return RSX_ERR_INVALID_ARG;
  *out_ctx = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n)
    return RSX_ERR_DEVICE; // no GPU: fail loudly, there is no CPU fallback
  if (hipSetDevice(device) != hipSuccess)
    return RSX_ERR_DEVICE;
  auto* ctx = new rsx_ctx();
  ctx->device = device;
  // (read once per context, not per call: RSX_HOST_NO_OVERLAP=1 keeps large host-pointer
  // calls of the unpack family in one piece -- what the tests compare the banded path with)
  ctx->host_overlap = getenv("RSX_HOST_NO_OVERLAP") == nullptr;
  // (likewise once per context: the launches of crw_parse_kernel behind a CRW plan's first pass;
  // 0 leaves every window behind the first to the settling kernel; at most 32, so that a timed
  // run's 9 + rounds launches fit the KernelTimer's 48 marks)
  if (const char* e = getenv("RSX_CRW_SPEC_ROUNDS"))
    ctx->crw_spec_rounds = uint32_t(std::min(std::max(atoi(e), 0), 32));
  if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
    delete ctx;
    return RSX_ERR_DEVICE;
  }
  *out_ctx = ctx;
  return RSX_OK;
}

extern "C" void rsx_ctx_destroy(rsx_ctx* ctx) {
  if (!ctx)
    return;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) {
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipStreamDestroy(ctx->stream);
  }
  for (auto& l : ctx->lanes_all) {
    // the cached plan first: its destructor synchronises the stream it last ran on,
    // which is this lane's
    if (l->stream)
      (void)hipStreamSynchronize(l->stream);
    if (l->cached_plan)
      rsx_plan_destroy(l->cached_plan);
    l->cached_plan = nullptr;
    if (l->stream)
      (void)hipStreamDestroy(l->stream);
    for (hipEvent_t e : l->ev_up)
      (void)hipEventDestroy(e);
    l->ev_up.clear();
    if (l->stream_up)
      (void)hipStreamDestroy(l->stream_up);
    l->d_in.release();
    l->d_out.release();
    if (l->h_pin)
      (void)hipHostFree(l->h_pin);
    l->h_pin = nullptr;
    for (hipEvent_t& e : l->ev_pin) {
      if (e)
        (void)hipEventDestroy(e);
      e = nullptr;
    }
  }
  if (ctx->fast_ev)
    (void)hipEventDestroy(ctx->fast_ev);
  if (ctx->null_ev)
    (void)hipEventDestroy(ctx->null_ev);
  delete ctx;
}

// (a copy made under the lock, per calling thread: host-pointer calls from several
// threads may be writing the context's string at the same time)
extern "C" const char* rsx_ctx_last_error(const rsx_ctx* ctx) {
  if (!ctx)
    return "";
  static thread_local std::string copy;
  {
    std::lock_guard<std::mutex> g(const_cast<rsx_ctx*>(ctx)->err_mu);
    copy = ctx->last_error;
  }
  return copy.c_str();
}

extern "C" uint64_t rsx_ctx_host_calls(const rsx_ctx* ctx) {
  return ctx ? ctx->host_calls.load() : 0;
}
extern "C" uint64_t rsx_ctx_chunked_calls(const rsx_ctx* ctx) {
  return ctx ? ctx->chunked_calls.load() : 0;
}

// Page-locked host memory (rsx.h: optional; replaces nothing in the reference, it changes
// where RawImageData::createData, RawImage.cpp:68-100, and the file Buffer get their bytes).
extern "C" int rsx_host_alloc(rsx_ctx* ctx, size_t bytes, void** out) {
  if (!ctx || !out || bytes == 0)
    return RSX_ERR_INVALID_ARG;
  *out = nullptr;
  if (hipSetDevice(ctx->device) != hipSuccess)
    return RSX_ERR_DEVICE;
  void* p = nullptr;
  if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess || !p) {
    (void)hipGetLastError();
    return RSX_ERR_NOMEM;
  }
  *out = p;
  return RSX_OK;
}

extern "C" int rsx_host_free(rsx_ctx* ctx, void* p) {
  if (!ctx)
    return RSX_ERR_INVALID_ARG;
  if (!p)
    return RSX_OK;
  if (hipSetDevice(ctx->device) != hipSuccess)
    return RSX_ERR_DEVICE;
  if (hipHostFree(p) != hipSuccess) {
    (void)hipGetLastError();
    return RSX_ERR_INVALID_ARG;
  }
  return RSX_OK;
}

extern "C" int rsx_host_register(rsx_ctx* ctx, void* p, size_t bytes) {
  if (!ctx || !p || bytes == 0)
    return RSX_ERR_INVALID_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess)
    return RSX_ERR_DEVICE;
  const hipError_t e = hipHostRegister(p, bytes, hipHostRegisterDefault);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return e == hipErrorHostMemoryAlreadyRegistered ? RSX_OK : RSX_ERR_NOMEM;
  }
  return RSX_OK;
}

extern "C" int rsx_host_unregister(rsx_ctx* ctx, void* p) {
  if (!ctx || !p)
    return RSX_ERR_INVALID_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess)
    return RSX_ERR_DEVICE;
  if (hipHostUnregister(p) != hipSuccess) {
    (void)hipGetLastError();
    return RSX_ERR_INVALID_ARG;
  }
  return RSX_OK;
}

extern "C" int rsx_unpack_validate(const rsx_unpack_desc* d, const rsx_image* img,
                                   size_t in_bytes) {
  if (!d || !img)
    return RSX_ERR_INVALID_ARG;
  return validate_unpack(*d, *img, in_bytes);
}

extern "C" int rsx_ljpeg_validate(const rsx_ljpeg_desc* d, const rsx_image* img,
                                  size_t in_bytes) {
  (void)in_bytes;
  if (!d || !img)
    return RSX_ERR_INVALID_ARG;
  return validate_ljpeg(*d, *img);
}

extern "C" int rsx_cr2_validate(const rsx_cr2_desc* d, const rsx_image* img,
                                size_t in_bytes) {
  (void)in_bytes;
  if (!d || !img)
    return RSX_ERR_INVALID_ARG;
  return validate_cr2(*d, *img);
}

// ---------------------------------------------------------------------------
// Plans
// ---------------------------------------------------------------------------
extern "C" int rsx_unpack_plan_create(rsx_ctx* ctx, int n_jobs,
                                      const rsx_unpack_job* jobs,
                                      rsx_plan** out_plan) {
  if (!ctx || !jobs || n_jobs < 1 || !out_plan)
    return RSX_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  auto plan = std::make_unique<rsx_plan>();
  plan->ctx = ctx;
  plan->kind = PLAN_UNPACK;
  plan->n_jobs = n_jobs;
  plan->job_status.assign(n_jobs, RSX_OK);
  std::vector<UnpackJobDev> per_order[4];
  for (int i = 0; i < n_jobs; ++i) {
    UnpackJobDev u;
    int order = 0;
    const int st = flatten_unpack_job(jobs[i], &u, &order);
    plan->job_status[i] = st;
    if (st == RSX_OK && u.n_rows > 0)
      per_order[order].push_back(u);
  }
  for (int order = 0; order < 4; ++order) {
    auto& v = per_order[order];
    if (v.empty())
      continue;
    plan->unpack.emplace_back();
    UnpackLaunch& L = plan->unpack.back();
    L.order = order;
    L.n_jobs = int(v.size());
    std::vector<uint32_t> starts(v.size() + 1, 0);
    for (size_t k = 0; k < v.size(); ++k)
      starts[k + 1] = starts[k] + v[k].n_rows * v[k].segs_per_row;
    L.total_blocks = starts.back();
    L.jobs = v;
    if (int st = upload(ctx, L.d_jobs, v.data(), v.size() * sizeof(UnpackJobDev)))
      return st;
    if (int st = upload(ctx, L.d_block_start, starts.data(),
                        starts.size() * sizeof(uint32_t)))
      return st;
  }
  *out_plan = plan.release();
  return RSX_OK;
}

// F32 images: readUncompressedRaw's floating-point branches (:212-245)
extern "C" int rsx_unpack_f32_validate(const rsx_unpack_desc* d, const rsx_image* img,
                                       size_t in_bytes) {
  if (!d || !img)
    return RSX_ERR_INVALID_ARG;
  return validate_unpack_f32(*d, *img, in_bytes);
}

extern "C" int rsx_unpack_f32_plan_create(rsx_ctx* ctx, int n_jobs,
                                          const rsx_unpack_job* jobs,
                                          rsx_plan** out_plan) {
  if (!ctx || !jobs || n_jobs < 1 || !out_plan)
    return RSX_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  auto plan = std::make_unique<rsx_plan>();
  plan->ctx = ctx;
  plan->kind = PLAN_UNPACK;
  plan->n_jobs = n_jobs;
  plan->job_status.assign(n_jobs, RSX_OK);
  struct Class {
    int order, bps;
    std::vector<UnpackJobDev> v;
  };
  Class classes[5] = {{RSX_ORDER_LSB, 32, {}}, {RSX_ORDER_LSB, 16, {}},
                      {RSX_ORDER_LSB, 24, {}}, {RSX_ORDER_MSB, 16, {}},
                      {RSX_ORDER_MSB, 24, {}}};
  for (int i = 0; i < n_jobs; ++i) {
    const rsx_unpack_job& j = jobs[i];
    const rsx_unpack_desc& d = j.desc;
    int st = validate_unpack_f32(d, j.img, size_t(j.in_bytes));
    if (st == RSX_OK && j.img.pitch_bytes % 4 != 0)
      st = RSX_ERR_INVALID_ARG;
    plan->job_status[i] = st;
    if (st != RSX_OK)
      continue;
    UnpackJobDev u{};
    u.in_offset = j.in_offset;
    u.stream_bytes = uint64_t(d.crop_h) * uint64_t(d.input_pitch_bytes);
    u.in_pitch = uint32_t(d.input_pitch_bytes);
    u.out_pitch = j.img.pitch_bytes;
    const int64_t rows_avail = int64_t(j.img.dim_y) - d.crop_y; // :209-210
    u.n_rows = uint32_t(std::min<int64_t>(d.crop_h, rows_avail));
    u.cols = uint32_t(d.crop_w) * uint32_t(j.img.cpp);
    u.bps = uint32_t(d.bits_per_pixel);
    // copyPixels starts at out(y, offset.x * cpp) (:216-217), decodePackedFP
    // writes out(row, offset.x + col) (:181)
    const uint64_t x0 = d.bits_per_pixel == 32 ? uint64_t(d.crop_x) * j.img.cpp
                                               : uint64_t(d.crop_x);
    u.out_offset = j.img_offset + uint64_t(d.crop_y) * j.img.pitch_bytes + x0 * 4;
    unpack_fp_blocks_for(&u);
    if (u.n_rows == 0)
      continue;
    int cls = 0;
    if (d.bits_per_pixel != 32)
      cls = (d.bit_order == RSX_ORDER_MSB ? 3 : 1) + (d.bits_per_pixel == 24 ? 1 : 0);
    classes[cls].v.push_back(u);
  }
  for (Class& c : classes) {
    if (c.v.empty())
      continue;
    plan->unpack.emplace_back();
    UnpackLaunch& L = plan->unpack.back();
    L.mode = UNPACK_MODE_FP;
    L.order = (c.bps << 8) | c.order;
    L.n_jobs = int(c.v.size());
    std::vector<uint32_t> starts(c.v.size() + 1, 0);
    for (size_t k = 0; k < c.v.size(); ++k)
      starts[k + 1] = starts[k] + c.v[k].n_rows * c.v[k].segs_per_row;
    L.total_blocks = starts.back();
    L.jobs = c.v;
    if (int st = upload(ctx, L.d_jobs, c.v.data(), c.v.size() * sizeof(UnpackJobDev)))
      return st;
    if (int st = upload(ctx, L.d_block_start, starts.data(),
                        starts.size() * sizeof(uint32_t)))
      return st;
  }
  *out_plan = plan.release();
  return RSX_OK;
}

// decode8BitRaw<true> is the 8-bit packed walk over rows of w bytes;
// decode12BitRawUnpackedLeftAligned<e> the 16-bit LSB/MSB walk + ">> 4";
// decode12BitRawWithControl<e> has its own kernel.  All three write from pixel
// (0,0) and count `w` in samples of the uncropped array (cpp is not applied).
extern "C" int rsx_unpack_variant_validate(const rsx_unpack_variant_desc* d,
                                           const rsx_image* img, size_t in_bytes) {
  if (!d || !img)
    return RSX_ERR_INVALID_ARG;
  return validate_unpack_variant(*d, *img, in_bytes);
}

extern "C" int rsx_unpack_variant_plan_create(rsx_ctx* ctx, int n_jobs,
                                              const rsx_unpack_variant_job* jobs,
                                              rsx_plan** out_plan) {
  if (!ctx || !jobs || n_jobs < 1 || !out_plan)
    return RSX_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  auto plan = std::make_unique<rsx_plan>();
  plan->ctx = ctx;
  plan->kind = PLAN_UNPACK;
  plan->n_jobs = n_jobs;
  plan->job_status.assign(n_jobs, RSX_OK);
  // launch classes: [mode][order]
  struct Class {
    int mode, order;
    std::vector<UnpackJobDev> v;
  };
  Class classes[6] = {{UNPACK_MODE_PACKED, RSX_ORDER_LSB, {}},
                      {UNPACK_MODE_SHIFT, RSX_ORDER_LSB, {}},
                      {UNPACK_MODE_SHIFT, RSX_ORDER_MSB, {}},
                      {UNPACK_MODE_CONTROL, RSX_ORDER_LSB, {}},
                      {UNPACK_MODE_CONTROL, RSX_ORDER_MSB, {}},
                      {UNPACK_MODE_LUT8, RSX_ORDER_LSB, {}}};
  std::vector<uint16_t> luts; // tables of the LUT8 class, in job order
  for (int i = 0; i < n_jobs; ++i) {
    const rsx_unpack_variant_job& j = jobs[i];
    int st = validate_unpack_variant(j.desc, j.img, size_t(j.in_bytes));
    if (st == RSX_OK && j.img.pitch_bytes % 2 != 0)
      st = RSX_ERR_INVALID_ARG;
    plan->job_status[i] = st;
    if (st != RSX_OK)
      continue;
    uint64_t bpl = 0;
    unpack_variant_bytes_per_line(j.desc, &bpl);
    UnpackJobDev u{};
    u.in_offset = j.in_offset;
    u.stream_bytes = bpl * uint64_t(j.desc.h);
    u.in_pitch = uint32_t(bpl);
    u.out_pitch = j.img.pitch_bytes;
    u.n_rows = uint32_t(j.desc.h);
    u.cols = uint32_t(j.desc.w);
    u.out_offset = j.img_offset;
    int cls = 0;
    switch (j.desc.variant) {
    case RSX_UNPACK_8BIT_RAW:
      u.bps = 8;
      unpack_blocks_for(&u);
      cls = 0;
      break;
    case RSX_UNPACK_8BIT_LOOKUP:
      u.bps = 8;
      u.post_shift = uint32_t(luts.size() / 256);
      luts.insert(luts.end(), j.desc.lut, j.desc.lut + 256);
      unpack_blocks_for(&u);
      cls = 5;
      break;
    case RSX_UNPACK_12BIT_UNPACKED_LEFT_ALIGNED:
      u.bps = 16;
      u.post_shift = 4;
      unpack_blocks_for(&u);
      cls = j.desc.big_endian ? 2 : 1;
      break;
    default:
      u.bps = j.desc.big_endian ? 1 : 0;
      unpack_control_blocks_for(&u);
      cls = j.desc.big_endian ? 4 : 3;
      break;
    }
    classes[cls].v.push_back(u);
  }
  for (Class& c : classes) {
    if (c.v.empty())
      continue;
    plan->unpack.emplace_back();
    UnpackLaunch& L = plan->unpack.back();
    L.mode = c.mode;
    L.order = c.order;
    L.n_jobs = int(c.v.size());
    std::vector<uint32_t> starts(c.v.size() + 1, 0);
    for (size_t k = 0; k < c.v.size(); ++k)
      starts[k + 1] = starts[k] + c.v[k].n_rows * c.v[k].segs_per_row;
    L.total_blocks = starts.back();
    L.jobs = c.v;
    // the LUT8 class keeps its tables right behind the job array
    std::vector<uint8_t> blob(c.v.size() * sizeof(UnpackJobDev) +
                              (c.mode == UNPACK_MODE_LUT8 ? luts.size() * 2 : 0));
    std::memcpy(blob.data(), c.v.data(), c.v.size() * sizeof(UnpackJobDev));
    if (c.mode == UNPACK_MODE_LUT8)
      std::memcpy(blob.data() + c.v.size() * sizeof(UnpackJobDev), luts.data(),
                  luts.size() * 2);
    if (int st = upload(ctx, L.d_jobs, blob.data(), blob.size()))
      return st;
    if (int st = upload(ctx, L.d_block_start, starts.data(),
                        starts.size() * sizeof(uint32_t)))
      return st;
  }
  *out_plan = plan.release();
  return RSX_OK;
}

// Whether 16-byte stores are legal depends on the run-time output base; the
// flag is re-resolved (and re-uploaded) only when the base pointer changes.
namespace {

int run_unpack(rsx_plan* p, const void* in_dev, void* out_dev, hipStream_t s) {
  rsx_ctx* ctx = p->ctx;
  for (UnpackLaunch& L : p->unpack) {
    const uintptr_t base = reinterpret_cast<uintptr_t>(out_dev);
    if (base != L.last_out_base) {
      bool changed = false;
      for (auto& u : L.jobs) {
        const uintptr_t a = base + u.out_offset;
        const uint32_t al = ((a & 15) == 0 && (u.out_pitch & 15) == 0) ? 1u : 0u;
        if (al != u.out_aligned) {
          u.out_aligned = al;
          changed = true;
        }
      }
      if (changed)
        RSX_HIP_CHECK(ctx, hipMemcpyAsync(L.d_jobs.ptr, L.jobs.data(),
                                          L.jobs.size() * sizeof(UnpackJobDev),
                                          hipMemcpyHostToDevice, s));
      L.last_out_base = base;
    }
    // timed: the kernel stamps its own begin and end (rsx_stamp.h); the launch is the same
    // single packet either way
    unsigned long long* stamps = p->timing && L.total_blocks ? next_stamps(p, s) : nullptr;
    RSX_HIP_CHECK(ctx, launch_unpack_mode(L.mode, L.order,
                                          static_cast<const UnpackJobDev*>(L.d_jobs.ptr),
                                          static_cast<const uint32_t*>(L.d_block_start.ptr),
                                          L.n_jobs, L.total_blocks, in_dev, out_dev, s, stamps));
  }
  return RSX_OK;
}

} // namespace

extern "C" int rsx_plan_run(rsx_plan* plan, const void* in_dev, void* out_dev,
                            void* stream) {
  if (!plan || !in_dev || !out_dev)
    return RSX_ERR_INVALID_ARG;
  rsx_ctx* ctx = plan->ctx;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
  if (!stream) {
    // The convenience path: the context's own stream is hipStreamNonBlocking, i.e. NOT ordered behind
    // what the caller has queued on the null stream -- a fill of the output buffer, a device-to-device
    // copy of the input, a hipMemset (asynchronous with respect to the host on this runtime).  The run is
    // put behind the null stream's work so far; a caller who passes a stream orders it himself.
    if (!ctx->null_ev)
      RSX_HIP_CHECK(ctx, hipEventCreateWithFlags(&ctx->null_ev, hipEventDisableTiming));
    RSX_HIP_CHECK(ctx, hipEventRecord(ctx->null_ev, nullptr));
    RSX_HIP_CHECK(ctx, hipStreamWaitEvent(s, ctx->null_ev, 0));
  }
  plan->last_stream = s;
  plan->ran = true;
  if (plan->kind == PLAN_UNPACK)
    return run_unpack(plan, in_dev, out_dev, s);
  if (plan->kind == PLAN_SRAW) {
    unsigned long long* stamps =
        plan->timing && plan->sraw_blocks ? next_stamps(plan, s) : nullptr;
    RSX_HIP_CHECK(ctx, launch_sraw(static_cast<const SrawJobDev*>(plan->d_sraw_jobs.ptr),
                                   static_cast<const uint32_t*>(plan->d_sraw_starts.ptr),
                                   plan->n_sraw, plan->sraw_blocks, plan->sraw_versions,
                                   in_dev, out_dev, s, stamps));
    return RSX_OK;
  }
  if (!plan->timing)
    return plan->dec->run(in_dev, out_dev, s, nullptr);
  if (int st = fold_kernel_timer(plan)) // (waits for the previous timed run)
    return st;
  if (!plan->ktimer)
    plan->ktimer = std::make_unique<KernelTimer>();
  plan->ktimer_pending = true;
  return plan->dec->run(in_dev, out_dev, s, plan->ktimer.get());
}

extern "C" int rsx_plan_results(rsx_plan* plan, int32_t* job_status,
                                uint32_t* job_consumed) {
  if (!plan)
    return RSX_ERR_INVALID_ARG;
  rsx_ctx* ctx = plan->ctx;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (plan->ran)
    RSX_HIP_CHECK(ctx, hipStreamSynchronize(plan->last_stream));
  int rc = RSX_OK;
  if (plan->kind == PLAN_UNPACK || plan->kind == PLAN_SRAW) {
    for (int i = 0; i < plan->n_jobs; ++i) {
      if (job_status)
        job_status[i] = plan->job_status[i];
      if (job_consumed)
        job_consumed[i] = 0;
      if (plan->job_status[i] != RSX_OK)
        rc = plan->job_status[i];
    }
    return rc;
  }
  return plan->dec->results(plan->last_stream, plan->ran, job_status, job_consumed);
}

extern "C" int rsx_plan_set_timing(rsx_plan* plan, int enable) {
  if (!plan)
    return RSX_ERR_INVALID_ARG;
  plan->timing = enable != 0;
  plan->stamps_used = 0;
  plan->ktotals.clear();
  plan->kruns = 0;
  plan->ktimer_pending = false;
  if (plan->kind == PLAN_DECODER)
    return RSX_OK; // its events are created on the first timed run
  rsx_ctx* ctx = plan->ctx;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (plan->timing && !plan->d_stamps.ptr) {
    // the slots are made and seeded here, outside timed regions
    if (int st = plan->d_stamps.ensure(TIMED_LAUNCHES * STAMP_WORDS * sizeof(unsigned long long)))
      return st;
    RSX_HIP_CHECK(ctx, hipDeviceGetAttribute(&plan->wall_clock_khz,
                                             hipDeviceAttributeWallClockRate, ctx->device));
    if (plan->wall_clock_khz <= 0)
      return RSX_ERR_DEVICE;
    return seed_stamps(plan, TIMED_LAUNCHES);
  }
  // what was timed and not read out is dropped
  return plan->stamps_dirty ? seed_stamps(plan, plan->stamps_dirty) : RSX_OK;
}

extern "C" int rsx_plan_kernel_table(rsx_plan* plan, int cap, const char** names,
                                     double* avg_ms, int* n_kernels, int* n_runs) {
  if (!plan || plan->kind != PLAN_DECODER || !plan->timing)
    return RSX_ERR_INVALID_ARG;
  rsx_ctx* ctx = plan->ctx;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (int st = fold_kernel_timer(plan))
    return st;
  if (plan->kruns == 0)
    return RSX_ERR_INVALID_ARG;
  int n = 0;
  for (const auto& kv : plan->ktotals) {
    if (n < cap) {
      if (names)
        names[n] = kv.first;
      if (avg_ms)
        avg_ms[n] = kv.second / plan->kruns;
    }
    ++n;
  }
  if (n_kernels)
    *n_kernels = n;
  if (n_runs)
    *n_runs = plan->kruns;
  return RSX_OK;
}

extern "C" int rsx_plan_kernel_time(rsx_plan* plan, const char** kernel_name,
                                    double* avg_ms, int* n_launches) {
  if (!plan || !plan->timing)
    return RSX_ERR_INVALID_ARG;
  rsx_ctx* ctx = plan->ctx;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (plan->kind == PLAN_DECODER) {
    // the dominant kernel = the one with the largest share of the timed runs
    if (int st = fold_kernel_timer(plan))
      return st;
    if (plan->kruns == 0 || plan->ktotals.empty())
      return RSX_ERR_INVALID_ARG;
    const auto* best = &plan->ktotals[0];
    for (const auto& kv : plan->ktotals)
      if (kv.second > best->second)
        best = &kv;
    if (kernel_name)
      *kernel_name = best->first;
    if (avg_ms)
      *avg_ms = best->second / plan->kruns;
    if (n_launches)
      *n_launches = plan->kruns;
    plan->ktotals.clear();
    plan->kruns = 0;
    return RSX_OK;
  }
  if (plan->stamps_used == 0)
    return RSX_ERR_INVALID_ARG;
  // per launch: last exit - first entry over its slots, in ticks of the device's wall clock
  const size_t n = plan->stamps_used;
  for (hipStream_t s : plan->timed_streams)
    RSX_HIP_CHECK(ctx, hipStreamSynchronize(s));
  std::vector<unsigned long long> w(n * STAMP_WORDS);
  RSX_HIP_CHECK(ctx, hipMemcpy(w.data(), plan->d_stamps.ptr,
                               w.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  double total = 0;
  for (size_t i = 0; i < n; ++i) {
    unsigned long long begin = ~0ull, end = 0;
    for (size_t k = 0; k < STAMP_WORDS; k += 2) {
      begin = std::min(begin, w[i * STAMP_WORDS + k]);
      end = std::max(end, w[i * STAMP_WORDS + k + 1]);
    }
    if (end > begin)
      total += double(end - begin) / double(plan->wall_clock_khz);
  }
  if (kernel_name)
    *kernel_name = plan->kind == PLAN_SRAW ? "sraw_kernel"
                   : (!plan->unpack.empty() &&
                      plan->unpack[0].mode == UNPACK_MODE_CONTROL)
                       ? "unpack_control_kernel"
                       : unpack_kernel_name();
  if (avg_ms)
    *avg_ms = total / double(n);
  if (n_launches)
    *n_launches = int(n);
  plan->stamps_used = 0;
  return seed_stamps(plan, plan->stamps_dirty);
}

extern "C" void rsx_plan_destroy(rsx_plan* plan) {
  if (!plan)
    return;
  rsx_ctx* ctx = plan->ctx;
  {
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    (void)hipSetDevice(ctx->device);
    if (plan->ran)
      (void)hipStreamSynchronize(plan->last_stream);
    for (auto& L : plan->unpack) {
      L.d_jobs.release();
      L.d_block_start.release();
    }
    plan->d_sraw_jobs.release();
    plan->d_sraw_starts.release();
    for (hipStream_t s : plan->timed_streams)
      (void)hipStreamSynchronize(s);
    plan->d_stamps.release();
    if (plan->ktimer)
      for (int i = 0; i < plan->ktimer->created; ++i)
        (void)hipEventDestroy(plan->ktimer->ev[i]);
    plan->dec.reset();
  }
  delete plan;
}

// ---------------------------------------------------------------------------
// Host-pointer calls: stage H2D, run a temporary plan, stage D2H.
// ---------------------------------------------------------------------------
namespace {

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Runs n unpack tiles that all write into the same host image.
int unpack_host(rsx_ctx* ctx, int n, const rsx_unpack_desc* descs,
                const uint8_t* const* ins, const size_t* in_bytes,
                const rsx_image* img, int32_t* statuses) {
  ++ctx->host_calls;
  // device-side layout: inputs back to back (16-byte aligned), one compact
  // output rectangle per tile
  std::vector<rsx_unpack_job> jobs(n);
  std::vector<int32_t> st(n, RSX_OK);
  size_t in_total = 0, out_total = 0;
  struct OutRect {
    size_t dev_off, dev_pitch, width_bytes, rows, host_off;
  };
  std::vector<OutRect> rects(n);
  for (int i = 0; i < n; ++i) {
    st[i] = validate_unpack(descs[i], *img, in_bytes[i]);
    if (st[i] != RSX_OK)
      continue;
    const rsx_unpack_desc& d = descs[i];
    const size_t strip = size_t(d.crop_h) * size_t(d.input_pitch_bytes);
    rsx_unpack_job& j = jobs[i];
    j.desc = d;
    j.in_offset = in_total;
    j.in_bytes = strip;
    in_total += align_up(strip, 16);
    const size_t cols = size_t(d.crop_w) * size_t(img->cpp);
    const int64_t rows =
        std::min<int64_t>(d.crop_h, int64_t(img->dim_y) - d.crop_y);
    const bool copy_path = d.bit_order == RSX_ORDER_LSB && d.bits_per_pixel == 16;
    OutRect r;
    r.dev_pitch = align_up(cols * 2, 16);
    r.width_bytes = cols * 2;
    r.rows = size_t(std::max<int64_t>(rows, 0));
    r.dev_off = out_total;
    r.host_off = size_t(d.crop_y) * img->pitch_bytes +
                 (copy_path ? size_t(d.crop_x) * img->cpp * 2 : 0);
    out_total += r.dev_pitch * r.rows;
    rects[i] = r;
    // The device image view is the compact rectangle: same dims as the host
    // image but re-based so that row crop_y, column 0 (or crop_x for the copy
    // path) is the rectangle's origin.
    j.img = *img;
    j.img.pitch_bytes = uint32_t(r.dev_pitch);
    j.img_offset = 0; // patched below via desc-relative offset
  }
  LaneGuard lane(ctx); // staging + stream of this call
  if (!lane.lane)
    return RSX_ERR_DEVICE;
  if (int e = lane.lane->d_in.ensure(in_total + 16))
    return e;
  if (int e = lane.lane->d_out.ensure(out_total + 16))
    return e;
  hipStream_t s = lane.lane->stream;
  auto upload_all = [&]() -> int {
    for (int i = 0; i < n; ++i) {
      if (st[i] != RSX_OK)
        continue;
      RSX_HIP_CHECK(ctx, hipMemcpyAsync(static_cast<uint8_t*>(lane.lane->d_in.ptr) +
                                            jobs[i].in_offset,
                                        ins[i], jobs[i].in_bytes,
                                        hipMemcpyHostToDevice, s));
    }
    return RSX_OK;
  };
  // Build device jobs directly (the compact rectangles are not expressible as
  // a plain image view when crop_y > 0, so bypass flatten's offset arithmetic).
  std::vector<UnpackJobDev> per_order[4];
  for (int i = 0; i < n; ++i) {
    if (st[i] != RSX_OK || rects[i].rows == 0)
      continue;
    const rsx_unpack_desc& d = descs[i];
    UnpackJobDev u{};
    u.in_offset = jobs[i].in_offset;
    u.stream_bytes = uint64_t(d.crop_h) * uint64_t(d.input_pitch_bytes);
    u.in_pitch = uint32_t(d.input_pitch_bytes);
    u.out_pitch = uint32_t(rects[i].dev_pitch);
    u.n_rows = uint32_t(rects[i].rows);
    u.cols = uint32_t(d.crop_w) * uint32_t(img->cpp);
    u.bps = uint32_t(d.bits_per_pixel);
    u.out_offset = rects[i].dev_off;
    unpack_blocks_for(&u);
    const uintptr_t a = reinterpret_cast<uintptr_t>(lane.lane->d_out.ptr) + u.out_offset;
    u.out_aligned = ((a & 15) == 0 && (u.out_pitch & 15) == 0) ? 1u : 0u;
    per_order[d.bit_order].push_back(u);
  }
  DeviceBuffer d_jobs, d_starts;
  // Large inputs (a whole frame through readUncompressedRaw, the tiles of an uncompressed
  // DNG): in row bands, the upload of band k + 1 (a helper thread, a stream of its own) under
  // the unpack and the download of band k.  PCIe is full duplex and the two directions have
  // DMA engines of their own, but a copy from or to pageable memory keeps its calling thread
  // until it is done -- so one thread per direction.  cfg 2: 78 MB up + 89 MB down took their
  // sum at 56 GB/s, 3.0 ms; banded 2.3 ms.
  {
    constexpr size_t BAND_BYTES = size_t(8) << 20, OVERLAP_MIN = size_t(16) << 20;
    constexpr int MAX_BANDS = 32;
    struct Band {
      UnpackJobDev u;
      int order;
      const uint8_t* src;
      uint8_t* dst;
      uint32_t blocks;
      size_t dev_pitch, width_bytes;
    };
    std::vector<Band> bands;
    size_t in_used_total = 0;
    for (int i = 0; i < n; ++i)
      if (st[i] == RSX_OK && rects[i].rows != 0)
        in_used_total += size_t(rects[i].rows) * size_t(descs[i].input_pitch_bytes);
    if (in_used_total >= OVERLAP_MIN && ctx->host_overlap) {
      size_t k_of_order[4] = {0, 0, 0, 0};
      for (int i = 0; i < n; ++i) {
        if (st[i] != RSX_OK || rects[i].rows == 0)
          continue;
        const rsx_unpack_desc& d = descs[i];
        const OutRect& r = rects[i];
        const UnpackJobDev base = per_order[d.bit_order][k_of_order[d.bit_order]++];
        const size_t in_used = size_t(r.rows) * size_t(d.input_pitch_bytes);
        const size_t nb = std::max<size_t>(1, std::min<size_t>(8, in_used / BAND_BYTES));
        const uint32_t rows_per = uint32_t((r.rows + nb - 1) / nb);
        for (uint32_t r0 = 0; r0 < r.rows; r0 += rows_per) {
          Band bd;
          bd.u = base;
          bd.u.n_rows = uint32_t(std::min<size_t>(rows_per, r.rows - r0));
          bd.u.in_offset = base.in_offset + uint64_t(r0) * base.in_pitch;
          bd.u.out_offset = base.out_offset + uint64_t(r0) * base.out_pitch;
          bd.u.stream_bytes = uint64_t(bd.u.n_rows) * base.in_pitch;
          bd.blocks = unpack_blocks_for(&bd.u);
          bd.order = d.bit_order;
          bd.src = ins[i] + size_t(r0) * base.in_pitch;
          bd.dst = static_cast<uint8_t*>(img->data) + r.host_off + size_t(r0) * img->pitch_bytes;
          bd.dev_pitch = r.dev_pitch;
          bd.width_bytes = r.width_bytes;
          bands.push_back(bd);
        }
      }
    }
    const int nb = int(bands.size());
    if (nb >= 2 && nb <= MAX_BANDS && lane.lane->ensure_overlap(nb)) {
      std::vector<UnpackJobDev> bj(nb);
      std::vector<uint32_t> starts(2 * size_t(nb));
      for (int b = 0; b < nb; ++b) {
        bj[b] = bands[b].u;
        starts[2 * b] = 0;
        starts[2 * b + 1] = bands[b].blocks;
      }
      if (int e = d_jobs.ensure(bj.size() * sizeof(UnpackJobDev)))
        return e;
      if (int e = d_starts.ensure(starts.size() * sizeof(uint32_t)))
        return e;
      {
        hipError_t e = hipMemcpyAsync(d_jobs.ptr, bj.data(), bj.size() * sizeof(UnpackJobDev),
                                      hipMemcpyHostToDevice, s);
        if (e == hipSuccess)
          e = hipMemcpyAsync(d_starts.ptr, starts.data(), starts.size() * sizeof(uint32_t),
                             hipMemcpyHostToDevice, s);
        if (e != hipSuccess) {
          (void)hipStreamSynchronize(s); // (bj / starts / the device temporaries outlive the copies)
          set_error(ctx, std::string("unpack (banded): ") + hipGetErrorString(e));
          return RSX_ERR_DEVICE;
        }
      }
      // progress of the uploader: bands whose copy + event are queued (under a mutex, the
      // caller sleeps on the condition variable)
      struct Progress {
        std::mutex m;
        std::condition_variable cv;
        int ready = 0;
        bool failed = false;
      } prog;
      uint8_t* d_in_base = static_cast<uint8_t*>(lane.lane->d_in.ptr);
      hipStream_t s_up = lane.lane->stream_up;
      const int device = ctx->device;
      auto upload_bands = [&]() {
        bool ok = hipSetDevice(device) == hipSuccess;
        for (int b = 0; b < nb; ++b) {
          if (ok) {
            hipError_t e = hipMemcpyAsync(d_in_base + bands[b].u.in_offset, bands[b].src,
                                          size_t(bands[b].u.stream_bytes), hipMemcpyHostToDevice,
                                          s_up);
            if (e == hipSuccess)
              e = hipEventRecord(lane.lane->ev_up[b], s_up);
            ok = e == hipSuccess;
          }
          {
            std::lock_guard<std::mutex> g(prog.m);
            prog.ready = b + 1;
            prog.failed = prog.failed || !ok;
          }
          prog.cv.notify_all();
        }
      };
      // (a persistent helper of the context; none to be had: the uploads first, then the rest)
      rsx::HelperPool::Handle uploader = ctx->helpers.submit(upload_bands);
      if (!uploader)
        upload_bands();
      hipError_t err = hipSuccess;
      bool up_failed = false;
      for (int b = 0; b < nb && err == hipSuccess; ++b) {
        {
          std::unique_lock<std::mutex> g(prog.m);
          prog.cv.wait(g, [&]() { return prog.ready > b; });
          up_failed = prog.failed;
        }
        if (up_failed)
          break;
        err = hipStreamWaitEvent(s, lane.lane->ev_up[b], 0);
        if (err == hipSuccess)
          err = launch_unpack(bands[b].order, static_cast<UnpackJobDev*>(d_jobs.ptr) + b,
                              static_cast<uint32_t*>(d_starts.ptr) + 2 * b, 1, bands[b].blocks,
                              lane.lane->d_in.ptr, lane.lane->d_out.ptr, s);
        if (err == hipSuccess) {
          // (download_rects: on the grid straight into the image, the rest through the lane's
          // page-locked staging; it returns with the band in the caller's memory -- the
          // uploader thread keeps the other direction of the link busy meanwhile)
          const DownRect dr{bands[b].dst, img->pitch_bytes,
                            static_cast<uint8_t*>(lane.lane->d_out.ptr) + bands[b].u.out_offset,
                            bands[b].dev_pitch, bands[b].width_bytes, bands[b].u.n_rows};
          const bool grid = on_grid(reinterpret_cast<uintptr_t>(dr.host)) && on_grid(dr.host_pitch) &&
                            on_grid(dr.bytes);
          if (grid) // (the usual frame: queued, not waited for -- band b + 1 is launched under it)
            err = hipMemcpy2DAsync(dr.host, dr.host_pitch, dr.dev, dr.dev_pitch, dr.bytes, dr.rows,
                                   hipMemcpyDeviceToHost, s);
          else if (download_rects(ctx, lane.lane, s, &dr, 1) != RSX_OK)
            err = hipErrorUnknown;
        }
      }
      ctx->helpers.wait(uploader);
      {
        std::lock_guard<std::mutex> g(prog.m);
        up_failed = prog.failed;
      }
      // BOTH streams drained on every way out, failed or not: the caller's input (s_up reads
      // it) and image (s writes it) may be freed the moment this call returns, and the
      // temporaries below are released
      const hipError_t e_up = hipStreamSynchronize(s_up), e_s = hipStreamSynchronize(s);
      if (err == hipSuccess)
        err = e_up != hipSuccess ? e_up : e_s;
      d_jobs.release();
      d_starts.release();
      if (err != hipSuccess || up_failed) {
        set_error(ctx, std::string("unpack (banded): ") +
                           (err != hipSuccess ? hipGetErrorString(err) : "upload failed"));
        return RSX_ERR_DEVICE;
      }
      int rc = RSX_OK;
      for (int i = 0; i < n; ++i) {
        if (statuses)
          statuses[i] = st[i];
        if (st[i] != RSX_OK)
          rc = st[i];
      }
      return rc;
    }
  }
  if (int e = upload_all())
    return e;
  for (int order = 0; order < 4; ++order) {
    auto& v = per_order[order];
    if (v.empty())
      continue;
    std::vector<uint32_t> starts(v.size() + 1, 0);
    for (size_t k = 0; k < v.size(); ++k)
      starts[k + 1] = starts[k] + v[k].n_rows * v[k].segs_per_row;
    // stream-ordered: sync before the temporaries are reused by the next order
    if (int e = d_jobs.ensure(v.size() * sizeof(UnpackJobDev)))
      return e;
    if (int e = d_starts.ensure(starts.size() * sizeof(uint32_t)))
      return e;
    RSX_HIP_CHECK(ctx, hipMemcpyAsync(d_jobs.ptr, v.data(),
                                      v.size() * sizeof(UnpackJobDev),
                                      hipMemcpyHostToDevice, s));
    RSX_HIP_CHECK(ctx, hipMemcpyAsync(d_starts.ptr, starts.data(),
                                      starts.size() * sizeof(uint32_t),
                                      hipMemcpyHostToDevice, s));
    RSX_HIP_CHECK(ctx, launch_unpack(order, static_cast<UnpackJobDev*>(d_jobs.ptr),
                                     static_cast<uint32_t*>(d_starts.ptr),
                                     int(v.size()), starts.back(), lane.lane->d_in.ptr,
                                     lane.lane->d_out.ptr, s));
    RSX_HIP_CHECK(ctx, hipStreamSynchronize(s));
  }
  {
    std::vector<DownRect> down;
    for (int i = 0; i < n; ++i) {
      if (st[i] != RSX_OK || rects[i].rows == 0)
        continue;
      const OutRect& r = rects[i];
      down.push_back({static_cast<uint8_t*>(img->data) + r.host_off, img->pitch_bytes,
                      static_cast<uint8_t*>(lane.lane->d_out.ptr) + r.dev_off, r.dev_pitch,
                      r.width_bytes, r.rows});
    }
    if (int e = download_rects(ctx, lane.lane, s, down.data(), down.size()))
      return e;
  }
  d_jobs.release();
  d_starts.release();
  int rc = RSX_OK;
  for (int i = 0; i < n; ++i) {
    if (statuses)
      statuses[i] = st[i];
    if (st[i] != RSX_OK)
      rc = st[i];
  }
  return rc;
}

} // namespace

extern "C" int rsx_unpack_u16(rsx_ctx* ctx, const rsx_unpack_desc* d,
                              const uint8_t* in, size_t in_bytes,
                              const rsx_image* img) {
  if (!ctx || !d || !in || !img || !img->data)
    return RSX_ERR_INVALID_ARG;
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return unpack_host(ctx, 1, d, &in, &in_bytes, img, nullptr);
}

extern "C" int rsx_unpack_f32(rsx_ctx* ctx, const rsx_unpack_desc* d, const uint8_t* in,
                              size_t in_bytes, const rsx_image* img) {
  if (!ctx || !d || !in || !img || !img->data)
    return RSX_ERR_INVALID_ARG;
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (int st = validate_unpack_f32(*d, *img, in_bytes))
    return st;
  const size_t used = size_t(d->crop_h) * size_t(d->input_pitch_bytes);
  const int64_t rows = std::min<int64_t>(d->crop_h, int64_t(img->dim_y) - d->crop_y);
  if (rows <= 0)
    return RSX_OK;
  // device image = the compact rectangle that is written
  const size_t width_bytes = size_t(d->crop_w) * img->cpp * 4;
  rsx_unpack_job job{};
  job.desc = *d;
  job.desc.crop_x = 0;
  job.desc.crop_y = 0;
  job.in_bytes = used;
  job.img = *img;
  job.img.dim_y = int32_t(rows);
  job.img.pitch_bytes = uint32_t(align_up(width_bytes, 16));
  LaneGuard lane(ctx); // staging + stream of this call
  if (!lane.lane)
    return RSX_ERR_DEVICE;
  if (int e = lane.lane->d_in.ensure(used + 16))
    return e;
  if (int e = lane.lane->d_out.ensure(size_t(job.img.pitch_bytes) * size_t(rows) + 16))
    return e;
  hipStream_t s = lane.lane->stream;
  RSX_HIP_CHECK(ctx, hipMemcpyAsync(lane.lane->d_in.ptr, in, used, hipMemcpyHostToDevice, s));
  rsx_plan* plan = nullptr;
  if (int st = rsx_unpack_f32_plan_create(ctx, 1, &job, &plan))
    return st;
  int rc = rsx_plan_run(plan, lane.lane->d_in.ptr, lane.lane->d_out.ptr, s);
  if (rc == RSX_OK) {
    const size_t x0 = d->bits_per_pixel == 32 ? size_t(d->crop_x) * img->cpp
                                              : size_t(d->crop_x);
    uint8_t* dst = static_cast<uint8_t*>(img->data) +
                   size_t(d->crop_y) * img->pitch_bytes + x0 * 4;
    const DownRect dr{dst, img->pitch_bytes, static_cast<uint8_t*>(lane.lane->d_out.ptr),
                      job.img.pitch_bytes, width_bytes, size_t(rows)};
    rc = download_rects(ctx, lane.lane, s, &dr, 1);
  }
  rsx_plan_destroy(plan);
  return rc;
}

extern "C" int rsx_unpack_variant_u16(rsx_ctx* ctx, const rsx_unpack_variant_desc* d,
                                      const uint8_t* in, size_t in_bytes,
                                      const rsx_image* img) {
  if (!ctx || !d || !in || !img || !img->data)
    return RSX_ERR_INVALID_ARG;
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (int st = validate_unpack_variant(*d, *img, in_bytes))
    return st;
  uint64_t bpl = 0;
  unpack_variant_bytes_per_line(*d, &bpl);
  const size_t used = size_t(bpl) * size_t(d->h);
  // device image = the compact w x h rectangle at the image origin
  rsx_unpack_variant_job job{};
  job.desc = *d;
  job.in_offset = 0;
  job.in_bytes = used;
  job.img_offset = 0;
  job.img = *img;
  job.img.pitch_bytes = uint32_t(align_up(size_t(d->w) * 2, 16));
  const size_t out_bytes = size_t(job.img.pitch_bytes) * size_t(d->h);
  LaneGuard lane(ctx); // staging + stream of this call
  if (!lane.lane)
    return RSX_ERR_DEVICE;
  if (int e = lane.lane->d_in.ensure(used + 16))
    return e;
  if (int e = lane.lane->d_out.ensure(out_bytes + 16))
    return e;
  hipStream_t s = lane.lane->stream;
  RSX_HIP_CHECK(ctx, hipMemcpyAsync(lane.lane->d_in.ptr, in, used, hipMemcpyHostToDevice, s));
  rsx_plan* plan = nullptr;
  if (int st = rsx_unpack_variant_plan_create(ctx, 1, &job, &plan))
    return st;
  int rc = rsx_plan_run(plan, lane.lane->d_in.ptr, lane.lane->d_out.ptr, s);
  if (rc == RSX_OK) {
    const DownRect dr{static_cast<uint8_t*>(img->data), img->pitch_bytes,
                      static_cast<uint8_t*>(lane.lane->d_out.ptr), job.img.pitch_bytes,
                      size_t(d->w) * 2, size_t(d->h)};
    rc = download_rects(ctx, lane.lane, s, &dr, 1);
  }
  rsx_plan_destroy(plan);
  return rc;
}

extern "C" int rsx_dng_decompress_uncompressed(rsx_ctx* ctx, int n_tiles,
                                               const rsx_dng_unpack_tile* tiles,
                                               const rsx_image* img,
                                               int32_t* tile_status) {
  if (!ctx || !tiles || n_tiles < 1 || !img || !img->data)
    return RSX_ERR_INVALID_ARG;
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  std::vector<rsx_unpack_desc> descs(n_tiles);
  std::vector<const uint8_t*> ins(n_tiles);
  std::vector<size_t> sizes(n_tiles);
  for (int i = 0; i < n_tiles; ++i) {
    descs[i] = tiles[i].desc;
    ins[i] = tiles[i].in;
    sizes[i] = tiles[i].in_bytes;
  }
  std::vector<int32_t> st(n_tiles, RSX_OK);
  const int rc = unpack_host(ctx, n_tiles, descs.data(), ins.data(), sizes.data(),
                             img, st.data());
  if (tile_status)
    std::copy(st.begin(), st.end(), tile_status);
  if (rc == RSX_ERR_DEVICE || rc == RSX_ERR_NOMEM)
    return rc;
  for (int i = 0; i < n_tiles; ++i)
    if (st[i] != RSX_OK)
      return RSX_ERR_TILE_ERRORS; // AbstractDngDecompressor.cpp:247-251
  return RSX_OK;
}

// ---------------------------------------------------------------------------
// LJPEG / CR2 entry points: see rsx_ljpeg.hip for the implementation.
// ---------------------------------------------------------------------------
namespace {
// Tables with the same CONTENTS are one table.  The reference binds a decoder per DHT
// slot (AbstractLJpegDecoder.h:112-125) and the shim de-duplicates by object address; a
// file that declares the same code twice (Canon's Th = 0 / Th = 1, many DNG writers) must
// not look like a two-table stream to the kernels: one table keeps the component phase
// out of the synchronisation state and takes the single-pass kernel.
struct UniqueTables {
  rsx_huff_table t[RSX_MAX_COMPONENTS];
};
bool same_table(const rsx_huff_table& a, const rsx_huff_table& b) {
  return a.n_code_values == b.n_code_values && a.fix_dng_bug16 == b.fix_dng_bug16 &&
         std::memcmp(a.n_codes_per_length, b.n_codes_per_length, 16) == 0 &&
         std::memcmp(a.code_values, b.code_values, a.n_code_values) == 0;
}
void dedupe_tables(LJpegJobIn& in, UniqueTables& store) {
  if (in.status != RSX_OK || in.n_tables <= 1 || in.n_tables > RSX_MAX_COMPONENTS)
    return;
  int map[RSX_MAX_COMPONENTS], n = 0;
  for (int t = 0; t < in.n_tables; ++t) {
    int u = 0;
    while (u < n && !same_table(store.t[u], in.tables[t]))
      ++u;
    if (u == n)
      store.t[n++] = in.tables[t];
    map[t] = u;
  }
  if (n == in.n_tables)
    return;
  for (uint8_t& c : in.geom.comp_of_phase)
    if (int(c) < in.n_tables)
      c = uint8_t(map[c]);
  in.tables = store.t;
  in.n_tables = n;
}

// The frame of every decoder's plan_create: the arguments, the context's lock and device, and
// the plan `make` builds for the jobs installed in a new rsx_plan.
template <typename JobT, typename MakeFn>
int decoder_plan_create(rsx_ctx* ctx, int n_jobs, const JobT* jobs, rsx_plan** out_plan,
                        MakeFn make) {
  if (!ctx || !jobs || n_jobs < 1 || !out_plan)
    return RSX_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  auto plan = std::make_unique<rsx_plan>();
  plan->ctx = ctx;
  plan->kind = PLAN_DECODER;
  plan->n_jobs = n_jobs;
  if (int st = make(ctx, n_jobs, jobs, &plan->dec))
    return st;
  *out_plan = plan.release();
  return RSX_OK;
}

// The frame of a decoder plan's per-job getters: a decoder plan, the context's lock, and what
// `get` takes from its DecoderPlan.
template <typename GetFn>
int decoder_plan_get(rsx_plan* plan, GetFn get) {
  if (!plan || plan->kind != PLAN_DECODER)
    return RSX_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock(plan->ctx->mu);
  return get(plan->dec.get());
}

// The plan a host call makes for itself and destroys on its way out, not kept in a lane (a
// stage's key would be its payloads, lists, tables or maps).
struct CallPlan {
  rsx_plan* plan = nullptr;
  CallPlan() = default;
  CallPlan(const CallPlan&) = delete;
  ~CallPlan() { rsx_plan_destroy(plan); }
  // in place on `dev`, a side input (the bad-pixel positions) at `in_dev` or none; returns when
  // the pass is done
  int run(const void* in_dev, void* dev, hipStream_t s) {
    if (int st = rsx_plan_run(plan, in_dev ? in_dev : dev, dev, s))
      return st;
    return rsx_plan_results(plan, nullptr, nullptr);
  }
};

// An LJPEG-family plan: `fill(job, in)` turns each job into its LJpegJobIn, status included.
template <typename JobT, typename FillFn>
int ljpeg_family_plan_create(rsx_ctx* ctx, int n_jobs, const JobT* jobs, rsx_plan** out_plan,
                             FillFn fill) {
  return decoder_plan_create(
      ctx, n_jobs, jobs, out_plan,
      [&](rsx_ctx* c, int n, const JobT* js, std::unique_ptr<DecoderPlan>* out) {
        std::vector<LJpegJobIn> in(n);
        std::vector<UniqueTables> unique(n);
        for (int i = 0; i < n; ++i) {
          fill(js[i], in[i]);
          dedupe_tables(in[i], unique[i]); // (nothing to do for a job of one table)
        }
        return ljpeg_plan_create(c, in, out);
      });
}

// the validation status of a raw decoder's job, with the odd pitch its 16-bit rows cannot have
int raw_status(int st, const rsx_image& img) {
  return st == RSX_OK && img.pitch_bytes % 2 != 0 ? RSX_ERR_INVALID_ARG : st;
}

// The stream of the raw decoders on the Nikon reconstruction kernels (Nikon, Pentax, SamsungV1,
// Sony ARW1): a plain MSB bit stream (kind 2) of `rows` rows of `row_samples` samples, two
// predictors alternating along a row
template <typename JobT>
void raw_pair_geom(const JobT& job, uint32_t rows, uint32_t row_samples, StreamGeom* g) {
  std::memset(g, 0, sizeof *g);
  g->kind = 2;
  g->raw = 1;
  g->in_offset = job.in_offset;
  g->in_bytes = job.in_bytes;
  g->img_offset = job.img_offset;
  g->img_pitch_bytes = job.img.pitch_bytes;
  g->n_comp = 2;
  g->period = 2;
  g->rows = rows;
  g->row_samples = row_samples;
  g->mcu_w = g->mcu_h = 1;
  g->keep_samples = row_samples;
}

} // namespace

extern "C" int rsx_ljpeg_plan_create(rsx_ctx* ctx, int n_jobs,
                                     const rsx_ljpeg_job* jobs,
                                     rsx_plan** out_plan) {
  return ljpeg_family_plan_create(ctx, n_jobs, jobs, out_plan,
                                  [](const rsx_ljpeg_job& j, LJpegJobIn& J) {
    J.status = build_ljpeg_stream(j.desc, j.img, &J.geom);
    J.geom.in_offset = j.in_offset;
    J.geom.in_bytes = j.in_bytes;
    J.geom.img_offset = j.img_offset;
    J.tables = j.desc.tables;
    J.n_tables = j.desc.n_tables;
    J.rows_per_restart_interval = j.desc.rows_per_restart_interval;
    J.frame_h = j.desc.frame_h;
  });
}

extern "C" int rsx_cr2_plan_create(rsx_ctx* ctx, int n_jobs,
                                   const rsx_cr2_job* jobs, rsx_plan** out_plan) {
  return ljpeg_family_plan_create(ctx, n_jobs, jobs, out_plan,
                                  [](const rsx_cr2_job& j, LJpegJobIn& J) {
    J.status = build_cr2_stream(j.desc, j.img, &J.geom);
    J.geom.in_offset = j.in_offset;
    J.geom.in_bytes = j.in_bytes;
    J.geom.img_offset = j.img_offset;
    J.tables = j.desc.tables;
    J.n_tables = j.desc.n_tables;
    J.rows_per_restart_interval = 0; // CR2 rejects DRI (Cr2LJpegDecoder.cpp:59-60)
    J.frame_h = 0;
  });
}

// ---------------------------------------------------------------------------
// SamsungV2Decompressor
// ---------------------------------------------------------------------------
extern "C" int rsx_samsung_v2_validate(const rsx_samsung_v2_desc* d, const rsx_image* img) {
  if (!d || !img)
    return RSX_ERR_INVALID_ARG;
  return samsung_v2_validate(*d, *img);
}

extern "C" int rsx_samsung_v2_plan_create(rsx_ctx* ctx, int n_jobs,
                                          const rsx_samsung_v2_job* jobs,
                                          rsx_plan** out_plan) {
  return decoder_plan_create(ctx, n_jobs, jobs, out_plan, samsung_v2_plan_create);
}

// ---------------------------------------------------------------------------
// Cr2sRawInterpolator
// ---------------------------------------------------------------------------
extern "C" int rsx_sraw_validate(const rsx_sraw_desc* d, const rsx_image* in,
                                 const rsx_image* out) {
  if (!d || !in || !out)
    return RSX_ERR_INVALID_ARG;
  return validate_sraw(*d, *in, *out);
}

extern "C" int rsx_sraw_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_sraw_job* jobs,
                                    rsx_plan** out_plan) {
  if (!ctx || !jobs || n_jobs < 1 || !out_plan)
    return RSX_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  auto plan = std::make_unique<rsx_plan>();
  plan->ctx = ctx;
  plan->kind = PLAN_SRAW;
  plan->n_jobs = n_jobs;
  plan->job_status.assign(n_jobs, RSX_OK);
  std::vector<SrawJobDev> v;
  std::vector<uint32_t> starts(1, 0);
  for (int i = 0; i < n_jobs; ++i) {
    const rsx_sraw_job& j = jobs[i];
    int st = validate_sraw(j.desc, j.in, j.img);
    // the kernel moves 16-byte pieces: RawImage rows are (pitch = roundUp(.., 16),
    // common/RawImage.cpp:80-83), the image bases must be as well
    if (st == RSX_OK && (j.in.pitch_bytes % 16 != 0 || j.img.pitch_bytes % 16 != 0 ||
                         j.in_offset % 16 != 0 || j.img_offset % 16 != 0))
      st = RSX_ERR_INVALID_ARG;
    plan->job_status[i] = st;
    if (st != RSX_OK)
      continue;
    SrawJobDev d{};
    d.in_offset = j.in_offset;
    d.out_offset = j.img_offset;
    d.in_pitch = j.in.pitch_bytes;
    d.out_pitch = j.img.pitch_bytes;
    d.rows = uint32_t(j.in.dim_y);
    d.gs = uint32_t(2 + 2 * j.desc.subsampling_y);
    d.num_mcus = uint32_t(j.in.dim_x) / d.gs;
    d.version = uint32_t(j.desc.version);
    for (int k = 0; k < 3; ++k)
      d.coeffs[k] = j.desc.sraw_coeffs[k];
    d.hue = j.desc.hue;
    starts.push_back(starts.back() + sraw_blocks_for(&d));
    v.push_back(d);
    plan->sraw_versions[j.desc.version] = true;
  }
  plan->n_sraw = int(v.size());
  plan->sraw_blocks = starts.back();
  if (int st = upload(ctx, plan->d_sraw_jobs, v.data(), v.size() * sizeof(SrawJobDev)))
    return st;
  if (int st = upload(ctx, plan->d_sraw_starts, starts.data(), starts.size() * 4))
    return st;
  *out_plan = plan.release();
  return RSX_OK;
}

extern "C" int rsx_sraw_interpolate(rsx_ctx* ctx, const rsx_sraw_desc* d,
                                    const rsx_image* in, const rsx_image* out) {
  if (!ctx || !d || !in || !out || !in->data || !out->data)
    return RSX_ERR_INVALID_ARG;
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (int st = validate_sraw(*d, *in, *out))
    return st;
  // compact device images (row padding never travels)
  rsx_sraw_job job{};
  job.desc = *d;
  job.in = *in;
  job.img = *out;
  const size_t in_w = size_t(in->dim_x) * 2, out_w = size_t(out->dim_x) * 3 * 2;
  job.in.pitch_bytes = uint32_t(align_up(in_w, 16));
  job.img.pitch_bytes = uint32_t(align_up(out_w, 16));
  const size_t in_bytes = size_t(job.in.pitch_bytes) * in->dim_y;
  const size_t out_bytes = size_t(job.img.pitch_bytes) * out->dim_y;
  LaneGuard lane(ctx); // staging + stream of this call
  if (!lane.lane)
    return RSX_ERR_DEVICE;
  if (int e = lane.lane->d_in.ensure(in_bytes + 16))
    return e;
  if (int e = lane.lane->d_out.ensure(out_bytes + 16))
    return e;
  hipStream_t s = lane.lane->stream;
  RSX_HIP_CHECK(ctx, hipMemcpy2DAsync(lane.lane->d_in.ptr, job.in.pitch_bytes, in->data,
                                      in->pitch_bytes, in_w, size_t(in->dim_y),
                                      hipMemcpyHostToDevice, s));
  CallPlan call;
  if (int st = rsx_sraw_plan_create(ctx, 1, &job, &call.plan))
    return st;
  if (int rc = rsx_plan_run(call.plan, lane.lane->d_in.ptr, lane.lane->d_out.ptr, s))
    return rc;
  const DownRect dr{static_cast<uint8_t*>(out->data), out->pitch_bytes,
                    static_cast<uint8_t*>(lane.lane->d_out.ptr), job.img.pitch_bytes, out_w,
                    size_t(out->dim_y)};
  return download_rects(ctx, lane.lane, s, &dr, 1);
}

extern "C" int rsx_nikon_validate(const rsx_nikon_desc* d, const rsx_image* img) {
  if (!d || !img)
    return RSX_ERR_INVALID_ARG;
  return validate_nikon(*d, *img);
}

extern "C" int rsx_nikon_plan_create(rsx_ctx* ctx, int n_jobs,
                                     const rsx_nikon_job* jobs, rsx_plan** out_plan) {
  return ljpeg_family_plan_create(ctx, n_jobs, jobs, out_plan,
                                  [](const rsx_nikon_job& j, LJpegJobIn& J) {
    const rsx_nikon_desc& d = j.desc;
    J.status = raw_status(validate_nikon(d, j.img), j.img);
    if (J.status != RSX_OK)
      return;
    // one table for the whole stream: the two columns alternate (:525-527) but
    // share it, so the "component" only matters to the reconstruction
    raw_pair_geom(j, uint32_t(d.split ? d.split : j.img.dim_y), // decompress(bits, 0, split) :555-556
                  uint32_t(j.img.dim_x), &J.geom);
    J.tables = &d.tables[0];
    J.n_tables = 1;
    NikonIn& N = J.nikon;
    for (int k = 0; k < 4; ++k)
      N.p_up[k] = (&d.p_up[0][0])[k];
    N.uncorrected = d.uncorrected_raw_values != 0;
    N.split = d.split;
    N.height = j.img.dim_y;
    N.seed_offset = j.in_offset;
    if (d.split)
      N.table_after_split = d.tables[1];
    if (!N.uncorrected)
      build_dither_table(d.curve, d.curve_size, &N.dither);
  });
}

extern "C" int rsx_pentax_validate(const rsx_pentax_desc* d, const rsx_image* img) {
  if (!d || !img)
    return RSX_ERR_INVALID_ARG;
  return validate_pentax(*d, *img);
}

extern "C" int rsx_pentax_plan_create(rsx_ctx* ctx, int n_jobs,
                                      const rsx_pentax_job* jobs, rsx_plan** out_plan) {
  return ljpeg_family_plan_create(ctx, n_jobs, jobs, out_plan,
                                  [](const rsx_pentax_job& j, LJpegJobIn& J) {
    J.status = raw_status(validate_pentax(j.desc, j.img), j.img);
    if (J.status != RSX_OK)
      return;
    // the Nikon reconstruction kernels, Pentax flavour
    raw_pair_geom(j, uint32_t(j.img.dim_y), uint32_t(j.img.dim_x), &J.geom);
    J.tables = &j.desc.table;
    J.n_tables = 1;
    J.nikon.uncorrected = true;
    J.nikon.pentax = true; // predictors start at 0, range check instead of clamp
    J.nikon.height = j.img.dim_y;
    J.nikon.seed_offset = j.in_offset;
  });
}

extern "C" int rsx_hasselblad_validate(const rsx_hasselblad_desc* d, const rsx_image* img) {
  if (!d || !img)
    return RSX_ERR_INVALID_ARG;
  return validate_hasselblad(*d, *img);
}

extern "C" int rsx_hasselblad_plan_create(rsx_ctx* ctx, int n_jobs,
                                          const rsx_hasselblad_job* jobs,
                                          rsx_plan** out_plan) {
  return ljpeg_family_plan_create(ctx, n_jobs, jobs, out_plan,
                                  [](const rsx_hasselblad_job& j, LJpegJobIn& J) {
    const rsx_image& img = j.img;
    J.status = raw_status(validate_hasselblad(j.desc, img), img);
    if (J.status != RSX_OK)
      return;
    StreamGeom& g = J.geom;
    std::memset(&g, 0, sizeof g);
    g.kind = 0; // rows of W samples written in place, like an LJPEG tile that is the image
    g.raw = 1;  // BitStreamerMSB32: no stuffing, no markers, 8-byte over-read budget
    g.pair = 1;
    g.no_vertical = 1; // "int p1 = rec.initPred; int p2 = rec.initPred;" per row (:83-85)
    g.in_offset = j.in_offset;
    g.in_bytes = j.in_bytes;
    g.img_offset = j.img_offset;
    g.img_pitch_bytes = img.pitch_bytes;
    g.n_comp = 2; // p1 / p2 alternate along the row (:86-96)
    g.period = 2;
    g.pred_of_phase[0] = 0;
    g.pred_of_phase[1] = 1;
    g.init_pred[0] = g.init_pred[1] = j.desc.init_pred;
    g.seed_pos[0] = 0;
    g.seed_pos[1] = 1;
    g.rows = uint32_t(img.dim_y);
    g.row_samples = uint32_t(img.dim_x);
    g.mcu_w = 2;
    g.mcu_h = 1;
    g.keep_samples = g.row_samples;
    J.tables = &j.desc.table;
    J.n_tables = 1;
  });
}

extern "C" int rsx_samsung_v1_validate(const rsx_samsung_v1_desc* d, const rsx_image* img) {
  if (!d || !img)
    return RSX_ERR_INVALID_ARG;
  return validate_samsung_v1(*d, *img);
}

extern "C" int rsx_samsung_v1_plan_create(rsx_ctx* ctx, int n_jobs,
                                          const rsx_samsung_v1_job* jobs,
                                          rsx_plan** out_plan) {
  return ljpeg_family_plan_create(ctx, n_jobs, jobs, out_plan,
                                  [](const rsx_samsung_v1_job& j, LJpegJobIn& J) {
    J.status = raw_status(validate_samsung_v1(j.desc, j.img), j.img);
    if (J.status != RSX_OK)
      return;
    // the Nikon / Pentax reconstruction kernels
    raw_pair_geom(j, uint32_t(j.img.dim_y), uint32_t(j.img.dim_x), &J.geom);
    // samsungDiff refills with fill(23), not fill(32) (.cpp:66): a symbol at bit c
    // needs 32 K - c >= 23, so symbols may start 9 bits later than with fill(32)
    J.geom.raw_limit = 32 * ((uint64_t(j.in_bytes) + 8) / 4) + 9 + 1;
    J.n_tables = 1;
    J.explicit_enc_len = j.desc.enc_len;
    J.explicit_diff_len = j.desc.diff_len;
    J.explicit_n = j.desc.n_entries;
    J.nikon.uncorrected = true;
    J.nikon.pentax = true;
    J.nikon.range_bits = j.desc.bits;
    J.nikon.height = j.img.dim_y;
    J.nikon.seed_offset = j.in_offset;
  });
}

extern "C" int rsx_sony_arw1_validate(const rsx_image* img) {
  if (!img)
    return RSX_ERR_INVALID_ARG;
  return validate_sony_arw1(*img);
}

namespace {
// SonyArw1Decompressor.cpp:76-83 as (code length, difference length) pairs in
// ascending code order of an 11-bit table: "00" + k zeros + "1" = 4 + k for
// k = 8 .. 0, "010" = 3, "011" = 0, "10" = 2, "11" = 1.  The first slot is the
// prefix of the lengths 13..17 (codes of 12..15 bits): such a difference is at
// least 4096 in magnitude, so the value always leaves 0..4095 and the
// reference throws (.cpp:88-89) -- an invalid code here, reported the same way.
constexpr uint8_t SONY_ENC[14] = {11, 11, 10, 9, 8, 7, 6, 5, 4, 3, 3, 3, 2, 2};
constexpr uint8_t SONY_DIF[14] = {0xFF, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 0, 2, 1};
} // namespace

extern "C" int rsx_sony_arw1_plan_create(rsx_ctx* ctx, int n_jobs,
                                         const rsx_sony_arw1_job* jobs,
                                         rsx_plan** out_plan) {
  return ljpeg_family_plan_create(ctx, n_jobs, jobs, out_plan,
                                  [](const rsx_sony_arw1_job& j, LJpegJobIn& J) {
    J.status = raw_status(validate_sony_arw1(j.img), j.img);
    if (J.status != RSX_OK)
      return;
    // int32 sums + range check, like Pentax; sony_* reconstruction kernels; BitStreamerMSB,
    // fill(32) per pixel (.cpp:70).  A stream row is an image column (.cpp:68-69): W rows of
    // H samples
    raw_pair_geom(j, uint32_t(j.img.dim_x), uint32_t(j.img.dim_y), &J.geom);
    J.n_tables = 1;
    J.explicit_enc_len = SONY_ENC;
    J.explicit_diff_len = SONY_DIF;
    J.explicit_n = 14;
    J.explicit_bits = 11;
    J.nikon.uncorrected = true;
    J.nikon.pentax = true;
    J.nikon.range_bits = 12;
    J.nikon.sony = true;
    J.nikon.height = j.img.dim_x;
    J.nikon.seed_offset = j.in_offset;
  });
}

namespace {

// Generic host-pointer runner for LJPEG-family jobs sharing one host image.
// rectangle of the host image a successful job has written (bytes)
struct HostRect {
  size_t row0, rows, byte0, bytes;
};
// true iff the rectangles lie inside an image of `rows` rows of `row_bytes` bytes, no two of them
// share a byte and together they are the whole image -- any number of them: a sweep down the rows
// over the rectangles that are still open, keyed by their first byte
bool rects_tile_image(std::vector<HostRect> rects, size_t rows, size_t row_bytes) {
  unsigned __int128 area = 0;
  for (const HostRect& r : rects) {
    if (r.rows == 0 || r.bytes == 0 || r.row0 >= rows || r.rows > rows - r.row0 ||
        r.byte0 >= row_bytes || r.bytes > row_bytes - r.byte0)
      return false;
    area += (unsigned __int128)r.rows * r.bytes;
  }
  if (area != (unsigned __int128)rows * row_bytes)
    return false;
  std::sort(rects.begin(), rects.end(), [](const HostRect& a, const HostRect& b) {
    return a.row0 != b.row0 ? a.row0 < b.row0 : a.byte0 < b.byte0;
  });
  std::map<size_t, std::pair<size_t, size_t>> open; // byte0 -> (byte end, row end)
  for (const HostRect& r : rects) {
    auto it = open.lower_bound(r.byte0);
    if (it != open.begin())
      --it;
    while (it != open.end() && it->first < r.byte0 + r.bytes) {
      if (it->second.first > r.byte0) {
        if (it->second.second > r.row0)
          return false; // (two rectangles share a byte)
        it = open.erase(it);
      } else {
        ++it;
      }
    }
    open[r.byte0] = {r.byte0 + r.bytes, r.row0 + r.rows};
  }
  return true; // (inside, disjoint, and the areas add up to the image)
}
HostRect out_rect(const rsx_ljpeg_job& j) {
  return {size_t(j.desc.tile_y), size_t(j.desc.tile_h),
          size_t(j.desc.tile_x) * j.img.cpp * 2, size_t(j.desc.tile_w) * j.img.cpp * 2};
}
HostRect out_rect(const rsx_cr2_job& j) {
  return {0, size_t(j.img.dim_y), 0, size_t(j.img.dim_x) * 2};
}
HostRect out_rect(const rsx_nikon_job& j) {
  return {0, size_t(j.img.dim_y), 0, size_t(j.img.dim_x) * 2};
}
HostRect out_rect(const rsx_pentax_job& j) {
  return {0, size_t(j.img.dim_y), 0, size_t(j.img.dim_x) * 2};
}
HostRect out_rect(const rsx_samsung_v1_job& j) {
  return {0, size_t(j.img.dim_y), 0, size_t(j.img.dim_x) * 2};
}
HostRect out_rect(const rsx_samsung_v2_job& j) {
  return {0, size_t(j.img.dim_y), 0, size_t(j.img.dim_x) * 2};
}
HostRect out_rect(const rsx_sony_arw1_job& j) {
  return {0, size_t(j.img.dim_y), 0, size_t(j.img.dim_x) * 2};
}
HostRect out_rect(const rsx_dng_deflate_job& j) {
  return {size_t(j.off_y), size_t(j.height), size_t(j.off_x) * 4, size_t(j.width) * 4};
}
HostRect out_rect(const rsx_hasselblad_job& j) {
  return {0, size_t(j.img.dim_y), 0, size_t(j.img.dim_x) * 2};
}

// ---------------------------------------------------------------------------------------
// The plan a host-pointer call runs is the lane's cached plan when the lane made it from the
// same key (a burst, a benchmark loop, the tiles of one camera's files), else a new one.
//   * A key is the plan's create function, then what the plan is made FROM: the jobs with the
//     host pointers cleared, and the CONTENTS of data behind host pointers (the Nikon curve, the
//     Phase One strip table), never an address -- a freed and re-allocated curve at the same
//     address, or one mutated in place, must not find the old plan.  ARW2's table stays out of
//     its key: it is call data and goes up on every call.
//   * A call that fails on the device or for memory drops the lane's plan; Phase One and ARW2
//     drop it on RSX_ERR_INVALID_ARG as well.
//   * The uploads and the downloads of the calls of a context take turns (upload_mu,
//     download_mu): calls side by side then share neither direction of the link.
//   * A build with RSX_FORCE_UNSUPPORTED refuses every LJPEG-family call (ljpeg_family_host):
//     the drop-in tests are checked against such a library.
// ---------------------------------------------------------------------------------------
template <typename JobT>
using PlanCreateFn = int (*)(rsx_ctx*, int, const JobT*, rsx_plan**);

// appends the bytes of v[0 .. n) to a key
template <typename T>
void key_append(std::vector<uint8_t>& key, const T* v, size_t n = 1) {
  const uint8_t* p = reinterpret_cast<const uint8_t*>(v);
  key.insert(key.end(), p, p + n * sizeof(T));
}

template <typename JobT>
void key_create(std::vector<uint8_t>& key, PlanCreateFn<JobT> create) {
  const void* fn = reinterpret_cast<const void*>(create);
  key_append(key, &fn);
}

template <typename JobT>
void key_job(std::vector<uint8_t>& key, const JobT& job) {
  JobT j = job;
  j.img.data = nullptr;
  key_append(key, &j);
}
template <>
void key_job<rsx_nikon_job>(std::vector<uint8_t>& key, const rsx_nikon_job& job) {
  rsx_nikon_job j = job;
  j.img.data = nullptr;
  j.desc.curve = nullptr;
  key_append(key, &j);
  if (job.desc.curve && job.desc.curve_size > 0 && job.desc.curve_size <= 65536)
    key_append(key, job.desc.curve, size_t(job.desc.curve_size));
}

// The job of a call of one job (single_image_host): all zeros, then the input size and the image
// without its host pointer.  The caller adds its descriptor's fields, leaving host pointers NULL ...
template <typename JobT>
void one_job_init(JobT& job, size_t in_bytes, const rsx_image* img) {
  std::memset(&job, 0, sizeof job);
  job.in_bytes = in_bytes;
  job.img = *img;
  job.img.data = nullptr;
}
// ... and starts its key from the create function and that job; the contents behind the host
// pointers follow (key_append), and the pointers go into the job last.
template <typename JobT>
std::vector<uint8_t> one_job_key(PlanCreateFn<JobT> create, const JobT& job) {
  std::vector<uint8_t> key;
  key_create(key, create);
  key_append(key, &job);
  return key;
}

// The lane's plan for `key` (*reused: the one it held), else a new one from create(ctx, n,
// jobs) in place of the one it held; when create fails, the lane holds none.
template <typename JobT>
int lane_plan(rsx_ctx* ctx, rsx_ctx::HostLane* L, std::vector<uint8_t>& key,
              PlanCreateFn<JobT> create, int n, const JobT* jobs, rsx_plan** plan,
              bool* reused = nullptr) {
  const bool hit = L->holds_plan(key);
  if (reused)
    *reused = hit;
  if (hit) {
    *plan = L->cached_plan;
    return RSX_OK;
  }
  if (L->cached_plan)
    rsx_plan_destroy(L->cached_plan);
  L->cached_plan = nullptr;
  if (int st = create(ctx, n, jobs, plan))
    return st;
  L->cached_plan = *plan;
  L->cached_key = std::move(key);
  return RSX_OK;
}

void evict_plan(rsx_ctx::HostLane* L) {
  rsx_plan_destroy(L->cached_plan);
  L->cached_plan = nullptr;
}

// the LJPEG-family plan behind a plan, or nullptr
LJpegPlan* ljpeg_of(const rsx_plan* p) {
  return p && p->dec ? p->dec->ljpeg() : nullptr;
}

// One large entropy-coded stream through a host-pointer call, in CHUNKS (round 6; the review's
// "download under decode").  Until now: the whole input up, the kernels, the whole image down,
// one after the other -- 0.55 + 0.1 + 1.07 ms for a 6720 x 4480 CR2 frame, on a link that is full
// duplex.  K0 and the single-pass kernel need nothing of a stream but the bytes of the
// workgroups they run on (and what the workgroups in front of them left), so the plan's blocks
// go in four launches, each behind the upload of ITS quarter of the bytes (a helper thread of the
// context, a stream of its own: a copy from pageable memory keeps its calling thread), and
// what a launch completes -- whole stream rows, whole rows of a CR2 strip -- comes down while
// the next quarter is on its way up and decodes.  The rectangles go through download_rects
// like every other download.  If the stream leaves the single-pass kernel after all (a second
// pass rewrites pixels), everything comes down once more at the end.
// CHUNKED_NOT_TAKEN: nothing done, the caller takes the plain way.
constexpr int CHUNKED_NOT_TAKEN = -1000;
int ljpeg_chunked_host(rsx_ctx* ctx, rsx_ctx::HostLane* L, rsx_plan* plan, size_t in_bytes,
                       size_t in_total, const uint8_t* in, const rsx_image* img,
                       const HostRect& whole, size_t out_skip, int32_t* status,
                       uint32_t* consumed) {
  constexpr int NCH = 4;
  LJpegPlan* lp = ljpeg_of(plan);
  const uint32_t nblk = ljpeg_plan_blocks(lp);
  if (nblk < 4 * NCH || !L->ensure_overlap(NCH))
    return CHUNKED_NOT_TAKEN;
  ++ctx->chunked_calls;
  hipStream_t s = L->stream, s_up = L->stream_up;
  uint8_t* d_in = static_cast<uint8_t*>(L->d_in.ptr);
  uint8_t* const out_row0 = static_cast<uint8_t*>(L->d_out.ptr) - out_skip;
  uint32_t blk_end[NCH];
  size_t byte_end[NCH];
  for (int c = 0; c < NCH; ++c) {
    blk_end[c] = uint32_t(uint64_t(nblk) * uint32_t(c + 1) / NCH);
    // (a workgroup reads its 255 slots, the slot in front of them and 16 bytes behind)
    byte_end[c] = c + 1 == NCH ? in_bytes : std::min(in_bytes, size_t(blk_end[c]) * LJ_R + 256);
  }
  struct Progress {
    std::mutex m;
    std::condition_variable cv;
    int ready = 0;
    bool failed = false;
  } prog;
  const int device = ctx->device;
  auto upload = [&]() {
    bool ok = hipSetDevice(device) == hipSuccess;
    std::lock_guard<std::mutex> up(ctx->upload_mu);
    // (the slack behind the input: zeros, as the plain way leaves them)
    if (ok)
      ok = hipMemsetAsync(d_in + (in_bytes & ~size_t(15)), 0, in_total + 64 - (in_bytes & ~size_t(15)), s_up) ==
           hipSuccess;
    size_t from = 0;
    for (int c = 0; c < NCH; ++c) {
      if (ok && byte_end[c] > from)
        ok = hipMemcpyAsync(d_in + from, in + from, byte_end[c] - from, hipMemcpyHostToDevice, s_up) ==
             hipSuccess;
      if (ok)
        ok = hipEventRecord(L->ev_up[c], s_up) == hipSuccess;
      from = std::max(from, byte_end[c]);
      {
        std::lock_guard<std::mutex> g(prog.m);
        prog.ready = c + 1;
        prog.failed = prog.failed || !ok;
      }
      prog.cv.notify_all();
    }
  };
  rsx::HelperPool::Handle up = ctx->helpers.submit(upload);
  if (!up)
    upload();
  int rc = RSX_OK;
  {
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    plan->last_stream = s;
    plan->ran = true;
  }
  rc = ljpeg_plan_run_begin(lp, d_in, out_row0, s);
  uint64_t done = 0;
  std::vector<LjRegion> reg;
  auto fetch = [&](uint64_t lo, uint64_t hi) -> int {
    ljpeg_plan_region(lp, lo, hi, &reg);
    for (const LjRegion& g : reg) {
      // (inside the rectangle the job owns; one rectangle a call of download_rects: each is a
      // rectangle by itself, not a ragged set)
      const size_t r0 = std::max(g.row0, whole.row0), r1 = std::min(g.row0 + g.rows, whole.row0 + whole.rows);
      const size_t b0 = std::max(g.byte0, whole.byte0), b1 = std::min(g.byte0 + g.bytes, whole.byte0 + whole.bytes);
      if (r1 <= r0 || b1 <= b0)
        continue;
      const size_t off = r0 * img->pitch_bytes + b0;
      const DownRect dr{static_cast<uint8_t*>(img->data) + off, img->pitch_bytes, out_row0 + off,
                        img->pitch_bytes, b1 - b0, r1 - r0};
      std::lock_guard<std::mutex> down(ctx->download_mu);
      if (int e = download_rects(ctx, L, s, &dr, 1))
        return e;
    }
    return RSX_OK;
  };
  bool up_failed = false;
  for (int c = 0; c < NCH && rc == RSX_OK; ++c) {
    {
      std::unique_lock<std::mutex> g(prog.m);
      prog.cv.wait(g, [&]() { return prog.ready > c; });
      up_failed = prog.failed;
    }
    if (up_failed)
      break;
    if (hipStreamWaitEvent(s, L->ev_up[c], 0) != hipSuccess) {
      rc = RSX_ERR_DEVICE;
      break;
    }
    rc = ljpeg_plan_run_blocks(lp, s, c ? blk_end[c - 1] : 0u, blk_end[c]);
    if (rc == RSX_OK && c + 1 < NCH) {
      uint64_t now = 0;
      rc = ljpeg_plan_symbols_done(lp, s, blk_end[c], &now);
      if (rc == RSX_OK && now > done) {
        rc = fetch(done, now);
        done = now;
      }
    }
  }
  ctx->helpers.wait(up);
  // (both streams drained on every way out: the caller's buffers may go the moment we return)
  const hipError_t e_up = hipStreamSynchronize(s_up);
  if (up_failed || e_up != hipSuccess || rc == RSX_ERR_DEVICE) {
    (void)hipStreamSynchronize(s);
    set_error(ctx, "ljpeg (chunked): upload or launch failed");
    return RSX_ERR_DEVICE;
  }
  if (rc == RSX_OK)
    rc = ljpeg_plan_run_end(lp, s);
  if (rc == RSX_OK)
    rc = rsx_plan_results(plan, status, consumed);
  if (rc == RSX_ERR_DEVICE || rc == RSX_ERR_NOMEM) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  if (*status == RSX_OK) {
    if (ljpeg_plan_single_pass_held(lp)) {
      if (int e = fetch(done, ~uint64_t(0)))
        return e;
    } else {
      // (the stream went through a second pass: what came down early may be stale)
      const size_t off = whole.row0 * img->pitch_bytes + whole.byte0;
      const DownRect dr{static_cast<uint8_t*>(img->data) + off, img->pitch_bytes, out_row0 + off,
                        img->pitch_bytes, whole.bytes, whole.rows};
      std::lock_guard<std::mutex> down(ctx->download_mu);
      if (int e = download_rects(ctx, L, s, &dr, 1))
        return e;
    }
  }
  return rc;
}

// What a call does to the decoded image on the device in front of the download, given the address
// row 0 of the image has and the stream (ljpeg_family_host, single_image_host).
typedef std::function<int(uint8_t*, hipStream_t)> DevicePostFn;

// before_download (may be NULL): the DNG opcode list and look-up.  The jobs' rectangles must tile
// the whole image (rects_tile_image, any number of them): a call whose jobs do not returns
// RSX_ERR_UNSUPPORTED before anything is uploaded or decoded, statuses untouched.  It runs only
// when every job decoded, and the whole image then goes back as one rectangle.  With a failing job
// the call is the plain call.
template <typename JobT>
int ljpeg_family_host(rsx_ctx* ctx, int n, std::vector<JobT>& jobs,
                      const uint8_t* const* ins, const rsx_image* img,
                      PlanCreateFn<JobT> create, int32_t* statuses, uint32_t* consumed,
                      bool count_call = true, const DevicePostFn* before_download = nullptr) {
  if (count_call)
    ++ctx->host_calls;
#ifdef RSX_FORCE_UNSUPPORTED
  // (experiment build: every LJPEG-family host-pointer call refuses -- the drop-in tests
  // must notice that the images then come from the reference's own loops)
  for (int i = 0; i < n; ++i)
    statuses[i] = RSX_ERR_UNSUPPORTED;
  return RSX_ERR_UNSUPPORTED;
#endif
  // (the image view sizes the staging: check it before anything is allocated or copied;
  // every decompressor's own validation rejects such an image as well)
  if (img->dim_x <= 0 || img->dim_y <= 0 || img->pitch_bytes == 0 || n < 1)
    return RSX_ERR_INVALID_ARG;
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  // inputs back to back (16-byte aligned) + 64 zero bytes of slack each
  size_t in_total = 0;
  for (int i = 0; i < n; ++i) {
    jobs[i].in_offset = in_total;
    in_total += align_up(size_t(jobs[i].in_bytes) + 64, 16);
    jobs[i].img = *img;
    jobs[i].img_offset = 0;
  }
  if (before_download) {
    std::vector<HostRect> all(static_cast<size_t>(n));
    for (int i = 0; i < n; ++i)
      all[size_t(i)] = out_rect(jobs[i]);
    if (img->cpp < 1 || !rects_tile_image(std::move(all), size_t(img->dim_y),
                                          size_t(img->dim_x) * size_t(img->cpp) * 2))
      return RSX_ERR_UNSUPPORTED;
  }
  // the output staging holds the image ROWS the jobs write (a DNG tile call: the tile's
  // rows, not the image); the kernels get the address row 0 would have
  size_t row_lo = size_t(img->dim_y), row_hi = 0;
  for (int i = 0; i < n; ++i) {
    const HostRect r = out_rect(jobs[i]);
    row_lo = std::min(row_lo, r.row0);
    row_hi = std::max(row_hi, std::min(r.row0 + r.rows, size_t(img->dim_y)));
  }
  if (row_hi <= row_lo) {
    row_lo = 0;
    row_hi = size_t(img->dim_y);
  }
  const size_t out_bytes = size_t(img->pitch_bytes) * (row_hi - row_lo);
  const size_t out_skip = size_t(img->pitch_bytes) * row_lo;
  // the lane's cached plan, if it was made from these very jobs (descriptors, sizes,
  // offsets, image geometry; not the host pointer of the image)
  std::vector<uint8_t> key;
  key.reserve(sizeof(void*) + size_t(n) * sizeof(JobT));
  key_create(key, create);
  for (int i = 0; i < n; ++i)
    key_job(key, jobs[i]);
  LaneGuard lane(ctx, &key); // staging + stream of this call
  if (!lane.lane)
    return RSX_ERR_DEVICE;
  if (int e = lane.lane->d_in.ensure(in_total + 64))
    return e;
  if (int e = lane.lane->d_out.ensure(out_bytes + 64))
    return e;
  hipStream_t s = lane.lane->stream;
  // ONE large stream of the single-pass kernel whose plan the lane holds (a frame decoded
  // again: a burst, a folder of one camera's files): in chunks -- see ljpeg_chunked_host.
  rsx_plan* const held = lane.lane->holds_plan(key) ? lane.lane->cached_plan : nullptr;
  if (n == 1 && !before_download && ctx->host_overlap && jobs[0].in_bytes >= (size_t(8) << 20) && held &&
      !held->timing && ljpeg_of(held) && ljpeg_plan_chunkable(ljpeg_of(held))) {
    int32_t st1 = RSX_OK;
    uint32_t cons1 = 0;
    const int rc = ljpeg_chunked_host(ctx, lane.lane, held, jobs[0].in_bytes, in_total,
                                      ins[0], img, out_rect(jobs[0]), out_skip, &st1, &cons1);
    if (rc != CHUNKED_NOT_TAKEN) {
      if (rc == RSX_ERR_DEVICE || rc == RSX_ERR_NOMEM) {
        evict_plan(lane.lane);
        return rc;
      }
      if (statuses)
        statuses[0] = st1;
      if (consumed)
        consumed[0] = cons1;
      return rc;
    }
  }
  {
    // (one upload at a time, one download at a time: calls that run side by side -- the
    // bands of a split DNG call, the files of several threads -- then take turns on each
    // direction of the link instead of sharing both, and one call's download runs under
    // the next one's upload)
    std::lock_guard<std::mutex> up(ctx->upload_mu);
    RSX_HIP_CHECK(ctx, hipMemsetAsync(lane.lane->d_in.ptr, 0, in_total + 64, s));
    for (int i = 0; i < n; ++i)
      RSX_HIP_CHECK(ctx, hipMemcpyAsync(static_cast<uint8_t*>(lane.lane->d_in.ptr) +
                                            jobs[i].in_offset,
                                        ins[i], jobs[i].in_bytes, hipMemcpyHostToDevice, s));
  }
  rsx_plan* plan = nullptr;
  if (int st = lane_plan(ctx, lane.lane, key, create, n, jobs.data(), &plan))
    return st;
  std::vector<int32_t> st(n, RSX_OK);
  std::vector<uint32_t> cons(n, 0);
  uint8_t* const out_row0 = static_cast<uint8_t*>(lane.lane->d_out.ptr) - out_skip;
  int rc = rsx_plan_run(plan, lane.lane->d_in.ptr, out_row0, s);
  if (rc == RSX_OK)
    rc = rsx_plan_results(plan, st.data(), cons.data());
  if (rc == RSX_ERR_DEVICE || rc == RSX_ERR_NOMEM) {
    evict_plan(lane.lane);
    return rc;
  }
  // only the rectangle a successful job decoded goes back to the host image:
  // pixels outside it (other tiles, padding) are never touched
  std::vector<HostRect> rects;
  for (int i = 0; i < n; ++i) {
    if (statuses)
      statuses[i] = st[i];
    if (consumed)
      consumed[i] = cons[i];
    if (st[i] == RSX_OK)
      rects.push_back(out_rect(jobs[i]));
  }
  const bool all_decoded = rects.size() == size_t(n);
  // Tiles that together fill their bounding box (the rule: every tile of a DNG decoded)
  // go back as ONE rectangle -- a pageable 2D copy per tile cost 2 ms more on the four
  // tiles of an 8192x5464 frame than the copy of the whole frame.
  if (rects.size() > 1) {
    size_t r0 = ~size_t(0), r1 = 0, b0 = ~size_t(0), b1 = 0, area = 0;
    for (const HostRect& r : rects) {
      r0 = std::min(r0, r.row0);
      r1 = std::max(r1, r.row0 + r.rows);
      b0 = std::min(b0, r.byte0);
      b1 = std::max(b1, r.byte0 + r.bytes);
      area += r.rows * r.bytes;
    }
    bool disjoint = true; // (tiles of one image never overlap; checked for the few there are)
    for (size_t x = 0; x < rects.size() && disjoint && rects.size() <= 64; ++x)
      for (size_t y = x + 1; y < rects.size(); ++y) {
        const HostRect &p = rects[x], &q = rects[y];
        if (p.row0 < q.row0 + q.rows && q.row0 < p.row0 + p.rows &&
            p.byte0 < q.byte0 + q.bytes && q.byte0 < p.byte0 + p.bytes)
          disjoint = false;
      }
    if (disjoint && rects.size() <= 64 && area == (r1 - r0) * (b1 - b0))
      rects.assign(1, HostRect{r0, r1 - r0, b0, b1 - b0});
  }
  if (before_download && all_decoded) {
    if (int e = (*before_download)(out_row0, s))
      return e;
    // (the jobs tile the image, checked on the way in: one rectangle, however many tiles)
    rects.assign(1, HostRect{0, size_t(img->dim_y), 0, size_t(img->dim_x) * size_t(img->cpp) * 2});
  }
  // Back into the caller's image: rectangles on the 16-byte grid straight, everything ragged
  // (3-sample pixels, odd widths, tiles of unequal heights) through the lane's page-locked
  // staging -- download_rects; until round 5 every rectangle was a 2-D copy of the runtime
  // into the pageable image, and one such copy of a rectangle on 2-byte boundaries left
  // sixteen bytes undelivered.
  {
    std::vector<DownRect> down;
    down.reserve(rects.size());
    for (const HostRect& r : rects) {
      const size_t off = r.row0 * img->pitch_bytes + r.byte0;
      down.push_back({static_cast<uint8_t*>(img->data) + off, img->pitch_bytes, out_row0 + off,
                      img->pitch_bytes, r.bytes, r.rows});
    }
    std::lock_guard<std::mutex> down_lock(ctx->download_mu);
    if (int e = download_rects(ctx, lane.lane, s, down.data(), down.size()))
      return e;
  }
  return rc;
}

// The one-job host-pointer calls: the job is the call's descriptor (none for DescT void: Sony
// ARW1) and input size.
template <typename JobT, typename DescT>
int one_job_host(rsx_ctx* ctx, const DescT* d, const uint8_t* in, size_t in_bytes,
                 const rsx_image* img, PlanCreateFn<JobT> create, uint32_t* consumed = nullptr) {
  constexpr bool has_desc = !std::is_void<DescT>::value;
  if (!ctx || (has_desc && !d) || !in || !img || !img->data)
    return RSX_ERR_INVALID_ARG;
  std::vector<JobT> jobs(1);
  if constexpr (has_desc)
    jobs[0].desc = *d;
  jobs[0].in_bytes = in_bytes;
  int32_t st = RSX_OK;
  uint32_t c = 0;
  const int rc = ljpeg_family_host(ctx, 1, jobs, &in, img, create, &st, &c);
  if (consumed)
    *consumed = c;
  return rc;
}

// One image through a host-pointer call of Phase One, ARW2, Panasonic, Panasonic V4, SamsungV0,
// sNEF or VC-5: `span` bytes from `src` up as one copy, the lane's plan for `key` run on them, the
// row statuses out, and the image back as one rectangle through download_rects -- only when
// every row decoded (the reference throws otherwise, and the caller's image stays as it was).
// The hooks of a call, an empty one skipped:
// on_reuse(plan, stream): this call's data onto a plan the lane held.
// on_done(plan, rc): what the call takes from the plan besides the image, behind the results; the
// status it returns decides about the download (Panasonic V4: the list, and an image that is
// complete although the list did not fit).
// before_download(device image, stream): what the call does to the decoded image on the device in
// front of the download (Phase One with corrections); a status but RSX_OK ends the call with it.
struct SingleImageHooks {
  std::function<int(rsx_plan*, hipStream_t)> on_reuse;
  std::function<int(rsx_plan*, int)> on_done;
  DevicePostFn before_download;
};

template <typename JobT>
int single_image_host(rsx_ctx* ctx, std::vector<uint8_t>& key, PlanCreateFn<JobT> create,
                      const JobT& job, const uint8_t* src, size_t span, const rsx_image* img,
                      int32_t* row_status, const SingleImageHooks& hooks = SingleImageHooks()) {
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  LaneGuard lane(ctx, &key);
  if (!lane.lane)
    return RSX_ERR_DEVICE;
  const size_t out_bytes = size_t(img->pitch_bytes) * size_t(img->dim_y);
  if (int e = lane.lane->d_in.ensure(span + 64))
    return e;
  if (int e = lane.lane->d_out.ensure(out_bytes + 64))
    return e;
  hipStream_t s = lane.lane->stream;
  if (span) {
    std::lock_guard<std::mutex> up(ctx->upload_mu);
    RSX_HIP_CHECK(ctx, hipMemcpyAsync(lane.lane->d_in.ptr, src, span, hipMemcpyHostToDevice, s));
  }
  rsx_plan* plan = nullptr;
  bool reused = false;
  if (int st = lane_plan(ctx, lane.lane, key, create, 1, &job, &plan, &reused))
    return st;
  // (the hooks' calls are inlined here: an out-of-line std::function::operator() would be one
  // more weak symbol in the library's dynamic table)
  int rc = RSX_OK;
  if (reused && hooks.on_reuse)
    [[clang::always_inline]] rc = hooks.on_reuse(plan, s);
  if (rc != RSX_OK)
    return rc;
  int32_t st = RSX_OK;
  rc = rsx_plan_run(plan, lane.lane->d_in.ptr, lane.lane->d_out.ptr, s);
  if (rc == RSX_OK)
    rc = rsx_plan_results(plan, &st, nullptr);
  if (rc == RSX_OK || rc == st) {
    if (row_status)
      if (int e = plan->dec->row_status(s, 0, row_status))
        rc = e;
  }
  if (hooks.on_done)
    [[clang::always_inline]] rc = hooks.on_done(plan, rc);
  if (rc == RSX_ERR_DEVICE || rc == RSX_ERR_NOMEM || rc == RSX_ERR_INVALID_ARG) {
    evict_plan(lane.lane);
    return rc;
  }
  if (rc != RSX_OK)
    return rc; // (a failing row: nothing goes back into the caller's image)
  uint8_t* const dev = static_cast<uint8_t*>(lane.lane->d_out.ptr);
  if (hooks.before_download)
    if (int e = hooks.before_download(dev, s))
      return e;
  DownRect dr{static_cast<uint8_t*>(img->data), img->pitch_bytes, dev, img->pitch_bytes,
              size_t(img->dim_x) * size_t(img->cpp) * 2, size_t(img->dim_y)};
  std::lock_guard<std::mutex> down_lock(ctx->download_mu);
  return download_rects(ctx, lane.lane, s, &dr, 1);
}

} // namespace

extern "C" int rsx_ljpeg_decode(rsx_ctx* ctx, const rsx_ljpeg_desc* d,
                                const uint8_t* in, size_t in_bytes,
                                const rsx_image* img, uint32_t* consumed) {
  return one_job_host<rsx_ljpeg_job>(ctx, d, in, in_bytes, img, rsx_ljpeg_plan_create, consumed);
}

extern "C" int rsx_cr2_decode(rsx_ctx* ctx, const rsx_cr2_desc* d,
                              const uint8_t* in, size_t in_bytes,
                              const rsx_image* img, uint32_t* consumed) {
  return one_job_host<rsx_cr2_job>(ctx, d, in, in_bytes, img, rsx_cr2_plan_create, consumed);
}

extern "C" int rsx_nikon_decompress(rsx_ctx* ctx, const rsx_nikon_desc* d,
                                    const uint8_t* in, size_t in_bytes,
                                    const rsx_image* img) {
  return one_job_host<rsx_nikon_job>(ctx, d, in, in_bytes, img, rsx_nikon_plan_create);
}

extern "C" int rsx_pentax_decompress(rsx_ctx* ctx, const rsx_pentax_desc* d,
                                     const uint8_t* in, size_t in_bytes,
                                     const rsx_image* img) {
  return one_job_host<rsx_pentax_job>(ctx, d, in, in_bytes, img, rsx_pentax_plan_create);
}

extern "C" int rsx_hasselblad_decompress(rsx_ctx* ctx, const rsx_hasselblad_desc* d,
                                         const uint8_t* in, size_t in_bytes,
                                         const rsx_image* img, uint32_t* consumed) {
  return one_job_host<rsx_hasselblad_job>(ctx, d, in, in_bytes, img, rsx_hasselblad_plan_create,
                                          consumed);
}

extern "C" int rsx_samsung_v1_decompress(rsx_ctx* ctx, const rsx_samsung_v1_desc* d,
                                         const uint8_t* in, size_t in_bytes,
                                         const rsx_image* img) {
  return one_job_host<rsx_samsung_v1_job>(ctx, d, in, in_bytes, img, rsx_samsung_v1_plan_create);
}

extern "C" int rsx_samsung_v2_decompress(rsx_ctx* ctx, const rsx_samsung_v2_desc* d,
                                         const uint8_t* in, size_t in_bytes,
                                         const rsx_image* img) {
  return one_job_host<rsx_samsung_v2_job>(ctx, d, in, in_bytes, img, rsx_samsung_v2_plan_create);
}

extern "C" int rsx_sony_arw1_decompress(rsx_ctx* ctx, const uint8_t* in, size_t in_bytes,
                                        const rsx_image* img) {
  return one_job_host<rsx_sony_arw1_job, void>(ctx, nullptr, in, in_bytes, img,
                                               rsx_sony_arw1_plan_create);
}

extern "C" int rsx_dng_decompress_ljpeg(rsx_ctx* ctx, int n_tiles,
                                        const rsx_dng_ljpeg_tile* tiles,
                                        const rsx_image* img,
                                        int32_t* tile_status,
                                        uint32_t* tile_consumed) {
  if (!ctx || !tiles || n_tiles < 1 || !img || !img->data)
    return RSX_ERR_INVALID_ARG;
  std::vector<rsx_ljpeg_job> jobs(n_tiles);
  std::vector<const uint8_t*> ins(n_tiles);
  for (int i = 0; i < n_tiles; ++i) {
    jobs[i].desc = tiles[i].desc;
    jobs[i].in_bytes = tiles[i].in_bytes;
    ins[i] = tiles[i].in;
  }
  constexpr int32_t ST_UNSET = INT32_MIN; // "ljpeg_family_host never got to this tile"
  std::vector<int32_t> st(n_tiles, RSX_OK);
  std::vector<uint32_t> cons(n_tiles, 0);
  // A large image: bands of its tile ROWS (up to four) as calls of their own, side by side on
  // helper threads -- the link is full duplex, and a copy from or to pageable memory keeps
  // its calling thread: while one band is downloading its pixels the next one uploads its
  // bytes and decodes (the calls take turns on each direction, ljpeg_family_host).  cfg 4:
  // 44 MB up, 0.2 ms of kernels, 89 MB down, one after the other 2.74 ms; as two bands 2.40.
  // By tile rows, so that each band's pixels go back as one rectangle.
  int rc = RSX_OK;
  {
    size_t total_in = 0;
    for (int i = 0; i < n_tiles; ++i)
      total_in += tiles[i].in_bytes;
    std::vector<int> band_of(n_tiles, 0);
    int n_bands = 1;
    if (ctx->host_overlap && n_tiles >= 2 && total_in >= (size_t(8) << 20)) {
      std::vector<int32_t> ys;
      for (int i = 0; i < n_tiles; ++i)
        ys.push_back(tiles[i].desc.tile_y);
      std::sort(ys.begin(), ys.end());
      ys.erase(std::unique(ys.begin(), ys.end()), ys.end());
      n_bands = int(std::min<size_t>(4, ys.size()));
      for (int i = 0; i < n_tiles; ++i) {
        const size_t row = size_t(std::lower_bound(ys.begin(), ys.end(), tiles[i].desc.tile_y) -
                                  ys.begin());
        band_of[i] = int(row * size_t(n_bands) / ys.size());
      }
    }
    if (n_bands >= 2) {
      struct Band {
        std::vector<rsx_ljpeg_job> jobs;
        std::vector<const uint8_t*> ins;
        std::vector<int> tile;
        std::vector<int32_t> st;
        std::vector<uint32_t> cons;
        int rc = RSX_OK;
      };
      std::vector<Band> bands(n_bands);
      for (int i = 0; i < n_tiles; ++i) {
        Band& bd = bands[band_of[i]];
        bd.jobs.push_back(jobs[i]);
        bd.ins.push_back(ins[i]);
        bd.tile.push_back(i);
      }
      auto run_band = [&](Band& bd, bool count) {
        bd.st.assign(bd.jobs.size(), ST_UNSET);
        bd.cons.assign(bd.jobs.size(), 0);
        bd.rc = ljpeg_family_host(ctx, int(bd.jobs.size()), bd.jobs, bd.ins.data(), img,
                                  rsx_ljpeg_plan_create, bd.st.data(), bd.cons.data(), count);
      };
      // (persistent helpers of the context; none to be had: in turn, on this thread)
      std::vector<rsx::HelperPool::Handle> helpers;
      std::vector<int> inline_bands;
      for (int k = 1; k < n_bands; ++k) {
        rsx::HelperPool::Handle h = ctx->helpers.submit([&, k]() { run_band(bands[k], false); });
        if (h)
          helpers.push_back(h);
        else
          inline_bands.push_back(k);
      }
      run_band(bands[0], true);
      for (int k : inline_bands)
        run_band(bands[k], false);
      for (const rsx::HelperPool::Handle& h : helpers)
        ctx->helpers.wait(h);
      for (const Band& bd : bands) {
        for (size_t k = 0; k < bd.tile.size(); ++k) {
          // (a band that came back early -- no plan, a bad argument -- never filled its
          // statuses in: its tiles were NOT decoded, whatever the initial value says)
          st[bd.tile[k]] = bd.st[k] == ST_UNSET ? (bd.rc != RSX_OK ? bd.rc : RSX_ERR_DEVICE) : bd.st[k];
          cons[bd.tile[k]] = bd.cons[k];
        }
        if (bd.rc == RSX_ERR_DEVICE || bd.rc == RSX_ERR_NOMEM)
          rc = bd.rc; // (only a device / memory failure of a band matters below)
      }
    } else {
      std::fill(st.begin(), st.end(), ST_UNSET);
      rc = ljpeg_family_host(ctx, n_tiles, jobs, ins.data(), img, rsx_ljpeg_plan_create,
                             st.data(), cons.data());
      for (int32_t& v : st)
        if (v == ST_UNSET)
          v = rc != RSX_OK ? rc : RSX_ERR_DEVICE;
    }
  }
  if (tile_status)
    std::copy(st.begin(), st.end(), tile_status);
  if (tile_consumed)
    std::copy(cons.begin(), cons.end(), tile_consumed);
  if (rc == RSX_ERR_DEVICE || rc == RSX_ERR_NOMEM)
    return rc;
  for (int i = 0; i < n_tiles; ++i)
    if (st[i] != RSX_OK)
      return RSX_ERR_TILE_ERRORS; // AbstractDngDecompressor.cpp:247-251
  return RSX_OK;
}

// ---------------------------------------------------------------------------
// AbstractDngDecompressor, compression 8 (deflate + floating-point predictor)
// ---------------------------------------------------------------------------
extern "C" int rsx_dng_deflate_validate(const rsx_dng_deflate_desc* desc,
                                        const rsx_dng_deflate_tile* tile, const rsx_image* img) {
  if (!desc || !tile || !img)
    return RSX_ERR_INVALID_ARG;
  return dng_deflate_validate(*desc, tile->tile_w, tile->tile_h, tile->off_x, tile->off_y,
                              tile->width, tile->height, tile->in_bytes, *img);
}

extern "C" int rsx_dng_deflate_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_dng_deflate_job* jobs,
                                           rsx_plan** out_plan) {
  return decoder_plan_create(ctx, n_jobs, jobs, out_plan, dng_deflate_plan_create);
}

// The host-pointer call, as rsx_dng_decompress_ljpeg's: the tiles' bytes packed into one upload,
// one plan run, the windows of the tiles that decoded back through download_rects.
extern "C" int rsx_dng_decompress_deflate(rsx_ctx* ctx, const rsx_dng_deflate_desc* desc, int n_tiles,
                                          const rsx_dng_deflate_tile* tiles, const rsx_image* img,
                                          int32_t* tile_status) {
  if (!ctx || !desc || !tiles || n_tiles < 1 || !img || !img->data)
    return RSX_ERR_INVALID_ARG;
  std::vector<rsx_dng_deflate_job> jobs(n_tiles);
  std::vector<const uint8_t*> ins(n_tiles);
  for (int i = 0; i < n_tiles; ++i) {
    const rsx_dng_deflate_tile& t = tiles[i];
    std::memset(&jobs[i], 0, sizeof jobs[i]);
    jobs[i].desc = *desc;
    jobs[i].tile_w = t.tile_w;
    jobs[i].tile_h = t.tile_h;
    jobs[i].off_x = t.off_x;
    jobs[i].off_y = t.off_y;
    jobs[i].width = t.width;
    jobs[i].height = t.height;
    jobs[i].in_bytes = t.in_bytes;
    ins[i] = t.in;
    if (t.in_bytes && !t.in)
      return RSX_ERR_INVALID_ARG;
  }
  constexpr int32_t ST_UNSET = INT32_MIN; // "ljpeg_family_host never got to this tile"
  std::vector<int32_t> st(n_tiles, ST_UNSET);
  const int rc = ljpeg_family_host(ctx, n_tiles, jobs, ins.data(), img, rsx_dng_deflate_plan_create,
                                   st.data(), nullptr);
  for (int32_t& v : st)
    if (v == ST_UNSET)
      v = rc != RSX_OK ? rc : RSX_ERR_DEVICE;
  if (tile_status)
    std::copy(st.begin(), st.end(), tile_status);
  if (rc == RSX_ERR_DEVICE || rc == RSX_ERR_NOMEM)
    return rc;
  for (int i = 0; i < n_tiles; ++i)
    if (st[i] != RSX_OK)
      return RSX_ERR_TILE_ERRORS; // AbstractDngDecompressor.cpp:247-251
  return RSX_OK;
}

// ---------------------------------------------------------------------------
// AbstractDngDecompressor, compression 0x884c (lossy JPEG)
// ---------------------------------------------------------------------------
extern "C" int rsx_dng_jpeg_validate(const rsx_dng_jpeg_tile* tile, const rsx_image* img,
                                     rsx_dng_jpeg_info* info) {
  return rsx_jpeg::validate_call(tile, img, info);
}

extern "C" int rsx_dng_jpeg_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_dng_jpeg_job* jobs,
                                        rsx_plan** out_plan) {
  return decoder_plan_create(ctx, n_jobs, jobs, out_plan, dng_jpeg_plan_create);
}

extern "C" int rsx_dng_jpeg_plan_tile_status(rsx_plan* plan, int job, int32_t* tile_status) {
  return decoder_plan_get(plan, [&](DecoderPlan* d) {
    return d->row_status(plan->last_stream, job, tile_status);
  });
}

// The host-pointer call: the tiles' bytes packed into one upload, one run of a plan made for the
// call (its key would be the streams themselves), the windows of the tiles that decoded back
// through download_rects -- as one rectangle where they fill their bounding box.
//
// before_download (may be NULL; rsx_dng_lossy_decompress): what the call does to the decoded image
// on the device in front of the download, as in ljpeg_family_host.  The tiles' windows must then
// tile the whole image (rects_tile_image): a call whose tiles parse and do not returns
// RSX_ERR_UNSUPPORTED before anything is uploaded or decoded.  It runs only when every tile
// decoded, and the whole image then goes back as one rectangle; with a failing tile the call is
// the plain call.  *wrote (may be NULL): the call reached its download (or had nothing to decode),
// so tile_status holds the tiles' statuses.
namespace {
int dng_jpeg_host(rsx_ctx* ctx, int n_tiles, const rsx_dng_jpeg_tile* tiles, const rsx_image* img,
                  int32_t* tile_status, bool count_call, const DevicePostFn* before_download,
                  bool* wrote) {
  if (wrote)
    *wrote = false;
  if (!ctx || !tiles || n_tiles < 1 || !img || !img->data)
    return RSX_ERR_INVALID_ARG;
  if (img->dim_x <= 0 || img->dim_y <= 0 || img->pitch_bytes == 0)
    return RSX_ERR_INVALID_ARG;
  if (count_call)
    ++ctx->host_calls;
  std::vector<uint64_t> offs(n_tiles);
  size_t in_total = 0;
  for (int i = 0; i < n_tiles; ++i) {
    if (!tiles[i].in || tiles[i].in_bytes >= (uint64_t(1) << 32))
      return tiles[i].in ? RSX_ERR_UNSUPPORTED : RSX_ERR_INVALID_ARG;
    offs[i] = in_total;
    in_total += align_up(tiles[i].in_bytes + 64, 16);
  }
  rsx_dng_jpeg_job job;
  std::memset(&job, 0, sizeof job);
  job.n_tiles = n_tiles;
  job.tiles = tiles;
  job.in_offsets = offs.data();
  job.img = *img;
  job.img.data = nullptr;
  CallPlan cp;
  if (int st = rsx_dng_jpeg_plan_create(ctx, 1, &job, &cp.plan))
    return st;
  const std::vector<JpegWindow>& win = dng_jpeg_plan_windows(cp.plan->dec.get(), 0);
  if (before_download) {
    bool parsed = true;
    std::vector<HostRect> all;
    all.reserve(win.size());
    for (const JpegWindow& w : win) {
      parsed = parsed && w.host_status == RSX_OK;
      all.push_back(HostRect{size_t(w.off_y), size_t(w.copy_h), size_t(w.off_x) * w.cpp * 2,
                             size_t(w.copy_w) * w.cpp * 2});
    }
    // (a tile that does not parse has no window: a failing tile, the plain call)
    if (parsed && (img->cpp < 1 || !rects_tile_image(std::move(all), size_t(img->dim_y),
                                                     size_t(img->dim_x) * size_t(img->cpp) * 2)))
      return RSX_ERR_UNSUPPORTED;
  }
  // the output staging holds the image rows the windows cover
  size_t row_lo = size_t(img->dim_y), row_hi = 0;
  for (const JpegWindow& w : win)
    if (w.host_status == RSX_OK) {
      row_lo = std::min(row_lo, size_t(w.off_y));
      row_hi = std::max(row_hi, size_t(w.off_y) + w.copy_h);
    }
  std::vector<int32_t> st(n_tiles, RSX_OK);
  int rc = RSX_OK;
  if (row_hi > row_lo) {
    RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    LaneGuard lane(ctx);
    if (!lane.lane)
      return RSX_ERR_DEVICE;
    const size_t out_skip = size_t(img->pitch_bytes) * row_lo;
    if (int e = lane.lane->d_in.ensure(in_total + 64))
      return e;
    if (int e = lane.lane->d_out.ensure(size_t(img->pitch_bytes) * (row_hi - row_lo) + 64))
      return e;
    hipStream_t s = lane.lane->stream;
    {
      std::lock_guard<std::mutex> up(ctx->upload_mu);
      RSX_HIP_CHECK(ctx, hipMemsetAsync(lane.lane->d_in.ptr, 0, in_total + 64, s));
      for (int i = 0; i < n_tiles; ++i)
        if (tiles[i].in_bytes)
          RSX_HIP_CHECK(ctx, hipMemcpyAsync(static_cast<uint8_t*>(lane.lane->d_in.ptr) + offs[i],
                                            tiles[i].in, tiles[i].in_bytes, hipMemcpyHostToDevice, s));
    }
    uint8_t* const out_row0 = static_cast<uint8_t*>(lane.lane->d_out.ptr) - out_skip;
    rc = rsx_plan_run(cp.plan, lane.lane->d_in.ptr, out_row0, s);
    if (rc == RSX_OK)
      rc = rsx_plan_results(cp.plan, nullptr, nullptr);
    if (rc == RSX_ERR_DEVICE || rc == RSX_ERR_NOMEM)
      return rc;
    if (int e = cp.plan->dec->row_status(s, 0, st.data()))
      return e;
    std::vector<HostRect> rects;
    for (int i = 0; i < n_tiles; ++i)
      if (st[i] == RSX_OK)
        rects.push_back(HostRect{size_t(win[i].off_y), size_t(win[i].copy_h),
                                 size_t(win[i].off_x) * win[i].cpp * 2,
                                 size_t(win[i].copy_w) * win[i].cpp * 2});
    const bool all_decoded = rects.size() == size_t(n_tiles);
    if (rects.size() > 1) {
      size_t r0 = ~size_t(0), r1 = 0, b0 = ~size_t(0), b1 = 0;
      for (const HostRect& r : rects) {
        r0 = std::min(r0, r.row0);
        r1 = std::max(r1, r.row0 + r.rows);
        b0 = std::min(b0, r.byte0);
        b1 = std::max(b1, r.byte0 + r.bytes);
      }
      // (rects_tile_image: inside, disjoint, and together the whole of their bounding box)
      std::vector<HostRect> rel(rects);
      for (HostRect& r : rel) {
        r.row0 -= r0;
        r.byte0 -= b0;
      }
      if (rects_tile_image(std::move(rel), r1 - r0, b1 - b0))
        rects.assign(1, HostRect{r0, r1 - r0, b0, b1 - b0});
    }
    if (before_download && all_decoded) {
      if (int e = (*before_download)(out_row0, s))
        return e;
      // (the windows tile the image, checked on the way in: one rectangle, however many tiles)
      rects.assign(1, HostRect{0, size_t(img->dim_y), 0, size_t(img->dim_x) * size_t(img->cpp) * 2});
    }
    std::vector<DownRect> down;
    down.reserve(rects.size());
    for (const HostRect& r : rects) {
      const size_t off = r.row0 * img->pitch_bytes + r.byte0;
      down.push_back({static_cast<uint8_t*>(img->data) + off, img->pitch_bytes, out_row0 + off,
                      img->pitch_bytes, r.bytes, r.rows});
    }
    std::lock_guard<std::mutex> down_lock(ctx->download_mu);
    if (int e = download_rects(ctx, lane.lane, s, down.data(), down.size()))
      return e;
  } else {
    for (int i = 0; i < n_tiles; ++i)
      st[i] = win[i].host_status;
  }
  if (wrote)
    *wrote = true;
  if (tile_status)
    std::copy(st.begin(), st.end(), tile_status);
  for (int i = 0; i < n_tiles; ++i)
    if (st[i] != RSX_OK)
      return RSX_ERR_TILE_ERRORS; // AbstractDngDecompressor.cpp:247-251
  return RSX_OK;
}
} // namespace

extern "C" int rsx_dng_decompress_jpeg(rsx_ctx* ctx, int n_tiles, const rsx_dng_jpeg_tile* tiles,
                                       const rsx_image* img, int32_t* tile_status) {
  return dng_jpeg_host(ctx, n_tiles, tiles, img, tile_status, true, nullptr, nullptr);
}

// ---------------------------------------------------------------------------
// PhaseOneDecompressor
// ---------------------------------------------------------------------------
extern "C" int rsx_phase_one_validate(int n_strips, const rsx_phase_one_strip* strips,
                                      size_t in_bytes, const rsx_image* img) {
  if (!img)
    return RSX_ERR_INVALID_ARG;
  return phase_one_validate(n_strips, strips, in_bytes, *img);
}

extern "C" int rsx_phase_one_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_phase_one_job* jobs,
                                         rsx_plan** out_plan) {
  return decoder_plan_create(ctx, n_jobs, jobs, out_plan, phase_one_plan_create);
}

// The host-pointer call (single_image_host): the bytes the strips cover go up as one copy; the
// plan's key holds the strip table.
namespace {
int phase_one_host(rsx_ctx* ctx, const uint8_t* in, int n_strips, const rsx_phase_one_strip* strips,
                   const rsx_image* img, int32_t* strip_status,
                   const SingleImageHooks& hooks = SingleImageHooks()) {
  uint64_t lo = ~uint64_t(0), hi = 0;
  for (int i = 0; i < n_strips; ++i) {
    lo = std::min<uint64_t>(lo, strips[i].offset);
    hi = std::max<uint64_t>(hi, strips[i].offset + strips[i].bytes);
  }
  std::vector<rsx_phase_one_strip> local(strips, strips + n_strips);
  for (rsx_phase_one_strip& s : local)
    s.offset -= lo;
  const size_t span = size_t(hi - lo);
  rsx_phase_one_job job;
  one_job_init(job, span, img);
  job.n_strips = n_strips;
  std::vector<uint8_t> key = one_job_key(rsx_phase_one_plan_create, job);
  key_append(key, local.data(), local.size());
  job.strips = local.data();
  return single_image_host(ctx, key, rsx_phase_one_plan_create, job, in + lo, span, img,
                           strip_status, hooks);
}
} // namespace

extern "C" int rsx_phase_one_decompress(rsx_ctx* ctx, const uint8_t* in, size_t in_bytes,
                                        int n_strips, const rsx_phase_one_strip* strips,
                                        const rsx_image* img, int32_t* strip_status) {
  if (!ctx || !in || !strips || !img || !img->data)
    return RSX_ERR_INVALID_ARG;
  ++ctx->host_calls;
  if (int st = phase_one_validate(n_strips, strips, in_bytes, *img))
    return st;
  return phase_one_host(ctx, in, n_strips, strips, img, strip_status);
}

// ---------------------------------------------------------------------------
// IiqDecoder::CorrectPhaseOneC (flat field, quadrant curves)
// ---------------------------------------------------------------------------
extern "C" int rsx_iiq_correct_validate(const rsx_iiq_corr* corr, const rsx_image* img) {
  return iiq_correct_validate(corr, img);
}

extern "C" int rsx_iiq_correct_plan_create(rsx_ctx* ctx, int n_jobs,
                                           const rsx_iiq_correct_job* jobs, rsx_plan** out_plan) {
  return decoder_plan_create(ctx, n_jobs, jobs, out_plan, iiq_correct_plan_create);
}

namespace {
// true iff the runtime knows `p` as device (or managed) memory
bool is_device_pointer(const void* p) {
  hipPointerAttribute_t attr;
  std::memset(&attr, 0, sizeof attr);
  if (hipPointerGetAttributes(&attr, p) == hipSuccess)
    return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
  (void)hipGetLastError(); // (plain host memory is unknown to the runtime)
  return false;
}

// A stage in place on the caller's image of rows of `row_bytes` bytes (rsx_iiq_correct,
// rsx_bad_pixels_fix, rsx_dng_post, rsx_dng_finish).  A device pointer: run(side, image, NULL),
// which puts the pass on the context's stream, behind the null stream's work so far, and returns
// when it is done.  A host pointer: the rows go up as one copy, run(side, rows, stream) on a lane,
// and the rows come back through download_rects.  The side input (the bad-pixel positions;
// side_bytes 0: none, run gets NULL) goes up in front of the pass in both cases: into a buffer of
// the call's own, or into the lane's input staging.  after (may be empty): what the call takes
// from its plans behind the pass and the download.
typedef std::function<int(const void* side_dev, void* dev, hipStream_t s)> InPlaceRunFn;
int in_place_call(rsx_ctx* ctx, const rsx_image* img, size_t row_bytes, const void* side,
                  size_t side_bytes, const InPlaceRunFn& run,
                  const std::function<int()>& after = nullptr) {
  if (is_device_pointer(img->data)) {
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    DeviceBuffer d_side;
    if (side_bytes) {
      if (int e = d_side.ensure(side_bytes + 16))
        return e;
      RSX_HIP_CHECK(ctx, hipMemcpyAsync(d_side.ptr, side, side_bytes, hipMemcpyHostToDevice,
                                        ctx->stream));
    }
    if (int st = run(d_side.ptr, img->data, nullptr))
      return st;
    return after ? after() : int(RSX_OK);
  }
  LaneGuard lane(ctx);
  if (!lane.lane)
    return RSX_ERR_DEVICE;
  rsx_ctx::HostLane* L = lane.lane;
  const size_t bytes = size_t(img->pitch_bytes) * size_t(img->dim_y - 1) + row_bytes;
  if (side_bytes)
    if (int e = L->d_in.ensure(side_bytes + 64))
      return e;
  if (int e = L->d_out.ensure(bytes + 64))
    return e;
  {
    std::lock_guard<std::mutex> up(ctx->upload_mu);
    if (side_bytes)
      RSX_HIP_CHECK(ctx, hipMemcpyAsync(L->d_in.ptr, side, side_bytes, hipMemcpyHostToDevice,
                                        L->stream));
    RSX_HIP_CHECK(ctx, hipMemcpyAsync(L->d_out.ptr, img->data, bytes, hipMemcpyHostToDevice,
                                      L->stream));
  }
  if (int st = run(side_bytes ? L->d_in.ptr : nullptr, L->d_out.ptr, L->stream))
    return st;
  DownRect dr{static_cast<uint8_t*>(img->data), img->pitch_bytes,
              static_cast<const uint8_t*>(L->d_out.ptr), img->pitch_bytes, row_bytes,
              size_t(img->dim_y)};
  {
    std::lock_guard<std::mutex> down_lock(ctx->download_mu);
    if (int e = download_rects(ctx, L, L->stream, &dr, 1))
      return e;
  }
  return after ? after() : int(RSX_OK);
}

// the correction plan of a host call (a CallPlan: a curve set alone is 512 KiB)
int iiq_call_create(rsx_ctx* ctx, const rsx_iiq_corr* corr, const rsx_image* img, CallPlan& call) {
  auto job = std::make_unique<rsx_iiq_correct_job>();
  job->corr = *corr;
  job->img_offset = 0;
  job->img = *img;
  job->img.data = nullptr;
  return rsx_iiq_correct_plan_create(ctx, 1, job.get(), &call.plan);
}
} // namespace

// In place (in_place_call).
extern "C" int rsx_iiq_correct(rsx_ctx* ctx, const rsx_iiq_corr* corr, const rsx_image* img) {
  if (!ctx || !corr || !img || !img->data)
    return RSX_ERR_INVALID_ARG;
  ++ctx->host_calls;
  if (int st = iiq_correct_validate(corr, img))
    return st;
  if (img->pitch_bytes % 2 != 0)
    return RSX_ERR_INVALID_ARG;
  if (corr->n_ops == 0)
    return RSX_OK;
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  CallPlan call;
  if (int st = iiq_call_create(ctx, corr, img, call))
    return st;
  return in_place_call(ctx, img, size_t(img->dim_x) * 2, nullptr, 0,
                       [&](const void*, void* dev, hipStream_t s) { return call.run(nullptr, dev, s); });
}

// rsx_phase_one_decompress with the corrections on the decoded image in front of the download
extern "C" int rsx_phase_one_decompress_corrected(rsx_ctx* ctx, const uint8_t* in, size_t in_bytes,
                                                  int n_strips, const rsx_phase_one_strip* strips,
                                                  const rsx_iiq_corr* corr, const rsx_image* img,
                                                  int32_t* strip_status) {
  if (!ctx || !in || !strips || !corr || !img || !img->data)
    return RSX_ERR_INVALID_ARG;
  ++ctx->host_calls;
  if (int st = phase_one_validate(n_strips, strips, in_bytes, *img))
    return st;
  if (int st = iiq_correct_validate(corr, img))
    return st;
  if (img->pitch_bytes % 2 != 0)
    return RSX_ERR_INVALID_ARG;
  CallPlan call;
  SingleImageHooks hooks;
  if (corr->n_ops != 0) { // (an empty list: no plan, the plain decode)
    if (int st = iiq_call_create(ctx, corr, img, call))
      return st;
    hooks.before_download = [&](uint8_t* dev, hipStream_t s) { return call.run(nullptr, dev, s); };
  }
  return phase_one_host(ctx, in, n_strips, strips, img, strip_status, hooks);
}

// ---------------------------------------------------------------------------
// RawImageData::fixBadPixels
// ---------------------------------------------------------------------------
extern "C" int rsx_bad_pixels_validate(const rsx_bad_pixels_desc* desc, const rsx_image* img) {
  return bad_pixels_validate(desc, img);
}

extern "C" int rsx_bad_pixels_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_bad_pixels_job* jobs,
                                          rsx_plan** out_plan) {
  return decoder_plan_create(ctx, n_jobs, jobs, out_plan, bad_pixels_plan_create);
}

extern "C" int rsx_bad_pixels_plan_result(rsx_plan* plan, int job, rsx_bad_pixels_result* out) {
  return decoder_plan_get(plan, [&](DecoderPlan* d) { return d->bad_pixels_result(job, out); });
}

namespace {
// the fix's plan of a host call (a CallPlan: it owns the call's two maps)
int bad_pixels_call_create(rsx_ctx* ctx, const rsx_bad_pixels_desc* desc, const rsx_image* img,
                           CallPlan& call) {
  rsx_bad_pixels_job job{};
  job.n_positions = desc->n_positions;
  job.map_in = desc->map_in;
  job.map_pitch = desc->map_in ? desc->map_pitch : 0u;
  job.is_f32 = desc->is_f32;
  job.img = *img;
  job.img.data = nullptr;
  return rsx_bad_pixels_plan_create(ctx, 1, &job, &call.plan);
}
// ... with the map from the zero pixels of a uint16 image
int bad_pixels_zero_call_create(rsx_ctx* ctx, const rsx_image* img, CallPlan& call) {
  rsx_bad_pixels_job job{};
  return decoder_plan_create(
      ctx, 1, &job, &call.plan,
      [&](rsx_ctx* c, int, const rsx_bad_pixels_job*, std::unique_ptr<DecoderPlan>* out) {
        return bad_pixels_zero_plan_create(c, img, out);
      });
}
// the counts and the map behind the fix's run
int bad_pixels_finish(const CallPlan& call, rsx_bad_pixels_result* result, uint8_t* map_out) {
  rsx_bad_pixels_result r;
  if (int st = call.plan->dec->bad_pixels_result(0, &r))
    return st;
  if (result)
    *result = r;
  if (map_out && r.map_made)
    return call.plan->dec->bad_pixels_map(0, map_out, call.plan->last_stream);
  return RSX_OK;
}

// The bad-pixel stage on a list of positions the host holds, behind a pass on the device image and
// in front of its download (the DNG _finish calls, rsx_phase_one_decompress_fixed): the positions
// go up and the fix runs on the same image and stream.
struct PositionsFixStage {
  uint8_t* map_out = nullptr;
  CallPlan fix;
  DeviceBuffer d_pos;
  bool ran = false;
  int run_positions(rsx_ctx* ctx, const uint32_t* positions, uint32_t n, int32_t is_f32,
                    const rsx_image* img, void* dev, hipStream_t s) {
    rsx_bad_pixels_desc d{};
    d.positions = positions;
    d.n_positions = n;
    d.is_f32 = is_f32;
    if (int e = bad_pixels_call_create(ctx, &d, img, fix))
      return e;
    if (int e = d_pos.ensure(size_t(n) * 4 + 16))
      return e;
    RSX_HIP_CHECK(ctx, hipMemcpyAsync(d_pos.ptr, positions, size_t(n) * 4, hipMemcpyHostToDevice,
                                      s ? s : ctx->stream));
    if (int e = fix.run(d_pos.ptr, dev, s))
      return e;
    ran = true;
    return RSX_OK;
  }
  // the map, behind the download
  int finish() { return ran && map_out ? bad_pixels_finish(fix, nullptr, map_out) : int(RSX_OK); }
};
} // namespace

// In place (in_place_call), the positions its side input.
extern "C" int rsx_bad_pixels_fix(rsx_ctx* ctx, const rsx_bad_pixels_desc* desc,
                                  const rsx_image* img, rsx_bad_pixels_result* result) {
  if (result)
    std::memset(result, 0, sizeof *result);
  if (!ctx || !desc || !img || !img->data)
    return RSX_ERR_INVALID_ARG;
  ++ctx->host_calls;
  if (int st = bad_pixels_validate(desc, img))
    return st;
  if (desc->n_positions == 0 && !desc->map_in)
    return RSX_OK; // (the reference makes no map and touches nothing)
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  CallPlan call;
  if (int st = bad_pixels_call_create(ctx, desc, img, call))
    return st;
  return in_place_call(
      ctx, img, size_t(img->dim_x) * (desc->is_f32 ? 4 : 2), desc->positions,
      size_t(desc->n_positions) * 4,
      [&](const void* pos_dev, void* dev, hipStream_t s) { return call.run(pos_dev, dev, s); },
      [&]() { return bad_pixels_finish(call, result, desc->map_out); });
}

// ---------------------------------------------------------------------------
// RawImageData::scaleBlackWhite
// ---------------------------------------------------------------------------
extern "C" int rsx_scale_validate(const rsx_scale_desc* desc, const rsx_image* img) {
  return scale_validate(desc, img);
}

extern "C" int rsx_scale_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_scale_job* jobs,
                                     rsx_plan** out_plan) {
  return decoder_plan_create(ctx, n_jobs, jobs, out_plan, scale_plan_create);
}

extern "C" int rsx_scale_plan_result(rsx_plan* plan, int job, rsx_scale_result* out) {
  return decoder_plan_get(plan, [&](DecoderPlan* d) { return d->scale_result(job, out); });
}

// In place (in_place_call): the estimate and the areas read the whole image, so the rows go up as
// one copy in front of the six launches.
extern "C" int rsx_scale_black_white(rsx_ctx* ctx, const rsx_scale_desc* desc, const rsx_image* img,
                                     rsx_scale_result* result) {
  if (result)
    std::memset(result, 0, sizeof *result);
  if (!ctx || !desc || !img || !img->data)
    return RSX_ERR_INVALID_ARG;
  ++ctx->host_calls;
  if (int st = scale_validate(desc, img))
    return st;
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  auto job = std::make_unique<rsx_scale_job>();
  std::memset(job.get(), 0, sizeof(rsx_scale_job));
  job->desc = *desc;
  job->img = *img;
  job->img.data = nullptr;
  CallPlan call;
  if (int st = rsx_scale_plan_create(ctx, 1, job.get(), &call.plan))
    return st;
  return in_place_call(
      ctx, img, size_t(img->dim_x) * size_t(img->cpp) * (desc->is_f32 ? 4 : 2), nullptr, 0,
      [&](const void*, void* dev, hipStream_t s) { return call.run(nullptr, dev, s); },
      [&]() { return result ? call.plan->dec->scale_result(0, result) : int(RSX_OK); });
}

// rsx_panasonic_v4_decompress, the map marked from the zero pixels of the decoded image and the
// fix on the device, ONE download.  The decode runs without its list: the map needs no capacity.
extern "C" int rsx_panasonic_v4_decompress_fixed(rsx_ctx* ctx, const rsx_panasonic_v4_desc* desc,
                                                 const uint8_t* in, size_t in_bytes,
                                                 const rsx_image* img, uint8_t* map_out,
                                                 uint32_t map_pitch,
                                                 rsx_bad_pixels_result* result) {
  if (result)
    std::memset(result, 0, sizeof *result);
  if (!ctx || !in || !img || !img->data)
    return RSX_ERR_INVALID_ARG;
  ++ctx->host_calls;
  uint64_t span = 0;
  if (int st = panasonic_v4_validate(desc, *img, in_bytes, &span))
    return st;
  if (int st = bad_pixels_validate_image(img, false))
    return st;
  if ((map_out || map_pitch != 0) && map_pitch != bad_pixels_map_pitch(uint32_t(img->dim_x)))
    return RSX_ERR_INVALID_ARG;
  CallPlan call;
  SingleImageHooks hooks;
  bool ran = false;
  if (desc->zero_is_bad) {
    if (int st = bad_pixels_zero_call_create(ctx, img, call))
      return st;
    hooks.before_download = [&](uint8_t* dev, hipStream_t s) {
      const int e = call.run(nullptr, dev, s);
      ran = e == RSX_OK;
      return e;
    };
  }
  rsx_panasonic_v4_job job;
  one_job_init(job, span, img);
  job.desc.section_split_offset = desc->section_split_offset;
  job.desc.zero_is_bad = 0;
  std::vector<uint8_t> key = one_job_key(rsx_panasonic_v4_plan_create, job);
  const int rc = single_image_host(ctx, key, rsx_panasonic_v4_plan_create, job, in, size_t(span),
                                   img, nullptr, hooks);
  if (rc != RSX_OK || !ran)
    return rc;
  // (an image without a zero pixel leaves mBadPixelPositions empty: the reference makes no map)
  rsx_bad_pixels_result r;
  if (int st = bad_pixels_finish(call, &r, nullptr))
    return st;
  if (r.n_bad == 0)
    return RSX_OK;
  if (result)
    *result = r;
  return map_out ? bad_pixels_finish(call, nullptr, map_out) : int(RSX_OK);
}

// rsx_phase_one_decompress_corrected, then the stage on the positions of the list's defects op
// (PositionsFixStage), ONE download.
extern "C" int rsx_iiq_defect_positions(const uint8_t* payload, uint32_t payload_bytes,
                                        int32_t dim_x, uint32_t* out, uint32_t cap, uint32_t* n) {
  return iiq_defect_positions(payload, payload_bytes, dim_x, out, cap, n);
}

extern "C" int rsx_phase_one_decompress_fixed(rsx_ctx* ctx, const uint8_t* in, size_t in_bytes,
                                               int n_strips, const rsx_phase_one_strip* strips,
                                               const rsx_iiq_corr* corr, const rsx_image* img,
                                               int32_t* strip_status, uint8_t* map_out,
                                               uint32_t map_pitch, rsx_bad_pixels_result* result) {
  if (result)
    std::memset(result, 0, sizeof *result);
  if (!ctx || !in || !strips || !corr || !img || !img->data)
    return RSX_ERR_INVALID_ARG;
  ++ctx->host_calls;
  if (int st = phase_one_validate(n_strips, strips, in_bytes, *img))
    return st;
  if (int st = iiq_correct_validate(corr, img))
    return st;
  if (img->pitch_bytes % 2 != 0)
    return RSX_ERR_INVALID_ARG;
  // the positions of the (one) defects op, and the stage's own checks on them
  std::vector<uint32_t> positions;
  for (int o = 0; o < corr->n_ops; ++o) {
    const rsx_iiq_op& op = corr->ops[o];
    if (op.kind != RSX_IIQ_OP_SENSOR_DEFECTS)
      continue;
    uint32_t n = 0;
    iiq_defect_positions(op.payload, op.payload_bytes, img->dim_x, nullptr, 0, &n);
    positions.resize(n);
    iiq_defect_positions(op.payload, op.payload_bytes, img->dim_x, positions.data(), n, &n);
  }
  rsx_bad_pixels_desc d{};
  d.positions = positions.data();
  d.n_positions = uint32_t(positions.size());
  d.map_pitch = map_pitch;
  d.map_out = map_out;
  if (int st = bad_pixels_validate(&d, img))
    return st;
  CallPlan call;
  PositionsFixStage fix;
  fix.map_out = map_out;
  SingleImageHooks hooks;
  if (corr->n_ops != 0) {
    if (int st = iiq_call_create(ctx, corr, img, call))
      return st;
    hooks.before_download = [&](uint8_t* dev, hipStream_t s) {
      if (int e = call.run(nullptr, dev, s))
        return e;
      if (positions.empty())
        return int(RSX_OK); // (the reference makes no map)
      return fix.run_positions(ctx, positions.data(), uint32_t(positions.size()), 0, img, dev, s);
    };
  }
  const int rc = phase_one_host(ctx, in, n_strips, strips, img, strip_status, hooks);
  if (rc != RSX_OK || !fix.ran)
    return rc;
  return bad_pixels_finish(fix.fix, result, map_out);
}

// ---------------------------------------------------------------------------
// DngDecoder behind the tiles: OpcodeList1 and the LinearizationTable look-up
// ---------------------------------------------------------------------------
extern "C" int rsx_dng_post_validate(const rsx_dng_post_desc* desc, const rsx_image* img,
                                     rsx_dng_post_result* result, uint32_t* bad,
                                     uint32_t bad_cap) {
  return dng_post_validate(desc, img, result, bad, bad_cap);
}

extern "C" int rsx_dng_post_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_dng_post_job* jobs,
                                        rsx_plan** out_plan) {
  return decoder_plan_create(ctx, n_jobs, jobs, out_plan, dng_post_plan_create);
}

extern "C" int rsx_dng_post_plan_result(rsx_plan* plan, int job, rsx_dng_post_result* out) {
  return decoder_plan_get(plan, [&](DecoderPlan* d) { return d->dng_post_result(job, out); });
}

extern "C" int rsx_dng_post_plan_bad_pixels(rsx_plan* plan, int job, uint32_t* out, uint32_t cap,
                                            uint64_t* n_bad) {
  if (n_bad)
    *n_bad = 0;
  return decoder_plan_get(plan, [&](DecoderPlan* d) { return d->bad_pixels(job, out, cap, n_bad); });
}

namespace {
// the pass's plan of a host call (a CallPlan: its key would be the list, up to 16 tables and the
// look-up table)
int dng_post_call_create(rsx_ctx* ctx, const rsx_dng_post_desc* desc, const rsx_image* img,
                         uint32_t bad_cap, CallPlan& call) {
  rsx_dng_post_job job{};
  job.desc = *desc;
  job.img = *img;
  job.img.data = nullptr;
  job.bad_cap = bad_cap;
  return rsx_dng_post_plan_create(ctx, 1, &job, &call.plan);
}
// in place on `dev`; returns when the pass is done.  A hit list past its capacity is no failure
// of the pass: dng_post_finish reports it.
int dng_post_run(CallPlan& call, void* dev, hipStream_t s) {
  if (int st = rsx_plan_run(call.plan, dev, dev, s))
    return st;
  const int st = rsx_plan_results(call.plan, nullptr, nullptr);
  return st == RSX_ERR_UNSUPPORTED ? int(RSX_OK) : st;
}
// the result and the positions behind the run; without a run (a failing tile) the parse's result
int dng_post_finish(const CallPlan& call, rsx_dng_post_result* result, uint32_t* bad,
                    uint32_t bad_cap, bool ran) {
  if (result)
    call.plan->dec->dng_post_result(0, result);
  if (!ran)
    return RSX_OK;
  uint64_t n = 0;
  return call.plan->dec->bad_pixels(0, bad, bad_cap, &n);
}

// The bad-pixel stage behind a pass (the _finish calls): the positions the pass composed go back
// up and the fix runs on the same image and stream, in front of the download.  A list past
// bad_cap leaves the image as the pass left it (the call then reports RSX_ERR_UNSUPPORTED, as the
// _post call does).  `on` false: the _post calls themselves, nothing happens.
struct DngFixStage : PositionsFixStage {
  bool on = false;
  // cpp > 1 with positions: refused before anything is decoded (section 5)
  static int refuse(const rsx_dng_post_desc* desc, const rsx_image* img) {
    if (img->cpp <= 1)
      return RSX_OK;
    rsx_dng_post_result r{};
    const int st = dng_post_validate(desc, img, &r, nullptr, 0);
    if (st != RSX_OK && st != RSX_ERR_UNSUPPORTED)
      return RSX_OK; // (the call itself reports it)
    return r.n_bad != 0 ? int(RSX_ERR_UNSUPPORTED) : int(RSX_OK);
  }
  int run(rsx_ctx* ctx, CallPlan& call, const rsx_dng_post_desc* desc, const rsx_image* img,
          uint32_t* bad, uint32_t bad_cap, void* dev, hipStream_t s) {
    if (!on)
      return RSX_OK;
    uint64_t n = 0;
    const int st = call.plan->dec->bad_pixels(0, bad, bad_cap, &n);
    if (st == RSX_ERR_UNSUPPORTED)
      return RSX_OK;
    if (st != RSX_OK)
      return st;
    if (n == 0)
      return RSX_OK; // (the reference makes no map)
    return run_positions(ctx, bad, uint32_t(n), desc->is_f32, img, dev, s);
  }
};

// In place (in_place_call): the pass, then the stage `fix`.
int dng_post_call(rsx_ctx* ctx, const rsx_dng_post_desc* desc, const rsx_image* img,
                  rsx_dng_post_result* result, uint32_t* bad, uint32_t bad_cap, DngFixStage& fix) {
  if (!ctx || !desc || !img || !img->data || (!bad && bad_cap != 0))
    return RSX_ERR_INVALID_ARG;
  ++ctx->host_calls;
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (fix.on)
    if (int st = DngFixStage::refuse(desc, img))
      return st;
  CallPlan call;
  if (int st = dng_post_call_create(ctx, desc, img, bad_cap, call))
    return st;
  return in_place_call(
      ctx, img, size_t(img->dim_x) * size_t(img->cpp) * (desc->is_f32 ? 4 : 2), nullptr, 0,
      [&](const void*, void* dev, hipStream_t s) {
        if (int st = dng_post_run(call, dev, s))
          return st;
        return fix.run(ctx, call, desc, img, bad, bad_cap, dev, s);
      },
      [&]() {
        if (int st = fix.finish())
          return st;
        return dng_post_finish(call, result, bad, bad_cap, true);
      });
}
} // namespace

extern "C" int rsx_dng_post(rsx_ctx* ctx, const rsx_dng_post_desc* desc, const rsx_image* img,
                            rsx_dng_post_result* result, uint32_t* bad, uint32_t bad_cap) {
  DngFixStage none;
  return dng_post_call(ctx, desc, img, result, bad, bad_cap, none);
}

// rsx_dng_post, then the bad-pixel stage on the positions the pass composed, in front of the
// download (a device pointer: in place)
extern "C" int rsx_dng_finish(rsx_ctx* ctx, const rsx_dng_post_desc* desc, const rsx_image* img,
                              rsx_dng_post_result* result, uint32_t* bad, uint32_t bad_cap,
                              uint8_t* map_out) {
  DngFixStage fix;
  fix.on = true;
  fix.map_out = map_out;
  return dng_post_call(ctx, desc, img, result, bad, bad_cap, fix);
}

// rsx_dng_decompress_ljpeg, the list and the look-up on the decoded image on the device, ONE
// download.  The tiles go up as one call (no bands: the pass needs the whole image).
namespace {
int dng_ljpeg_post_call(rsx_ctx* ctx, int n_tiles, const rsx_dng_ljpeg_tile* tiles,
                        const rsx_dng_post_desc* desc, const rsx_image* img, int32_t* tile_status,
                        uint32_t* tile_consumed, rsx_dng_post_result* result, uint32_t* bad,
                        uint32_t bad_cap, DngFixStage& fix) {
  if (!ctx || !tiles || n_tiles < 1 || !desc || !img || !img->data || (!bad && bad_cap != 0))
    return RSX_ERR_INVALID_ARG;
  if (desc->is_f32)
    return RSX_ERR_INVALID_ARG; // (LJPEG tiles decode to uint16)
  if (fix.on)
    if (int st = DngFixStage::refuse(desc, img))
      return st;
  CallPlan call;
  if (int st = dng_post_call_create(ctx, desc, img, bad_cap, call))
    return st;
  std::vector<rsx_ljpeg_job> jobs(n_tiles);
  std::vector<const uint8_t*> ins(n_tiles);
  for (int i = 0; i < n_tiles; ++i) {
    jobs[i].desc = tiles[i].desc;
    jobs[i].in_bytes = tiles[i].in_bytes;
    ins[i] = tiles[i].in;
  }
  constexpr int32_t ST_UNSET = INT32_MIN;
  std::vector<int32_t> st(n_tiles, ST_UNSET);
  std::vector<uint32_t> cons(n_tiles, 0);
  bool ran = false;
  const DevicePostFn post = [&](uint8_t* dev, hipStream_t s) {
    int e = dng_post_run(call, dev, s);
    if (e == RSX_OK)
      e = fix.run(ctx, call, desc, img, bad, bad_cap, dev, s);
    ran = e == RSX_OK;
    return e;
  };
  const int rc = ljpeg_family_host(ctx, n_tiles, jobs, ins.data(), img, rsx_ljpeg_plan_create,
                                   st.data(), cons.data(), true, &post);
  bool tile_failed = false, reached = true;
  for (int32_t& v : st) {
    reached = reached && v != ST_UNSET; // (unset: the call came back before its plan's results)
    tile_failed = tile_failed || (v != RSX_OK && v != ST_UNSET);
  }
  // tile_status and tile_consumed are written only by a call that wrote the image: every tile
  // decoded and the pass ran, or a tile failed and the call was the plain call.  A call that
  // returns without a download (tiles that do not tile the image, a device failure, a failure
  // of the pass) leaves them as the caller set them.
  if (!reached || rc == RSX_ERR_DEVICE || rc == RSX_ERR_NOMEM || (rc != RSX_OK && !tile_failed) ||
      (rc == RSX_OK && !tile_failed && !ran))
    return rc != RSX_OK ? rc : int(RSX_ERR_DEVICE);
  if (tile_status)
    std::copy(st.begin(), st.end(), tile_status);
  if (tile_consumed)
    std::copy(cons.begin(), cons.end(), tile_consumed);
  if (tile_failed) {
    dng_post_finish(call, result, nullptr, 0, false);
    return RSX_ERR_TILE_ERRORS; // (the plain call's verdict; nothing of the list was applied)
  }
  if (int e = fix.finish())
    return e;
  return dng_post_finish(call, result, bad, bad_cap, true);
}
} // namespace

extern "C" int rsx_dng_decompress_ljpeg_post(rsx_ctx* ctx, int n_tiles,
                                             const rsx_dng_ljpeg_tile* tiles,
                                             const rsx_dng_post_desc* desc, const rsx_image* img,
                                             int32_t* tile_status, uint32_t* tile_consumed,
                                             rsx_dng_post_result* result, uint32_t* bad,
                                             uint32_t bad_cap) {
  DngFixStage none;
  return dng_ljpeg_post_call(ctx, n_tiles, tiles, desc, img, tile_status, tile_consumed, result, bad,
                             bad_cap, none);
}

// rsx_dng_decompress_ljpeg_post with the bad-pixel stage behind the look-up, in front of the download
extern "C" int rsx_dng_decompress_ljpeg_finish(rsx_ctx* ctx, int n_tiles,
                                               const rsx_dng_ljpeg_tile* tiles,
                                               const rsx_dng_post_desc* desc, const rsx_image* img,
                                               int32_t* tile_status, uint32_t* tile_consumed,
                                               rsx_dng_post_result* result, uint32_t* bad,
                                               uint32_t bad_cap, uint8_t* map_out) {
  DngFixStage fix;
  fix.on = true;
  fix.map_out = map_out;
  return dng_ljpeg_post_call(ctx, n_tiles, tiles, desc, img, tile_status, tile_consumed, result, bad,
                             bad_cap, fix);
}

// rsx_dng_decompress_uncompressed, the list and the look-up on the device, ONE download.  The
// tiles are unpacked into the image's own layout on the device (the plain call keeps a compact
// rectangle per tile and downloads in bands); tiles that do not all
// validate make this the plain call (a tile fails: nothing of the list is applied); tiles that do
// not cover the image are RSX_ERR_UNSUPPORTED, nothing written.
namespace {
int dng_uncompressed_post_call(rsx_ctx* ctx, int n_tiles, const rsx_dng_unpack_tile* tiles,
                               const rsx_dng_post_desc* desc, const rsx_image* img,
                               int32_t* tile_status, rsx_dng_post_result* result, uint32_t* bad,
                               uint32_t bad_cap, DngFixStage& fix) {
  if (!ctx || !tiles || n_tiles < 1 || !desc || !img || !img->data || (!bad && bad_cap != 0))
    return RSX_ERR_INVALID_ARG;
  if (desc->is_f32)
    return RSX_ERR_INVALID_ARG; // (rsx_unpack_f32 images: rsx_dng_post on the result)
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (fix.on)
    if (int st = DngFixStage::refuse(desc, img))
      return st;
  CallPlan call;
  if (int st = dng_post_call_create(ctx, desc, img, bad_cap, call))
    return st;
  std::vector<rsx_unpack_job> jobs(n_tiles);
  size_t in_total = 0;
  std::vector<HostRect> rects(static_cast<size_t>(n_tiles));
  bool plain = img->pitch_bytes % 2 != 0;
  for (int i = 0; i < n_tiles && !plain; ++i) {
    const rsx_unpack_desc& d = tiles[i].desc;
    if (!tiles[i].in || validate_unpack(d, *img, tiles[i].in_bytes) != RSX_OK) {
      plain = true;
      break;
    }
    // (a packed tile is written from column 0 whatever its crop_x, as the reference's packed
    // paths do: tiles side by side land on each other, in the plain call one after the other --
    // one launch over the image's own layout has no such order)
    if (d.crop_x != 0 && !(d.bit_order == RSX_ORDER_LSB && d.bits_per_pixel == 16))
      return RSX_ERR_UNSUPPORTED;
    jobs[i].desc = d;
    jobs[i].in_offset = in_total;
    jobs[i].in_bytes = size_t(d.crop_h) * size_t(d.input_pitch_bytes);
    jobs[i].img_offset = 0;
    jobs[i].img = *img;
    jobs[i].img.data = nullptr;
    in_total += align_up(size_t(jobs[i].in_bytes), 16);
    const int64_t rows = std::min<int64_t>(d.crop_h, int64_t(img->dim_y) - d.crop_y);
    rects[size_t(i)] = HostRect{size_t(d.crop_y), size_t(std::max<int64_t>(rows, 0)),
                                size_t(d.crop_x) * size_t(img->cpp) * 2,
                                size_t(d.crop_w) * size_t(img->cpp) * 2};
  }
  if (plain) {
    dng_post_finish(call, result, nullptr, 0, false);
    return rsx_dng_decompress_uncompressed(ctx, n_tiles, tiles, img, tile_status);
  }
  // (inside the image, disjoint, all of it: the pass needs the whole image, and a byte no tile
  // wrote would be looked up and downloaded)
  if (!rects_tile_image(std::move(rects), size_t(img->dim_y),
                        size_t(img->dim_x) * size_t(img->cpp) * 2))
    return RSX_ERR_UNSUPPORTED; // (nothing decoded, nothing written, tile_status untouched)
  ++ctx->host_calls;
  LaneGuard lane(ctx);
  if (!lane.lane)
    return RSX_ERR_DEVICE;
  const size_t row_bytes = size_t(img->dim_x) * size_t(img->cpp) * 2;
  const size_t out_bytes = size_t(img->pitch_bytes) * size_t(img->dim_y);
  if (int e = lane.lane->d_in.ensure(in_total + 64))
    return e;
  if (int e = lane.lane->d_out.ensure(out_bytes + 64))
    return e;
  hipStream_t s = lane.lane->stream;
  {
    std::lock_guard<std::mutex> up(ctx->upload_mu);
    for (int i = 0; i < n_tiles; ++i)
      RSX_HIP_CHECK(ctx, hipMemcpyAsync(static_cast<uint8_t*>(lane.lane->d_in.ptr) + jobs[i].in_offset,
                                        tiles[i].in, jobs[i].in_bytes, hipMemcpyHostToDevice, s));
  }
  std::vector<int32_t> st(n_tiles, RSX_OK);
  {
    CallPlan unpack;
    if (int e = rsx_unpack_plan_create(ctx, n_tiles, jobs.data(), &unpack.plan))
      return e;
    int rc = rsx_plan_run(unpack.plan, lane.lane->d_in.ptr, lane.lane->d_out.ptr, s);
    if (rc == RSX_OK)
      rc = rsx_plan_results(unpack.plan, st.data(), nullptr);
    if (rc != RSX_OK)
      return rc; // (every tile validated: a device failure; tile_status untouched)
  }
  if (int e = dng_post_run(call, lane.lane->d_out.ptr, s))
    return e;
  if (int e = fix.run(ctx, call, desc, img, bad, bad_cap, lane.lane->d_out.ptr, s))
    return e;
  DownRect dr{static_cast<uint8_t*>(img->data), img->pitch_bytes,
              static_cast<const uint8_t*>(lane.lane->d_out.ptr), img->pitch_bytes, row_bytes,
              size_t(img->dim_y)};
  {
    std::lock_guard<std::mutex> down_lock(ctx->download_mu);
    if (int e = download_rects(ctx, lane.lane, s, &dr, 1))
      return e;
  }
  // (tile_status is written only by a call that wrote the image)
  if (tile_status)
    std::copy(st.begin(), st.end(), tile_status);
  if (int e = fix.finish())
    return e;
  return dng_post_finish(call, result, bad, bad_cap, true);
}
} // namespace

extern "C" int rsx_dng_decompress_uncompressed_post(rsx_ctx* ctx, int n_tiles,
                                                    const rsx_dng_unpack_tile* tiles,
                                                    const rsx_dng_post_desc* desc,
                                                    const rsx_image* img, int32_t* tile_status,
                                                    rsx_dng_post_result* result, uint32_t* bad,
                                                    uint32_t bad_cap) {
  DngFixStage none;
  return dng_uncompressed_post_call(ctx, n_tiles, tiles, desc, img, tile_status, result, bad,
                                    bad_cap, none);
}

// rsx_dng_decompress_uncompressed_post with the bad-pixel stage behind the look-up, in front of
// the download
extern "C" int rsx_dng_decompress_uncompressed_finish(rsx_ctx* ctx, int n_tiles,
                                                      const rsx_dng_unpack_tile* tiles,
                                                      const rsx_dng_post_desc* desc,
                                                      const rsx_image* img, int32_t* tile_status,
                                                      rsx_dng_post_result* result, uint32_t* bad,
                                                      uint32_t bad_cap, uint8_t* map_out) {
  DngFixStage fix;
  fix.on = true;
  fix.map_out = map_out;
  return dng_uncompressed_post_call(ctx, n_tiles, tiles, desc, img, tile_status, result, bad,
                                    bad_cap, fix);
}

// ---------------------------------------------------------------------------
// DngDecoder's branch for lossy DNGs: JPEG tiles, OpcodeList1 and the look-up, scaleBlackWhite,
// OpcodeList2, fixBadPixels -- every stage the plan its stand-alone call runs, on the one staged
// image and the one stream, ONE download.
// ---------------------------------------------------------------------------
namespace {
// a list's verdict and its FixBadPixelsList positions, whatever their number
int dng_lossy_parse(const rsx_dng_post_desc* d, const rsx_image* img, rsx_dng_post_result* r,
                    std::vector<uint32_t>* fixed) {
  fixed->clear();
  std::memset(r, 0, sizeof *r);
  int st = dng_post_validate(d, img, r, nullptr, 0);
  if (st == RSX_ERR_UNSUPPORTED && r->n_bad != 0) { // (refused for the capacity alone)
    fixed->resize(size_t(r->n_bad));
    st = dng_post_validate(d, img, r, fixed->data(), uint32_t(fixed->size()));
  }
  return st;
}

// Every check of the chain that needs no pixel, in this order: list 1, list 2, the scale stage's
// crop and descriptor, the fix.  `r` receives both parses, *d2 list 2 as a descriptor of its own.
int dng_lossy_check(const rsx_dng_lossy_desc* desc, const rsx_image* img, rsx_dng_lossy_result* r,
                    std::vector<uint32_t>* fixed1, std::vector<uint32_t>* fixed2,
                    rsx_dng_post_desc* d2) {
  std::memset(r, 0, sizeof *r);
  fixed1->clear();
  fixed2->clear();
  if (!desc || !img)
    return RSX_ERR_INVALID_ARG;
  if (desc->stage1.is_f32)
    return RSX_ERR_INVALID_ARG; // (JPEG tiles decode to uint16)
  if (int st = dng_lossy_parse(&desc->stage1, img, &r->list1, fixed1))
    return st;
  if (desc->has_list2) {
    // (DngDecoder.cpp:628 has no `count > 0` guard: the constructor's getU32 throws IOException)
    if (desc->opcodes2_bytes == 0)
      return RSX_ERR_IO;
    std::memset(d2, 0, sizeof *d2);
    d2->opcodes = desc->opcodes2;
    d2->opcodes_bytes = desc->opcodes2_bytes;
    d2->crop_x = r->list1.crop_x;
    d2->crop_y = r->list1.crop_y;
    d2->crop_w = r->list1.crop_w;
    d2->crop_h = r->list1.crop_h;
    if (int st = dng_lossy_parse(d2, img, &r->list2, fixed2)) {
      std::memset(&r->list2, 0, sizeof r->list2);
      return st;
    }
    const rsx_scale_desc& sc = desc->scale;
    if (sc.is_f32 || sc.off_x != r->list1.crop_x || sc.off_y != r->list1.crop_y ||
        sc.crop_x != r->list1.crop_w || sc.crop_y != r->list1.crop_h)
      return RSX_ERR_INVALID_ARG;
    if (int st = scale_validate(&sc, img))
      return st;
  }
  // cpp > 1 with positions: refused before anything is decoded (section 5)
  if (desc->fix && img->cpp > 1 && (!fixed1->empty() || !fixed2->empty()))
    return RSX_ERR_UNSUPPORTED;
  return RSX_OK;
}

// mBadPixelPositions behind both lists: list 2's FixBadPixelsList entries went to the front, its
// constant hits to the back (common/DngOpcodes.cpp:180, :320).  b1, b2: what each pass composed,
// n_fixed2 of b2 list entries.
void dng_lossy_merge(const std::vector<uint32_t>& b1, const std::vector<uint32_t>& b2,
                     size_t n_fixed2, uint32_t* out) {
  out = std::copy(b2.begin(), b2.begin() + n_fixed2, out);
  out = std::copy(b1.begin(), b1.end(), out);
  std::copy(b2.begin() + n_fixed2, b2.end(), out);
}

// the positions a pass composed; RSX_ERR_UNSUPPORTED (with *n exact) when they are more than cap
int dng_lossy_positions(const CallPlan& call, uint64_t cap, std::vector<uint32_t>* out, uint64_t* n) {
  out->clear();
  const int st = call.plan->dec->bad_pixels(0, nullptr, 0, n);
  if (st != RSX_OK && st != RSX_ERR_UNSUPPORTED)
    return st;
  if (*n == 0)
    return RSX_OK;
  if (*n > cap)
    return RSX_ERR_UNSUPPORTED;
  out->resize(size_t(*n));
  return call.plan->dec->bad_pixels(0, out->data(), uint32_t(*n), n);
}
} // namespace

extern "C" int rsx_dng_lossy_validate(const rsx_dng_lossy_desc* desc, const rsx_image* img,
                                      rsx_dng_lossy_result* result, uint32_t* bad,
                                      uint32_t bad_cap) {
  if (result)
    std::memset(result, 0, sizeof *result);
  if (!bad && bad_cap != 0)
    return RSX_ERR_INVALID_ARG;
  rsx_dng_lossy_result r;
  std::vector<uint32_t> f1, f2;
  rsx_dng_post_desc d2;
  const int st = dng_lossy_check(desc, img, &r, &f1, &f2, &d2);
  if (result)
    *result = r;
  if (st != RSX_OK)
    return st;
  if (f1.size() + f2.size() > bad_cap)
    return RSX_ERR_UNSUPPORTED;
  if (bad)
    dng_lossy_merge(f1, f2, f2.size(), bad);
  return RSX_OK;
}

extern "C" int rsx_dng_lossy_decompress(rsx_ctx* ctx, int n_tiles, const rsx_dng_jpeg_tile* tiles,
                                        const rsx_dng_lossy_desc* desc, const rsx_image* img,
                                        int32_t* tile_status, rsx_dng_lossy_result* result,
                                        uint32_t* bad, uint32_t bad_cap, uint8_t* map_out) {
  if (result)
    std::memset(result, 0, sizeof *result);
  if (!ctx || !tiles || n_tiles < 1 || !desc || !img || !img->data || (!bad && bad_cap != 0))
    return RSX_ERR_INVALID_ARG;
  ++ctx->host_calls;
  rsx_dng_lossy_result R;
  std::vector<uint32_t> f1, f2;
  rsx_dng_post_desc d2;
  const int checked = dng_lossy_check(desc, img, &R, &f1, &f2, &d2);
  if (result)
    *result = R;
  if (checked != RSX_OK)
    return checked;
  const bool two = desc->has_list2 != 0;
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  CallPlan list1, scale, list2;
  if (int st = dng_post_call_create(ctx, &desc->stage1, img, bad_cap, list1))
    return st;
  if (two) {
    auto job = std::make_unique<rsx_scale_job>();
    std::memset(job.get(), 0, sizeof(rsx_scale_job));
    job->desc = desc->scale;
    job->img = *img;
    job->img.data = nullptr;
    if (int st = rsx_scale_plan_create(ctx, 1, job.get(), &scale.plan))
      return st;
    if (int st = dng_post_call_create(ctx, &d2, img, bad_cap, list2))
      return st;
  }
  PositionsFixStage fix;
  uint32_t stages = 0;
  uint64_t n1 = 0, n2 = 0;
  std::vector<uint32_t> b1, b2;
  bool refused = false, fits = false;
  const DevicePostFn post = [&](uint8_t* dev, hipStream_t s) {
    if (int e = dng_post_run(list1, dev, s))
      return e;
    stages = RSX_DNG_LOSSY_STAGE1;
    if (two) {
      if (int e = rsx_plan_run(scale.plan, dev, dev, s))
        return e;
      const int e = rsx_plan_results(scale.plan, nullptr, nullptr);
      if (e == RSX_ERR_UNSUPPORTED) { // (refused from the image's contents: nothing written)
        refused = true;
      } else if (e != RSX_OK) {
        return e;
      } else {
        stages |= RSX_DNG_LOSSY_SCALED;
        if (int e2 = dng_post_run(list2, dev, s))
          return e2;
        stages |= RSX_DNG_LOSSY_LIST2;
      }
    }
    // the positions: the image is complete whether they fit or not
    const int p1 = dng_lossy_positions(list1, bad_cap, &b1, &n1);
    if (p1 != RSX_OK && p1 != RSX_ERR_UNSUPPORTED)
      return p1;
    int p2 = RSX_OK;
    if (stages & RSX_DNG_LOSSY_LIST2) {
      p2 = dng_lossy_positions(list2, bad_cap, &b2, &n2);
      if (p2 != RSX_OK && p2 != RSX_ERR_UNSUPPORTED)
        return p2;
    }
    fits = p1 == RSX_OK && p2 == RSX_OK && n1 + n2 <= bad_cap;
    if (!fits)
      return int(RSX_OK);
    // (b2 is what list 2's pass composed: empty, list entries included, where it did not run)
    if (n1 + n2 != 0)
      dng_lossy_merge(b1, b2, std::min(f2.size(), b2.size()), bad);
    if (!desc->fix || refused)
      return int(RSX_OK);
    if (n1 + n2 != 0) // (none: the reference makes no map)
      if (int e = fix.run_positions(ctx, bad, uint32_t(n1 + n2), 0, img, dev, s))
        return e;
    stages |= RSX_DNG_LOSSY_FIXED;
    return int(RSX_OK);
  };
  std::vector<int32_t> st(size_t(n_tiles), RSX_OK);
  bool wrote = false;
  const int rc = dng_jpeg_host(ctx, n_tiles, tiles, img, st.data(), false, &post, &wrote);
  // (tile_status is written only by a call that wrote the image)
  if (!wrote)
    return rc != RSX_OK ? rc : int(RSX_ERR_DEVICE);
  if (tile_status)
    std::copy(st.begin(), st.end(), tile_status);
  if (rc != RSX_OK)
    return rc; // (a tile failed: the plain call; the result carries the parses alone)
  if (stages == 0)
    return RSX_ERR_DEVICE;
  dng_post_finish(list1, &R.list1, nullptr, 0, false); // (n_bad: the exact count behind the run)
  if (stages & RSX_DNG_LOSSY_SCALED)
    if (int e = scale.plan->dec->scale_result(0, &R.scale))
      return e;
  if (stages & RSX_DNG_LOSSY_LIST2)
    dng_post_finish(list2, &R.list2, nullptr, 0, false);
  else
    R.list2.n_bad = 0; // (the parse's verdict stays; none of its positions is in `bad`)
  if (fix.ran)
    if (int e = bad_pixels_finish(fix.fix, &R.fixed, map_out))
      return e;
  R.stages = stages;
  if (result)
    *result = R;
  return refused || !fits ? int(RSX_ERR_UNSUPPORTED) : int(RSX_OK);
}

// ---------------------------------------------------------------------------
// SonyArw2Decompressor
// ---------------------------------------------------------------------------
extern "C" int rsx_sony_arw2_validate(const rsx_sony_arw2_desc* desc, const rsx_image* img,
                                      size_t in_bytes) {
  if (!img)
    return RSX_ERR_INVALID_ARG;
  return sony_arw2_validate(desc, *img, in_bytes);
}

extern "C" int rsx_sony_arw2_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_sony_arw2_job* jobs,
                                         rsx_plan** out_plan) {
  return decoder_plan_create(ctx, n_jobs, jobs, out_plan, sony_arw2_plan_create);
}

// The host-pointer call (single_image_host): the w * h bytes go up as one copy.  The plan is
// keyed by the geometry and the table mode; the table itself is call data and goes up on every
// call.
extern "C" int rsx_sony_arw2_decompress(rsx_ctx* ctx, const rsx_sony_arw2_desc* desc,
                                        const uint8_t* in, size_t in_bytes, const rsx_image* img,
                                        int32_t* row_status) {
  if (!ctx || !in || !img || !img->data)
    return RSX_ERR_INVALID_ARG;
  ++ctx->host_calls;
  if (int st = sony_arw2_validate(desc, *img, in_bytes))
    return st;
  const size_t span = size_t(img->dim_x) * size_t(img->dim_y);
  rsx_sony_arw2_job job;
  one_job_init(job, span, img);
  job.desc.table_mode = desc->table_mode;
  // (desc.table is NULL here: not in the key)
  std::vector<uint8_t> key = one_job_key(rsx_sony_arw2_plan_create, job);
  job.desc.table = desc->table;
  // this call's table onto a plan the lane held, ordered before the run on the lane's stream
  SingleImageHooks hooks;
  hooks.on_reuse = [desc](rsx_plan* plan, hipStream_t s) {
    return sony_arw2_plan_set_table(plan->dec.get(), 0, desc, s);
  };
  return single_image_host(ctx, key, rsx_sony_arw2_plan_create, job, in, span, img, row_status,
                           hooks);
}

// ---------------------------------------------------------------------------
// NefDecoder::DecodeNikonSNef
// ---------------------------------------------------------------------------
extern "C" int rsx_nikon_snef_validate(const rsx_nikon_snef_desc* desc, const rsx_image* img,
                                       size_t in_bytes) {
  if (!img)
    return RSX_ERR_INVALID_ARG;
  return nikon_snef_validate(desc, *img, in_bytes);
}

extern "C" int rsx_nikon_snef_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_nikon_snef_job* jobs,
                                          rsx_plan** out_plan) {
  return decoder_plan_create(ctx, n_jobs, jobs, out_plan, nikon_snef_plan_create);
}

// The host-pointer call (single_image_host): the 3 w h bytes go up as one copy.  The plan is
// keyed by the geometry and the white balance; the table itself is call data and goes up on
// every call.
extern "C" int rsx_nikon_snef_decompress(rsx_ctx* ctx, const rsx_nikon_snef_desc* desc,
                                         const uint8_t* in, size_t in_bytes, const rsx_image* img) {
  if (!ctx || !in || !img || !img->data)
    return RSX_ERR_INVALID_ARG;
  ++ctx->host_calls;
  if (int st = nikon_snef_validate(desc, *img, in_bytes))
    return st;
  const size_t span = size_t(img->dim_x) * size_t(img->dim_y) * 3u;
  rsx_nikon_snef_job job;
  one_job_init(job, span, img);
  job.desc.inv_wb_r = desc->inv_wb_r;
  job.desc.inv_wb_b = desc->inv_wb_b;
  // (desc.table is NULL here: not in the key)
  std::vector<uint8_t> key = one_job_key(rsx_nikon_snef_plan_create, job);
  job.desc.table = desc->table;
  // this call's table onto a plan the lane held, ordered before the run on the lane's stream
  SingleImageHooks hooks;
  hooks.on_reuse = [desc](rsx_plan* plan, hipStream_t s) {
    return nikon_snef_plan_set_table(plan->dec.get(), 0, desc, s);
  };
  return single_image_host(ctx, key, rsx_nikon_snef_plan_create, job, in, span, img, nullptr,
                           hooks);
}

// ---------------------------------------------------------------------------
// VC5Decompressor (DNG compression 9)
// ---------------------------------------------------------------------------
extern "C" int rsx_vc5_validate(const rsx_vc5_desc* desc, const rsx_image* img, size_t in_bytes) {
  if (!img)
    return RSX_ERR_INVALID_ARG;
  return vc5_validate(desc, *img, in_bytes);
}

extern "C" int rsx_vc5_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_vc5_job* jobs,
                                   rsx_plan** out_plan) {
  return decoder_plan_create(ctx, n_jobs, jobs, out_plan, vc5_plan_create);
}

extern "C" int rsx_vc5_plan_bands(rsx_plan* plan, int job, int32_t* band_status, uint32_t* windows,
                                  uint32_t* rounds) {
  return decoder_plan_get(
      plan, [&](DecoderPlan* d) { return vc5_plan_bands(d, job, band_status, windows, rounds); });
}

// The host-pointer call (single_image_host): the tile's bytes go up as one copy.  The plan is
// keyed by the whole descriptor, the code words and the log table included, so a plan the lane
// held is this call's plan as it stands.
extern "C" int rsx_vc5_decompress(rsx_ctx* ctx, const rsx_vc5_desc* desc, const uint8_t* in,
                                  size_t in_bytes, const rsx_image* img) {
  if (!ctx || !in || !img || !img->data)
    return RSX_ERR_INVALID_ARG;
  ++ctx->host_calls;
  if (int st = vc5_validate(desc, *img, in_bytes))
    return st;
  rsx_vc5_job job;
  one_job_init(job, in_bytes, img);
  job.desc = *desc;
  job.desc.log_table = nullptr;
  job.desc.codes = nullptr;
  std::vector<uint8_t> key = one_job_key(rsx_vc5_plan_create, job);
  key_append(key, desc->codes, size_t(desc->n_codes));
  key_append(key, desc->log_table, size_t(4096));
  job.desc.log_table = desc->log_table;
  job.desc.codes = desc->codes;
  return single_image_host(ctx, key, rsx_vc5_plan_create, job, in, in_bytes, img, nullptr);
}

// ---------------------------------------------------------------------------
// PanasonicV5Decompressor, PanasonicV6Decompressor, PanasonicV7Decompressor
// ---------------------------------------------------------------------------
extern "C" int rsx_panasonic_validate(const rsx_panasonic_desc* desc, const rsx_image* img,
                                      size_t in_bytes) {
  if (!img)
    return RSX_ERR_INVALID_ARG;
  return panasonic_validate(desc, *img, in_bytes);
}

extern "C" int rsx_panasonic_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_panasonic_job* jobs,
                                         rsx_plan** out_plan) {
  return decoder_plan_create(ctx, n_jobs, jobs, out_plan, panasonic_plan_create);
}

// The host-pointer call (single_image_host): the bytes the constructor's peekStream takes go up
// as one copy.  The plan is keyed by version, bps and geometry; nothing is per-call data.
extern "C" int rsx_panasonic_decompress(rsx_ctx* ctx, const rsx_panasonic_desc* desc,
                                        const uint8_t* in, size_t in_bytes, const rsx_image* img) {
  if (!ctx || !in || !img || !img->data)
    return RSX_ERR_INVALID_ARG;
  ++ctx->host_calls;
  uint64_t span = 0;
  if (int st = panasonic_validate(desc, *img, in_bytes, &span))
    return st;
  rsx_panasonic_job job;
  one_job_init(job, span, img);
  job.desc = *desc;
  std::vector<uint8_t> key = one_job_key(rsx_panasonic_plan_create, job);
  return single_image_host(ctx, key, rsx_panasonic_plan_create, job, in, size_t(span), img, nullptr);
}

// ---------------------------------------------------------------------------
// PanasonicV4Decompressor
// ---------------------------------------------------------------------------
extern "C" int rsx_panasonic_v4_validate(const rsx_panasonic_v4_desc* desc, const rsx_image* img,
                                         size_t in_bytes) {
  if (!img)
    return RSX_ERR_INVALID_ARG;
  return panasonic_v4_validate(desc, *img, in_bytes);
}

extern "C" int rsx_panasonic_v4_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_panasonic_v4_job* jobs,
                                            rsx_plan** out_plan) {
  return decoder_plan_create(ctx, n_jobs, jobs, out_plan, panasonic_v4_plan_create);
}

extern "C" int rsx_panasonic_v4_plan_bad_pixels(rsx_plan* plan, int job, uint32_t* out, uint32_t cap,
                                                uint64_t* n_bad) {
  if (n_bad)
    *n_bad = 0;
  return decoder_plan_get(plan, [&](DecoderPlan* d) { return d->bad_pixels(job, out, cap, n_bad); });
}

// The host-pointer call (single_image_host): the bytes the constructor's peekStream takes go up
// as one copy.  The plan is keyed by the split, the flag, the capacity and the geometry.  Behind
// the results the list and its count go to the caller; an image whose list did not fit is
// complete, and comes down like any other before the call reports RSX_ERR_UNSUPPORTED.
extern "C" int rsx_panasonic_v4_decompress(rsx_ctx* ctx, const rsx_panasonic_v4_desc* desc,
                                           const uint8_t* in, size_t in_bytes, const rsx_image* img,
                                           uint32_t* bad, uint32_t bad_cap, uint64_t* n_bad) {
  if (n_bad)
    *n_bad = 0;
  if (!ctx || !in || !img || !img->data || (!bad && bad_cap != 0))
    return RSX_ERR_INVALID_ARG;
  ++ctx->host_calls;
  uint64_t span = 0;
  if (int st = panasonic_v4_validate(desc, *img, in_bytes, &span))
    return st;
  rsx_panasonic_v4_job job;
  one_job_init(job, span, img);
  job.desc.section_split_offset = desc->section_split_offset;
  job.desc.zero_is_bad = desc->zero_is_bad != 0;
  job.bad_cap = uint32_t(std::min<uint64_t>(bad_cap, uint64_t(img->dim_x) * uint64_t(img->dim_y)));
  std::vector<uint8_t> key = one_job_key(rsx_panasonic_v4_plan_create, job);
  int list_rc = RSX_OK;
  SingleImageHooks hooks;
  hooks.on_done = [&](rsx_plan* plan, int st) {
    if (st != RSX_OK && st != RSX_ERR_UNSUPPORTED)
      return st;
    list_rc = plan->dec->bad_pixels(0, bad, job.bad_cap, n_bad);
    return list_rc == RSX_OK || list_rc == RSX_ERR_UNSUPPORTED ? int(RSX_OK) : list_rc;
  };
  const int rc = single_image_host(ctx, key, rsx_panasonic_v4_plan_create, job, in, size_t(span),
                                   img, nullptr, hooks);
  return rc != RSX_OK ? rc : list_rc;
}

// ---------------------------------------------------------------------------
// SamsungV0Decompressor
// ---------------------------------------------------------------------------
extern "C" int rsx_samsung_v0_validate(const uint32_t* row_offsets, int n_offsets, size_t in_bytes,
                                       const rsx_image* img) {
  if (!img)
    return RSX_ERR_INVALID_ARG;
  return samsung_v0_validate(row_offsets, n_offsets, in_bytes, *img);
}

extern "C" int rsx_samsung_v0_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_samsung_v0_job* jobs,
                                          rsx_plan** out_plan) {
  return decoder_plan_create(ctx, n_jobs, jobs, out_plan, samsung_v0_plan_create);
}

// The host-pointer call (single_image_host): the bytes from the first row's offset up go up as
// one copy; the plan's key holds the row offsets.
extern "C" int rsx_samsung_v0_decompress(rsx_ctx* ctx, const uint8_t* in, size_t in_bytes,
                                         const uint32_t* row_offsets, int n_offsets,
                                         const rsx_image* img, int32_t* row_status) {
  if (!ctx || !in || !img || !img->data)
    return RSX_ERR_INVALID_ARG;
  ++ctx->host_calls;
  if (int st = samsung_v0_validate(row_offsets, n_offsets, in_bytes, *img))
    return st;
  const uint32_t lo = row_offsets[0];
  std::vector<uint32_t> local(row_offsets, row_offsets + img->dim_y);
  for (uint32_t& o : local)
    o -= lo;
  const size_t span = in_bytes - lo;
  rsx_samsung_v0_job job;
  one_job_init(job, span, img);
  job.n_offsets = img->dim_y;
  std::vector<uint8_t> key = one_job_key(rsx_samsung_v0_plan_create, job);
  key_append(key, local.data(), local.size());
  job.row_offsets = local.data();
  return single_image_host(ctx, key, rsx_samsung_v0_plan_create, job, in + lo, span, img,
                           row_status);
}

// ---------------------------------------------------------------------------
// FujiDecompressor
// ---------------------------------------------------------------------------
extern "C" int rsx_fuji_parse(const uint8_t* in, size_t in_bytes, rsx_fuji_desc* desc) {
  return rsx_fuji::parse(in, in_bytes, desc);
}

extern "C" int rsx_fuji_validate(const rsx_fuji_desc* desc, const rsx_image* img) {
  return rsx_fuji::validate(desc, img);
}

extern "C" int rsx_fuji_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_fuji_job* jobs,
                                    rsx_plan** out_plan) {
  return decoder_plan_create(ctx, n_jobs, jobs, out_plan, fuji_plan_create);
}

extern "C" int rsx_fuji_plan_strip_status(rsx_plan* plan, int job, int32_t* strip_status) {
  return decoder_plan_get(plan, [&](DecoderPlan* d) {
    return d->row_status(plan->last_stream, job, strip_status);
  });
}

// Device pointers: a plan of the call's own runs on them, on the context's stream behind the null
// stream's work so far, and the call returns when it is done.  Host pointers (single_image_host):
// the bytes from the first strip's up go up as one copy; the plan's key holds the descriptor.
extern "C" int rsx_fuji_decompress(rsx_ctx* ctx, const rsx_fuji_desc* desc, const uint8_t* in,
                                   size_t in_bytes, const rsx_image* img, int32_t* strip_status) {
  if (!ctx || !desc || !in || !img || !img->data)
    return RSX_ERR_INVALID_ARG;
  ++ctx->host_calls;
  if (int st = rsx_fuji::validate(desc, img))
    return st;
  if (int st = rsx_fuji::check_strips(*desc, in_bytes))
    return st;
  if (img->pitch_bytes % 2 != 0)
    return RSX_ERR_INVALID_ARG;
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const bool in_dev = is_device_pointer(in), out_dev = is_device_pointer(img->data);
  if (in_dev != out_dev)
    return RSX_ERR_INVALID_ARG;
  rsx_fuji_job job;
  if (in_dev) {
    one_job_init(job, in_bytes, img);
    job.desc = *desc;
    CallPlan call;
    if (int st = rsx_fuji_plan_create(ctx, 1, &job, &call.plan))
      return st;
    const int rc = call.run(in, img->data, nullptr);
    if (rc == RSX_ERR_DEVICE || rc == RSX_ERR_NOMEM)
      return rc;
    if (strip_status)
      if (int e = call.plan->dec->row_status(call.plan->last_stream, 0, strip_status))
        return e;
    return rc;
  }
  uint64_t lo = desc->strip_offset[0];
  for (int32_t s = 1; s < desc->n_strips; ++s)
    lo = std::min(lo, desc->strip_offset[s]);
  const size_t span = in_bytes - size_t(lo);
  one_job_init(job, span, img);
  job.desc = *desc;
  for (int32_t s = 0; s < desc->n_strips; ++s)
    job.desc.strip_offset[s] -= lo;
  std::vector<uint8_t> key = one_job_key(rsx_fuji_plan_create, job);
  return single_image_host(ctx, key, rsx_fuji_plan_create, job, in + lo, span, img, strip_status);
}

// ---------------------------------------------------------------------------
// OlympusDecompressor
// ---------------------------------------------------------------------------
extern "C" int rsx_olympus_validate(size_t in_bytes, const rsx_image* img) {
  return rsx_olympus::validate(in_bytes, img);
}

extern "C" int rsx_olympus_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_olympus_job* jobs,
                                       rsx_plan** out_plan) {
  return decoder_plan_create(ctx, n_jobs, jobs, out_plan, olympus_plan_create);
}

extern "C" int rsx_olympus_plan_job_status(rsx_plan* plan, int job, int32_t* status) {
  return decoder_plan_get(plan, [&](DecoderPlan* d) {
    return d->row_status(plan->last_stream, job, status);
  });
}

// Device pointers: a plan of the call's own runs on them, on the context's stream behind the null
// stream's work so far, and the call returns when it is done.  Host pointers (single_image_host):
// the whole stream goes up as one copy; the plan is keyed by the geometry and the stream's size.
extern "C" int rsx_olympus_decompress(rsx_ctx* ctx, const uint8_t* in, size_t in_bytes,
                                      const rsx_image* img) {
  if (!ctx || !in || !img || !img->data)
    return RSX_ERR_INVALID_ARG;
  ++ctx->host_calls;
  if (int st = rsx_olympus::validate(in_bytes, img))
    return st;
  if (img->pitch_bytes % 2 != 0)
    return RSX_ERR_INVALID_ARG;
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const bool in_dev = is_device_pointer(in), out_dev = is_device_pointer(img->data);
  if (in_dev != out_dev)
    return RSX_ERR_INVALID_ARG;
  rsx_olympus_job job;
  one_job_init(job, in_bytes, img);
  if (in_dev) {
    CallPlan call;
    if (int st = rsx_olympus_plan_create(ctx, 1, &job, &call.plan))
      return st;
    return call.run(in, img->data, nullptr);
  }
  std::vector<uint8_t> key = one_job_key(rsx_olympus_plan_create, job);
  return single_image_host(ctx, key, rsx_olympus_plan_create, job, in, in_bytes, img, nullptr);
}

// ---------------------------------------------------------------------------
// KodakDecompressor
// ---------------------------------------------------------------------------
extern "C" int rsx_kodak_validate(const rsx_kodak_desc* desc, const rsx_image* img,
                                  size_t in_bytes) {
  return rsx_kodak::validate(desc, img, in_bytes);
}

extern "C" int rsx_kodak_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_kodak_job* jobs,
                                     rsx_plan** out_plan) {
  return decoder_plan_create(ctx, n_jobs, jobs, out_plan, kodak_plan_create);
}

// Device pointers: a plan of the call's own runs on them, on the context's stream behind the null
// stream's work so far, and the call returns when it is done.  Host pointers (single_image_host):
// the bytes the image can consume go up as one copy; the plan is keyed by the geometry, that
// size, the depth and the table mode; the table itself is call data and goes up on every call.
extern "C" int rsx_kodak_decompress(rsx_ctx* ctx, const rsx_kodak_desc* desc, const uint8_t* in,
                                    size_t in_bytes, const rsx_image* img) {
  if (!ctx || !in || !img || !img->data)
    return RSX_ERR_INVALID_ARG;
  ++ctx->host_calls;
  if (int st = rsx_kodak::validate(desc, img, in_bytes))
    return st;
  if (img->pitch_bytes % 2 != 0)
    return RSX_ERR_INVALID_ARG;
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const bool in_dev = is_device_pointer(in), out_dev = is_device_pointer(img->data);
  if (in_dev != out_dev)
    return RSX_ERR_INVALID_ARG;
  const size_t span = size_t(
      std::min<uint64_t>(in_bytes, rsx_kodak::image_bound(img->dim_x, img->dim_y)));
  rsx_kodak_job job;
  one_job_init(job, span, img);
  job.desc.bps = desc->bps;
  job.desc.table_mode = desc->table_mode;
  if (in_dev) {
    job.desc.table = desc->table;
    CallPlan call;
    if (int st = rsx_kodak_plan_create(ctx, 1, &job, &call.plan))
      return st;
    return call.run(in, img->data, nullptr);
  }
  // (desc.table is NULL here: not in the key)
  std::vector<uint8_t> key = one_job_key(rsx_kodak_plan_create, job);
  job.desc.table = desc->table;
  SingleImageHooks hooks;
  hooks.on_reuse = [desc](rsx_plan* plan, hipStream_t s) {
    return kodak_plan_set_table(plan->dec.get(), 0, desc, s);
  };
  return single_image_host(ctx, key, rsx_kodak_plan_create, job, in, span, img, nullptr, hooks);
}

// ---------------------------------------------------------------------------
// CrwDecompressor
// ---------------------------------------------------------------------------
extern "C" int rsx_crw_validate(const rsx_crw_desc* desc, const rsx_image* img, size_t in_bytes,
                                size_t low_bytes) {
  return rsx_crw::validate(desc, img, in_bytes, low_bytes);
}

extern "C" int rsx_crw_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_crw_job* jobs,
                                   rsx_plan** out_plan) {
  return decoder_plan_create(ctx, n_jobs, jobs, out_plan, crw_plan_create);
}

extern "C" int rsx_crw_plan_stats(rsx_plan* plan, int job, uint32_t stats[4]) {
  return decoder_plan_get(plan, [&](DecoderPlan* d) { return crw_plan_stats(d, job, stats); });
}

// Device pointers: a plan of the call's own runs on them (the scan and the low bits are two
// ranges from the lower of the two addresses), on the context's stream behind the null stream's
// work so far, and the call returns when it is done.  Host pointers (single_image_host): the
// bytes the image can consume and the low bits it needs go up as one copy, the low bits behind
// the scan; the plan is keyed by the geometry, those sizes, the table number and the flag.
extern "C" int rsx_crw_decompress(rsx_ctx* ctx, const rsx_crw_desc* desc, const uint8_t* in,
                                  size_t in_bytes, const uint8_t* low, size_t low_bytes,
                                  const rsx_image* img) {
  if (!ctx || !in || !img || !img->data || !desc || (desc->has_lowbits && !low))
    return RSX_ERR_INVALID_ARG;
  ++ctx->host_calls;
  if (int st = rsx_crw::validate(desc, img, in_bytes, low_bytes))
    return st;
  if (img->pitch_bytes % 2 != 0)
    return RSX_ERR_INVALID_ARG;
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const bool with_low = desc->has_lowbits != 0;
  const bool in_dev = is_device_pointer(in), out_dev = is_device_pointer(img->data);
  if (in_dev != out_dev || (with_low && is_device_pointer(low) != in_dev))
    return RSX_ERR_INVALID_ARG;
  const size_t span =
      size_t(std::min<uint64_t>(in_bytes, rsx_crw::image_bound(img->dim_x, img->dim_y)));
  const size_t low_need = with_low ? size_t(img->dim_x) * size_t(img->dim_y) / 4 : 0;
  rsx_crw_job job;
  one_job_init(job, span, img);
  job.desc.dec_table = desc->dec_table;
  job.desc.has_lowbits = with_low ? 1u : 0u;
  job.low_bytes = low_need;
  if (in_dev) {
    const uint8_t* base = with_low && low < in ? low : in;
    job.in_offset = uint64_t(in - base);
    job.low_offset = with_low ? uint64_t(low - base) : 0;
    CallPlan call;
    if (int st = rsx_crw_plan_create(ctx, 1, &job, &call.plan))
      return st;
    return call.run(base, img->data, nullptr);
  }
  job.low_offset = (span + 15) / 16 * 16;
  std::vector<uint8_t> key = one_job_key(rsx_crw_plan_create, job);
  if (!with_low)
    return single_image_host(ctx, key, rsx_crw_plan_create, job, in, span, img, nullptr);
  std::vector<uint8_t> both(size_t(job.low_offset) + low_need);
  std::memcpy(both.data(), in, span);
  std::memcpy(both.data() + job.low_offset, low, low_need);
  return single_image_host(ctx, key, rsx_crw_plan_create, job, both.data(), both.size(), img,
                           nullptr);
}

// ---------------------------------------------------------------------------
// RafDecoder::applyCorrections: the SuperCCD rotation
// ---------------------------------------------------------------------------
extern "C" int rsx_raf_rotate_geometry(const rsx_raf_rotate_desc* desc, int32_t* out_dim_x,
                                        int32_t* out_dim_y, int32_t* rotation_pos) {
  return rsx_fujirot::geometry(desc, out_dim_x, out_dim_y, rotation_pos);
}

extern "C" int rsx_raf_rotate_validate(const rsx_raf_rotate_desc* desc, const rsx_image* src,
                                        const rsx_image* dst) {
  return rsx_fujirot::validate(desc, src, dst);
}

extern "C" int rsx_raf_rotate_plan_create(rsx_ctx* ctx, int n_jobs,
                                           const rsx_raf_rotate_job* jobs, rsx_plan** out_plan) {
  return decoder_plan_create(ctx, n_jobs, jobs, out_plan, fuji_rotate_plan_create);
}

// Device pointers: a plan of the call's own runs on them (the two images are two ranges from the
// lower of the two addresses), on the context's stream behind the null stream's work so far, and
// the call returns when it is done.  Host pointers: the rows of the crop go up as one copy, the
// pass writes a compact image (pitch roundUp(2 R, 16)) on a lane, and that comes back through
// download_rects -- about twice the bytes that went up.
extern "C" int rsx_raf_rotate(rsx_ctx* ctx, const rsx_raf_rotate_desc* desc,
                               const rsx_image* src, const rsx_image* dst) {
  if (!ctx || !desc || !src || !dst)
    return RSX_ERR_INVALID_ARG;
  ++ctx->host_calls;
  if (int st = rsx_fujirot::validate(desc, src, dst))
    return st;
  if (!src->data || !dst->data || reinterpret_cast<uintptr_t>(src->data) % 2 != 0 ||
      reinterpret_cast<uintptr_t>(dst->data) % 2 != 0)
    return RSX_ERR_INVALID_ARG;
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const bool in_dev = is_device_pointer(src->data), out_dev = is_device_pointer(dst->data);
  if (in_dev != out_dev)
    return RSX_ERR_INVALID_ARG;
  rsx_raf_rotate_job job;
  std::memset(&job, 0, sizeof job);
  job.desc = *desc;
  job.in = *src;
  job.img = *dst;
  job.in.data = job.img.data = nullptr;
  if (in_dev) {
    const uint8_t* a = static_cast<const uint8_t*>(src->data);
    uint8_t* b = static_cast<uint8_t*>(dst->data);
    const uint8_t* base = a < b ? a : b;
    job.in_offset = uint64_t(a - base);
    job.img_offset = uint64_t(b - base);
    CallPlan call;
    if (int st = rsx_raf_rotate_plan_create(ctx, 1, &job, &call.plan))
      return st;
    return call.run(base, const_cast<uint8_t*>(base), nullptr);
  }
  // the rows [crop_y, crop_y + size_y) of the source, whole, become the job's image
  job.desc.crop_y = 0;
  job.in.dim_y = desc->size_y;
  job.img.pitch_bytes = uint32_t(align_up(size_t(dst->dim_x) * 2, 16));
  const size_t in_bytes = size_t(rsx_fujirot::image_span(&job.in));
  const size_t out_bytes = size_t(job.img.pitch_bytes) * size_t(dst->dim_y);
  LaneGuard lane(ctx);
  if (!lane.lane)
    return RSX_ERR_DEVICE;
  if (int e = lane.lane->d_in.ensure(in_bytes + 64))
    return e;
  if (int e = lane.lane->d_out.ensure(out_bytes + 64))
    return e;
  hipStream_t s = lane.lane->stream;
  {
    std::lock_guard<std::mutex> up(ctx->upload_mu);
    RSX_HIP_CHECK(ctx, hipMemcpyAsync(lane.lane->d_in.ptr,
                                      static_cast<const uint8_t*>(src->data) +
                                          size_t(desc->crop_y) * src->pitch_bytes,
                                      in_bytes, hipMemcpyHostToDevice, s));
  }
  CallPlan call;
  if (int st = rsx_raf_rotate_plan_create(ctx, 1, &job, &call.plan))
    return st;
  if (int rc = rsx_plan_run(call.plan, lane.lane->d_in.ptr, lane.lane->d_out.ptr, s))
    return rc;
  const DownRect dr{static_cast<uint8_t*>(dst->data), dst->pitch_bytes,
                    static_cast<uint8_t*>(lane.lane->d_out.ptr), job.img.pitch_bytes,
                    size_t(dst->dim_x) * 2, size_t(dst->dim_y)};
  std::lock_guard<std::mutex> down_lock(ctx->download_mu);
  return download_rects(ctx, lane.lane, s, &dr, 1);
}

// ---------------------------------------------------------------------------
// ArwDecoder::SonyDecrypt, ArwDecoder::decodeSRF
// ---------------------------------------------------------------------------
extern "C" int rsx_sony_srf_validate(size_t in_bytes, const rsx_image* img) {
  return rsx_sony_srf::validate(in_bytes, img);
}

extern "C" int rsx_sony_srf_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_sony_srf_job* jobs,
                                        rsx_plan** out_plan) {
  return decoder_plan_create(ctx, n_jobs, jobs, out_plan, sony_srf_plan_create);
}

// Device pointers: a plan of the call's own runs on them, on the context's stream behind the null
// stream's work so far, and the call returns when it is done.  Host pointers: the words go up as
// one copy, are decrypted in place on a lane and come back as one.
extern "C" int rsx_sony_decrypt(rsx_ctx* ctx, const uint8_t* in, uint8_t* out, size_t n_words,
                                uint32_t key) {
  if (!ctx)
    return RSX_ERR_INVALID_ARG;
  ++ctx->host_calls;
  if (n_words == 0)
    return RSX_OK;
  if (!in || !out)
    return RSX_ERR_INVALID_ARG;
  if (uint64_t(n_words) > 0xFFFFFFFFull)
    return RSX_ERR_UNSUPPORTED;
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const bool in_dev = is_device_pointer(in), out_dev = is_device_pointer(out);
  if (in_dev != out_dev)
    return RSX_ERR_INVALID_ARG;
  rsx_sony_srf_job none{};
  CallPlan call;
  if (int st = decoder_plan_create(
          ctx, 1, &none, &call.plan,
          [&](rsx_ctx* c, int, const rsx_sony_srf_job*, std::unique_ptr<DecoderPlan>* o) {
            return sony_decrypt_plan_create(c, n_words, key, o);
          }))
    return st;
  if (in_dev) {
    if (int st = rsx_plan_run(call.plan, in, out, nullptr))
      return st;
    return rsx_plan_results(call.plan, nullptr, nullptr);
  }
  const size_t bytes = n_words * 4;
  LaneGuard lane(ctx);
  if (!lane.lane)
    return RSX_ERR_DEVICE;
  if (int e = lane.lane->d_out.ensure(bytes + 64))
    return e;
  hipStream_t s = lane.lane->stream;
  {
    std::lock_guard<std::mutex> up(ctx->upload_mu);
    RSX_HIP_CHECK(ctx, hipMemcpyAsync(lane.lane->d_out.ptr, in, bytes, hipMemcpyHostToDevice, s));
  }
  if (int rc = rsx_plan_run(call.plan, lane.lane->d_out.ptr, lane.lane->d_out.ptr, s))
    return rc;
  // (download_rects stages what is off the 16-byte grid row by row: rows of 64 KiB, then the rest)
  const uint8_t* dev = static_cast<const uint8_t*>(lane.lane->d_out.ptr);
  constexpr size_t ROW = size_t(64) << 10;
  const size_t rows = bytes / ROW;
  const DownRect body{out, ROW, dev, ROW, ROW, rows};
  const DownRect rest{out + rows * ROW, 0, dev + rows * ROW, 0, bytes - rows * ROW, 1};
  std::lock_guard<std::mutex> down_lock(ctx->download_mu);
  if (int e = download_rects(ctx, lane.lane, s, &body, 1))
    return e;
  return download_rects(ctx, lane.lane, s, &rest, 1);
}

// Device pointers: as above.  Host pointers (single_image_host): the 2 dim_x dim_y bytes go up as
// one copy; the plan is keyed by the geometry and the key, whose table it holds.
extern "C" int rsx_sony_srf_decompress(rsx_ctx* ctx, const uint8_t* in, size_t in_bytes,
                                       uint32_t key, const rsx_image* img) {
  if (!ctx || !in || !img || !img->data)
    return RSX_ERR_INVALID_ARG;
  ++ctx->host_calls;
  if (int st = rsx_sony_srf::validate(in_bytes, img))
    return st;
  if (reinterpret_cast<uintptr_t>(img->data) % 2 != 0)
    return RSX_ERR_INVALID_ARG;
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const bool in_dev = is_device_pointer(in), out_dev = is_device_pointer(img->data);
  if (in_dev != out_dev)
    return RSX_ERR_INVALID_ARG;
  const size_t span = 2 * size_t(img->dim_x) * size_t(img->dim_y);
  rsx_sony_srf_job job;
  one_job_init(job, span, img);
  job.key = key;
  if (in_dev) {
    CallPlan call;
    if (int st = rsx_sony_srf_plan_create(ctx, 1, &job, &call.plan))
      return st;
    return call.run(in, img->data, nullptr);
  }
  std::vector<uint8_t> plan_key = one_job_key(rsx_sony_srf_plan_create, job);
  return single_image_host(ctx, plan_key, rsx_sony_srf_plan_create, job, in, span, img, nullptr);
}

// ---------------------------------------------------------------------------
// rstest's imgDataHash, rawspeed-identify's sums
// ---------------------------------------------------------------------------
extern "C" int rsx_image_hash_validate(const rsx_image* img, int32_t sample_bytes) {
  return rsx_imghash::validate(img, sample_bytes);
}

extern "C" int rsx_image_hash_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_image_hash_job* jobs,
                                          rsx_plan** out_plan) {
  return decoder_plan_create(ctx, n_jobs, jobs, out_plan, image_hash_plan_create);
}

// A plan of one job whose outputs are one block of 16 dim_y + 32 bytes: the digests, the result
// behind them.  A device pointer: the plan runs on the image where it lies, on the context's
// stream behind the null stream's work so far, and the block alone comes back.  A host pointer:
// the rows go up as one copy into a lane.
extern "C" int rsx_image_hash(rsx_ctx* ctx, const rsx_image* img, int32_t sample_bytes,
                              uint8_t* line_md5, rsx_image_hash_result* out) {
  if (!ctx || !img || !img->data || !out)
    return RSX_ERR_INVALID_ARG;
  ++ctx->host_calls;
  if (int st = rsx_imghash::validate(img, sample_bytes))
    return st;
  if (reinterpret_cast<uintptr_t>(img->data) % uintptr_t(sample_bytes) != 0)
    return RSX_ERR_INVALID_ARG;
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const size_t lines_bytes = size_t(img->dim_y) * 16;
  const size_t back_bytes = lines_bytes + sizeof(rsx_image_hash_result);
  rsx_image_hash_job job;
  std::memset(&job, 0, sizeof job);
  job.result_offset = lines_bytes;
  job.sample_bytes = sample_bytes;
  job.img = *img;
  job.img.data = nullptr;
  CallPlan call;
  if (int st = rsx_image_hash_plan_create(ctx, 1, &job, &call.plan))
    return st;
  std::vector<uint8_t> back(back_bytes);
  if (is_device_pointer(img->data)) {
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    DeviceBuffer d_back;
    if (int e = d_back.ensure(back_bytes + 16))
      return e;
    if (int st = rsx_plan_run(call.plan, img->data, d_back.ptr, nullptr))
      return st;
    RSX_HIP_CHECK(ctx, hipMemcpyAsync(back.data(), d_back.ptr, back_bytes, hipMemcpyDeviceToHost,
                                      ctx->stream));
    if (int st = rsx_plan_results(call.plan, nullptr, nullptr)) // (waits for the stream)
      return st;
  } else {
    LaneGuard lane(ctx);
    if (!lane.lane)
      return RSX_ERR_DEVICE;
    rsx_ctx::HostLane* L = lane.lane;
    const size_t row_bytes = size_t(img->dim_x) * size_t(img->cpp) * size_t(sample_bytes);
    const size_t bytes = size_t(img->pitch_bytes) * size_t(img->dim_y - 1) + row_bytes;
    if (int e = L->d_in.ensure(bytes + 64))
      return e;
    if (int e = L->d_out.ensure(back_bytes + 64))
      return e;
    {
      std::lock_guard<std::mutex> up(ctx->upload_mu);
      RSX_HIP_CHECK(ctx, hipMemcpyAsync(L->d_in.ptr, img->data, bytes, hipMemcpyHostToDevice,
                                        L->stream));
    }
    if (int st = rsx_plan_run(call.plan, L->d_in.ptr, L->d_out.ptr, L->stream))
      return st;
    const DownRect dr{back.data(), 0, static_cast<const uint8_t*>(L->d_out.ptr), 0, back_bytes, 1};
    std::lock_guard<std::mutex> down_lock(ctx->download_mu);
    if (int e = download_rects(ctx, L, L->stream, &dr, 1))
      return e;
  }
  if (line_md5)
    std::memcpy(line_md5, back.data(), lines_bytes);
  std::memcpy(out, back.data() + lines_bytes, sizeof *out);
  return RSX_OK;
}

// ---------------------------------------------------------------------------
// Writers: BitVacuumer{LSB,MSB,MSB16,MSB32,JPEG}, PrefixCodeVectorEncoder (rsx.h section 7)
// ---------------------------------------------------------------------------
extern "C" int rsx_encode_pack_validate(const rsx_unpack_desc* d, const rsx_image* img,
                                        size_t out_cap) {
  return rsx_encode::validate_pack(d, img, out_cap);
}

extern "C" int rsx_encode_pack_plan_create(rsx_ctx* ctx, int n_jobs,
                                           const rsx_encode_pack_job* jobs, rsx_plan** out_plan) {
  return decoder_plan_create(ctx, n_jobs, jobs, out_plan, encode_pack_plan_create);
}

namespace {
// Both device pointers or both host pointers (`*dev` says which); RSX_ERR_INVALID_ARG for a mix.
int same_side(const void* a, const void* b, bool* dev) {
  const bool da = is_device_pointer(a), db = is_device_pointer(b);
  *dev = da;
  return da == db ? RSX_OK : RSX_ERR_INVALID_ARG;
}

// The base a plan of one job runs on when its image and its output are two device pointers: the
// lower of the two on the samples' grid, and the offsets of both from it.
const uint8_t* device_base(const void* img, const void* out, uint64_t* img_off, uint64_t* out_off) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(img), b = reinterpret_cast<uintptr_t>(out);
  const uintptr_t base = (a < b ? a : b) & ~uintptr_t(1);
  *img_off = a - base;
  *out_off = b - base;
  return reinterpret_cast<const uint8_t*>(base);
}

// Rows [y0, y0 + rows) of the caller's image, whole, into the lane's input buffer as one copy.
int upload_rows(rsx_ctx* ctx, rsx_ctx::HostLane* L, const rsx_image* img, int32_t y0, int32_t rows) {
  const size_t bytes = size_t(img->pitch_bytes) * size_t(rows - 1) +
                       size_t(img->dim_x) * size_t(img->cpp) * 2;
  if (int e = L->d_in.ensure(bytes + 64))
    return e;
  std::lock_guard<std::mutex> up(ctx->upload_mu);
  RSX_HIP_CHECK(ctx, hipMemcpyAsync(L->d_in.ptr,
                                    static_cast<const uint8_t*>(img->data) +
                                        size_t(y0) * img->pitch_bytes,
                                    bytes, hipMemcpyHostToDevice, L->stream));
  return RSX_OK;
}

int download_bytes(rsx_ctx* ctx, rsx_ctx::HostLane* L, uint8_t* out, size_t bytes) {
  if (bytes == 0)
    return RSX_OK;
  const DownRect dr{out, 0, static_cast<const uint8_t*>(L->d_out.ptr), 0, bytes, 1};
  std::lock_guard<std::mutex> down_lock(ctx->download_mu);
  return download_rects(ctx, L, L->stream, &dr, 1);
}
} // namespace

// Device pointers: a plan of one job runs on them where they lie, on the context's stream behind
// the null stream's work so far, and the call returns when it is done.  Host pointers: the rows
// crop_y .. go up as one copy into a lane and the stream comes back as one.
extern "C" int rsx_encode_pack_u16(rsx_ctx* ctx, const rsx_unpack_desc* d, const rsx_image* img,
                                   uint8_t* out, size_t out_cap, rsx_encode_pack_result* bytes) {
  if (bytes)
    std::memset(bytes, 0, sizeof *bytes);
  if (!ctx || !d || !img || !img->data || !out || !bytes)
    return RSX_ERR_INVALID_ARG;
  ++ctx->host_calls;
  if (int st = rsx_encode::validate_pack(d, img, out_cap))
    return st;
  if (reinterpret_cast<uintptr_t>(img->data) % 2 != 0)
    return RSX_ERR_INVALID_ARG;
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  bool dev = false;
  if (int st = same_side(img->data, out, &dev))
    return st;
  rsx_encode_pack_job job;
  std::memset(&job, 0, sizeof job);
  job.desc = *d;
  job.img = *img;
  job.img.data = nullptr;
  job.out_cap = out_cap;
  const uint64_t stream_bytes = uint64_t(d->crop_h) * uint64_t(d->input_pitch_bytes);
  const uint64_t written = rsx_encode::round_up4(stream_bytes);
  CallPlan call;
  if (dev) {
    const uint8_t* base = device_base(img->data, out, &job.img_offset, &job.out_offset);
    if (int st = rsx_encode_pack_plan_create(ctx, 1, &job, &call.plan))
      return st;
    if (int st = call.run(base, const_cast<uint8_t*>(base), nullptr))
      return st;
  } else {
    job.desc.crop_y = 0;
    job.img.dim_y = d->crop_h;
    if (int st = rsx_encode_pack_plan_create(ctx, 1, &job, &call.plan))
      return st;
    LaneGuard lane(ctx);
    if (!lane.lane)
      return RSX_ERR_DEVICE;
    if (int e = upload_rows(ctx, lane.lane, img, d->crop_y, d->crop_h))
      return e;
    if (int e = lane.lane->d_out.ensure(size_t(written) + 64))
      return e;
    if (int st = rsx_plan_run(call.plan, lane.lane->d_in.ptr, lane.lane->d_out.ptr, lane.lane->stream))
      return st;
    if (int e = download_bytes(ctx, lane.lane, out, size_t(written)))
      return e;
  }
  bytes->bytes_written = written;
  bytes->stream_bytes = stream_bytes;
  return RSX_OK;
}

extern "C" int rsx_encode_ljpeg_validate(const rsx_ljpeg_desc* d, const rsx_image* img) {
  if (!d || !img)
    return RSX_ERR_INVALID_ARG;
  if (int st = validate_ljpeg(*d, *img))
    return st;
  return rsx_encode::validate_ljpeg_subset(*d, *img);
}

extern "C" uint64_t rsx_encode_ljpeg_bound(const rsx_ljpeg_desc* d, const rsx_image* img) {
  if (rsx_encode_ljpeg_validate(d, img) != RSX_OK)
    return 0;
  rsx_encode::LJpegGeom g;
  rsx_encode::ljpeg_geom(*d, *img, 0, 0, 0, 0, &g);
  return rsx_encode::ljpeg_bound(g);
}

extern "C" int rsx_encode_ljpeg_plan_create(rsx_ctx* ctx, int n_jobs,
                                            const rsx_encode_ljpeg_job* jobs, rsx_plan** out_plan) {
  return decoder_plan_create(ctx, n_jobs, jobs, out_plan, encode_ljpeg_plan_create);
}

extern "C" int rsx_encode_ljpeg_plan_result(rsx_plan* plan, int job, rsx_encode_result* out) {
  return decoder_plan_get(plan, [&](DecoderPlan* d) { return d->encode_result(job, out); });
}

// Device pointers: as above, and only the result comes back.  Host pointers: the tile's rows go up
// as one copy into a lane; the stream is written there (into at most the bound's bytes) and the
// bytes the result counts come back.
extern "C" int rsx_encode_ljpeg(rsx_ctx* ctx, const rsx_ljpeg_desc* d, const rsx_image* img,
                                uint32_t flags, uint8_t* out, size_t out_cap,
                                rsx_encode_result* result) {
  if (result)
    std::memset(result, 0, sizeof *result);
  if (!ctx || !d || !img || !img->data || !out || !result || flags > RSX_ENCODE_TAIL_VACUUMER)
    return RSX_ERR_INVALID_ARG;
  ++ctx->host_calls;
  if (int st = rsx_encode_ljpeg_validate(d, img))
    return result->status = st;
  if (reinterpret_cast<uintptr_t>(img->data) % 2 != 0)
    return RSX_ERR_INVALID_ARG;
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  bool dev = false;
  if (int st = same_side(img->data, out, &dev))
    return st;
  rsx_encode_ljpeg_job job;
  std::memset(&job, 0, sizeof job);
  job.desc = *d;
  job.flags = flags;
  job.img = *img;
  job.img.data = nullptr;
  job.out_cap = out_cap;
  CallPlan call;
  if (dev) {
    const uint8_t* base = device_base(img->data, out, &job.img_offset, &job.out_offset);
    if (int st = rsx_encode_ljpeg_plan_create(ctx, 1, &job, &call.plan))
      return st;
    if (int st = rsx_plan_run(call.plan, base, const_cast<uint8_t*>(base), nullptr))
      return st;
    rsx_plan_results(call.plan, nullptr, nullptr);
    if (int st = rsx_encode_ljpeg_plan_result(call.plan, 0, result))
      return st;
    return result->status;
  }
  job.desc.tile_y = 0;
  job.img.dim_y = d->tile_h;
  const uint64_t bound = rsx_encode_ljpeg_bound(d, img);
  const size_t room = size_t(uint64_t(out_cap) < bound ? uint64_t(out_cap) : bound);
  job.out_cap = room;
  if (int st = rsx_encode_ljpeg_plan_create(ctx, 1, &job, &call.plan))
    return st;
  LaneGuard lane(ctx);
  if (!lane.lane)
    return RSX_ERR_DEVICE;
  if (int e = upload_rows(ctx, lane.lane, img, d->tile_y, d->tile_h))
    return e;
  if (int e = lane.lane->d_out.ensure(room + 64))
    return e;
  if (int st = rsx_plan_run(call.plan, lane.lane->d_in.ptr, lane.lane->d_out.ptr, lane.lane->stream))
    return st;
  rsx_plan_results(call.plan, nullptr, nullptr);
  if (int st = rsx_encode_ljpeg_plan_result(call.plan, 0, result))
    return st;
  if (result->status == RSX_OK)
    if (int e = download_bytes(ctx, lane.lane, out, size_t(result->bytes)))
      return e;
  return result->status;
}

extern "C" int rsx_encode_ljpeg_container(const rsx_ljpeg_desc* d, const rsx_image* img,
                                          int32_t precision, uint64_t entropy_bytes,
                                          uint8_t* hdr_out, size_t hdr_cap, size_t* hdr_bytes) {
  (void)entropy_bytes; // (no field of the layout holds the scan's length)
  if (!hdr_out || !hdr_bytes || precision < 2 || precision > 16)
    return RSX_ERR_INVALID_ARG;
  if (int st = rsx_encode_ljpeg_validate(d, img))
    return st;
  const bool markers = d->rows_per_restart_interval < d->tile_h;
  if (d->frame_w > 0xFFFF || d->frame_h > 0xFFFF ||
      (markers && int64_t(d->rows_per_restart_interval) * d->frame_w > 0xFFFF))
    return RSX_ERR_INVALID_ARG;
  *hdr_bytes = rsx_encode::ljpeg_container(*d, precision, hdr_out, hdr_cap);
  return *hdr_bytes ? RSX_OK : RSX_ERR_INVALID_ARG;
}

extern "C" int rsx_encode_huff_from_histogram(const uint64_t* counts, uint32_t flags,
                                              rsx_huff_table* out) {
  if (!counts || !out || (flags & ~uint32_t(RSX_ENCODE_TABLE_ALL_CATEGORIES)))
    return RSX_ERR_INVALID_ARG;
  return rsx_encode::huff_from_histogram(counts, (flags & RSX_ENCODE_TABLE_ALL_CATEGORIES) != 0, out);
}

// A histogram plan of one job whose output is the 4 x 17 counts.  A device pointer: the plan runs
// on the image where it lies and the counts alone come back.  A host pointer: the tile's rows go
// up as one copy into a lane.
extern "C" int rsx_encode_ljpeg_histogram(rsx_ctx* ctx, const rsx_ljpeg_desc* d,
                                          const rsx_image* img, uint64_t* counts) {
  if (!ctx || !d || !img || !img->data || !counts)
    return RSX_ERR_INVALID_ARG;
  ++ctx->host_calls;
  if (int st = rsx_encode_ljpeg_validate(d, img))
    return st;
  if (reinterpret_cast<uintptr_t>(img->data) % 2 != 0)
    return RSX_ERR_INVALID_ARG;
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  constexpr size_t BYTES = 4 * rsx_encode::N_CATEGORIES * sizeof(uint64_t);
  rsx_encode_ljpeg_job job;
  std::memset(&job, 0, sizeof job);
  job.desc = *d;
  job.img = *img;
  job.img.data = nullptr;
  job.out_cap = BYTES;
  const bool dev = is_device_pointer(img->data);
  if (!dev) {
    job.desc.tile_y = 0;
    job.img.dim_y = d->tile_h;
  }
  CallPlan call;
  if (int st = decoder_plan_create(ctx, 1, &job, &call.plan, encode_histogram_plan_create))
    return st;
  if (dev) {
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    DeviceBuffer d_back;
    if (int e = d_back.ensure(BYTES + 16))
      return e;
    if (int st = rsx_plan_run(call.plan, img->data, d_back.ptr, nullptr))
      return st;
    RSX_HIP_CHECK(ctx, hipMemcpyAsync(counts, d_back.ptr, BYTES, hipMemcpyDeviceToHost, ctx->stream));
    return rsx_plan_results(call.plan, nullptr, nullptr); // (waits for the stream)
  }
  LaneGuard lane(ctx);
  if (!lane.lane)
    return RSX_ERR_DEVICE;
  if (int e = upload_rows(ctx, lane.lane, img, d->tile_y, d->tile_h))
    return e;
  if (int e = lane.lane->d_out.ensure(BYTES + 64))
    return e;
  if (int st = rsx_plan_run(call.plan, lane.lane->d_in.ptr, lane.lane->d_out.ptr, lane.lane->stream))
    return st;
  return download_bytes(ctx, lane.lane, reinterpret_cast<uint8_t*>(counts), BYTES);
}

// ---------------------------------------------------------------------------
// Writers of F32 images: exact narrowing, packed strips, the width of windows (rsx.h section 7d)
// ---------------------------------------------------------------------------
extern "C" int rsx_fpwrite_pack_validate(const rsx_unpack_desc* d, const rsx_image* img,
                                         size_t out_cap) {
  return rsx_fpwrite::validate_pack(d, img, out_cap);
}

extern "C" int rsx_fpwrite_pack_plan_create(rsx_ctx* ctx, int n_jobs,
                                            const rsx_fpwrite_pack_job* jobs, rsx_plan** out_plan) {
  return decoder_plan_create(ctx, n_jobs, jobs, out_plan, fpwrite_pack_plan_create);
}

extern "C" int rsx_fpwrite_pack_plan_result(rsx_plan* plan, int job, rsx_fpwrite_pack_result* out) {
  return decoder_plan_get(plan, [&](DecoderPlan* d) { return d->fpwrite_pack_result(job, out); });
}

// As rsx_encode_pack_u16: device pointers run in place on the context's stream, host pointers go
// through a lane.  The stream comes back only when every sample had its narrow pattern.
extern "C" int rsx_fpwrite_pack(rsx_ctx* ctx, const rsx_unpack_desc* d, const rsx_image* img,
                                uint8_t* out, size_t out_cap, rsx_fpwrite_pack_result* result) {
  if (result)
    std::memset(result, 0, sizeof *result);
  if (!ctx || !d || !img || !img->data || !out || !result)
    return RSX_ERR_INVALID_ARG;
  ++ctx->host_calls;
  if (int st = rsx_fpwrite::validate_pack(d, img, out_cap))
    return st;
  if (reinterpret_cast<uintptr_t>(img->data) % 4 != 0)
    return RSX_ERR_INVALID_ARG;
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  bool dev = false;
  if (int st = same_side(img->data, out, &dev))
    return st;
  rsx_fpwrite_pack_job job;
  std::memset(&job, 0, sizeof job);
  job.desc = *d;
  job.img = *img;
  job.img.data = nullptr;
  job.out_cap = out_cap;
  CallPlan call;
  if (dev) {
    // the lower of the two pointers on the samples' grid, and the offsets of both from it
    const uintptr_t a = reinterpret_cast<uintptr_t>(img->data), b = reinterpret_cast<uintptr_t>(out);
    const uintptr_t base = (a < b ? a : b) & ~uintptr_t(3);
    job.img_offset = a - base;
    job.out_offset = b - base;
    if (int st = rsx_fpwrite_pack_plan_create(ctx, 1, &job, &call.plan))
      return st;
    if (int st = rsx_plan_run(call.plan, reinterpret_cast<const void*>(base),
                              reinterpret_cast<void*>(base), nullptr))
      return st;
    (void)rsx_plan_results(call.plan, nullptr, nullptr); // (waits; the status follows)
    return rsx_fpwrite_pack_plan_result(call.plan, 0, result);
  }
  job.desc.crop_y = 0;
  job.img.dim_y = d->crop_h;
  if (int st = rsx_fpwrite_pack_plan_create(ctx, 1, &job, &call.plan))
    return st;
  LaneGuard lane(ctx);
  if (!lane.lane)
    return RSX_ERR_DEVICE;
  rsx_ctx::HostLane* L = lane.lane;
  const size_t row_bytes = size_t(img->dim_x) * size_t(img->cpp) * 4;
  const size_t up_bytes = size_t(img->pitch_bytes) * size_t(d->crop_h - 1) + row_bytes;
  const size_t written = size_t(rsx_fpwrite::round_up4(uint64_t(d->crop_h) * uint64_t(d->input_pitch_bytes)));
  if (int e = L->d_in.ensure(up_bytes + 64))
    return e;
  if (int e = L->d_out.ensure(written + 64))
    return e;
  {
    std::lock_guard<std::mutex> up(ctx->upload_mu);
    RSX_HIP_CHECK(ctx, hipMemcpyAsync(L->d_in.ptr,
                                      static_cast<const uint8_t*>(img->data) +
                                          size_t(d->crop_y) * img->pitch_bytes,
                                      up_bytes, hipMemcpyHostToDevice, L->stream));
  }
  if (int st = rsx_plan_run(call.plan, L->d_in.ptr, L->d_out.ptr, L->stream))
    return st;
  (void)rsx_plan_results(call.plan, nullptr, nullptr);
  const int st = rsx_fpwrite_pack_plan_result(call.plan, 0, result);
  if (st != RSX_OK)
    return st;
  return download_bytes(ctx, L, out, written);
}

extern "C" int rsx_fpwrite_deflate_validate(const rsx_dng_deflate_desc* desc,
                                            const rsx_fpwrite_deflate_tile* t, const rsx_image* img) {
  if (!desc || !t || !img)
    return RSX_ERR_INVALID_ARG;
  return fpwrite_deflate_validate(*desc, t->tile_w, t->tile_h, t->off_x, t->off_y, t->width, t->height,
                                  *img);
}

extern "C" uint64_t rsx_fpwrite_deflate_bound(const rsx_dng_deflate_desc* desc,
                                              const rsx_fpwrite_deflate_tile* t,
                                              const rsx_image* img) {
  if (rsx_fpwrite_deflate_validate(desc, t, img) != RSX_OK)
    return 0;
  return rsx_deflate::bound_of(uint64_t(desc->bps / 8) * t->tile_w * t->tile_h);
}

extern "C" int rsx_fpwrite_deflate_plan_create(rsx_ctx* ctx, int n_jobs,
                                               const rsx_fpwrite_deflate_job* jobs,
                                               rsx_plan** out_plan) {
  return decoder_plan_create(ctx, n_jobs, jobs, out_plan, fpwrite_deflate_plan_create);
}

extern "C" int rsx_fpwrite_deflate_plan_result(rsx_plan* plan, int job,
                                               rsx_fpwrite_deflate_result* out) {
  return decoder_plan_get(plan, [&](DecoderPlan* d) { return d->fpwrite_deflate_result(job, out); });
}

// The tiles of one image as the jobs of one plan.  Device pointers: the plan runs on the lowest of
// them, on the context's stream behind the null stream's work so far.  Host pointers: the image
// goes up as one copy into a lane, the streams lie one behind the other in the lane's output (each
// in room for the lesser of its out_cap and its bound) and come back as one copy.
extern "C" int rsx_fpwrite_deflate(rsx_ctx* ctx, const rsx_dng_deflate_desc* desc, int n_tiles,
                                   const rsx_fpwrite_deflate_tile* tiles, const rsx_image* img,
                                   rsx_fpwrite_deflate_result* results) {
  if (!ctx || !desc || !tiles || n_tiles < 1 || !img || !img->data || !results)
    return RSX_ERR_INVALID_ARG;
  ++ctx->host_calls;
  std::memset(results, 0, sizeof *results * size_t(n_tiles));
  if (reinterpret_cast<uintptr_t>(img->data) % 4 != 0)
    return RSX_ERR_INVALID_ARG;
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const bool dev = is_device_pointer(img->data);
  uintptr_t base = reinterpret_cast<uintptr_t>(img->data);
  for (int i = 0; i < n_tiles; ++i) {
    if (!tiles[i].out || is_device_pointer(tiles[i].out) != dev)
      return RSX_ERR_INVALID_ARG;
    base = std::min(base, reinterpret_cast<uintptr_t>(tiles[i].out));
  }
  base &= ~uintptr_t(3);
  std::vector<rsx_fpwrite_deflate_job> jobs(static_cast<size_t>(n_tiles));
  std::vector<uint64_t> room(static_cast<size_t>(n_tiles), 0);
  uint64_t staged = 0;
  for (int i = 0; i < n_tiles; ++i) {
    const rsx_fpwrite_deflate_tile& t = tiles[i];
    rsx_fpwrite_deflate_job& j = jobs[i];
    std::memset(&j, 0, sizeof j);
    j.desc = *desc;
    j.tile_w = t.tile_w, j.tile_h = t.tile_h, j.off_x = t.off_x, j.off_y = t.off_y;
    j.width = t.width, j.height = t.height;
    j.out_cap = t.out_cap;
    j.img = *img;
    j.img.data = nullptr;
    if (dev) {
      j.img_offset = reinterpret_cast<uintptr_t>(img->data) - base;
      j.out_offset = reinterpret_cast<uintptr_t>(t.out) - base;
    } else {
      room[i] = std::min<uint64_t>(t.out_cap, rsx_fpwrite_deflate_bound(desc, &t, img));
      j.out_offset = staged;
      staged += (room[i] + 15u) & ~uint64_t(15);
    }
  }
  CallPlan call;
  if (int st = rsx_fpwrite_deflate_plan_create(ctx, n_tiles, jobs.data(), &call.plan))
    return st;
  auto collect = [&]() {
    int rc = RSX_OK;
    for (int i = 0; i < n_tiles; ++i)
      if (rsx_fpwrite_deflate_plan_result(call.plan, i, &results[i]) != RSX_OK)
        rc = RSX_ERR_TILE_ERRORS;
    return rc;
  };
  if (dev) {
    if (int st = rsx_plan_run(call.plan, reinterpret_cast<const void*>(base),
                              reinterpret_cast<void*>(base), nullptr))
      return st;
    (void)rsx_plan_results(call.plan, nullptr, nullptr); // (waits; the tiles' statuses follow)
    return collect();
  }
  LaneGuard lane(ctx);
  if (!lane.lane)
    return RSX_ERR_DEVICE;
  rsx_ctx::HostLane* L = lane.lane;
  const size_t up_bytes = size_t(img->pitch_bytes) * size_t(img->dim_y > 0 ? img->dim_y - 1 : 0) +
                          size_t(img->dim_x > 0 ? img->dim_x : 0) * size_t(img->cpp > 0 ? img->cpp : 0) * 4;
  if (int e = L->d_in.ensure(up_bytes + 64))
    return e;
  if (int e = L->d_out.ensure(size_t(staged) + 64))
    return e;
  {
    std::lock_guard<std::mutex> up(ctx->upload_mu);
    RSX_HIP_CHECK(ctx, hipMemcpyAsync(L->d_in.ptr, img->data, up_bytes, hipMemcpyHostToDevice,
                                      L->stream));
  }
  if (int st = rsx_plan_run(call.plan, L->d_in.ptr, L->d_out.ptr, L->stream))
    return st;
  (void)rsx_plan_results(call.plan, nullptr, nullptr);
  const int rc = collect();
  std::vector<uint8_t> back(static_cast<size_t>(staged));
  if (int e = download_bytes(ctx, L, back.data(), back.size()))
    return e;
  for (int i = 0; i < n_tiles; ++i)
    if (results[i].status == RSX_OK)
      std::memcpy(tiles[i].out, back.data() + jobs[i].out_offset, size_t(results[i].bytes));
  return rc;
}

extern "C" int rsx_fpwrite_fit(rsx_ctx* ctx, const rsx_image* img, int n_windows,
                               const rsx_fpwrite_window* windows, int32_t* min_bps_out) {
  if (!ctx || !img || !img->data || !windows || !min_bps_out)
    return RSX_ERR_INVALID_ARG;
  ++ctx->host_calls;
  if (int st = rsx_fpwrite::validate_fit(img, n_windows, windows))
    return st;
  if (reinterpret_cast<uintptr_t>(img->data) % 4 != 0)
    return RSX_ERR_INVALID_ARG;
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  FpFitJob job{*img, n_windows, windows};
  job.img.data = nullptr;
  CallPlan call;
  if (int st = decoder_plan_create(ctx, 1, &job, &call.plan, fpwrite_fit_plan_create))
    return st;
  const size_t back_bytes = size_t(n_windows) * 4;
  std::vector<uint32_t> cls(static_cast<size_t>(n_windows), 0u);
  if (is_device_pointer(img->data)) {
    // the words come back through a lane's output buffer (kept between calls: nothing is allocated
    // or freed here); the run itself is on the context's stream, behind the null stream's work
    LaneGuard lane(ctx);
    if (!lane.lane)
      return RSX_ERR_DEVICE;
    if (int e = lane.lane->d_out.ensure(back_bytes + 64))
      return e;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    if (int st = rsx_plan_run(call.plan, img->data, lane.lane->d_out.ptr, nullptr))
      return st;
    RSX_HIP_CHECK(ctx, hipMemcpyAsync(cls.data(), lane.lane->d_out.ptr, back_bytes,
                                      hipMemcpyDeviceToHost, ctx->stream));
    if (int st = rsx_plan_results(call.plan, nullptr, nullptr)) // (waits for the stream)
      return st;
  } else {
    LaneGuard lane(ctx);
    if (!lane.lane)
      return RSX_ERR_DEVICE;
    rsx_ctx::HostLane* L = lane.lane;
    const size_t bytes = size_t(img->pitch_bytes) * size_t(img->dim_y - 1) +
                         size_t(img->dim_x) * size_t(img->cpp) * 4;
    if (int e = L->d_in.ensure(bytes + 64))
      return e;
    if (int e = L->d_out.ensure(back_bytes + 64))
      return e;
    {
      std::lock_guard<std::mutex> up(ctx->upload_mu);
      RSX_HIP_CHECK(ctx, hipMemcpyAsync(L->d_in.ptr, img->data, bytes, hipMemcpyHostToDevice,
                                        L->stream));
    }
    if (int st = rsx_plan_run(call.plan, L->d_in.ptr, L->d_out.ptr, L->stream))
      return st;
    if (int e = download_bytes(ctx, L, reinterpret_cast<uint8_t*>(cls.data()), back_bytes))
      return e;
  }
  for (int i = 0; i < n_windows; ++i)
    min_bps_out[i] = rsx_fpwrite::fit_bps_of_class(cls[i]);
  return RSX_OK;
}

extern "C" int rsx_dctwrite_quality_tables(int quality, uint16_t* luma, uint16_t* chroma) {
  return rsx_dctw::quality_tables(quality, luma, chroma);
}

extern "C" int rsx_dctwrite_validate(const rsx_dctwrite_desc* desc, const rsx_image* img) {
  return rsx_dctw::validate(desc, img);
}

extern "C" uint64_t rsx_dctwrite_bound(const rsx_dctwrite_desc* desc, const rsx_image* img) {
  if (rsx_dctw::validate(desc, img) != RSX_OK)
    return 0;
  rsx_dctw::Geom g;
  rsx_dctw::geom_of(*desc, *img, 0, 0, 0, &g);
  return rsx_dctw::bound_of(g);
}

extern "C" int rsx_dctwrite_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_dctwrite_job* jobs,
                                        rsx_plan** out_plan) {
  return decoder_plan_create(ctx, n_jobs, jobs, out_plan, dctwrite_plan_create);
}

extern "C" int rsx_dctwrite_plan_result(rsx_plan* plan, int job, rsx_dctwrite_result* out) {
  return decoder_plan_get(plan, [&](DecoderPlan* d) { return d->dctwrite_result(job, out); });
}

// The tiles of one image as the jobs of one plan.  Device pointers: the plan runs on the lowest of
// them, on the context's stream behind the null stream's work so far.  Host pointers: the image
// goes up as one copy into a lane, the streams lie one behind the other in the lane's output (each
// in room for the lesser of its out_cap and its bound) and come back as one copy.
extern "C" int rsx_dctwrite(rsx_ctx* ctx, int n_tiles, const rsx_dctwrite_tile* tiles,
                            const rsx_image* img, rsx_dctwrite_result* results) {
  if (!ctx || !tiles || n_tiles < 1 || !img || !img->data || !results)
    return RSX_ERR_INVALID_ARG;
  ++ctx->host_calls;
  std::memset(results, 0, sizeof *results * size_t(n_tiles));
  if (reinterpret_cast<uintptr_t>(img->data) % 2 != 0)
    return RSX_ERR_INVALID_ARG;
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const bool dev = is_device_pointer(img->data);
  uintptr_t base = reinterpret_cast<uintptr_t>(img->data);
  for (int i = 0; i < n_tiles; ++i) {
    if (!tiles[i].out || is_device_pointer(tiles[i].out) != dev)
      return RSX_ERR_INVALID_ARG;
    base = std::min(base, reinterpret_cast<uintptr_t>(tiles[i].out));
  }
  base &= ~uintptr_t(1);
  std::vector<rsx_dctwrite_job> jobs(static_cast<size_t>(n_tiles));
  uint64_t staged = 0;
  for (int i = 0; i < n_tiles; ++i) {
    const rsx_dctwrite_tile& t = tiles[i];
    rsx_dctwrite_job& j = jobs[i];
    std::memset(&j, 0, sizeof j);
    j.desc = t.desc;
    j.out_cap = t.out_cap;
    j.img = *img;
    j.img.data = nullptr;
    if (dev) {
      j.img_offset = reinterpret_cast<uintptr_t>(img->data) - base;
      j.out_offset = reinterpret_cast<uintptr_t>(t.out) - base;
    } else {
      const uint64_t room = std::min<uint64_t>(t.out_cap, rsx_dctwrite_bound(&t.desc, img));
      j.out_offset = staged;
      staged += (room + 15u) & ~uint64_t(15);
    }
  }
  CallPlan call;
  if (int st = rsx_dctwrite_plan_create(ctx, n_tiles, jobs.data(), &call.plan))
    return st;
  auto collect = [&]() {
    int rc = RSX_OK;
    for (int i = 0; i < n_tiles; ++i)
      if (rsx_dctwrite_plan_result(call.plan, i, &results[i]) != RSX_OK || results[i].status != RSX_OK)
        rc = RSX_ERR_TILE_ERRORS;
    return rc;
  };
  if (dev) {
    if (int st = rsx_plan_run(call.plan, reinterpret_cast<const void*>(base),
                              reinterpret_cast<void*>(base), nullptr))
      return st;
    (void)rsx_plan_results(call.plan, nullptr, nullptr); // (waits; the tiles' statuses follow)
    return collect();
  }
  LaneGuard lane(ctx);
  if (!lane.lane)
    return RSX_ERR_DEVICE;
  rsx_ctx::HostLane* L = lane.lane;
  const size_t up_bytes = size_t(img->pitch_bytes) * size_t(img->dim_y > 0 ? img->dim_y - 1 : 0) +
                          size_t(img->dim_x > 0 ? img->dim_x : 0) * size_t(img->cpp > 0 ? img->cpp : 0) * 2;
  if (int e = L->d_in.ensure(up_bytes + 64))
    return e;
  if (int e = L->d_out.ensure(size_t(staged) + 64))
    return e;
  {
    std::lock_guard<std::mutex> up(ctx->upload_mu);
    RSX_HIP_CHECK(ctx, hipMemcpyAsync(L->d_in.ptr, img->data, up_bytes, hipMemcpyHostToDevice,
                                      L->stream));
  }
  if (int st = rsx_plan_run(call.plan, L->d_in.ptr, L->d_out.ptr, L->stream))
    return st;
  (void)rsx_plan_results(call.plan, nullptr, nullptr);
  const int rc = collect();
  std::vector<uint8_t> back(static_cast<size_t>(staged));
  if (int e = download_bytes(ctx, L, back.data(), back.size()))
    return e;
  for (int i = 0; i < n_tiles; ++i)
    if (results[i].status == RSX_OK)
      std::memcpy(tiles[i].out, back.data() + jobs[i].out_offset, size_t(results[i].bytes));
  return rc;
}

extern "C" int rsx_probe_stream_copy(rsx_ctx* ctx, const void* in_dev, size_t in_bytes,
                                     void* out_dev, size_t out_bytes, void* stream,
                                     int reps, double* avg_ms) {
  if (!ctx || !in_dev || !out_dev || reps < 1 || !avg_ms)
    return RSX_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  RSX_HIP_CHECK(ctx, hipEventCreate(&e0));
  RSX_HIP_CHECK(ctx, hipEventCreate(&e1));
  hipError_t err = hipEventRecord(e0, s);
  for (int i = 0; i < reps && err == hipSuccess; ++i)
    err = launch_stream_probe(in_dev, in_bytes, out_dev, out_bytes, s);
  if (err == hipSuccess)
    err = hipEventRecord(e1, s);
  if (err == hipSuccess)
    err = hipEventSynchronize(e1);
  float ms = 0.f;
  if (err == hipSuccess)
    err = hipEventElapsedTime(&ms, e0, e1);
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  RSX_HIP_CHECK(ctx, err);
  *avg_ms = double(ms) / reps;
  return RSX_OK;
}
