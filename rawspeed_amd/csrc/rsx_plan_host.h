// rsx_plan_host.h -- the host side the decoder plans share: the uploads of a plan's creation,
// the fetch of status words, and the fold of per-job statuses in results().  Host code only.
// Everything here has internal linkage: the library's dynamic table stays the C-ABI.
#pragma once

#include "rsx_internal.h"

#include <cstddef>
#include <cstdint>
#include <vector>

namespace rsx {
namespace {

// A status word of the device that nothing has written (the host's one spelling of it; the
// kernels have their own).
constexpr uint32_t STATUS_NONE = 0xFFFFFFFFu;

// Room for v and `pad` bytes behind it, and v in it when this returns.  `pad` is slack for loads
// wider than an entry; a caller passes 0 where the kernel reads the buffer entry by entry.
template <class T>
int upload(rsx_ctx* ctx, DeviceBuffer& d, const std::vector<T>& v, size_t pad = 16) {
  if (int st = d.ensure(v.size() * sizeof(T) + pad))
    return st;
  if (!v.empty())
    RSX_HIP_CHECK(ctx, hipMemcpy(d.ptr, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return RSX_OK;
}

// Words [first, first + n) of d into out on stream s, which has passed them when this returns.
inline int fetch_words(rsx_ctx* ctx, hipStream_t s, const DeviceBuffer& d, size_t first, size_t n,
                       uint32_t* out) {
  RSX_HIP_CHECK(ctx, hipMemcpyAsync(out, static_cast<const uint32_t*>(d.ptr) + first, n * 4,
                                    hipMemcpyDeviceToHost, s));
  RSX_HIP_CHECK(ctx, hipStreamSynchronize(s));
  return RSX_OK;
}

// ... as the statuses of a job's rows or strips, through the plan's staging vector.
inline int fetch_words(rsx_ctx* ctx, hipStream_t s, const DeviceBuffer& d, size_t first, size_t n,
                       std::vector<uint32_t>& staging, int32_t* out) {
  staging.resize(n);
  if (int st = fetch_words(ctx, s, d, first, n, staging.data()))
    return st;
  for (size_t r = 0; r < n; ++r)
    out[r] = int32_t(staging[r]);
  return RSX_OK;
}

// Which failing job's status results() returns: the last one's (every decoder but one), or the
// lowest-numbered one's (Olympus).
enum class FoldOrder { LAST_FAILING, LOWEST_FAILING };

// status_of(i) of every job into job_status (may be NULL); returns the status `order` picks
// among the failing ones, or RSX_OK.
template <class StatusOf>
int fold_jobs(size_t n_jobs, FoldOrder order, int32_t* job_status, StatusOf status_of) {
  int rc = RSX_OK;
  for (size_t k = 0; k < n_jobs; ++k) {
    const size_t i = order == FoldOrder::LAST_FAILING ? k : n_jobs - 1 - k;
    const int st = status_of(i);
    if (job_status)
      job_status[i] = st;
    if (st != RSX_OK)
      rc = st;
  }
  return rc;
}

// The per-job statuses of a plan: what the host's validation said, the words the kernels write
// (STATUS_NONE = fine), and the host's copy of those.
struct JobStatus {
  std::vector<int32_t> host;   // validation result per job
  std::vector<uint32_t> words; // of the last fetch
  DeviceBuffer dev;
  bool fetched = false;        // `words` are the last run's

  // (after `host` has its size)
  int init(size_t words_per_job = 1) {
    words.assign(host.size() * words_per_job, STATUS_NONE);
    return dev.ensure(words.size() * 4 + 16);
  }
  // run(): no word written, on the stream of the kernels that write them
  int reset(rsx_ctx* ctx, hipStream_t s) {
    fetched = false;
    RSX_HIP_CHECK(ctx, hipMemsetAsync(dev.ptr, 0xFF, words.size() * 4, s));
    return RSX_OK;
  }
  int fetch(rsx_ctx* ctx, hipStream_t s) {
    if (int st = fetch_words(ctx, s, dev, 0, words.size(), words.data()))
      return st;
    fetched = true;
    return RSX_OK;
  }
  // results() of a plan with one word a job: the words are fetched if the plan `ran_with_work`
  // (it ran and some job went to the device); a job the host accepted then has its word & mask
  // unless that is STATUS_NONE
  int fold(rsx_ctx* ctx, hipStream_t s, bool ran_with_work, uint32_t mask, FoldOrder order,
           int32_t* job_status) {
    if (ran_with_work)
      if (int st = fetch(ctx, s))
        return st;
    return fold_jobs(host.size(), order, job_status, [&](size_t i) {
      return host[i] == RSX_OK && ran_with_work && words[i] != STATUS_NONE ? int(words[i] & mask)
                                                                            : int(host[i]);
    });
  }
};

} // namespace
} // namespace rsx
