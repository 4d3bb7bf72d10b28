// PhaseOneDecompressor plans (rsx_phase_one.hip), used by rsx_api.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "rsx.h"

namespace rsx {

struct P1Plan;
struct KernelTimer;

int phase_one_validate(int n_strips, const rsx_phase_one_strip* strips, size_t in_bytes,
                       const rsx_image& img);
int phase_one_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_phase_one_job* jobs, P1Plan** out);
void phase_one_plan_destroy(P1Plan* p);
int phase_one_plan_run(P1Plan* p, const void* in_dev, void* out_dev, hipStream_t s,
                       KernelTimer* timer);
int phase_one_plan_results(P1Plan* p, hipStream_t s, bool ran, int32_t* job_status);
// the status of every image row of job `job` of the last run (after phase_one_plan_results)
int phase_one_plan_row_status(P1Plan* p, hipStream_t s, int job, int32_t* row_status);

} // namespace rsx
