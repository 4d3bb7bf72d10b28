// SonyArw2Decompressor plans (rsx_sony_arw2.hip), used by rsx_api.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "rsx.h"

namespace rsx {

struct Arw2Plan;
struct KernelTimer;

int sony_arw2_validate(const rsx_sony_arw2_desc* desc, const rsx_image& img, size_t in_bytes);
int sony_arw2_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_sony_arw2_job* jobs, Arw2Plan** out);
void sony_arw2_plan_destroy(Arw2Plan* p);
// replace job `job`'s table (same mode) on stream `s`, ahead of the next run on that stream
int sony_arw2_plan_set_table(Arw2Plan* p, int job, const rsx_sony_arw2_desc* desc, hipStream_t s);
int sony_arw2_plan_run(Arw2Plan* p, const void* in_dev, void* out_dev, hipStream_t s,
                       KernelTimer* timer);
int sony_arw2_plan_results(Arw2Plan* p, hipStream_t s, bool ran, int32_t* job_status);
// the status of every image row of job `job` of the last run (after sony_arw2_plan_results)
int sony_arw2_plan_row_status(Arw2Plan* p, hipStream_t s, int job, int32_t* row_status);

} // namespace rsx
