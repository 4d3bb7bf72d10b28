// SonyArw2Decompressor plans (rsx_sony_arw2.hip), used by rsx_api.hip.
#pragma once
#include "rsx_internal.h"

namespace rsx {

int sony_arw2_validate(const rsx_sony_arw2_desc* desc, const rsx_image& img, size_t in_bytes);
// (a job reads exactly its dim_x * dim_y bytes: the plan reports them as consumed)
int sony_arw2_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_sony_arw2_job* jobs,
                          std::unique_ptr<DecoderPlan>* out);
// replace job `job`'s table (same mode) of an ARW2 plan on stream `s`, ahead of the next run on
// that stream
int sony_arw2_plan_set_table(DecoderPlan* plan, int job, const rsx_sony_arw2_desc* desc, hipStream_t s);

} // namespace rsx
