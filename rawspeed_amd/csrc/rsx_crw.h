// CrwDecompressor plans (rsx_crw.hip), used by rsx_api.hip.
#pragma once
#include "rsx_internal.h"

namespace rsx {

int crw_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_crw_job* jobs,
                    std::unique_ptr<DecoderPlan>* out);
// windows, inner rounds, outer rounds used and settling work of job `job` of the last run
int crw_plan_stats(DecoderPlan* plan, int job, uint32_t* stats);

} // namespace rsx
