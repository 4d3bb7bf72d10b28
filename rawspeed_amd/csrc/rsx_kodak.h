// KodakDecompressor plans (rsx_kodak.hip), used by rsx_api.hip.
#pragma once
#include "rsx_internal.h"

namespace rsx {

int kodak_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_kodak_job* jobs,
                      std::unique_ptr<DecoderPlan>* out);
// this call's table onto job `job` of a plan made for the same depth and table mode, on `s`
int kodak_plan_set_table(DecoderPlan* plan, int job, const rsx_kodak_desc* desc, hipStream_t s);

} // namespace rsx
