// Baseline-DCT JPEG writer plan (rsx_dctwrite.hip), used by rsx_api.hip.
#pragma once
#include "rsx_internal.h"

namespace rsx {

int dctwrite_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_dctwrite_job* jobs,
                         std::unique_ptr<DecoderPlan>* out);

} // namespace rsx
