// OlympusDecompressor plans (rsx_olympus.hip), used by rsx_api.hip.
#pragma once
#include "rsx_internal.h"

namespace rsx {

int olympus_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_olympus_job* jobs,
                        std::unique_ptr<DecoderPlan>* out);

} // namespace rsx
