// FujiDecompressor plans (rsx_fuji.hip), used by rsx_api.hip.
#pragma once
#include "rsx_internal.h"

namespace rsx {

int fuji_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_fuji_job* jobs,
                     std::unique_ptr<DecoderPlan>* out);

} // namespace rsx
