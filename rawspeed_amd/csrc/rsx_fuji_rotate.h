// SuperCCD rotation plans (rsx_fuji_rotate.hip), used by rsx_api.hip.
#pragma once
#include "rsx_internal.h"

namespace rsx {

int fuji_rotate_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_raf_rotate_job* jobs,
                            std::unique_ptr<DecoderPlan>* out);

} // namespace rsx
