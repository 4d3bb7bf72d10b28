// Image hash plans (rsx_image_hash.hip), used by rsx_api.hip.
#pragma once
#include "rsx_internal.h"

namespace rsx {

int image_hash_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_image_hash_job* jobs,
                           std::unique_ptr<DecoderPlan>* out);

} // namespace rsx
