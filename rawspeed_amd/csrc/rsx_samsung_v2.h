// SamsungV2Decompressor plans (rsx_samsung_v2.hip), used by rsx_api.hip.
#pragma once
#include "rsx_internal.h"

namespace rsx {

int samsung_v2_validate(const rsx_samsung_v2_desc& d, const rsx_image& img);
int samsung_v2_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_samsung_v2_job* jobs,
                           std::unique_ptr<DecoderPlan>* out);

} // namespace rsx
