// RawImageData::scaleBlackWhite on the device (rsx_scale.hip), used by rsx_api.hip.
#pragma once
#include "rsx_internal.h"

namespace rsx {

int scale_validate(const rsx_scale_desc* desc, const rsx_image* img);
int scale_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_scale_job* jobs,
                      std::unique_ptr<DecoderPlan>* out);

} // namespace rsx
