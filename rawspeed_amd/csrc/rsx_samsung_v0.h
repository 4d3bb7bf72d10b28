// SamsungV0Decompressor plans (rsx_samsung_v0.hip), used by rsx_api.hip.
#pragma once
#include "rsx_internal.h"

namespace rsx {

int samsung_v0_validate(const uint32_t* row_offsets, int n_offsets, size_t in_bytes,
                        const rsx_image& img);
int samsung_v0_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_samsung_v0_job* jobs,
                           std::unique_ptr<DecoderPlan>* out);

} // namespace rsx
