// DngDecoder's opcode list and linearization look-up (rsx_dng_post.hip), used by rsx_api.hip.
#pragma once
#include "rsx_internal.h"

namespace rsx {

int dng_post_validate(const rsx_dng_post_desc* desc, const rsx_image* img,
                      rsx_dng_post_result* result, uint32_t* bad, uint32_t bad_cap);
int dng_post_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_dng_post_job* jobs,
                         std::unique_ptr<DecoderPlan>* out);

} // namespace rsx
