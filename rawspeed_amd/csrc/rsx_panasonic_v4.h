// PanasonicV4Decompressor plans (rsx_panasonic_v4.hip), used by rsx_api.hip.
#pragma once
#include "rsx_internal.h"

namespace rsx {

// *consumed (may be NULL): the bytes the constructor's peekStream takes (bufSize), set whenever
// the geometry and the split passed (also when the input is too short)
int panasonic_v4_validate(const rsx_panasonic_v4_desc* desc, const rsx_image& img, size_t in_bytes,
                          uint64_t* consumed = nullptr);
int panasonic_v4_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_panasonic_v4_job* jobs,
                             std::unique_ptr<DecoderPlan>* out);

} // namespace rsx
