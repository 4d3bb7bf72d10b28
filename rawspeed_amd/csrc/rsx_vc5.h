// VC5Decompressor plans (rsx_vc5.hip), used by rsx_api.hip.
#pragma once
#include "rsx_internal.h"

namespace rsx {

int vc5_validate(const rsx_vc5_desc* desc, const rsx_image& img, size_t in_bytes);
int vc5_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_vc5_job* jobs,
                    std::unique_ptr<DecoderPlan>* out);
// per band of job `job` after the plan's results: status, windows walked, parse rounds
// ([channel][subband], 40 entries each; any may be NULL)
int vc5_plan_bands(DecoderPlan* plan, int job, int32_t* band_status, uint32_t* windows,
                   uint32_t* rounds);

} // namespace rsx
