// PhaseOneDecompressor plans (rsx_phase_one.hip), used by rsx_api.hip.
#pragma once
#include "rsx_internal.h"

namespace rsx {

int phase_one_validate(int n_strips, const rsx_phase_one_strip* strips, size_t in_bytes,
                       const rsx_image& img);
int phase_one_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_phase_one_job* jobs,
                          std::unique_ptr<DecoderPlan>* out);

} // namespace rsx
