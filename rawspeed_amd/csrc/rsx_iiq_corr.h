// IiqDecoder::CorrectPhaseOneC plans (rsx_iiq_corr.hip), used by rsx_api.hip.
#pragma once
#include "rsx_internal.h"

namespace rsx {

int iiq_correct_validate(const rsx_iiq_corr* corr, const rsx_image* img);
int iiq_correct_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_iiq_correct_job* jobs,
                            std::unique_ptr<DecoderPlan>* out);

} // namespace rsx
