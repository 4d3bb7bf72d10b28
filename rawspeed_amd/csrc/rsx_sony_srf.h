// SonyDecrypt / decodeSRF plans (rsx_sony_srf.hip), used by rsx_api.hip.
#pragma once
#include "rsx_internal.h"

namespace rsx {

int sony_srf_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_sony_srf_job* jobs,
                         std::unique_ptr<DecoderPlan>* out);
// the generator alone over n_words words at the run's input, into the run's output (which may be
// the same address)
int sony_decrypt_plan_create(rsx_ctx* ctx, uint64_t n_words, uint32_t key,
                             std::unique_ptr<DecoderPlan>* out);

} // namespace rsx
