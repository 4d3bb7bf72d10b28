// Writer plans (rsx_encode_pack.hip, rsx_encode_ljpeg.hip), used by rsx_api.hip.
#pragma once
#include "rsx_internal.h"

namespace rsx {

int encode_pack_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_encode_pack_job* jobs,
                            std::unique_ptr<DecoderPlan>* out);
int encode_ljpeg_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_encode_ljpeg_job* jobs,
                             std::unique_ptr<DecoderPlan>* out);
// the histogram form of the same plan: no tables read, no stream written; the 4 x 17 counts of
// job i go to out_offset (a multiple of 8) of the run's output buffer
int encode_histogram_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_encode_ljpeg_job* jobs,
                                 std::unique_ptr<DecoderPlan>* out);

} // namespace rsx
