// NefDecoder::DecodeNikonSNef plans (rsx_nikon_snef.hip), used by rsx_api.hip.
#pragma once
#include "rsx_internal.h"

namespace rsx {

int nikon_snef_validate(const rsx_nikon_snef_desc* desc, const rsx_image& img, size_t in_bytes);
// (a job reads exactly its 3 * dim_x * dim_y bytes: the plan reports them as consumed)
int nikon_snef_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_nikon_snef_job* jobs,
                           std::unique_ptr<DecoderPlan>* out);
// replace job `job`'s table of an sNEF plan on stream `s`, ahead of the next run on that stream
// (the white balance is part of the job, and so of a cached plan's key)
int nikon_snef_plan_set_table(DecoderPlan* plan, int job, const rsx_nikon_snef_desc* desc, hipStream_t s);

} // namespace rsx
