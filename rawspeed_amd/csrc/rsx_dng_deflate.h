// Deflate DNG tile plans (rsx_dng_deflate.hip), used by rsx_api.hip.
#pragma once
#include "rsx_internal.h"

namespace rsx {

int dng_deflate_validate(const rsx_dng_deflate_desc& d, uint32_t tile_w, uint32_t tile_h, uint32_t off_x,
                         uint32_t off_y, uint32_t width, uint32_t height, uint64_t in_bytes,
                         const rsx_image& img);
int dng_deflate_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_dng_deflate_job* jobs,
                            std::unique_ptr<DecoderPlan>* out);

} // namespace rsx
