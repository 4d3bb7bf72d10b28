// Lossy-JPEG DNG tile plans (rsx_dng_jpeg.hip), used by rsx_api.hip.
#pragma once
#include "rsx_internal.h"

namespace rsx {

// a tile's window and what the host made of its header
struct JpegWindow {
  uint32_t off_x, off_y, copy_w, copy_h, cpp;
  int32_t host_status;
};

int dng_jpeg_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_dng_jpeg_job* jobs,
                         std::unique_ptr<DecoderPlan>* out);
// the tiles of job `job` of a plan dng_jpeg_plan_create made
const std::vector<JpegWindow>& dng_jpeg_plan_windows(const DecoderPlan* plan, int job);

} // namespace rsx
