// Floating-point writer plans (rsx_fpwrite_pack.hip), used by rsx_api.hip.
#pragma once
#include "rsx_internal.h"

namespace rsx {

int fpwrite_pack_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_fpwrite_pack_job* jobs,
                             std::unique_ptr<DecoderPlan>* out);

// rsx_fpwrite_fit as a plan of one job: the windows of one image in one launch.  The run's input
// is the image's base; its output gets one 32-bit word a window, the width class (0, 1, 2 for 16,
// 24, 32 bits).
struct FpFitJob {
  rsx_image img; // .data ignored
  int n_windows;
  const rsx_fpwrite_window* windows;
};
int fpwrite_fit_plan_create(rsx_ctx* ctx, int n_jobs, const FpFitJob* jobs,
                            std::unique_ptr<DecoderPlan>* out);

// deflate tiles (rsx_fpwrite_deflate.hip)
int fpwrite_deflate_validate(const rsx_dng_deflate_desc& d, uint32_t tile_w, uint32_t tile_h,
                             uint32_t off_x, uint32_t off_y, uint32_t width, uint32_t height,
                             const rsx_image& img);
int fpwrite_deflate_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_fpwrite_deflate_job* jobs,
                                std::unique_ptr<DecoderPlan>* out);

} // namespace rsx
