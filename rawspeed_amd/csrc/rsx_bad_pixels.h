// RawImageData::fixBadPixels on the device (rsx_bad_pixels.hip), used by rsx_api.hip.
#pragma once
#include "rsx_internal.h"

namespace rsx {

int bad_pixels_validate(const rsx_bad_pixels_desc* desc, const rsx_image* img);
// the image checks alone (the fused calls, whose positions come from the device)
int bad_pixels_validate_image(const rsx_image* img, bool is_f32);
uint32_t bad_pixels_map_pitch(uint32_t dim_x);
int bad_pixels_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_bad_pixels_job* jobs,
                           std::unique_ptr<DecoderPlan>* out);
// one job whose map is marked from the zero pixels of its uint16 image (Panasonic V4)
int bad_pixels_zero_plan_create(rsx_ctx* ctx, const rsx_image* img,
                                std::unique_ptr<DecoderPlan>* out);

} // namespace rsx
