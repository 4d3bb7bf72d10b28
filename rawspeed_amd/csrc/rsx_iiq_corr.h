// IiqDecoder::CorrectPhaseOneC plans (rsx_iiq_corr.hip, rsx_iiq_defects.hip), used by rsx_api.hip.
#pragma once
#include "rsx_internal.h"

namespace rsx {

int iiq_correct_validate(const rsx_iiq_corr* corr, const rsx_image* img);
// rsx_iiq_defect_positions
int iiq_defect_positions(const uint8_t* payload, uint32_t payload_bytes, int32_t dim_x,
                         uint32_t* out, uint32_t cap, uint32_t* n);
int iiq_correct_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_iiq_correct_job* jobs,
                            std::unique_ptr<DecoderPlan>* out);

// a bad-column record of a plan: job `job` of the plan, column `col` of its image
struct IiqBadColumn {
  uint32_t job, col;
};
// One level of a plan's bad columns (rsx_iiq_defects.hip): n_cols records that touch disjoint
// columns, max_rows the most rows (dim_y - 4) a job of the level has; jobs_dev: the plan's JobDev.
void iiq_bad_columns_launch(uint8_t* out_base, const void* jobs_dev, const IiqBadColumn* cols_dev,
                            uint32_t n_cols, uint32_t max_rows, hipStream_t s);

} // namespace rsx
