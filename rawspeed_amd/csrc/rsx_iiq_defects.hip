// The bad columns of IiqDecoder::correctSensorDefects on the device (include/rsx.h section 3n,
// RSX_IIQ_OP_SENSOR_DEFECTS).
//
// What the reference does (decoders/IiqDecoder.cpp:499-576): for every record of type 131 / 137 in
// entry 0x400 one thread walks the rows 2 .. dim_y - 3 of the record's column and replaces each
// pixel by a value computed from four (green) or six (other colours) pixels of the columns beside
// it.  A column is written from other columns only, so the rows of a record are independent, and
// so are records whose columns lie more than 2 apart; the plan (rsx_iiq_corr.hip) sorts the records
// of its jobs into levels (rsx_iiq_corr_core.h, defects_levels) and launches
//
//   iiq_bad_columns_kernel   one lane per (record of the level, row): four or six 2-byte gathers
//                            from the columns beside its own -- a column is a stride of
//                            pitch_bytes, so adjacent lanes read adjacent rows and no two lanes
//                            share a cache line; with a few thousand lanes in all the launch
//                            itself is the cost -- and one 2-byte store.
//
// once per level, on the plan's stream, between the fused passes in front of and behind the op.
// A list of columns far apart has one level.  No LDS, no scratch (tests/test_iiq_defects_build.py).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rsx_iiq_corr.h"
#include "rsx_iiq_corr_core.h"

namespace rsx {

namespace {

using namespace rsx_iiq;

constexpr uint32_t DF_THREADS = 256;

__global__ void __launch_bounds__(DF_THREADS)
    iiq_bad_columns_kernel(uint8_t* out_base, const JobDev* jobs, const IiqBadColumn* cols) {
  const IiqBadColumn c = cols[blockIdx.y];
  const JobDev& J = jobs[c.job];
  // (J.h >= 5 and 2 <= c.col <= J.w - 3: the validation)
  const uint32_t row = 2u + blockIdx.x * DF_THREADS + threadIdx.x;
  if (row + 2u >= J.h)
    return;
  uint8_t* img = out_base + J.img_offset;
  const uint32_t colour = J.cfa[c.col % J.cfa_w + (row % J.cfa_h) * J.cfa_w];
  *reinterpret_cast<uint16_t*>(img + size_t(row) * J.pitch + 2u * size_t(c.col)) =
      bad_column_pixel(img, J.pitch, row, c.col, colour);
}

} // namespace

void iiq_bad_columns_launch(uint8_t* out_base, const void* jobs_dev, const IiqBadColumn* cols_dev,
                            uint32_t n_cols, uint32_t max_rows, hipStream_t s) {
  const uint32_t bx = (max_rows + DF_THREADS - 1u) / DF_THREADS;
  for (uint32_t at = 0; at < n_cols; at += 65535u) // (a grid's second dimension)
    hipLaunchKernelGGL(iiq_bad_columns_kernel, dim3(bx, std::min(n_cols - at, 65535u)),
                       dim3(DF_THREADS), 0, s, out_base, static_cast<const JobDev*>(jobs_dev),
                       cols_dev + at);
}

} // namespace rsx
