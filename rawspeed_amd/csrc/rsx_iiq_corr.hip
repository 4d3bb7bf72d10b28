// The pixel passes of IiqDecoder::CorrectPhaseOneC on the device (include/rsx.h section 3n).
//
// What the reference does (decoders/IiqDecoder.cpp:280-479): behind the Phase One decode, one
// thread walks the whole image once per correction entry -- a flat field in binary32 for luma, one
// for chroma, a 65536-entry curve per sensor quadrant.  Every one of these reads and writes only
// the pixel it stands on, so a list of them is one pass; what is serial in the flat field is the
// multiplier row, which advances by one binary32 addition per image row (and, inside a row, by one
// per column of a cell).  The arithmetic is rsx_iiq_corr_core.h, shared with the host build.
//
//   iiq_ff_rows_kernel   one lane per (flat-field op, cell column x, plane): walks the op's blocks
//                        and rows in the reference's order and stores mrow(x, c) as it stands when
//                        each touched image row is processed -- a chain of at most 8854 dependent
//                        additions; the table is [row][x][plane] floats.  It depends on the list
//                        and the geometry alone, so it runs once, at plan creation (and again in a
//                        timed run, to be measured).
//   iiq_ff_cols_kernel   ops whose cells are wider than 32 columns: one lane per (touched row, cell,
//                        plane) walks the cell's additions and keeps mult as it stands every 32
//                        columns, so that the fused pass never replays more than 31 (DESIGN 4.14
//                        has the measurement that asked for it).  Plan creation, like the rows.
//   iiq_correct_kernel   the fused pass: a lane owns 8 adjacent pixels of a row -- one 16-byte load
//                        and one 16-byte store where the address allows, else 16-bit halves -- and
//                        applies the job's ops in order.  For a flat field it takes mult and step
//                        from the table at the left edge of its first pixel's cell (or the
//                        start value in front of it), replays the additions of the columns in
//                        between (at most 31) and carries
//                        on across cell boundaries.  The curves (512 KiB an op) are read from
//                        global memory.  A lane none of whose pixels an op stood on stores nothing.
//                        A defects op (rsx_iiq_defects.hip: it reads neighbouring columns) splits
//                        a job's list into the run in front of it and the run behind it; `part`
//                        says which of the two a launch applies, and the plan launches the pass,
//                        the levels of the bad columns and the pass again on one stream.
// No LDS, no scratch (tests/test_iiq_corr_build.py holds the numbers).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "rsx_internal.h"
#include "rsx_ljpeg_dev.h"
#include "rsx_plan_host.h"
#include "rsx_iiq_corr.h"
#include "rsx_iiq_corr_core.h"

namespace rsx {

namespace {

using namespace rsx_iiq;

constexpr int IQ_ROW_THREADS = 64, IQ_THREADS = 256;

struct IqArgs {
  uint8_t* out_base;
  const JobDev* jobs;
  const OpDev* ops;
  float* tables;
  const uint16_t* curves;
  const uint8_t* payloads;
};

__global__ void __launch_bounds__(IQ_ROW_THREADS) iiq_ff_rows_kernel(IqArgs A) {
  const OpDev& op = A.ops[blockIdx.y];
  if (op.kind != RSX_IIQ_OP_FLAT_FIELD || op.F.n_rows == 0u)
    return;
  const uint32_t id = blockIdx.x * IQ_ROW_THREADS + threadIdx.x;
  if (id >= op.F.tcols * op.F.planes)
    return;
  ff_walk_rows(A.payloads + op.payload_off, op.F, id / op.F.planes, id % op.F.planes,
               A.tables + op.table_off);
}

__global__ void __launch_bounds__(IQ_THREADS) iiq_ff_cols_kernel(IqArgs A) {
  const OpDev& op = A.ops[blockIdx.y];
  const FlatField& F = op.F;
  if (op.kind != RSX_IIQ_OP_FLAT_FIELD || F.n_rows == 0u || F.nck == 0u)
    return;
  const uint32_t per_row = (F.tcols - 1u) * F.planes;
  const uint64_t id = uint64_t(blockIdx.x) * IQ_THREADS + threadIdx.x;
  if (id >= uint64_t(F.n_rows) * per_row)
    return;
  const uint32_t r = uint32_t(id / per_row), i = uint32_t(id - uint64_t(r) * per_row);
  ff_walk_cols(A.tables + op.table_off + size_t(r) * F.tcols * F.planes, F, 1u + i / F.planes,
               i % F.planes, A.tables + op.ck_off + size_t(r) * ff_ck_row_floats(F));
}

__global__ void __launch_bounds__(IQ_THREADS) iiq_correct_kernel(IqArgs A, uint32_t part) {
  const JobDev& J = A.jobs[blockIdx.y];
  const uint32_t id = blockIdx.x * IQ_THREADS + threadIdx.x;
  // part 0: the ops in front of the job's defects op (all of them without one); 1: those behind it
  const uint32_t first = part ? J.split + 1u : 0u, end = part ? J.n_ops : J.split;
  if (first >= end || id >= J.h * J.vpr)
    return;
  const uint32_t row = id / J.vpr, v = id - row * J.vpr;
  const uint32_t col0 = 8u * v, n = min(8u, J.w - col0);
  uint8_t* p = A.out_base + J.img_offset + uint64_t(row) * J.pitch + 16u * v;
  const bool whole = n == 8u && (reinterpret_cast<uintptr_t>(p) & 15u) == 0u;
  uint16_t px[8];
  if (whole) {
    const uint4 q = *reinterpret_cast<const uint4*>(p);
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      px[2 * k] = uint16_t(w[k]);
      px[2 * k + 1] = uint16_t(w[k] >> 16);
    }
  } else {
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i)
      px[i] = i < n ? reinterpret_cast<const uint16_t*>(p)[i] : uint16_t(0);
  }
  const uint32_t touched = correct_pixels(J, A.ops, A.tables, A.curves, first, end, row, col0, n, px);
  if (touched == 0u)
    return;
  if (whole) {
    *reinterpret_cast<uint4*>(p) =
        make_uint4(px[0] | uint32_t(px[1]) << 16, px[2] | uint32_t(px[3]) << 16,
                   px[4] | uint32_t(px[5]) << 16, px[6] | uint32_t(px[7]) << 16);
  } else {
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i)
      if (i < n && (touched >> i & 1u))
        reinterpret_cast<uint16_t*>(p)[i] = px[i];
  }
}

struct IqPlan final : DecoderPlan {
  rsx_ctx* ctx = nullptr;
  size_t n_jobs = 0, n_ops = 0;
  DeviceBuffer d_jobs, d_ops, d_tables, d_curves, d_payloads, d_bad_cols;
  uint32_t max_blocks[2] = {0, 0}; // the fused pass in front of and behind the defects ops
  uint32_t max_row_blocks = 0, max_col_blocks = 0;
  // the bad columns of all jobs, sorted by level: level l is [level_end[l - 1], level_end[l]) of
  // d_bad_cols, level_rows[l] the most rows one of its records walks
  std::vector<uint32_t> level_end, level_rows;
  IqArgs args(void* out_dev) const {
    IqArgs A{};
    A.out_base = static_cast<uint8_t*>(out_dev);
    A.jobs = static_cast<const JobDev*>(d_jobs.ptr);
    A.ops = static_cast<const OpDev*>(d_ops.ptr);
    A.tables = static_cast<float*>(d_tables.ptr);
    A.curves = static_cast<const uint16_t*>(d_curves.ptr);
    A.payloads = static_cast<const uint8_t*>(d_payloads.ptr);
    return A;
  }
  int launch_rows(hipStream_t s) {
    if (max_row_blocks == 0)
      return RSX_OK;
    hipLaunchKernelGGL(iiq_ff_rows_kernel, dim3(max_row_blocks, uint32_t(n_ops)),
                       dim3(IQ_ROW_THREADS), 0, s, args(nullptr));
    RSX_HIP_CHECK(ctx, hipGetLastError());
    return RSX_OK;
  }
  int launch_cols(hipStream_t s) {
    if (max_col_blocks == 0)
      return RSX_OK;
    hipLaunchKernelGGL(iiq_ff_cols_kernel, dim3(max_col_blocks, uint32_t(n_ops)), dim3(IQ_THREADS),
                       0, s, args(nullptr));
    RSX_HIP_CHECK(ctx, hipGetLastError());
    return RSX_OK;
  }
  int run(const void*, void* out_dev, hipStream_t s, KernelTimer* timer) override {
    if (max_blocks[0] == 0 && max_blocks[1] == 0 && level_end.empty())
      return RSX_OK; // (no job has an op that writes)
    if (timer) {
      timer->begin(s);
      // (the tables stand since plan creation; a timed run writes the same values again)
      if (int st = launch_rows(s))
        return st;
      timer->mark("iiq_ff_rows_kernel");
      if (max_col_blocks) {
        if (int st = launch_cols(s))
          return st;
        timer->mark("iiq_ff_cols_kernel");
      }
    }
    for (uint32_t part = 0; part < 2u; ++part) {
      if (max_blocks[part]) {
        hipLaunchKernelGGL(iiq_correct_kernel, dim3(max_blocks[part], uint32_t(n_jobs)),
                           dim3(IQ_THREADS), 0, s, args(out_dev), part);
        if (timer)
          timer->mark("iiq_correct_kernel");
      }
      if (part == 1u)
        break;
      for (size_t l = 0; l < level_end.size(); ++l) { // (a list of columns far apart: one level)
        const uint32_t lo = l ? level_end[l - 1] : 0u;
        iiq_bad_columns_launch(static_cast<uint8_t*>(out_dev), d_jobs.ptr,
                               static_cast<const IiqBadColumn*>(d_bad_cols.ptr) + lo,
                               level_end[l] - lo, level_rows[l], s);
        if (timer)
          timer->mark("iiq_bad_columns_kernel");
      }
    }
    RSX_HIP_CHECK(ctx, hipGetLastError());
    return RSX_OK;
  }
  int results(hipStream_t, bool, int32_t* job_status, uint32_t* job_consumed) override {
    // (nothing in the pixels can fail, and a refused job fails the plan's creation)
    if (job_status)
      std::fill(job_status, job_status + n_jobs, int32_t(RSX_OK));
    if (job_consumed)
      std::fill(job_consumed, job_consumed + n_jobs, 0u);
    return RSX_OK;
  }
};

} // namespace

int iiq_correct_validate(const rsx_iiq_corr* corr, const rsx_image* img) {
  return rsx_iiq::validate(corr, img);
}

int iiq_defect_positions(const uint8_t* payload, uint32_t payload_bytes, int32_t dim_x,
                         uint32_t* out, uint32_t cap, uint32_t* n) {
  return rsx_iiq::defect_positions(payload, payload_bytes, dim_x, out, cap, n);
}

int iiq_correct_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_iiq_correct_job* jobs,
                            std::unique_ptr<DecoderPlan>* out) {
  auto p = std::make_unique<IqPlan>();
  p->ctx = ctx;
  p->n_jobs = size_t(n_jobs);
  std::vector<JobDev> jd;
  jd.resize(size_t(n_jobs));
  std::vector<OpDev> ops;
  std::vector<uint8_t> payloads;
  std::vector<const uint16_t*> curves;
  std::vector<std::vector<IiqBadColumn>> levels; // [level]: the records of every job
  uint64_t table_floats = 0;
  for (int i = 0; i < n_jobs; ++i) {
    const rsx_iiq_correct_job& j = jobs[i];
    if (int st = rsx_iiq::validate(&j.corr, &j.img))
      return st;
    if (j.img_offset % 2 != 0 || j.img.pitch_bytes % 2 != 0)
      return RSX_ERR_INVALID_ARG;
    JobDev& J = jd[size_t(i)];
    std::memset(&J, 0, sizeof J);
    J.img_offset = j.img_offset;
    J.pitch = j.img.pitch_bytes;
    J.w = uint32_t(j.img.dim_x);
    J.h = uint32_t(j.img.dim_y);
    J.vpr = (J.w + 7u) / 8u;
    const uint64_t lanes = uint64_t(J.h) * J.vpr;
    if (lanes >= (1ull << 31))
      return RSX_ERR_UNSUPPORTED; // (lane numbers are 32-bit on the device)
    J.op0 = uint32_t(ops.size());
    J.n_ops = J.split = uint32_t(j.corr.n_ops);
    J.cfa_w = uint32_t(std::max(j.corr.cfa_w, 0));
    J.cfa_h = uint32_t(std::max(j.corr.cfa_h, 0));
    if (uint64_t(J.cfa_w) * J.cfa_h <= 64)
      for (uint32_t k = 0; k < J.cfa_w * J.cfa_h; ++k)
        J.sel[k] = cfa_select(J.cfa[k] = j.corr.cfa[k]);
    for (int o = 0; o < j.corr.n_ops; ++o)
      if (j.corr.ops[o].kind == RSX_IIQ_OP_SENSOR_DEFECTS)
        J.split = uint32_t(o);
    const uint32_t blocks = uint32_t((lanes + IQ_THREADS - 1) / IQ_THREADS);
    if (J.split > 0)
      p->max_blocks[0] = std::max(p->max_blocks[0], blocks);
    if (J.split + 1u < J.n_ops)
      p->max_blocks[1] = std::max(p->max_blocks[1], blocks);
    for (int o = 0; o < j.corr.n_ops; ++o) {
      const rsx_iiq_op& in = j.corr.ops[o];
      OpDev op;
      std::memset(&op, 0, sizeof op);
      op.kind = uint32_t(in.kind);
      if (in.kind == RSX_IIQ_OP_QUADRANT_CURVES) {
        op.black_level = in.black_level;
        op.split_row = in.split_row;
        op.split_col = in.split_col;
        op.curves_off = uint64_t(curves.size()) * 4u * 65536u;
        curves.push_back(in.curves);
      } else if (in.kind == RSX_IIQ_OP_SENSOR_DEFECTS) {
        std::vector<uint32_t> cols, ends;
        defects_levels(in.payload, in.payload_bytes, j.img.dim_x, j.img.dim_y, &cols, &ends);
        if (levels.size() < ends.size()) {
          levels.resize(ends.size());
          p->level_rows.resize(ends.size(), 0u);
        }
        for (size_t l = 0, k = 0; l < ends.size(); ++l) {
          for (; k < ends[l]; ++k)
            levels[l].push_back(IiqBadColumn{uint32_t(i), cols[k]});
          p->level_rows[l] = std::max(p->level_rows[l], J.h - 4u);
        }
      } else {
        ff_parse(in.payload, in.payload_bytes, in.chroma != 0, j.img.dim_x, j.img.dim_y, &op.F);
        if (op.F.n_rows) {
          op.table_off = table_floats;
          table_floats += ff_table_floats(op.F);
          op.ck_off = table_floats;
          table_floats += ff_ck_floats(op.F);
          if (op.F.nck) {
            const uint64_t lanes_c = uint64_t(op.F.n_rows) * (op.F.tcols - 1u) * op.F.planes;
            p->max_col_blocks =
                std::max(p->max_col_blocks, uint32_t((lanes_c + IQ_THREADS - 1) / IQ_THREADS));
          }
          op.payload_off = payloads.size();
          const size_t used = 16u + 2u * size_t(op.F.high) * op.F.wide * op.F.planes;
          payloads.insert(payloads.end(), in.payload, in.payload + used);
          const uint32_t lanes_r = op.F.tcols * op.F.planes;
          p->max_row_blocks =
              std::max(p->max_row_blocks, (lanes_r + IQ_ROW_THREADS - 1) / IQ_ROW_THREADS);
        }
      }
      ops.push_back(op);
    }
  }
  p->n_ops = ops.size();
  std::vector<IiqBadColumn> bad_cols;
  for (const std::vector<IiqBadColumn>& l : levels) {
    bad_cols.insert(bad_cols.end(), l.begin(), l.end());
    p->level_end.push_back(uint32_t(bad_cols.size()));
  }
  if (n_jobs > 65535 || ops.size() > 65535)
    return RSX_ERR_UNSUPPORTED; // (a grid's second dimension)
  RSX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int st;
  if ((st = upload(ctx, p->d_jobs, jd)) || (st = upload(ctx, p->d_ops, ops)) ||
      (st = p->d_tables.ensure(size_t(table_floats) * 4 + 16)) ||
      (st = p->d_curves.ensure(curves.size() * 4 * 65536 * 2 + 16)) ||
      (st = upload(ctx, p->d_payloads, payloads)) || (st = upload(ctx, p->d_bad_cols, bad_cols)))
    return st;
  for (size_t k = 0; k < curves.size(); ++k)
    RSX_HIP_CHECK(ctx, hipMemcpy(static_cast<uint16_t*>(p->d_curves.ptr) + k * 4 * 65536, curves[k],
                                 size_t(4) * 65536 * 2, hipMemcpyHostToDevice));
  // the row tables and the start values inside wide cells: once, here
  if (int e = p->launch_rows(ctx->stream))
    return e;
  if (int e = p->launch_cols(ctx->stream))
    return e;
  RSX_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  *out = std::move(p);
  return RSX_OK;
}

} // namespace rsx
