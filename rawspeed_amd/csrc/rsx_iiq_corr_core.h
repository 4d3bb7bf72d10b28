// The arithmetic of IiqDecoder::CorrectPhaseOneC's pixel passes (include/rsx.h section 3n), shared
// by the kernels of rsx_iiq_corr.hip and by a host build (rsx_iiq_corr_host.cpp): the geometry of a
// flat-field entry, the walk of one column of its multiplier rows, the multiply of one pixel, the
// quadrant curve of one pixel, and the validation of a whole list.  Everything here compiles as
// host C++, so the same functions are pinned against the reference on the CPU and run on the card.
//
// PhaseOneFlatField (decoders/IiqDecoder.cpp:410-479) keeps one row of multipliers mrow(x, c) per
// cell column x and advances it by REPEATED binary32 additions of a slope, once per image row; along
// a row it does the same between two neighbouring cell columns.  Nothing here may be contracted or
// re-associated: on the device every operation is an explicit round-to-nearest intrinsic, the host
// build is compiled with -ffp-contract=off.  The decomposition:
//   ff_walk_rows  one (x, plane): the values mrow(x, c) has when each touched image row is
//                 processed, into a table [row][x][plane] -- a chain of dependent additions, one per
//                 row (at most 8854)
//   ff_cell       at (row, col): the cell, mult = mrow(x - 1, c) and step = (mrow(x, c) - mult) /
//                 head[4] from that table; the caller replays `k` additions to reach its column
//   ff_walk_cols  one (row, cell, plane) of an op whose cells are wider than CK_COLS columns: mult as
//                 it stands after every CK_COLS additions, so that a replay never takes more than
//                 CK_COLS - 1 of them
//   ff_pixel      the multiply, the truncation and the clamp
//
// The sensor defects of entry 0x400 (correctSensorDefects, :499-576) are no such pass: a bad column
// is interpolated from the columns beside it.  defects_walk visits the records in file order,
// defects_check makes the checks of the validation, bad_column_pixel computes one pixel of a bad
// column from its neighbours (bad_column_green / bad_column_other the arithmetic), defects_levels
// orders the columns of a list into levels of records that do not touch each other, and
// defect_positions collects the type-129 records.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "rsx.h"

#if defined(__HIPCC__)
#define RSX_IIQ_FN __host__ __device__ __forceinline__
#else
#define RSX_IIQ_FN inline
#endif

namespace rsx_iiq {

// every binary32 operation rounded on its own
#if defined(__HIP_DEVICE_COMPILE__)
RSX_IIQ_FN float f_add(float a, float b) { return __fadd_rn(a, b); }
RSX_IIQ_FN float f_sub(float a, float b) { return __fsub_rn(a, b); }
RSX_IIQ_FN float f_mul(float a, float b) { return __fmul_rn(a, b); }
RSX_IIQ_FN float f_div(float a, float b) { return __fdiv_rn(a, b); }
#else
RSX_IIQ_FN float f_add(float a, float b) { return a + b; }
RSX_IIQ_FN float f_sub(float a, float b) { return a - b; }
RSX_IIQ_FN float f_mul(float a, float b) { return a * b; }
RSX_IIQ_FN float f_div(float a, float b) { return a / b; }
#endif

// the row table of one flat-field op may hold this many floats (256 MiB)
constexpr uint64_t MAX_TABLE_FLOATS = 1ull << 26;

// cells wider than this keep a start value of mult every CK_COLS columns (ff_walk_cols)
constexpr uint32_t CK_COLS = 32;

// A flat-field entry against an image: what the loops of :438-478 touch.
struct FlatField {
  uint32_t head[8];
  uint32_t planes; // nc / 2: 1 luma, 2 chroma
  uint32_t wide, high;
  uint32_t n_rows;  // image rows head[1] .. head[1] + n_rows - 1 are touched (0: none)
  uint32_t col_end; // ... and the columns head[0] .. col_end - 1
  uint32_t tcols;   // cell columns x = 0 .. tcols - 1 are read by those columns
  uint32_t nck;     // start values inside a cell: after CK_COLS, 2 CK_COLS .. additions (0: none)
};

RSX_IIQ_FN uint32_t rd16(const uint8_t* p) { return uint32_t(p[0]) | (uint32_t(p[1]) << 8); }

// RSX_OK / RSX_ERR_IO (the payload ends before the values the reference reads); F->n_rows == 0
// when the op writes nothing (a zero head field, an area outside the image, wide == 1, high == 1)
RSX_IIQ_FN int ff_parse(const uint8_t* payload, uint32_t bytes, bool chroma, int32_t dim_x,
                        int32_t dim_y, FlatField* F) {
  F->planes = chroma ? 2u : 1u;
  F->wide = F->high = F->n_rows = F->col_end = F->tcols = F->nck = 0;
  if (bytes < 16u)
    return RSX_ERR_IO;
  for (int i = 0; i < 8; ++i)
    F->head[i] = rd16(payload + 2 * i);
  const uint32_t* h = F->head;
  if (h[2] == 0 || h[3] == 0 || h[4] == 0 || h[5] == 0)
    return RSX_OK;
  F->wide = (h[2] + h[4] - 1u) / h[4];
  F->high = (h[3] + h[5] - 1u) / h[5];
  if (uint64_t(bytes) < 16u + 2ull * F->high * F->wide * F->planes)
    return RSX_ERR_IO;
  // rows: head[1] + (y - 1) head[5] <= row < min(dim_y, head[1] + y head[5], head[1] + head[3] -
  // head[5]) for y = 1 .. high - 1: one run from head[1]
  int64_t row_end = int64_t(h[1]) + int64_t(F->high - 1u) * h[5];
  if (row_end > int64_t(dim_y))
    row_end = dim_y;
  if (row_end > int64_t(h[1]) + int64_t(h[3]) - int64_t(h[5]))
    row_end = int64_t(h[1]) + int64_t(h[3]) - int64_t(h[5]);
  int64_t col_end = int64_t(h[0]) + int64_t(F->wide - 1u) * h[4];
  if (col_end > int64_t(dim_x))
    col_end = dim_x;
  if (col_end > int64_t(h[0]) + int64_t(h[2]) - int64_t(h[4]))
    col_end = int64_t(h[0]) + int64_t(h[2]) - int64_t(h[4]);
  if (row_end <= int64_t(h[1]) || col_end <= int64_t(h[0]))
    return RSX_OK;
  F->n_rows = uint32_t(row_end - h[1]);
  F->col_end = uint32_t(col_end);
  F->tcols = (F->col_end - h[0] + h[4] - 1u) / h[4] + 1u; // (<= wide: col_end stops a cell early)
  F->nck = (h[4] - 1u) / CK_COLS;
  return RSX_OK;
}

RSX_IIQ_FN uint64_t ff_table_floats(const FlatField& F) {
  return uint64_t(F.n_rows) * F.tcols * F.planes;
}

// the start values: [row][cell x - 1][j - 1][plane], j = 1 .. nck.  Never more than the row table
// of 1 x 1 cells over the same area would hold, / CK_COLS.
RSX_IIQ_FN uint64_t ff_ck_row_floats(const FlatField& F) {
  return F.tcols ? uint64_t(F.tcols - 1u) * F.nck * F.planes : 0u;
}
RSX_IIQ_FN uint64_t ff_ck_floats(const FlatField& F) { return uint64_t(F.n_rows) * ff_ck_row_floats(F); }

// num of (y, x, plane): the u16 behind the head, / 32768.0F (exact)
RSX_IIQ_FN float ff_num(const uint8_t* payload, const FlatField& F, uint32_t y, uint32_t x,
                        uint32_t plane) {
  const size_t i = 16u + 2u * ((size_t(y) * F.wide + x) * F.planes + plane);
  return f_div(float(rd16(payload + i)), 32768.0F);
}

// One (x, plane) of an op with n_rows > 0, x < tcols: table[(r * tcols + x) * planes + plane] =
// mrow(x, c) as it stands when image row head[1] + r is processed.  Blocks behind the last touched
// row change nothing that is read.
RSX_IIQ_FN void ff_walk_rows(const uint8_t* payload, const FlatField& F, uint32_t x, uint32_t plane,
                             float* table) {
  float m = ff_num(payload, F, 0, x, plane);
  const float h5 = float(F.head[5]);
  uint32_t r = 0;
  for (uint32_t y = 1; y < F.high && r < F.n_rows; ++y) {
    const float slope = f_div(f_sub(ff_num(payload, F, y, x, plane), m), h5);
    const uint64_t block_end = uint64_t(y) * F.head[5];
    const uint32_t end = block_end < F.n_rows ? uint32_t(block_end) : F.n_rows;
    for (; r < end; ++r) {
      table[(size_t(r) * F.tcols + x) * F.planes + plane] = m;
      m = f_add(m, slope);
    }
  }
}

// mult and step of plane `plane` in the cell right of cell column x - 1 (x >= 1), table row `trow`
RSX_IIQ_FN void ff_cell(const float* trow, const FlatField& F, uint32_t x, uint32_t plane,
                        float* mult, float* step) {
  const float a = trow[size_t(x - 1u) * F.planes + plane];
  const float b = trow[size_t(x) * F.planes + plane];
  *mult = a;
  *step = f_div(f_sub(b, a), float(F.head[4]));
}

// One (cell x >= 1, plane) of table row `trow`, nck > 0: ck[((x - 1) * nck + j - 1) * planes + plane]
// = mult after j * CK_COLS additions (`ck`: the row's start values)
RSX_IIQ_FN void ff_walk_cols(const float* trow, const FlatField& F, uint32_t x, uint32_t plane,
                             float* ck) {
  float m, s;
  ff_cell(trow, F, x, plane, &m, &s);
  for (uint32_t j = 1; j <= F.nck; ++j) {
    for (uint32_t t = 0; t < CK_COLS; ++t)
      m = f_add(m, s);
    ck[(size_t(x - 1u) * F.nck + (j - 1u)) * F.planes + plane] = m;
  }
}

// val = unsigned(float(pixel) * mult), min(val, 0xFFFF) (:467-468); a product below 0 gives 0
RSX_IIQ_FN uint16_t ff_pixel(uint16_t px, float mult) {
  const float v = f_mul(float(px), mult);
  if (!(v > 0.0F))
    return 0;
  return v >= 65535.0F ? uint16_t(0xFFFF) : uint16_t(uint32_t(v));
}

// what a CFA position does in a chroma op: 0 plane 0 (red), 1 plane 1 (blue), 2 nothing
RSX_IIQ_FN uint8_t cfa_select(uint8_t colour) {
  return colour == 0 ? 0 : colour == 2 ? 1 : 2;
}

// :397-400
RSX_IIQ_FN uint16_t quad_pixel(uint16_t px, const uint16_t* curve, uint32_t black_level) {
  const uint16_t diff = uint32_t(px) < black_level ? px : uint16_t(black_level);
  return uint16_t(curve[uint16_t(px - diff)] + diff);
}

// ------------------------------------------------------------------------------------------
// Sensor defects (entry 0x400): 8-byte records of little-endian u16 col, row, type and 2 ignored
// bytes, in file order.
// ------------------------------------------------------------------------------------------
// a list may hold this many bad-column records inside the image (real lists hold a handful)
constexpr uint32_t MAX_BAD_COLUMNS = 4096;

struct DefectRecord {
  uint32_t col, row, type;
};

RSX_IIQ_FN DefectRecord defect_record(const uint8_t* payload, uint32_t i) {
  const uint8_t* p = payload + size_t(8) * i;
  return DefectRecord{rd16(p), rd16(p + 2), rd16(p + 4)};
}

// a record that correctBadColumn runs for: type 131 / 137 inside the image.  With dim_y < 5 its
// loop has no row.
RSX_IIQ_FN bool defect_is_column(const DefectRecord& r, int32_t dim_x, int32_t dim_y) {
  return (r.type == 131u || r.type == 137u) && int64_t(r.col) < int64_t(dim_x) && dim_y >= 5;
}

// the checks of one defects op (include/rsx.h section 3n, in its order)
inline int defects_check(const rsx_iiq_op& op, const rsx_iiq_corr* corr, const rsx_image* img) {
  if (!op.payload && op.payload_bytes > 0)
    return RSX_ERR_INVALID_ARG;
  if (op.payload_bytes % 8u != 0)
    return RSX_ERR_IO;
  uint32_t n_cols = 0;
  for (uint32_t i = 0; i < op.payload_bytes / 8u; ++i) {
    const DefectRecord r = defect_record(op.payload, i);
    if (!defect_is_column(r, img->dim_x, img->dim_y))
      continue;
    if (corr->cfa_w <= 0 || corr->cfa_h <= 0 || int64_t(corr->cfa_w) * int64_t(corr->cfa_h) > 64)
      return RSX_ERR_INVALID_ARG; // ("No CFA size set")
    if (r.col < 2u || int64_t(r.col) > int64_t(img->dim_x) - 3)
      return RSX_ERR_UNSUPPORTED; // (the reference reads outside the row)
    if (++n_cols > MAX_BAD_COLUMNS)
      return RSX_ERR_UNSUPPORTED;
  }
  return RSX_OK;
}

// rsx_iiq_defect_positions: the type-129 records inside the image as handleBadPixel inserts them
inline int defect_positions(const uint8_t* payload, uint32_t payload_bytes, int32_t dim_x,
                            uint32_t* out, uint32_t cap, uint32_t* n) {
  if (n)
    *n = 0;
  if ((!payload && payload_bytes > 0) || (!out && cap > 0) || !n)
    return RSX_ERR_INVALID_ARG;
  if (payload_bytes % 8u != 0)
    return RSX_ERR_IO;
  uint32_t count = 0;
  for (uint32_t i = 0; i < payload_bytes / 8u; ++i) {
    const DefectRecord r = defect_record(payload, i);
    if (int64_t(r.col) >= int64_t(dim_x) || r.type != 129u)
      continue;
    if (count < cap)
      out[count] = (r.row << 16) + r.col;
    ++count;
  }
  *n = count;
  return RSX_OK;
}

// The bad columns of a checked op in an order the device can take: `cols` holds the columns of
// the records correctBadColumn runs for, sorted by level (file order inside a level), and
// level_end[l] the end of level l in it.  A record's level is one above the highest level of an
// earlier record whose column lies within 2 of its own (it reads that column, or that record reads
// or writes this one); the records of one level touch disjoint columns and read none that the
// level writes, so a level is one launch over (record, row), and the levels run in order.
inline void defects_levels(const uint8_t* payload, uint32_t payload_bytes, int32_t dim_x,
                           int32_t dim_y, std::vector<uint32_t>* cols,
                           std::vector<uint32_t>* level_end) {
  cols->clear();
  level_end->clear();
  std::vector<int32_t> last(size_t(dim_x) + 4u, -1); // the highest level so far at column + 2
  std::vector<uint32_t> col, level;
  for (uint32_t i = 0; i < payload_bytes / 8u; ++i) {
    const DefectRecord r = defect_record(payload, i);
    if (!defect_is_column(r, dim_x, dim_y))
      continue;
    int32_t l = -1;
    for (uint32_t c = r.col; c <= r.col + 4u; ++c)
      l = last[c] > l ? last[c] : l;
    last[r.col + 2u] = l + 1;
    col.push_back(r.col);
    level.push_back(uint32_t(l + 1));
    if (level_end->size() < size_t(l + 2))
      level_end->resize(size_t(l + 2), 0u);
    ++(*level_end)[size_t(l + 1)];
  }
  uint32_t at = 0;
  std::vector<uint32_t> next(level_end->size());
  for (size_t l = 0; l < level_end->size(); ++l) {
    next[l] = at;
    at += (*level_end)[l];
    (*level_end)[l] = at;
  }
  cols->resize(col.size());
  for (size_t i = 0; i < col.size(); ++i)
    (*cols)[next[level[i]]++] = col[i];
}

// binary64, every operation rounded on its own
#if defined(__HIP_DEVICE_COMPILE__)
RSX_IIQ_FN double d_add(double a, double b) { return __dadd_rn(a, b); }
RSX_IIQ_FN double d_mul(double a, double b) { return __dmul_rn(a, b); }
#else
RSX_IIQ_FN double d_add(double a, double b) { return a + b; }
RSX_IIQ_FN double d_mul(double a, double b) { return a * b; }
#endif

// :541-556.  v: the diagonal neighbours (row - 1, col - 1), (row + 1, col - 1), (row - 1, col + 1),
// (row + 1, col + 1); the FIRST largest deviation from their mean is left out
RSX_IIQ_FN uint16_t bad_column_green(const uint32_t (&v)[4]) {
  const int32_t sum = int32_t(v[0] + v[1] + v[2] + v[3]);
  uint32_t out = v[0];
  int32_t worst = -1;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < 4; ++i) {
    const int32_t d = int32_t(4u * v[i]) - sum;
    const int32_t dev = d < 0 ? -d : d;
    if (worst < dev) {
      worst = dev;
      out = v[i];
    }
  }
  return uint16_t((uint32_t(sum) - out + 1u) / 3u);
}

// :568-573.  lround of a value that is never negative and never above 65535.000...; x - r is exact
RSX_IIQ_FN uint16_t bad_column_other(uint32_t diags, uint32_t horiz) {
  const double x = d_add(d_mul(double(diags), 0.0732233), d_mul(double(horiz), 0.3535534));
  uint32_t r = uint32_t(x);
  if (x - double(r) >= 0.5)
    ++r;
  return uint16_t(r);
}

RSX_IIQ_FN uint32_t px_at(const uint8_t* img, uint32_t pitch, uint32_t row, uint32_t col) {
  return *reinterpret_cast<const uint16_t*>(img + size_t(row) * pitch + 2u * size_t(col));
}

// the new value of (row, col) of a bad column: 2 <= row <= h - 3, 2 <= col <= w - 3; colour =
// cfa[(col mod cfa_w) + (row mod cfa_h) cfa_w], the reference's getColorAt(col, row)
RSX_IIQ_FN uint16_t bad_column_pixel(const uint8_t* img, uint32_t pitch, uint32_t row, uint32_t col,
                                     uint32_t colour) {
  if (colour == 1u) {
    const uint32_t v[4] = {px_at(img, pitch, row - 1u, col - 1u), px_at(img, pitch, row + 1u, col - 1u),
                           px_at(img, pitch, row - 1u, col + 1u), px_at(img, pitch, row + 1u, col + 1u)};
    return bad_column_green(v);
  }
  const uint32_t diags = px_at(img, pitch, row + 2u, col - 2u) + px_at(img, pitch, row - 2u, col - 2u) +
                         px_at(img, pitch, row + 2u, col + 2u) + px_at(img, pitch, row - 2u, col + 2u);
  const uint32_t horiz = px_at(img, pitch, row, col - 2u) + px_at(img, pitch, row, col + 2u);
  return bad_column_other(diags, horiz);
}

// rsx_iiq_correct_validate (include/rsx.h section 3n, in its order)
inline int validate(const rsx_iiq_corr* corr, const rsx_image* img) {
  if (!corr || !img || img->cpp != 1 || img->dim_x <= 0 || img->dim_y <= 0 ||
      uint64_t(img->pitch_bytes) < 2ull * uint64_t(img->dim_x))
    return RSX_ERR_INVALID_ARG;
  if (corr->n_ops < 0 || corr->n_ops > RSX_IIQ_MAX_OPS)
    return RSX_ERR_INVALID_ARG;
  for (int i = 0; i < corr->n_ops; ++i) {
    const rsx_iiq_op& op = corr->ops[i];
    if (op.kind != RSX_IIQ_OP_FLAT_FIELD && op.kind != RSX_IIQ_OP_QUADRANT_CURVES &&
        op.kind != RSX_IIQ_OP_SENSOR_DEFECTS)
      return RSX_ERR_INVALID_ARG;
    if (op.kind == RSX_IIQ_OP_SENSOR_DEFECTS)
      continue; // (its checks come last: defects_check)
    if (op.kind == RSX_IIQ_OP_FLAT_FIELD ? !op.payload : !op.curves)
      return RSX_ERR_INVALID_ARG;
  }
  for (int i = 0; i < corr->n_ops; ++i) {
    const rsx_iiq_op& op = corr->ops[i];
    if (op.kind == RSX_IIQ_OP_FLAT_FIELD) {
      FlatField F;
      if (int st = ff_parse(op.payload, op.payload_bytes, op.chroma != 0, img->dim_x, img->dim_y, &F))
        return st;
    }
  }
  for (int i = 0; i < corr->n_ops; ++i) {
    const rsx_iiq_op& op = corr->ops[i];
    if (op.kind != RSX_IIQ_OP_FLAT_FIELD || !op.chroma)
      continue;
    const int64_t n = int64_t(corr->cfa_w) * int64_t(corr->cfa_h);
    if (corr->cfa_w <= 0 || corr->cfa_h <= 0 || n > 64)
      return RSX_ERR_INVALID_ARG;
  }
  for (int i = 0; i < corr->n_ops; ++i) {
    const rsx_iiq_op& op = corr->ops[i];
    if (op.kind != RSX_IIQ_OP_FLAT_FIELD || !op.chroma)
      continue;
    for (int k = 0; k < corr->cfa_w * corr->cfa_h; ++k)
      if ((corr->cfa[k] & 1u) == 0 && corr->cfa[k] != 0 && corr->cfa[k] != 2)
        return RSX_ERR_UNSUPPORTED;
  }
  for (int i = 0; i < corr->n_ops; ++i) {
    const rsx_iiq_op& op = corr->ops[i];
    if (op.kind == RSX_IIQ_OP_QUADRANT_CURVES &&
        (op.split_row > uint32_t(img->dim_y) || op.split_col > uint32_t(img->dim_x)))
      return RSX_ERR_INVALID_ARG;
  }
  for (int i = 0; i < corr->n_ops; ++i) {
    const rsx_iiq_op& op = corr->ops[i];
    if (op.kind != RSX_IIQ_OP_FLAT_FIELD)
      continue;
    FlatField F;
    ff_parse(op.payload, op.payload_bytes, op.chroma != 0, img->dim_x, img->dim_y, &F);
    if (ff_table_floats(F) > MAX_TABLE_FLOATS)
      return RSX_ERR_UNSUPPORTED;
  }
  int n_defects = 0;
  for (int i = 0; i < corr->n_ops; ++i)
    if (corr->ops[i].kind == RSX_IIQ_OP_SENSOR_DEFECTS && ++n_defects > 1)
      return RSX_ERR_INVALID_ARG; // ("Second sensor defects entry seen")
  for (int i = 0; i < corr->n_ops; ++i)
    if (corr->ops[i].kind == RSX_IIQ_OP_SENSOR_DEFECTS)
      if (int st = defects_check(corr->ops[i], corr, img))
        return st;
  return RSX_OK;
}

// ------------------------------------------------------------------------------------------
// The fused pass: a job's ops as the kernels (and the host build) hold them, and the work of one
// lane -- up to 8 adjacent pixels of a row through the whole list.
// ------------------------------------------------------------------------------------------
struct OpDev {
  uint32_t kind, black_level;
  uint32_t split_row, split_col;
  uint64_t table_off;   // flat field: first float of the op's row table
  uint64_t ck_off;      // ... and of its start values inside the cells (nck > 0)
  uint64_t curves_off;  // quadrant curves: first u16 of the op's four curves
  uint64_t payload_off; // flat field: first byte of the op's payload
  FlatField F;
};

struct JobDev {
  uint64_t img_offset;
  uint32_t pitch, w, h;
  uint32_t op0, n_ops; // the job's ops in the plan's list
  uint32_t split;      // the job's defects op (n_ops: none): the fused pass stops in front of it
  uint32_t cfa_w, cfa_h;
  uint32_t vpr;        // 8-pixel vectors of a row
  uint8_t sel[64];     // cfa_select of every CFA position
  uint8_t cfa[64];     // ... and its colour
};

// px[0 .. n) are the pixels (row, col0 ..) of job J, through the job's ops first .. end - 1 (none of
// them a defects op); returns the mask of those an op stood on.
RSX_IIQ_FN uint32_t correct_pixels(const JobDev& J, const OpDev* ops, const float* tables,
                                   const uint16_t* curves, uint32_t first, uint32_t end, uint32_t row,
                                   uint32_t col0, uint32_t n, uint16_t (&px)[8]) {
  uint32_t touched = 0;
  for (uint32_t o = first; o < end; ++o) {
    const OpDev& op = ops[J.op0 + o];
    if (op.kind == RSX_IIQ_OP_QUADRANT_CURVES) {
      const uint16_t* rowc = curves + op.curves_off + (row >= op.split_row ? 131072u : 0u);
#if defined(__HIPCC__)
#pragma unroll
#endif
      for (uint32_t i = 0; i < 8; ++i)
        if (i < n)
          px[i] = quad_pixel(px[i], rowc + (col0 + i >= op.split_col ? 65536u : 0u), op.black_level);
      touched |= (1u << n) - 1u;
      continue;
    }
    const FlatField& F = op.F;
    const uint32_t h0 = F.head[0], h1 = F.head[1], h4 = F.head[4];
    if (row < h1 || row - h1 >= F.n_rows)
      continue;
    const uint32_t c = col0 > h0 ? col0 : h0; // the lane's first column inside the area
    if (c >= F.col_end || c >= col0 + n)
      continue;
    const float* trow = tables + op.table_off + size_t(row - h1) * F.tcols * F.planes;
    uint32_t x = (c - h0) / h4 + 1u, k = (c - h0) % h4;
    float m0, s0, m1 = 0.0F, s1 = 0.0F;
    ff_cell(trow, F, x, 0, &m0, &s0);
    if (F.planes == 2u)
      ff_cell(trow, F, x, 1, &m1, &s1);
    uint32_t replay = k;
    if (k >= CK_COLS) { // from the last start value in front of the lane
      const uint32_t j = k / CK_COLS;
      const float* ck = tables + op.ck_off + size_t(row - h1) * ff_ck_row_floats(F) +
                        (size_t(x - 1u) * F.nck + (j - 1u)) * F.planes;
      m0 = ck[0];
      if (F.planes == 2u)
        m1 = ck[1];
      replay = k - j * CK_COLS;
    }
    for (uint32_t j = 0; j < replay; ++j) { // the additions of the columns in front of the lane
      m0 = f_add(m0, s0);
      m1 = f_add(m1, s1);
    }
    const uint32_t rm = F.planes == 2u ? row % J.cfa_w : 0u;
    uint32_t cm = F.planes == 2u ? c % J.cfa_h : 0u;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t i = 0; i < 8; ++i) {
      const uint32_t col = col0 + i;
      if (i >= n || col < h0 || col >= F.col_end)
        continue;
      if (k == h4) { // the next cell
        ++x;
        k = 0;
        ff_cell(trow, F, x, 0, &m0, &s0);
        if (F.planes == 2u)
          ff_cell(trow, F, x, 1, &m1, &s1);
      }
      const uint32_t sel = F.planes == 2u ? J.sel[rm + cm * J.cfa_w] : 0u;
      if (sel < 2u) {
        px[i] = ff_pixel(px[i], sel ? m1 : m0);
        touched |= 1u << i;
      }
      m0 = f_add(m0, s0);
      m1 = f_add(m1, s1);
      ++k;
      cm = cm + 1u == J.cfa_h ? 0u : cm + 1u;
    }
  }
  return touched;
}

} // namespace rsx_iiq
