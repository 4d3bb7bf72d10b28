// What DngDecoder does to the pixels behind the tile decode (include/rsx.h section 4d), shared by
// the kernel of rsx_dng_post.hip and by a host build (rsx_dng_post_host.cpp): the parse of an
// OpcodeList1 entry with every check of DngOpcodes::DngOpcodes, the opcode constructors and their
// setup() (common/DngOpcodes.cpp), the dithering table of TableLookUp::setTable
// (common/TableLookUp.cpp:68-84), and the lane that takes 8 samples of a row (4 of an F32 image)
// through the list and through RawImageDataU16::doLookup (common/RawImageDataU16.cpp:488-519).
//
// The generator of doLookup.  v' = 15700 (v & 65535) + (v >> 16) is a lag-1 multiply-with-carry:
// v' = v 15700 (mod m), m = 15700 * 2^16 - 1 (rsx_dither_dev.h has the argument for seeds below
// m).  doLookup STEPS, THEN USES, so sample x of a row sees the state x + 1 steps behind the row's
// seed (dim.x + 13 y) ^ 0x45694584.  That seed is not below m: its high half is 0x4560..0x456F
// (validate() holds dim.x + 13 dim.y below 2^20), so it lies in (m, 2 m).  One step from any v
// gives v' = 15700 l + c (l the low, c the high half), and v' >= m exactly when l == 65535 and
// c >= 15699.  From a seed of this kind (c >= 0x4560 > 15699) the state after ONE step therefore
// is a proper residue below m unless the seed's low half is 65535, when it is m + (c - 15699) --
// congruent to, but not equal to, (seed mod m) 15700 mod m; (dim.x + 13 y) mod 2^16 == 0xBA7B is
// such a row (7998 x 3057 is enough).  After TWO steps the state is below m in either case (the
// state in between has c == 15700 and l <= 15700), and from a state below m the only way to
// reach m again is from m itself, which no seed of this kind is congruent to (m's high half is
// 15699).  So: the state n >= 2 steps behind the seed is ((seed mod m) 15700^n) mod m, and the
// lane that owns sample 0 starts from the unreduced seed and steps it as the reference does.
// tests/test_dng_post_dither_model.py holds both statements against the plain loop.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "rsx.h"

#if defined(__HIPCC__)
#define RSX_DP_FN __host__ __device__ __forceinline__
#else
#define RSX_DP_FN inline
#endif

namespace rsx_dngpost {

constexpr uint64_t DITHER_M = 15700ull * 65536ull - 1ull;

enum OpKind : uint32_t {
  OP_TABLE = 0,     // MapTable (7), MapPolynomial (8): 65536 uint16 at data_off
  OP_OFFSET_ROW,    // DeltaPerRow (10)
  OP_OFFSET_COL,    // DeltaPerColumn (11)
  OP_SCALE_ROW,     // ScalePerRow (12)
  OP_SCALE_COL,     // ScalePerColumn (13)
  OP_BAD_CONSTANT   // FixBadPixelsConstant (4): the ROI is the crop it met
};

// A pixel opcode as a lane meets it: the ROI in pixels of the UNCROPPED image (the crop the opcode
// met is added), rows [y0, y1), pixels [x0, x1).
struct OpDev {
  uint32_t kind;
  uint32_t y0, y1, x0, x1;
  uint32_t first_plane, planes, row_pitch, col_pitch;
  uint32_t data_off; // OP_TABLE: uint16 index into the tables; deltas: index into the deltas
  uint32_t value;    // OP_BAD_CONSTANT
  uint32_t reserved;
};

struct JobDev {
  uint64_t img_offset;
  uint64_t bad_base;    // the job's first entry in the plan's hit buffer
  uint32_t bad_cap;     // entries the job's hit buffer holds
  uint32_t pitch;       // bytes
  uint32_t ws;          // samples of an uncropped row: dim_x * cpp
  uint32_t w_px, h;     // uncropped dim
  uint32_t cpp;
  uint32_t vpr;         // lanes a row: ceil(ws / 8) (u16) or ceil(ws / 4) (F32)
  uint32_t op0, n_ops;
  uint32_t lut_on;      // the dithering table stands at lut_off
  uint32_t lut_off;     // uint32 index into the look-up tables
  uint32_t has_bad;     // some op is OP_BAD_CONSTANT
  uint32_t is_f32;
  uint32_t job;         // its number in the plan (the hit counter)
  uint32_t reserved[2];
};

RSX_DP_FN uint32_t clamp16(int32_t v) { return v < 0 ? 0u : v > 65535 ? 65535u : uint32_t(v); }

RSX_DP_FN uint32_t dither_step(uint32_t v) { return 15700u * (v & 65535u) + (v >> 16); }

// One lane: N = 8 uint16 samples (4 floats) of row `row` from sample s0, `n` of them inside the
// row.  px holds the samples' bits.  Returns the mask of the samples that were written; hits[0] /
// hits[1] receive, per OP_BAD_CONSTANT op j of the job (j < 8 / j >= 8), the 8-bit mask of the
// samples that equal its constant at that point of the list.
template <bool F32>
RSX_DP_FN uint32_t lane(const JobDev& J, const OpDev* ops, const uint16_t* tables,
                        const int32_t* deltas, const uint32_t* luts, const uint32_t* pw,
                        uint32_t row, uint32_t s0, uint32_t n, uint32_t* px, uint64_t* hits) {
  constexpr uint32_t N = F32 ? 4u : 8u;
  const uint32_t cpp = J.cpp;
  const uint32_t px0 = cpp == 1u ? s0 : cpp == 2u ? s0 >> 1 : cpp == 3u ? s0 / 3u : s0 >> 2;
  const uint32_t c0 = s0 - px0 * cpp;
  uint32_t touched = 0;
  for (uint32_t o = 0; o < J.n_ops; ++o) {
    const OpDev& op = ops[J.op0 + o];
    if (row < op.y0 || row >= op.y1)
      continue;
    const uint32_t ry = row - op.y0;
    uint32_t yi;
    if (op.row_pitch == 1u) {
      yi = ry;
    } else if (op.row_pitch == 2u) {
      if (ry & 1u)
        continue;
      yi = ry >> 1;
    } else {
      yi = ry / op.row_pitch;
      if (yi * op.row_pitch != ry)
        continue;
    }
    if (s0 + n <= op.x0 * cpp || s0 >= op.x1 * cpp)
      continue;
    if (op.kind == OP_BAD_CONSTANT) {
      // (cpp == 1: a sample is a pixel)
      if (!F32) {
        uint64_t m = 0;
        for (uint32_t i = 0; i < N; ++i)
          if (i < n && s0 + i >= op.x0 && s0 + i < op.x1 && px[i] == op.value)
            m |= 1ull << i;
        hits[o >> 3] |= m << (8u * (o & 7u));
      }
      continue;
    }
    // the pixel the lane's first sample belongs to, relative to the ROI: rel; from rel == 0 on
    // xi = rel / col_pitch and xr = rel % col_pitch, kept by counting
    int32_t rel = int32_t(px0) - int32_t(op.x0);
    const int32_t width = int32_t(op.x1 - op.x0);
    const uint32_t cp = op.col_pitch;
    uint32_t xi = 0, xr = 0;
    if (rel > 0) {
      if (cp == 1u) {
        xi = uint32_t(rel);
      } else if (cp == 2u) {
        xi = uint32_t(rel) >> 1;
        xr = uint32_t(rel) & 1u;
      } else {
        xi = uint32_t(rel) / cp;
        xr = uint32_t(rel) - xi * cp;
      }
    }
    const bool by_row = op.kind == OP_OFFSET_ROW || op.kind == OP_SCALE_ROW;
    const int32_t drow = by_row ? deltas[op.data_off + yi] : 0;
    uint32_t c = c0;
    for (uint32_t i = 0; i < N; ++i) {
      if (i < n && rel >= 0 && rel < width && xr == 0u && c >= op.first_plane &&
          c < op.first_plane + op.planes) {
        const int32_t d = by_row ? drow : op.kind == OP_TABLE ? 0 : deltas[op.data_off + xi];
        if (F32) {
          float f, v;
          __builtin_memcpy(&f, &d, 4);
          __builtin_memcpy(&v, &px[i], 4);
          const float r = (op.kind == OP_OFFSET_ROW || op.kind == OP_OFFSET_COL) ? f + v : f * v;
          __builtin_memcpy(&px[i], &r, 4);
        } else if (op.kind == OP_TABLE) {
          px[i] = tables[size_t(op.data_off) + px[i]];
        } else if (op.kind == OP_OFFSET_ROW || op.kind == OP_OFFSET_COL) {
          px[i] = clamp16(d + int32_t(px[i]));
        } else {
          // (d <= (2^31 - 1 - 512) / 65535: the product and the rounding fit an int)
          px[i] = clamp16((d * int32_t(px[i]) + 512) >> 10);
        }
        touched |= 1u << i;
      }
      if (++c == cpp) {
        c = 0;
        ++rel;
        if (rel > 0 && ++xr == cp) {
          xr = 0;
          ++xi;
        }
      }
    }
  }
  if (!F32 && J.lut_on) { // (every row of the uncropped image)
    const uint32_t* lut = luts + J.lut_off;
    const uint32_t seed = (J.w_px + 13u * row) ^ 0x45694584u;
    uint32_t r = seed; // (the lane of sample 0 steps the seed itself: see the head of this file)
    if (s0 != 0u) {
      const uint64_t reduced = seed >= DITHER_M ? seed - DITHER_M : seed;
      r = uint32_t(reduced * pw[s0 >> 3] % DITHER_M);
    }
    for (uint32_t i = 0; i < N; ++i) {
      if (i >= n)
        break;
      r = dither_step(r);
      const uint32_t e = lut[px[i] & 0xFFFFu];
      const uint32_t pix = (e & 0xFFFFu) + (((e >> 16) * (r & 2047u) + 1024u) >> 12);
      px[i] = pix > 65535u ? 65535u : pix;
      touched |= 1u << i;
    }
  }
  return touched;
}

} // namespace rsx_dngpost

// ---------------------------------------------------------------------------------------
// host only: the parse, the verdicts, the tables
// ---------------------------------------------------------------------------------------
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace rsx_dngpost {

struct Rect {
  int32_t x, y, w, h;
};

// one entry of the list as applyOpCodes walks it
struct Item {
  uint32_t code;
  int32_t pixel_op;   // index into Parsed::all_ops, or -1
  uint32_t fixed_off; // FixBadPixelsList: its positions in Parsed::fixed
  uint32_t fixed_n;
  Rect crop;          // the crop the opcode meets
  Rect roi;           // TrimBounds
  uint32_t delta_off, delta_n;
  float f2i;          // 65535.0F / 1024.0F
};

struct Parsed {
  int32_t list_status = RSX_OK, list_reason = RSX_DNG_POST_REASON_NONE;
  int32_t n_opcodes = 0, n_applied = 0;
  Rect crop{};                  // the crop behind the applied part of the list
  std::vector<Item> items;      // every opcode of a list that constructed
  std::vector<OpDev> all_ops;   // pixel opcodes, list order
  std::vector<OpDev> ops;       // those among the first n_applied
  std::vector<int32_t> op_item; // ops[j] is items[op_item[j]]
  std::vector<uint16_t> tables; // 65536 a table opcode
  std::vector<float> deltas_f;  // as the file has them
  std::vector<int32_t> deltas;  // as the lane takes them: int(f2i * f), or the float's bits (F32)
  std::vector<uint32_t> fixed;  // FixBadPixelsList positions, file order
  std::vector<uint32_t> lut;    // base | delta << 16, 65536 entries; empty: no look-up
};

// a big-endian ByteStream: every read checks its bounds (IOException in the reference)
struct Reader {
  const uint8_t* p;
  uint64_t size, pos = 0;
  bool io = false; // a read went out of bounds
  Reader(const uint8_t* d, uint64_t n) : p(d), size(n) {}
  bool check(uint64_t n) {
    if (io || n > size - pos)
      io = true;
    return !io;
  }
  bool check(uint64_t nmemb, uint64_t sz) {
    if (sz && nmemb > 0xFFFFFFFFull / sz)
      io = true;
    return !io && check(uint32_t(nmemb * sz));
  }
  void skip(uint64_t n) {
    if (check(n))
      pos += n;
  }
  uint32_t u32() {
    if (!check(4))
      return 0;
    const uint8_t* q = p + pos;
    pos += 4;
    return uint32_t(q[0]) << 24 | uint32_t(q[1]) << 16 | uint32_t(q[2]) << 8 | q[3];
  }
  uint32_t u16() {
    if (!check(2))
      return 0;
    const uint8_t* q = p + pos;
    pos += 2;
    return uint32_t(q[0]) << 8 | q[1];
  }
  float f32() {
    const uint32_t b = u32();
    float f;
    std::memcpy(&f, &b, 4);
    return f;
  }
  double f64() {
    const uint64_t hi = u32(), lo = u32();
    const uint64_t b = hi << 32 | lo;
    double d;
    std::memcpy(&d, &b, 8);
    return d;
  }
  Reader sub(uint64_t n) {
    if (!check(n))
      return Reader(p, 0);
    Reader r(p + pos, n);
    pos += n;
    return r;
  }
};

// ROIOpcode's constructor: top, left, bottom, right against {0, 0, dim} inclusive.  0: fine,
// else the reason.
inline int read_roi(Reader& bs, int32_t dim_w, int32_t dim_h, Rect* roi) {
  const int32_t top = int32_t(bs.u32()), left = int32_t(bs.u32());
  const int32_t bottom = int32_t(bs.u32()), right = int32_t(bs.u32());
  if (bs.io)
    return 0;
  auto inside = [&](int32_t x, int32_t y) { return x >= 0 && y >= 0 && x <= dim_w && y <= dim_h; };
  if (!(inside(left, top) && inside(right, bottom) && right >= left && bottom >= top))
    return RSX_DNG_POST_REASON_ROI;
  *roi = Rect{left, top, right - left, bottom - top};
  return 0;
}

// The dithering table of TableLookUp::setTable(): entry i = base | delta << 16.
inline void build_lut(const uint16_t* table, uint32_t n, std::vector<uint32_t>* out) {
  out->assign(65536, 0u);
  for (uint32_t i = 0; i < n; ++i) {
    const int center = table[i];
    int lower = i > 0 ? table[i - 1] : center;
    int upper = i < n - 1 ? table[i + 1] : center;
    lower = std::min(lower, center);
    upper = std::max(upper, center);
    const int delta = upper - lower;
    (*out)[i] = clamp16(center - ((upper - lower + 2) / 4)) | uint32_t(delta) << 16;
  }
  for (uint32_t i = n; i < 65536; ++i)
    (*out)[i] = table[n - 1];
}

// The checks on the image and the descriptor that do not depend on the list.
inline int check_args(const rsx_dng_post_desc* d, const rsx_image* img) {
  if (!d || !img)
    return RSX_ERR_INVALID_ARG;
  if (img->cpp < 1 || img->cpp > 4 || img->dim_x <= 0 || img->dim_y <= 0)
    return RSX_ERR_INVALID_ARG;
  const uint64_t bpc = d->is_f32 ? 4u : 2u;
  if (uint64_t(img->pitch_bytes) < uint64_t(img->dim_x) * uint64_t(img->cpp) * bpc ||
      img->pitch_bytes % bpc != 0)
    return RSX_ERR_INVALID_ARG;
  if (d->crop_x < 0 || d->crop_y < 0 || d->crop_w <= 0 || d->crop_h <= 0 ||
      int64_t(d->crop_x) + d->crop_w > img->dim_x || int64_t(d->crop_y) + d->crop_h > img->dim_y)
    return RSX_ERR_INVALID_ARG;
  if ((d->opcodes_bytes != 0 && !d->opcodes) || (d->table_count != 0 && !d->table) ||
      d->table_count > 65536)
    return RSX_ERR_INVALID_ARG;
  if (d->is_f32 && d->table_count != 0)
    return RSX_ERR_UNSUPPORTED; // (the reference logs "not implemented" from a worker)
  // hit entries hold 24 bits a coordinate; the seeds' high half (see the head of this file)
  if (uint64_t(img->dim_x) * uint64_t(img->cpp) >= (1u << 24) || img->dim_y >= (1 << 24) ||
      uint64_t(img->dim_x) + 13ull * uint64_t(img->dim_y) >= (1u << 20))
    return RSX_ERR_UNSUPPORTED;
  return RSX_OK;
}

// DngOpcodes::DngOpcodes and applyOpCodes' setup()s.  RSX_OK, RSX_ERR_IO (an IOException: the file
// fails) or what check_args gives; a RawDecoderException is P->list_status / list_reason.
inline int parse(const rsx_dng_post_desc* d, const rsx_image* img, Parsed* P) {
  if (int st = check_args(d, img))
    return st;
  const int32_t cpp = img->cpp;
  const Rect crop0{d->crop_x, d->crop_y, d->crop_w, d->crop_h};
  P->crop = crop0;
  bool constructed = d->opcodes_bytes != 0;
  if (constructed) {
    Reader bs(d->opcodes, d->opcodes_bytes);
    const uint32_t count = bs.u32();
    const uint64_t orig = bs.pos;
    for (uint32_t i = 0; i < count && !bs.io; ++i) {
      bs.skip(12);
      const uint32_t size = bs.u32();
      bs.skip(size);
    }
    if (bs.io)
      return RSX_ERR_IO;
    bs.pos = orig;
    Rect sub = crop0; // integrated_subimg
    int reason = 0;
    for (uint32_t i = 0; i < count && !reason; ++i) {
      const uint32_t code = bs.u32();
      bs.skip(4);
      const uint32_t flags = bs.u32();
      const uint32_t size = bs.u32();
      Reader ob = bs.sub(size);
      if (bs.io)
        return RSX_ERR_IO;
      Item it{};
      it.code = code;
      it.pixel_op = -1;
      it.crop = sub;
      if (code == 0 || code > 13) {
        reason = RSX_DNG_POST_REASON_UNKNOWN_OPCODE;
        break;
      }
      if (code == 1 || code == 2 || code == 3 || code == 9) {
        if (!(flags & 1u)) {
          reason = RSX_DNG_POST_REASON_UNSUPPORTED_OPCODE;
          break;
        }
        // (an optional one: its bytes stay unread, and "Inconsistent length" follows unless
        // the opcode is empty)
      } else if (code == 4) {
        OpDev op{};
        op.kind = OP_BAD_CONSTANT;
        op.value = ob.u32();
        ob.u32();
        op.y0 = uint32_t(sub.y);
        op.y1 = uint32_t(sub.y + sub.h);
        op.x0 = uint32_t(sub.x);
        op.x1 = uint32_t(sub.x + sub.w);
        op.row_pitch = op.col_pitch = 1;
        op.planes = 1;
        it.pixel_op = int32_t(P->all_ops.size());
        P->all_ops.push_back(op);
      } else if (code == 5) {
        ob.u32();
        const uint32_t n_points = ob.u32(), n_rects = ob.u32();
        const uint64_t at = ob.pos;
        if (ob.check(n_points, 8))
          ob.pos += uint64_t(n_points) * 8;
        if (ob.check(n_rects, 16))
          ob.pos += uint64_t(n_rects) * 16;
        if (ob.io)
          return RSX_ERR_IO;
        ob.pos = at;
        it.fixed_off = uint32_t(P->fixed.size());
        for (uint32_t k = 0; k < n_points && !reason; ++k) {
          const int32_t y = int32_t(ob.u32()), x = int32_t(ob.u32());
          if (!(x >= 0 && y >= 0 && x < img->dim_x && y < img->dim_y))
            reason = RSX_DNG_POST_REASON_BAD_POINT;
          else
            P->fixed.push_back(uint32_t(y) << 16 | uint32_t(x));
        }
        for (uint32_t k = 0; k < n_rects && !reason; ++k) {
          Rect r{};
          reason = read_roi(ob, img->dim_x, img->dim_y, &r);
          if (reason)
            break;
          // (the total is bounded by the caller's image only: refuse what no list can mean)
          if (P->fixed.size() + uint64_t(r.w) * uint64_t(r.h) > (1u << 26))
            return RSX_ERR_UNSUPPORTED;
          for (int32_t y = 0; y < r.h; ++y)
            for (int32_t x = 0; x < r.w; ++x)
              P->fixed.push_back(uint32_t(r.y + y) << 16 | uint32_t(r.x + x));
        }
        it.fixed_n = uint32_t(P->fixed.size()) - it.fixed_off;
      } else if (code == 6) {
        reason = read_roi(ob, sub.w, sub.h, &it.roi);
        if (!reason && !ob.io) {
          sub.x += it.roi.x;
          sub.y += it.roi.y;
          sub.w = it.roi.w;
          sub.h = it.roi.h;
        }
      } else {
        // PixelOpcode
        Rect roi{};
        reason = read_roi(ob, sub.w, sub.h, &roi);
        OpDev op{};
        if (!reason) {
          op.first_plane = ob.u32();
          op.planes = ob.u32();
          if (!ob.io && (op.planes == 0 || op.first_plane > uint32_t(cpp) ||
                         op.planes > uint32_t(cpp) || op.first_plane + op.planes > uint32_t(cpp)))
            reason = RSX_DNG_POST_REASON_PLANES;
        }
        if (!reason) {
          op.row_pitch = ob.u32();
          op.col_pitch = ob.u32();
          if (!ob.io && (op.row_pitch < 1 || op.row_pitch > uint32_t(roi.h) || op.col_pitch < 1 ||
                         op.col_pitch > uint32_t(roi.w)))
            reason = RSX_DNG_POST_REASON_PITCH;
        }
        if (!reason && !ob.io) {
          op.y0 = uint32_t(sub.y + roi.y);
          op.y1 = op.y0 + uint32_t(roi.h);
          op.x0 = uint32_t(sub.x + roi.x);
          op.x1 = op.x0 + uint32_t(roi.w);
          if (code == 7 || code == 8) {
            op.kind = OP_TABLE;
            if (P->tables.size() / 65536 >= RSX_DNG_POST_MAX_PIXEL_OPS)
              return RSX_ERR_UNSUPPORTED; // (more tables than a list this core takes can hold)
            const size_t base = P->tables.size();
            if (code == 7) {
              const uint32_t n = ob.u32();
              if (!ob.io && (n == 0 || n > 65536))
                reason = RSX_DNG_POST_REASON_TABLE_SIZE;
              if (!reason && !ob.io) {
                P->tables.resize(base + 65536);
                for (uint32_t k = 0; k < n; ++k)
                  P->tables[base + k] = uint16_t(ob.u16());
                if (!ob.io)
                  for (uint32_t k = n; k < 65536; ++k)
                    P->tables[base + k] = P->tables[base + n - 1];
              }
            } else {
              const uint64_t n = uint64_t(ob.u32()) + 1u;
              ob.check(uint32_t(8u * n));
              if (!ob.io && n > 9)
                reason = RSX_DNG_POST_REASON_POLY_DEGREE;
              if (!reason && !ob.io) {
                double poly[9];
                for (uint64_t k = 0; k < n; ++k)
                  poly[k] = ob.f64();
                P->tables.resize(base + 65536);
                for (uint32_t k = 0; k < 65536; ++k) {
                  double val = poly[0];
                  for (uint64_t j = 1; j < n; ++j)
                    val += poly[j] * std::pow(double(k) / 65536.0, double(j));
                  const double s = val * 65535.5;
                  // (a NaN: the reference's conversion is undefined; 0 here)
                  P->tables[base + k] = !(s == s) ? 0 : uint16_t(s < 0.0 ? 0.0 : s > 65535.0 ? 65535.0 : s);
                }
              }
            }
            op.data_off = uint32_t(base);
          } else {
            const bool by_col = code == 11 || code == 13;
            op.kind = code == 10 ? OP_OFFSET_ROW : code == 11 ? OP_OFFSET_COL
                      : code == 12 ? OP_SCALE_ROW : OP_SCALE_COL;
            const uint32_t n = ob.u32();
            ob.check(n, 4);
            if (!ob.io) {
              const uint64_t extent = by_col ? uint64_t(roi.w) : uint64_t(roi.h);
              const uint64_t pitch = by_col ? op.col_pitch : op.row_pitch;
              if ((extent + pitch - 1) / pitch != n)
                reason = RSX_DNG_POST_REASON_DELTA_COUNT;
            }
            if (!reason && !ob.io) {
              it.delta_off = op.data_off = uint32_t(P->deltas_f.size());
              it.delta_n = n;
              it.f2i = code <= 11 ? 65535.0F : 1024.0F;
              for (uint32_t k = 0; k < n && !reason; ++k) {
                const float f = ob.f32();
                if (!std::isfinite(f))
                  reason = RSX_DNG_POST_REASON_DELTA_NOT_FINITE;
                P->deltas_f.push_back(f);
              }
            }
          }
          it.pixel_op = int32_t(P->all_ops.size());
          P->all_ops.push_back(op);
        }
      }
      if (ob.io)
        return RSX_ERR_IO;
      if (!reason && ob.pos != ob.size)
        reason = RSX_DNG_POST_REASON_INCONSISTENT_LENGTH;
      if (!reason)
        P->items.push_back(it);
    }
    if (reason) {
      P->list_status = RSX_ERR_INVALID_ARG;
      P->list_reason = reason;
      P->items.clear();
      P->all_ops.clear();
      P->fixed.clear();
      constructed = false;
    } else {
      P->n_opcodes = int32_t(count);
    }
  }
  // applyOpCodes: setup(), then apply(), opcode by opcode
  P->deltas.resize(P->deltas_f.size());
  if (constructed) {
    for (size_t i = 0; i < P->items.size(); ++i) {
      const Item& it = P->items[i];
      int reason = 0;
      if (it.code == 4) {
        if (d->is_f32)
          reason = RSX_DNG_POST_REASON_SETUP_NOT_U16;
        else if (cpp > 1)
          reason = RSX_DNG_POST_REASON_SETUP_CPP;
      } else if (it.code == 7 || it.code == 8) {
        if (d->is_f32)
          reason = RSX_DNG_POST_REASON_SETUP_NOT_U16;
      } else if (it.code >= 10 && it.code <= 13) {
        const bool offset = it.code <= 11;
        const double lim = offset ? 65535.0 / double(it.f2i)
                                  : (double(2147483647 - 512) / 65535.0) / double(it.f2i);
        for (uint32_t k = 0; k < it.delta_n && !reason; ++k) {
          const float f = P->deltas_f[it.delta_off + k];
          if (d->is_f32) {
            std::memcpy(&P->deltas[it.delta_off + k], &f, 4);
            continue;
          }
          const bool ok = offset ? double(std::fabs(f)) <= lim : (f >= 0.0F && double(f) <= lim);
          if (!ok)
            reason = RSX_DNG_POST_REASON_SETUP_DELTA_RANGE;
          else
            P->deltas[it.delta_off + k] = int32_t(it.f2i * f);
        }
      } else if (it.code == 6) {
        if (it.roi.w <= 0 || it.roi.h <= 0)
          reason = RSX_DNG_POST_REASON_TRIM_EMPTY; // (subFrame: "No positive crop area")
      }
      if (reason) {
        P->list_status = RSX_ERR_INVALID_ARG;
        P->list_reason = reason;
        break;
      }
      if (it.code == 6)
        P->crop = Rect{it.crop.x + it.roi.x, it.crop.y + it.roi.y, it.roi.w, it.roi.h};
      if (it.pixel_op >= 0) {
        P->ops.push_back(P->all_ops[size_t(it.pixel_op)]);
        P->op_item.push_back(int32_t(i));
      }
      P->n_applied = int32_t(i) + 1;
    }
  }
  if (P->ops.size() > RSX_DNG_POST_MAX_PIXEL_OPS)
    return RSX_ERR_UNSUPPORTED;
  if (d->table_count != 0) {
    build_lut(d->table, d->table_count, &P->lut);
    // (the look-up covers every row of the uncropped image: APPLY_LOOKUP carries
    // RawImageWorkerTask::FULL_IMAGE, so startWorker takes uncropped_dim.y whatever `cropped`
    // says, common/RawImage.cpp:270-279)
  }
  return RSX_OK;
}

// a hit as the lanes record it: the op's number in the job, and the pixel relative to the crop
RSX_DP_FN uint64_t hit_entry(uint32_t op, uint32_t rel_row, uint32_t rel_col) {
  return uint64_t(op) << 48 | uint64_t(rel_row) << 24 | rel_col;
}

// What mRaw->mBadPixelPositions gains, in the reference's final order: `hits` are the lanes'
// entries in any order (sorted here).
inline void compose_bad(const Parsed& P, std::vector<uint64_t>& hits, std::vector<uint32_t>* out) {
  std::sort(hits.begin(), hits.end());
  out->clear();
  size_t at = 0;
  int32_t j = 0; // number among the applied pixel ops
  for (int32_t i = 0; i < P.n_applied; ++i) {
    const Item& it = P.items[size_t(i)];
    if (it.code == 5) {
      out->insert(out->begin(), P.fixed.begin() + it.fixed_off,
                  P.fixed.begin() + it.fixed_off + it.fixed_n);
    } else if (it.code == 4) {
      const uint32_t offset = uint32_t(it.crop.x) | uint32_t(it.crop.y) << 16;
      for (; at < hits.size() && int32_t(hits[at] >> 48) == j; ++at)
        out->push_back(offset + (uint32_t(hits[at] >> 24 & 0xFFFFFFu) << 16 |
                                 uint32_t(hits[at] & 0xFFFFFFu)));
    }
    if (it.pixel_op >= 0)
      ++j;
  }
}

// the positions that need no pixel: FixBadPixelsList entries of the applied part
inline uint64_t fixed_count(const Parsed& P) {
  uint64_t n = 0;
  for (int32_t i = 0; i < P.n_applied; ++i)
    n += P.items[size_t(i)].code == 5 ? P.items[size_t(i)].fixed_n : 0u;
  return n;
}

inline void fill_result(const Parsed& P, uint64_t n_bad, rsx_dng_post_result* r) {
  if (!r)
    return;
  r->list_status = P.list_status;
  r->list_reason = P.list_reason;
  r->n_opcodes = P.n_opcodes;
  r->n_applied = P.n_applied;
  r->crop_x = P.crop.x;
  r->crop_y = P.crop.y;
  r->crop_w = P.crop.w;
  r->crop_h = P.crop.h;
  r->n_bad = n_bad;
}

// rsx_dng_post_validate: the verdict, the crop and the positions that need no pixel
inline int validate(const rsx_dng_post_desc* desc, const rsx_image* img, rsx_dng_post_result* result,
                    uint32_t* bad, uint32_t bad_cap) {
  Parsed P;
  if (int st = parse(desc, img, &P))
    return st;
  std::vector<uint32_t> fixed;
  for (int32_t i = 0; i < P.n_applied; ++i) {
    const Item& it = P.items[size_t(i)];
    if (it.code == 5)
      fixed.insert(fixed.begin(), P.fixed.begin() + it.fixed_off,
                   P.fixed.begin() + it.fixed_off + it.fixed_n);
  }
  fill_result(P, fixed.size(), result);
  if (fixed.size() > bad_cap)
    return RSX_ERR_UNSUPPORTED;
  if (!fixed.empty() && bad)
    std::memcpy(bad, fixed.data(), fixed.size() * sizeof(uint32_t));
  return RSX_OK;
}

// [k] = 15700^(8 k) mod m, k < n
inline std::vector<uint32_t> dither_powers8(uint32_t n) {
  std::vector<uint32_t> p(n);
  uint64_t step = 1;
  for (int i = 0; i < 8; ++i)
    step = step * 15700u % DITHER_M;
  uint64_t x = 1;
  for (uint32_t k = 0; k < n; ++k) {
    p[k] = uint32_t(x);
    x = x * step % DITHER_M;
  }
  return p;
}

inline void fill_job(const rsx_dng_post_desc* d, const rsx_image* img, const Parsed& P, JobDev* J) {
  std::memset(J, 0, sizeof *J);
  J->pitch = img->pitch_bytes;
  J->cpp = uint32_t(img->cpp);
  J->w_px = uint32_t(img->dim_x);
  J->h = uint32_t(img->dim_y);
  J->ws = J->w_px * J->cpp;
  J->is_f32 = d->is_f32 ? 1u : 0u;
  J->vpr = d->is_f32 ? (J->ws + 3u) / 4u : (J->ws + 7u) / 8u;
  J->n_ops = uint32_t(P.ops.size());
  J->lut_on = P.lut.empty() ? 0u : 1u;
  for (const OpDev& op : P.ops)
    J->has_bad |= op.kind == OP_BAD_CONSTANT ? 1u : 0u;
}

} // namespace rsx_dngpost
