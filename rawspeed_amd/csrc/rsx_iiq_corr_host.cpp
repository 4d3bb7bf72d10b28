// rsx_iiq_corr_core.h as host C++ (librsx_iiq_corr_host.so): the same validation, row walk and
// fused 8-pixel lane as the kernels of rsx_iiq_corr.hip, driven by loops that mirror the two
// kernels -- every (x, plane) walks its rows into the table, every (row, cell, plane) of a wide
// cell its start values, then every vector of every row goes through the whole list -- so that the
// test cases meet the code on the CPU first.  A defects op ends a run of the list: its bad columns
// are walked in file order, one after the other, as the reference does (the device sorts them into
// levels), and the ops behind it are the next run.  Compiled with
// -ffp-contract=off.  With -DRSX_IIQ_CORR_HOST_MAIN the file is a program (built with
// AddressSanitizer and UBSan where g++ has them) that runs the validation cases and the
// clipped-area cases against a pass-per-entry restatement with running sums.
#include "rsx_iiq_corr_core.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace rsx_iiq;

extern "C" int rsx_iiq_corr_host_validate(const rsx_iiq_corr* corr, const rsx_image* img) {
  return validate(corr, img);
}

extern "C" int rsx_iiq_corr_host_defect_positions(const uint8_t* payload, uint32_t payload_bytes,
                                                  int32_t dim_x, uint32_t* out, uint32_t cap,
                                                  uint32_t* n) {
  return defect_positions(payload, payload_bytes, dim_x, out, cap, n);
}

// the levels of a defects payload as the device plan orders them: cols[0 .. return value), the
// end of each level in level_end[0 .. *n_levels) (both of `cap` entries)
extern "C" uint32_t rsx_iiq_corr_host_defect_levels(const uint8_t* payload, uint32_t payload_bytes,
                                                    int32_t dim_x, int32_t dim_y, uint32_t* cols,
                                                    uint32_t* level_end, uint32_t cap,
                                                    uint32_t* n_levels) {
  std::vector<uint32_t> c, e;
  defects_levels(payload, payload_bytes, dim_x, dim_y, &c, &e);
  for (size_t i = 0; i < c.size() && i < cap; ++i)
    cols[i] = c[i];
  for (size_t i = 0; i < e.size() && i < cap; ++i)
    level_end[i] = e[i];
  *n_levels = uint32_t(e.size());
  return uint32_t(c.size());
}

// the bad columns of a checked defects op, in file order, in place
static void apply_defects(const rsx_iiq_op& op, const JobDev& J, const rsx_iiq_corr* corr,
                          uint8_t* img) {
  for (uint32_t i = 0; i < op.payload_bytes / 8u; ++i) {
    const DefectRecord r = defect_record(op.payload, i);
    if (!defect_is_column(r, int32_t(J.w), int32_t(J.h)))
      continue;
    for (uint32_t row = 2; row + 2u < J.h; ++row) {
      const uint32_t colour = corr->cfa[r.col % J.cfa_w + (row % J.cfa_h) * J.cfa_w];
      *reinterpret_cast<uint16_t*>(img + size_t(row) * J.pitch + 2u * size_t(r.col)) =
          bad_column_pixel(img, J.pitch, row, r.col, colour);
    }
  }
}

// rsx_iiq_correct on the host: img->data is corrected in place (untouched unless RSX_OK)
extern "C" int rsx_iiq_corr_host_apply(const rsx_iiq_corr* corr, const rsx_image* img) {
  if (int st = validate(corr, img))
    return st;
  if (!img->data || img->pitch_bytes % 2 != 0)
    return RSX_ERR_INVALID_ARG;
  JobDev J;
  std::memset(&J, 0, sizeof J);
  J.pitch = img->pitch_bytes;
  J.w = uint32_t(img->dim_x);
  J.h = uint32_t(img->dim_y);
  J.n_ops = uint32_t(corr->n_ops);
  J.cfa_w = uint32_t(corr->cfa_w);
  J.cfa_h = uint32_t(corr->cfa_h);
  J.vpr = (J.w + 7u) / 8u;
  for (uint32_t k = 0; k < 64 && k < J.cfa_w * J.cfa_h; ++k)
    J.sel[k] = cfa_select(corr->cfa[k]);
  std::vector<OpDev> ops(J.n_ops);
  std::vector<float> tables;
  for (uint32_t o = 0; o < J.n_ops; ++o) {
    const rsx_iiq_op& in = corr->ops[o];
    OpDev& op = ops[o];
    std::memset(&op, 0, sizeof op);
    op.kind = uint32_t(in.kind);
    if (in.kind == RSX_IIQ_OP_QUADRANT_CURVES) {
      op.black_level = in.black_level;
      op.split_row = in.split_row;
      op.split_col = in.split_col;
      continue;
    }
    if (in.kind == RSX_IIQ_OP_SENSOR_DEFECTS)
      continue;
    ff_parse(in.payload, in.payload_bytes, in.chroma != 0, img->dim_x, img->dim_y, &op.F);
    op.table_off = tables.size();
    tables.resize(tables.size() + size_t(ff_table_floats(op.F)));
    op.ck_off = tables.size();
    tables.resize(tables.size() + size_t(ff_ck_floats(op.F)));
    if (op.F.n_rows)
      for (uint32_t x = 0; x < op.F.tcols; ++x)
        for (uint32_t p = 0; p < op.F.planes; ++p)
          ff_walk_rows(in.payload, op.F, x, p, tables.data() + op.table_off);
    if (op.F.n_rows && op.F.nck)
      for (uint32_t r = 0; r < op.F.n_rows; ++r)
        for (uint32_t x = 1; x < op.F.tcols; ++x)
          for (uint32_t p = 0; p < op.F.planes; ++p)
            ff_walk_cols(tables.data() + op.table_off + size_t(r) * op.F.tcols * op.F.planes, op.F, x, p,
                         tables.data() + op.ck_off + size_t(r) * ff_ck_row_floats(op.F));
  }
  // the runs of the list: [first, end) holds no defects op
  for (uint32_t first = 0, end = 0; first <= J.n_ops; first = end + 1u) {
    for (end = first; end < J.n_ops && ops[end].kind != RSX_IIQ_OP_SENSOR_DEFECTS;)
      ++end;
    for (uint32_t row = 0; row < J.h && first < end; ++row) {
      uint16_t* line = reinterpret_cast<uint16_t*>(static_cast<uint8_t*>(img->data) + size_t(row) * J.pitch);
      for (uint32_t v = 0; v < J.vpr; ++v) {
        const uint32_t col0 = 8u * v, n = J.w - col0 < 8u ? J.w - col0 : 8u;
        uint16_t px[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (uint32_t i = 0; i < n; ++i)
          px[i] = line[col0 + i];
        uint32_t touched = 0;
        // (one op at a time: its curves stay where the caller has them, at offset 0)
        for (uint32_t o = first; o < end; ++o)
          touched |= correct_pixels(J, ops.data(), tables.data(), corr->ops[o].curves, o, o + 1u, row,
                                    col0, n, px);
        for (uint32_t i = 0; i < n; ++i)
          if (touched >> i & 1u)
            line[col0 + i] = px[i];
      }
    }
    if (end < J.n_ops)
      apply_defects(corr->ops[end], J, corr, static_cast<uint8_t*>(img->data));
  }
  return RSX_OK;
}

#ifdef RSX_IIQ_CORR_HOST_MAIN
namespace {

// pass per entry, running sums: the loops of PhaseOneFlatField restated
void plain_flat_field(const uint8_t* d, bool chroma, const rsx_iiq_corr& corr, uint16_t* img, int w,
                      int h, int pitch_px) {
  const int nc = chroma ? 4 : 2;
  int head[8];
  for (int i = 0; i < 8; ++i)
    head[i] = int(rd16(d + 2 * i));
  if (!head[2] || !head[3] || !head[4] || !head[5])
    return;
  const int wide = (head[2] + head[4] - 1) / head[4], high = (head[3] + head[5] - 1) / head[5];
  std::vector<float> mrow(size_t(wide) * nc, 0.0F);
  const uint8_t* p = d + 16;
  for (int y = 0; y < high; ++y) {
    for (int x = 0; x < wide; ++x)
      for (int c = 0; c < nc; c += 2, p += 2) {
        const float num = float(rd16(p)) / 32768.0F;
        if (y == 0)
          mrow[x * nc + c] = num;
        else
          mrow[x * nc + c + 1] = (num - mrow[x * nc + c]) / float(head[5]);
      }
    if (y == 0)
      continue;
    const int rend = head[1] + y * head[5];
    for (int row = rend - head[5]; row < h && row < rend && row < head[1] + head[3] - head[5]; ++row) {
      for (int x = 1; x < wide; ++x) {
        float mult[4] = {0, 0, 0, 0};
        for (int c = 0; c < nc; c += 2) {
          mult[c] = mrow[(x - 1) * nc + c];
          mult[c + 1] = (mrow[x * nc + c] - mult[c]) / float(head[4]);
        }
        const int cend = head[0] + x * head[4];
        for (int col = cend - head[4]; col < w && col < cend && col < head[0] + head[2] - head[4]; ++col) {
          const int c = chroma ? corr.cfa[(row % corr.cfa_w) + (col % corr.cfa_h) * corr.cfa_w] : 0;
          if (!(c & 1)) {
            const float v = float(img[size_t(row) * pitch_px + col]) * mult[c];
            const unsigned val = v > 0.0F ? unsigned(v) : 0u;
            img[size_t(row) * pitch_px + col] = uint16_t(val < 0xFFFFu ? val : 0xFFFFu);
          }
          for (int c2 = 0; c2 < nc; c2 += 2)
            mult[c2] += mult[c2 + 1];
        }
      }
      for (int x = 0; x < wide; ++x)
        for (int c = 0; c < nc; c += 2)
          mrow[x * nc + c] += mrow[x * nc + c + 1];
    }
  }
}

void plain_quadrant(const rsx_iiq_op& op, uint16_t* img, int w, int h, int pitch_px) {
  for (int row = 0; row < h; ++row)
    for (int col = 0; col < w; ++col) {
      const uint16_t* curve =
          op.curves + 65536u * ((uint32_t(row) >= op.split_row ? 2u : 0u) + (uint32_t(col) >= op.split_col ? 1u : 0u));
      uint16_t& px = img[size_t(row) * pitch_px + col];
      const uint16_t diff = px < op.black_level ? px : uint16_t(op.black_level);
      px = uint16_t(curve[px - diff] + diff);
    }
}

uint32_t rng_state = 12345;
uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

std::vector<uint8_t> payload(int h0, int h1, int h2, int h3, int h4, int h5, int planes, int mode) {
  const int head[8] = {h0, h1, h2, h3, h4, h5, 0, 0};
  std::vector<uint8_t> d(16);
  for (int i = 0; i < 8; ++i) {
    d[2 * i] = uint8_t(head[i]);
    d[2 * i + 1] = uint8_t(head[i] >> 8);
  }
  if (!h2 || !h3 || !h4 || !h5)
    return d;
  const int wide = (h2 + h4 - 1) / h4, high = (h3 + h5 - 1) / h5;
  for (int k = 0; k < wide * high * planes; ++k) {
    uint32_t v = mode == 0 ? 24000u + rnd() % 20000u : mode == 1 ? (rnd() & 1u ? 65535u : 0u) : rnd() % 65536u;
    d.push_back(uint8_t(v));
    d.push_back(uint8_t(v >> 8));
  }
  return d;
}

int fails = 0;
void expect(bool ok, const char* what) {
  if (!ok) {
    std::fprintf(stderr, "FAILED: %s\n", what);
    ++fails;
  }
}

} // namespace

int main() {
  std::vector<uint16_t> curves(4 * 65536);
  for (size_t k = 0; k < curves.size(); ++k)
    curves[k] = uint16_t(rnd());
  struct Geo { int w, h, pitch_px; };
  const Geo geos[] = {{64, 40, 64}, {72, 38, 77}, {13, 9, 13}};
  // {head[0..5]}: offset areas, cells that divide nothing, areas past the image, 1 x 1 cells, a
  // cell wider than the image, wide == 1, high == 1, a zero field, head[5] above the height
  const int heads[][6] = {{3, 2, 56, 30, 7, 5},   {0, 0, 64, 40, 8, 8},   {5, 3, 130, 121, 13, 11},
                          {0, 0, 40, 20, 1, 1},   {0, 0, 400, 40, 200, 4}, {0, 0, 8, 40, 8, 4},
                          {0, 0, 64, 8, 8, 8},    {0, 0, 64, 0, 8, 8},     {2, 1, 60, 300, 6, 100},
                          {70, 50, 64, 64, 8, 8}, {0, 0, 65535, 65535, 255, 255},
                          {1, 0, 140, 40, 70, 8}, {0, 0, 99, 40, 33, 8}, {3, 1, 128, 64, 64, 32}};
  for (const Geo& g : geos)
    for (const auto& hd : heads)
      for (int chroma = 0; chroma < 2; ++chroma)
        for (int mode = 0; mode < 3; ++mode) {
          rsx_iiq_corr corr;
          std::memset(&corr, 0, sizeof corr);
          corr.cfa_w = 2;
          corr.cfa_h = chroma && mode == 1 ? 4 : 2;
          const uint8_t cfa[8] = {1, 0, 2, 1, 0, 1, 1, 2};
          std::memcpy(corr.cfa, cfa, 8);
          std::vector<uint8_t> pl = payload(hd[0], hd[1], hd[2], hd[3], hd[4], hd[5], chroma ? 2 : 1, mode);
          corr.n_ops = 3;
          corr.ops[0].kind = RSX_IIQ_OP_FLAT_FIELD;
          corr.ops[0].chroma = chroma;
          corr.ops[0].payload = pl.data();
          corr.ops[0].payload_bytes = uint32_t(pl.size());
          corr.ops[1].kind = RSX_IIQ_OP_QUADRANT_CURVES;
          corr.ops[1].curves = curves.data();
          corr.ops[1].split_row = uint32_t(g.h / 2 + 1);
          corr.ops[1].split_col = uint32_t(g.w / 2 - 3);
          corr.ops[1].black_level = 1000;
          corr.ops[2] = corr.ops[0];
          std::vector<uint16_t> a(size_t(g.pitch_px) * g.h), b;
          for (uint16_t& v : a)
            v = uint16_t(mode == 1 ? 65535u - (rnd() & 1u) : rnd());
          b = a;
          rsx_image img{a.data(), uint32_t(2 * g.pitch_px), g.w, g.h, 1, 1};
          const int st = rsx_iiq_corr_host_apply(&corr, &img);
          expect(st == RSX_OK, "apply status");
          plain_flat_field(pl.data(), chroma, corr, b.data(), g.w, g.h, g.pitch_px);
          plain_quadrant(corr.ops[1], b.data(), g.w, g.h, g.pitch_px);
          plain_flat_field(pl.data(), chroma, corr, b.data(), g.w, g.h, g.pitch_px);
          expect(a == b, "fused pass against pass per entry");
          // the validation cases on this list
          std::vector<uint16_t> keep = a;
          rsx_iiq_corr bad = corr;
          bad.ops[2].payload_bytes = 15;
          expect(rsx_iiq_corr_host_apply(&bad, &img) == RSX_ERR_IO && a == keep, "short head");
          if (hd[2] && hd[3] && hd[4] && hd[5]) {
            bad = corr;
            bad.ops[2].payload_bytes -= 1;
            expect(rsx_iiq_corr_host_apply(&bad, &img) == RSX_ERR_IO && a == keep, "short payload");
          }
          bad = corr;
          bad.ops[1].split_col = uint32_t(g.w + 1);
          expect(rsx_iiq_corr_host_apply(&bad, &img) == RSX_ERR_INVALID_ARG && a == keep, "split");
          bad = corr;
          bad.ops[1].kind = 2;
          expect(rsx_iiq_corr_host_apply(&bad, &img) == RSX_ERR_INVALID_ARG && a == keep, "kind");
          bad = corr;
          bad.n_ops = 17;
          expect(rsx_iiq_corr_host_apply(&bad, &img) == RSX_ERR_INVALID_ARG && a == keep, "n_ops");
          if (chroma) {
            bad = corr;
            bad.cfa_w = 0;
            expect(rsx_iiq_corr_host_apply(&bad, &img) == RSX_ERR_INVALID_ARG && a == keep, "no cfa");
            bad = corr;
            bad.cfa[1] = 4;
            expect(rsx_iiq_corr_host_apply(&bad, &img) == RSX_ERR_UNSUPPORTED && a == keep, "colour 4");
          }
          rsx_image narrow = img;
          narrow.pitch_bytes = uint32_t(2 * g.w - 2);
          expect(rsx_iiq_corr_host_apply(&corr, &narrow) == RSX_ERR_INVALID_ARG && a == keep, "pitch");
        }
  // The sensor defects: random record lists -- bad columns in clusters and far apart, the same
  // column again, bad pixels, unknown types and columns outside the image between them -- applied
  // in file order (apply_defects) and level by level, each level from its LAST record to its first
  // (what the device's launches are free to do).  Both must give the same image.
  for (int round = 0; round < 300; ++round) {
    const int w = 5 + int(rnd() % 60), h = 4 + int(rnd() % 12), pitch_px = w + int(rnd() % 3);
    std::vector<uint8_t> pl;
    const int n_rec = int(rnd() % 40);
    for (int k = 0; k < n_rec; ++k) {
      const uint32_t kind = rnd() % 8;
      uint32_t col = kind < 5 ? 2u + rnd() % uint32_t(w - 4) : rnd() % uint32_t(w + 6);
      if (kind < 2 && pl.size() >= 8) // (beside the record in front)
        col = std::min(uint32_t(w - 3), std::max(2u, rd16(pl.data() + pl.size() - 8) + rnd() % 5u - 2u));
      const uint32_t type = kind < 5 ? (rnd() & 1u ? 131u : 137u) : kind == 5 ? 129u : kind == 6 ? 7u : 131u;
      if (kind == 7 && col < uint32_t(w))
        col += uint32_t(w); // (a bad column outside the image: skipped, whatever it holds)
      const uint32_t rec[4] = {col, rnd() % 65536u, type, rnd() % 65536u};
      for (uint32_t v : rec) {
        pl.push_back(uint8_t(v));
        pl.push_back(uint8_t(v >> 8));
      }
    }
    rsx_iiq_corr corr;
    std::memset(&corr, 0, sizeof corr);
    corr.cfa_w = 2;
    corr.cfa_h = round % 3 == 0 ? 4 : 2;
    const uint8_t cfa[8] = {1, 0, 2, 1, 0, 1, 1, 2};
    std::memcpy(corr.cfa, cfa, 8);
    corr.n_ops = 1;
    corr.ops[0].kind = RSX_IIQ_OP_SENSOR_DEFECTS;
    corr.ops[0].payload = pl.data();
    corr.ops[0].payload_bytes = uint32_t(pl.size());
    std::vector<uint16_t> a(size_t(pitch_px) * h), b;
    for (uint16_t& v : a)
      v = uint16_t(rnd());
    b = a;
    rsx_image img{a.data(), uint32_t(2 * pitch_px), w, h, 1, 1};
    expect(rsx_iiq_corr_host_apply(&corr, &img) == RSX_OK, "defects: apply status");
    std::vector<uint32_t> cols, ends;
    defects_levels(pl.data(), uint32_t(pl.size()), w, h, &cols, &ends);
    uint8_t* bytes = reinterpret_cast<uint8_t*>(b.data());
    for (size_t l = 0; l < ends.size(); ++l) {
      // (every lane of a launch may read before any of them writes, or after)
      std::vector<uint16_t> before = b;
      for (uint32_t k = ends[l]; k-- > (l ? ends[l - 1] : 0u);)
        for (uint32_t row = 2; row + 2u < uint32_t(h); ++row) {
          const uint32_t colour = corr.cfa[cols[k] % 2u + (row % uint32_t(corr.cfa_h)) * 2u];
          const uint8_t* from = (k & 1u) ? reinterpret_cast<const uint8_t*>(before.data()) : bytes;
          b[size_t(row) * pitch_px + cols[k]] = bad_column_pixel(from, uint32_t(2 * pitch_px), row, cols[k], colour);
        }
    }
    expect(a == b, "defects: level order against file order");
    uint32_t n = 0, two[2] = {0, 0};
    expect(defect_positions(pl.data(), uint32_t(pl.size()), w, two, 2, &n) == RSX_OK, "defects: positions");
    expect(defect_positions(pl.data(), uint32_t(pl.size()) - (pl.empty() ? 0u : 3u), w, two, 2, &n) ==
               (pl.empty() ? RSX_OK : RSX_ERR_IO), "defects: a cut record");
  }
  if (fails)
    return 1;
  std::puts("rsx_iiq_corr_host_check OK");
  return 0;
}
#endif
