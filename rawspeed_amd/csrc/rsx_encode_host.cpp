// rsx_encode_host.cpp -- rsx_encode_core.h as host C++: the single-threaded reference walk of whole
// jobs that the device kernels (rsx_encode_pack.hip, rsx_encode_ljpeg.hip) are held against, built
// into rawspeed_amd/librsx_encode_host.so.  With -DRSX_ENCODE_HOST_MAIN the same source is a
// program (AddressSanitizer + UBSan where the runtimes exist) that walks every geometry up to
// 9 x 5 samples, every container layout, and the case file a test hands it (the case list of
// tests/encode_files.py).
#include "rsx_encode_core.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace rsx_encode;

extern "C" {

// what a workgroup covers: output bytes of the pack kernel, samples of the LJPEG kernels
int rsx_encode_host_pack_block_bytes(void) { return PACK_BLOCK_BYTES; }
int rsx_encode_host_ljpeg_run(void) { return LJPEG_RUN; }

int rsx_encode_host_pack_validate(const rsx_unpack_desc* d, const rsx_image* img, size_t out_cap) {
  return validate_pack(d, img, out_cap);
}

// img->data: the image in host memory
int rsx_encode_host_pack(const rsx_unpack_desc* d, const rsx_image* img, uint8_t* out,
                         size_t out_cap, rsx_encode_pack_result* res) {
  if (!d || !img || !img->data || !out || !res)
    return RSX_ERR_INVALID_ARG;
  if (int st = validate_pack(d, img, out_cap))
    return st;
  PackGeom g;
  pack_geom(*d, *img, 0, 0, &g);
  pack_walk(static_cast<const uint8_t*>(img->data), g, out);
  res->bytes_written = g.out_bytes;
  res->stream_bytes = g.stream_bytes;
  return RSX_OK;
}

// step 2 of rsx_encode_ljpeg_validate (step 1, the reader's constructor, lives in librsx.so)
int rsx_encode_host_ljpeg_subset(const rsx_ljpeg_desc* d, const rsx_image* img) {
  return d && img ? validate_ljpeg_subset(*d, *img) : RSX_ERR_INVALID_ARG;
}

uint64_t rsx_encode_host_ljpeg_bound(const rsx_ljpeg_desc* d, const rsx_image* img) {
  if (!d || !img || validate_ljpeg_subset(*d, *img))
    return 0;
  LJpegGeom g;
  ljpeg_geom(*d, *img, 0, 0, 0, 0, &g);
  return ljpeg_bound(g);
}

// One job of a descriptor rsx_ljpeg_validate accepts.  hist (4 x 17 counts, may be NULL) gets the
// categories per component whatever the tables hold.  Returns the job's status.
int rsx_encode_host_ljpeg(const rsx_ljpeg_desc* d, const rsx_image* img, uint32_t flags,
                          uint8_t* out, size_t out_cap, rsx_encode_result* res, uint64_t* hist) {
  if (!d || !img || !img->data || !res || flags > RSX_ENCODE_TAIL_VACUUMER)
    return RSX_ERR_INVALID_ARG;
  std::memset(res, 0, sizeof *res);
  if (int st = validate_ljpeg_subset(*d, *img))
    return res->status = st;
  LJpegGeom g;
  ljpeg_geom(*d, *img, 0, 0, out_cap, flags, &g);
  EncTable tabs[RSX_MAX_COMPONENTS];
  for (int i = 0; i < d->n_tables && i < RSX_MAX_COMPONENTS; ++i)
    build_enc_table(d->tables[i], &tabs[i]);
  LJpegWalkResult w;
  ljpeg_walk(static_cast<const uint8_t*>(img->data), g, tabs, out, &w);
  res->status = w.status;
  res->bytes = w.bytes;
  res->symbol_bits = w.symbol_bits;
  if (hist)
    std::memcpy(hist, w.hist, sizeof w.hist);
  return w.status;
}

int rsx_encode_host_huff(const uint64_t* counts, uint32_t flags, rsx_huff_table* out) {
  if (!counts || !out || (flags & ~uint32_t(RSX_ENCODE_TABLE_ALL_CATEGORIES)))
    return RSX_ERR_INVALID_ARG;
  return huff_from_histogram(counts, (flags & RSX_ENCODE_TABLE_ALL_CATEGORIES) != 0, out);
}

size_t rsx_encode_host_container(const rsx_ljpeg_desc* d, int precision, uint8_t* hdr,
                                 size_t hdr_cap) {
  return ljpeg_container(*d, precision, hdr, hdr_cap);
}

} // extern "C"

#ifdef RSX_ENCODE_HOST_MAIN
namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return uint32_t(rng_state >> 16);
}

// stream byte s of a packed strip in memory
uint8_t stream_byte(const std::vector<uint8_t>& m, int order, size_t s) {
  return m[order == RSX_ORDER_MSB16 ? s ^ 1u : order == RSX_ORDER_MSB32 ? s ^ 3u : s];
}

// the sample at (r, x) of a packed strip, read bit by bit
uint32_t read_sample(const std::vector<uint8_t>& m, int order, int bps, size_t pitch, int r, int x) {
  uint32_t v = 0;
  for (int i = 0; i < bps; ++i) {
    const size_t bit = size_t(r) * pitch * 8 + size_t(x) * bps + i;
    const uint8_t byte = stream_byte(m, order, bit / 8);
    if (order == RSX_ORDER_LSB)
      v |= uint32_t(byte >> (bit % 8) & 1u) << i;
    else
      v = v << 1 | (byte >> (7 - bit % 8) & 1u);
  }
  return v;
}

int check_pack() {
  int n = 0;
  for (int order = 0; order < 4; ++order)
    for (int bps : {1, 7, 8, 10, 12, 14, 16})
      for (int h = 1; h <= 5; ++h)
        for (int w = 1; w <= 72; ++w)
          for (int pad : {0, 3}) {
            if (w * bps % 8 != 0 || (w > 9 && w % 8 != 0))
              continue;
            const int pitch = w * bps / 8 + pad;
            if (h * pitch < 4)
              continue;
            std::vector<uint16_t> img(size_t(h + 1) * (w + 1));
            for (uint16_t& v : img)
              v = uint16_t(rnd());
            rsx_image im{img.data(), uint32_t(2 * (w + 1)), w, h + 1, 1, 1};
            rsx_unpack_desc d{0, 1, w, h, pitch, bps, order};
            const size_t cap = size_t(round_up4(uint64_t(h) * pitch));
            std::vector<uint8_t> out(cap);
            rsx_encode_pack_result res;
            if (rsx_encode_host_pack(&d, &im, out.data(), cap, &res) != RSX_OK ||
                res.bytes_written != cap)
              return std::printf("pack: status order %d bps %d %dx%d\n", order, bps, w, h), 1;
            // the 64-bit form of the gather (streams past 4 GiB, rows past 2^28 bytes) gives the
            // same words as the 32-bit one that served the call
            PackGeom g;
            pack_geom(d, im, 0, 0, &g);
            for (uint64_t k = 0; k * 16u < g.out_bytes; ++k) {
              uint32_t a[4], b[4];
              pack_chunk_t<uint32_t>(reinterpret_cast<const uint8_t*>(img.data()), g, uint32_t(k), a);
              pack_chunk_t<uint64_t>(reinterpret_cast<const uint8_t*>(img.data()), g, k, b);
              if (std::memcmp(a, b, sizeof a) != 0)
                return std::printf("pack: 32/64 order %d bps %d %dx%d\n", order, bps, w, h), 1;
            }
            for (int r = 0; r < h; ++r)
              for (int x = 0; x < w; ++x)
                if (read_sample(out, order, bps, pitch, r, x) !=
                    (img[size_t(r + 1) * (w + 1) + x] & ((1u << bps) - 1u)))
                  return std::printf("pack: sample order %d bps %d %dx%d\n", order, bps, w, h), 1;
            ++n;
          }
  std::printf("pack: %d geometries round-trip\n", n);
  return 0;
}

int check_ljpeg() {
  // a code of all 17 categories, lengths 4 x 15 and 5 x 2
  rsx_ljpeg_desc d;
  std::memset(&d, 0, sizeof d);
  d.n_tables = 1;
  rsx_huff_table& t = d.tables[0];
  t.n_codes_per_length[3] = 15;
  t.n_codes_per_length[4] = 2;
  t.n_code_values = 17;
  for (int i = 0; i < 17; ++i)
    t.code_values[i] = uint8_t(i);
  int n = 0;
  for (int fix = 0; fix < 2; ++fix)
    for (int nc = 1; nc <= 4; ++nc)
      for (int h = 1; h <= 5; ++h)
        for (int w = nc; w <= 9; w += nc)
          for (int rpi = 1; rpi <= h; ++rpi)
            for (uint32_t tail = 0; tail < 2; ++tail) {
              t.fix_dng_bug16 = uint8_t(fix);
              std::vector<uint16_t> img(size_t(h) * w);
              for (uint16_t& v : img)
                v = uint16_t(rnd() % 5 == 0 ? rnd() : 0x8000u + rnd() % 3);
              rsx_image im{img.data(), uint32_t(2 * w), w, h, 1, 1};
              d.tile_w = w, d.tile_h = h, d.mcu_w = nc, d.mcu_h = 1, d.frame_w = w / nc;
              d.frame_h = h, d.n_comp = nc, d.rows_per_restart_interval = rpi;
              const size_t cap = size_t(rsx_encode_host_ljpeg_bound(&d, &im));
              std::vector<uint8_t> out(cap);
              rsx_encode_result res;
              uint64_t hist[4 * N_CATEGORIES];
              if (rsx_encode_host_ljpeg(&d, &im, tail, out.data(), cap, &res, hist) != RSX_OK ||
                  res.bytes == 0 || res.bytes > cap)
                return std::printf("ljpeg: %dx%d nc %d rpi %d\n", w, h, nc, rpi), 1;
              // one byte short of what it takes
              std::vector<uint8_t> tight(size_t(res.bytes) - 1);
              rsx_encode_result r2;
              if (rsx_encode_host_ljpeg(&d, &im, tail, tight.data(), tight.size(), &r2, nullptr) !=
                      RSX_ERR_INPUT_OVERFLOW || r2.bytes != 0)
                return std::printf("ljpeg: overflow %dx%d\n", w, h), 1;
              ++n;
            }
  std::printf("ljpeg: %d jobs walked\n", n);
  // tables from histograms
  for (int k = 0; k < 200; ++k) {
    uint64_t counts[N_CATEGORIES];
    for (uint64_t& c : counts)
      c = rnd() % 3 == 0 ? 0 : uint64_t(rnd()) << (rnd() % 30);
    counts[k % N_CATEGORIES] = 1 + rnd();
    rsx_huff_table out;
    if (rsx_encode_host_huff(counts, k & 1, &out) != RSX_OK)
      return std::printf("huff: %d\n", k), 1;
  }
  std::printf("huff: 200 histograms\n");
  return 0;
}

// the container of every component count, table count and table size up to the largest layout
// there is (four components, four tables of 162 values, a restart interval), into a buffer of
// exactly its size and into one a byte short
int check_container() {
  int n = 0;
  for (int nc = 1; nc <= 4; ++nc)
    for (int nt = 1; nt <= 4; ++nt)
      for (int nv : {1, 17, RSX_MAX_CODE_VALUES})
        for (int rpi : {1, 8}) {
          rsx_ljpeg_desc d;
          std::memset(&d, 0, sizeof d);
          d.tile_w = 4 * nc, d.tile_h = 8, d.mcu_w = nc, d.mcu_h = 1, d.frame_w = 4, d.frame_h = 8;
          d.n_comp = nc, d.rows_per_restart_interval = rpi, d.n_tables = nt;
          for (int t = 0; t < nt; ++t) {
            d.tables[t].n_code_values = uint8_t(nv);
            for (int v = 0; v < nv; ++v)
              d.tables[t].code_values[v] = uint8_t(v % 17);
          }
          const size_t want = 2 + (10 + 3 * nc) + size_t(nt) * (21 + nv) + (rpi < 8 ? 6 : 0) +
                              (8 + 2 * nc);
          std::vector<uint8_t> hdr(want), tight(want - 1);
          if (rsx_encode_host_container(&d, 14, hdr.data(), want) != want ||
              rsx_encode_host_container(&d, 14, tight.data(), want - 1) != 0)
            return std::printf("container: nc %d nt %d nv %d\n", nc, nt, nv), 1;
          ++n;
        }
  rsx_ljpeg_desc bad;
  std::memset(&bad, 0, sizeof bad);
  bad.n_comp = 5, bad.n_tables = 9;
  uint8_t hdr[16];
  if (rsx_encode_host_container(&bad, 14, hdr, sizeof hdr) != 0)
    return std::printf("container: refused descriptor\n"), 1;
  std::printf("container: %d layouts\n", n);
  return 0;
}

// The case list of tests/encode_files.py (the file its --write-cases writes; the format is
// described in scripts/record_encode_ref.cpp): a pack line is packed as one row and read back bit
// by bit, an ljpeg line becomes a one-row tile of one component with init_pred 0 whose
// differences are the line's, walked in both tail modes, into exactly the bytes it takes and into
// one byte less.
int check_case_file(const char* path) {
  std::FILE* f = std::fopen(path, "r");
  if (!f)
    return std::printf("cases: cannot open %s\n", path), 1;
  int n_pack = 0, n_ljpeg = 0;
  char kind[16], name[128];
  while (std::fscanf(f, "%15s %127s", kind, name) == 2) {
    if (!std::strcmp(kind, "pack")) {
      int order, bps, n;
      if (std::fscanf(f, "%d %d %d", &order, &bps, &n) != 3 || n < 1)
        return 1;
      std::vector<uint16_t> px(static_cast<size_t>(n), uint16_t(0));
      for (uint16_t& v : px) {
        unsigned t;
        if (std::fscanf(f, "%u", &t) != 1)
          return 1;
        v = uint16_t(t);
      }
      rsx_image im{px.data(), uint32_t(2 * n), n, 1, 1, 1};
      rsx_unpack_desc d{0, 0, n, 1, n * bps / 8, bps, order};
      const size_t cap = size_t(round_up4(uint64_t(n) * bps / 8));
      std::vector<uint8_t> out(cap);
      rsx_encode_pack_result res;
      if (rsx_encode_host_pack(&d, &im, out.data(), cap, &res) != RSX_OK)
        return std::printf("cases: pack %s\n", name), 1;
      for (int x = 0; x < n; ++x)
        if (read_sample(out, order, bps, size_t(n) * bps / 8, 0, x) != (px[x] & ((1u << bps) - 1u)))
          return std::printf("cases: pack %s sample %d\n", name, x), 1;
      ++n_pack;
    } else if (!std::strcmp(kind, "ljpeg")) {
      rsx_ljpeg_desc d;
      std::memset(&d, 0, sizeof d);
      int fix16, nv, n, t;
      if (std::fscanf(f, "%d", &fix16) != 1)
        return 1;
      rsx_huff_table& tab = d.tables[0];
      for (int l = 0; l < 16; ++l) {
        if (std::fscanf(f, "%d", &t) != 1)
          return 1;
        tab.n_codes_per_length[l] = uint8_t(t);
      }
      if (std::fscanf(f, "%d", &nv) != 1 || nv < 0 || nv > RSX_MAX_CODE_VALUES)
        return 1;
      for (int v = 0; v < nv; ++v) {
        if (std::fscanf(f, "%d", &t) != 1)
          return 1;
        tab.code_values[v] = uint8_t(t);
      }
      tab.n_code_values = uint8_t(nv);
      tab.fix_dng_bug16 = uint8_t(fix16);
      if (std::fscanf(f, "%d", &n) != 1 || n < 1)
        return 1;
      std::vector<uint16_t> px(static_cast<size_t>(n), uint16_t(0));
      uint32_t acc = 0;
      for (uint16_t& v : px) {
        if (std::fscanf(f, "%d", &t) != 1)
          return 1;
        acc += uint32_t(t);
        v = uint16_t(acc);
      }
      rsx_image im{px.data(), uint32_t(2 * n), n, 1, 1, 1};
      d.tile_w = n, d.tile_h = 1, d.mcu_w = 1, d.mcu_h = 1, d.frame_w = n, d.frame_h = 1;
      d.n_comp = 1, d.rows_per_restart_interval = 1, d.n_tables = 1;
      for (uint32_t tail = 0; tail < 2; ++tail) {
        rsx_encode_result count, res, r2;
        std::vector<uint8_t> big(size_t(rsx_encode_host_ljpeg_bound(&d, &im)));
        if (rsx_encode_host_ljpeg(&d, &im, tail, big.data(), big.size(), &count, nullptr) != RSX_OK)
          return std::printf("cases: ljpeg %s\n", name), 1;
        std::vector<uint8_t> exact(size_t(count.bytes)), tight(size_t(count.bytes) - 1);
        if (rsx_encode_host_ljpeg(&d, &im, tail, exact.data(), exact.size(), &res, nullptr) != RSX_OK ||
            res.bytes != count.bytes || std::memcmp(exact.data(), big.data(), exact.size()) != 0 ||
            rsx_encode_host_ljpeg(&d, &im, tail, tight.data(), tight.size(), &r2, nullptr) !=
                RSX_ERR_INPUT_OVERFLOW)
          return std::printf("cases: ljpeg %s tail %u\n", name, tail), 1;
      }
      ++n_ljpeg;
    } else
      return std::printf("cases: line kind %s\n", kind), 1;
  }
  std::fclose(f);
  std::printf("cases: %d pack, %d ljpeg\n", n_pack, n_ljpeg);
  return 0;
}

} // namespace

int main(int argc, char** argv) {
  if (check_pack() || check_ljpeg() || check_container())
    return 1;
  if (argc > 1 && check_case_file(argv[1]))
    return 1;
  std::printf("rsx_encode_host_check OK\n");
  return 0;
}
#endif
