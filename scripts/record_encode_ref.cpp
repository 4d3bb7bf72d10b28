// Records what the reference's writers make of the case list of tests/encode_files.py:
// tests/golden/encode_ref.json comes from this program's output.  It is not part of any build or
// test; it needs the reference's sources (REF below) and the reference library that
// oracle/Makefile builds.  From the repository root:
//
//   python tests/encode_files.py --write-cases /tmp/encode_cases.txt
//   /opt/rocm/lib/llvm/bin/clang++ -std=c++20 -O2 -march=x86-64-v2 -w \
//       -Ioracle/ref_config -I$REF/src/librawspeed -I$REF/src/external \
//       scripts/record_encode_ref.cpp oracle/_ref/librawspeed_ref.so \
//       -Wl,-rpath,$PWD/oracle/_ref -Wl,-rpath,/opt/rocm/lib/llvm/lib -o /tmp/record_encode_ref
//   /tmp/record_encode_ref /tmp/encode_cases.txt > /tmp/encode_ref.jsonl
//   python tests/encode_files.py --golden /tmp/encode_ref.jsonl
//
// A line of the case file is one case, fields separated by blanks:
//   pack NAME ORDER BPS N v[0] .. v[N-1]
//       BitVacuumer{LSB,MSB,MSB16,MSB32} (ORDER 0..3): put(v[i], BPS) for every sample, then the
//       destructor's flush
//   ljpeg NAME FIX16 c[0] .. c[15] NV values[0] .. values[NV-1] N d[0] .. d[N-1]
//       a HuffmanCode<BaselineCodeTag> of the 16 counts and the NV values, a
//       PrefixCodeVectorEncoder over it set up for full decoding with fixDNGBug16 = FIX16, and
//       encodeDifference(bv, d[i]) on a BitVacuumerJPEG for every difference, then the flush
// Per case one JSON line: the name and the bytes written as hex.  The differences, not images,
// are the input: the tests compute differences with their own model of the predictor.
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "adt/Array1DRef.h"
#include "adt/PartitioningOutputIterator.h"
#include "bitstreams/BitVacuumerJPEG.h"
#include "bitstreams/BitVacuumerLSB.h"
#include "bitstreams/BitVacuumerMSB.h"
#include "bitstreams/BitVacuumerMSB16.h"
#include "bitstreams/BitVacuumerMSB32.h"
#include "codes/AbstractPrefixCode.h"
#include "codes/HuffmanCode.h"
#include "codes/PrefixCode.h"
#include "codes/PrefixCodeVectorEncoder.h"
#include "io/Buffer.h"

using namespace rawspeed;

namespace {

template <template <typename> class Vacuumer>
std::vector<uint8_t> pack(const std::vector<uint32_t>& v, int bps) {
  std::vector<uint8_t> out;
  {
    auto it = PartitioningOutputIterator(std::back_inserter(out));
    Vacuumer<decltype(it)> bv(it);
    for (uint32_t s : v)
      bv.put(s, bps);
  }
  return out;
}

std::vector<uint8_t> ljpeg(const std::vector<uint8_t>& counts, const std::vector<uint8_t>& values,
                           bool fix16, const std::vector<int>& diffs) {
  HuffmanCode<BaselineCodeTag> hc;
  hc.setNCodesPerLength(Buffer(counts.data(), Buffer::size_type(counts.size())));
  hc.setCodeValues(Array1DRef<const uint8_t>(values.data(), int(values.size())));
  PrefixCodeVectorEncoder<BaselineCodeTag> enc(static_cast<PrefixCode<BaselineCodeTag>>(hc));
  enc.setup(/*fullDecode=*/true, fix16);
  std::vector<uint8_t> out;
  {
    auto it = PartitioningOutputIterator(std::back_inserter(out));
    BitVacuumerJPEG<decltype(it)> bv(it);
    for (int d : diffs)
      enc.encodeDifference(bv, d);
  }
  return out;
}

void print(const std::string& kind, const std::string& name, const std::vector<uint8_t>& bytes) {
  std::printf("{\"kind\": \"%s\", \"name\": \"%s\", \"hex\": \"", kind.c_str(), name.c_str());
  for (uint8_t b : bytes)
    std::printf("%02x", b);
  std::printf("\"}\n");
}

} // namespace

int main(int argc, char** argv) {
  if (argc != 2)
    return 2;
  std::ifstream f(argv[1]);
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream in(line);
    std::string kind, name;
    in >> kind >> name;
    if (kind == "pack") {
      int order, bps, n;
      in >> order >> bps >> n;
      std::vector<uint32_t> v(n);
      for (uint32_t& s : v)
        in >> s;
      print(kind, name,
            order == 0   ? pack<BitVacuumerLSB>(v, bps)
            : order == 1 ? pack<BitVacuumerMSB>(v, bps)
            : order == 2 ? pack<BitVacuumerMSB16>(v, bps)
                         : pack<BitVacuumerMSB32>(v, bps));
    } else if (kind == "ljpeg") {
      int fix16, nv, n, t;
      in >> fix16;
      std::vector<uint8_t> counts(16);
      for (uint8_t& c : counts)
        in >> t, c = uint8_t(t);
      in >> nv;
      std::vector<uint8_t> values(nv);
      for (uint8_t& c : values)
        in >> t, c = uint8_t(t);
      in >> n;
      std::vector<int> d(n);
      for (int& x : d)
        in >> x;
      print(kind, name, ljpeg(counts, values, fix16 != 0, d));
    } else if (!kind.empty())
      return 2;
  }
  return 0;
}
