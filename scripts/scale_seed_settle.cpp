// Settles what rsx_dither_dev.h's Mwc<18000>::jump_settled relies on: scaleValues_plain seeds a
// row with crop_x + y 36969, an int, so the call admits every seed in 0 .. INT32_MAX, and the
// generator's jump r_n = r_0 18000^n mod m is valid only for r_0 < m = 18000 2^16 - 1.  This
// program steps EVERY such seed and reports after how many steps the state is below m; the one
// seed that never gets there is m itself, a fixed point.  It is not part of any build or test:
//
//   g++ -O2 -std=c++17 -fopenmp -Irawspeed_amd/csrc scripts/scale_seed_settle.cpp -o /tmp/settle
//   /tmp/settle
//
// Output of the run the header quotes:
//   seeds 0 .. 2147483647: below m after 0 steps: 1179647999, after 1: 967820880, after 2: 14768,
//   after more: 0;
//   never: 1 (the seed m, which stays m); SETTLE = 2 holds
#include <cstdint>
#include <cstdio>

#include "rsx_dither_dev.h"

int main() {
  typedef rsx::Mwc<18000> G;
  const uint64_t m = G::MOD;
  uint64_t after[8] = {0}, never = 0;
  int worst = 0;
#pragma omp parallel for reduction(+ : after[:8], never) reduction(max : worst)
  for (int64_t seed = 0; seed <= 0x7FFFFFFFll; ++seed) {
    uint32_t s = uint32_t(seed);
    int n = 0;
    while (s >= m && n < 7) {
      s = G::step(s);
      ++n;
    }
    if (s >= m) {
      ++never;
      if (uint32_t(seed) != m || G::step(s) != m)
        worst = 99; // (a seed other than the fixed point that does not settle)
    } else {
      ++after[n];
      worst = n > worst ? n : worst;
    }
  }
  std::printf("seeds 0 .. 2147483647: below m after 0 steps: %llu, after 1: %llu, after 2: %llu, "
              "after more: %llu;\nnever: %llu (the seed m, which stays m); SETTLE = %u %s\n",
              (unsigned long long)after[0], (unsigned long long)after[1], (unsigned long long)after[2],
              (unsigned long long)(after[3] + after[4] + after[5] + after[6] + after[7]),
              (unsigned long long)never, G::SETTLE,
              worst <= int(G::SETTLE) && never == 1 ? "holds" : "DOES NOT HOLD");
  return worst <= int(G::SETTLE) && never == 1 ? 0 : 1;
}
