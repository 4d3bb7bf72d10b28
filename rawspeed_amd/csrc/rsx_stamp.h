// rsx_stamp.h -- the in-run kernel time of a timed launch, taken by the kernel itself.
//
// A timed launch gets STAMP_SLOTS (first entry, last exit) pairs of the device's wall clock:
// lane 0 of every workgroup folds its clock on entry into the first word of slot
// `blockIdx.x % STAMP_SLOTS` (minimum) and on exit into the second (maximum); the host
// reduces the slots (rsx_plan_kernel_time).  The launch itself is an ordinary one: nothing
// else goes on the queue, where a hipEventRecord before and after is a barrier packet each,
// and events bound to the dispatch (hipExtLaunchKernelGGL) still cost the queue 7 us a step
// (DESIGN.md 4.1).  Untimed launches pass a null pointer: a block-uniform branch.
#pragma once

#include "rsx_device.h"

namespace rsx {

struct BlockStamp {
  unsigned long long* stamps;
  __device__ __forceinline__ explicit BlockStamp(unsigned long long* s) : stamps(s) {
    if (stamps && threadIdx.x == 0)
      atomicMin(stamps + 2 * (blockIdx.x & (STAMP_SLOTS - 1)), wall_clock64());
  }
  // (runs on every way out of the kernel)
  __device__ __forceinline__ ~BlockStamp() {
    if (stamps && threadIdx.x == 0)
      atomicMax(stamps + 2 * (blockIdx.x & (STAMP_SLOTS - 1)) + 1, wall_clock64());
  }
};

} // namespace rsx
