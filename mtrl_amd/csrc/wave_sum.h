// wave_sum.h -- the fixed shuffle tree the Gram-form solves (pcgrad.hip, cagrad.hip, gradnorm.hip) reduce
// over the tasks with: one wavefront of 64 lanes, every lane gets the sum, the order of the additions is
// the same at every call.
#pragma once
#include <hip/hip_runtime.h>

namespace mtsac {

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

}  // namespace mtsac
