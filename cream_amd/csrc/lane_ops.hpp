// lane_ops.hpp — cross-lane helpers that need nothing but the HIP runtime (gfx950, 64-lane waves).
#pragma once
#include <hip/hip_runtime.h>

namespace cream {

// sum of v over the 64 lanes of the wave in a fixed butterfly (same order every run); every lane gets the total
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

}  // namespace cream
