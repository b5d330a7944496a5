// hamming64.h -- the 64-bit Hamming distance of the search kernels (hamming.hip, hamming_multi.hip): one text for every
// translation unit, since a device function cannot cross them without relocatable device code.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ucfp {

__device__ __forceinline__ uint32_t hamming64(uint64_t q, uint64_t x) {
    const uint32_t lo = (uint32_t)q ^ (uint32_t)x;
    const uint32_t hi = (uint32_t)(q >> 32) ^ (uint32_t)(x >> 32);
    return __builtin_popcount(hi) + __builtin_popcount(lo);
}

}  // namespace ucfp
