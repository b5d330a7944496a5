// idf_math.h -- the integer arithmetic of fitted IDF weights, one statement for the host entries
// (idf_host.cpp), the finalize kernel (text_idf.hip) and nothing else: no float, no logf, so they agree by construction.
#pragma once
#include <stdint.h>

#if (defined(__HIP__) || defined(__HIPCC__)) && !defined(UCFP_IDF_HOST_ONLY)
#define UCFP_IDF_FN __host__ __device__ static inline
#else
#define UCFP_IDF_FN static inline
#endif

namespace ucfp {

// floor-ish log2 in Q16 (tests/simhash_idf_ref.py log2_q16 is the definition): the integer part from the leading bit, 16
// fraction bits by squaring the Q1.63 mantissa.  x = 0 gives 0.
UCFP_IDF_FN uint32_t idf_log2_q16(uint64_t x) {
    if (x == 0) return 0;
    const int n = 63 - __builtin_clzll(x);
    uint64_t y = x << (63 - n);   // [2^63, 2^64)
    uint32_t r = (uint32_t)n << 16;
    for (int i = 0; i < 16; i++) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(UCFP_IDF_HOST_ONLY)
        const uint64_t hi = __umul64hi(y, y);
#else
        const uint64_t hi = (uint64_t)(((unsigned __int128)y * y) >> 64);
#endif
        const uint64_t lo = y * y;
        if (hi >> 63) {   // y^2 >> 63 has bit 64: halve, the fraction bit is set
            y = hi;
            r |= 1u << (15 - i);
        } else {
            y = (hi << 1) | (lo >> 63);
        }
    }
    return r;
}

// weight(df) of a table of n_docs documents, Q16.16: 1.0 + L(n_docs + 1) - L(df + 1); >= 1.0 while df <= n_docs
UCFP_IDF_FN uint32_t idf_weight_q16(uint64_t n_docs, uint64_t df) {
    return 0x10000u + idf_log2_q16(n_docs + 1) - idf_log2_q16(df + 1);
}

}  // namespace ucfp
