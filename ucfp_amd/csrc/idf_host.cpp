// idf_host.cpp -- the host-only entries of the IDF block (include/ucfp_hip.h): no device, no
// context, no HIP header, so a plain C++ compiler builds this file for the stand-alone check (tests/native/idf_log2_check.cpp).

#include <cstddef>
#include <cstdint>

#define UCFP_XXH3_HOST       // the plain functions, also when the HIP compiler builds this file
#define UCFP_IDF_HOST_ONLY
#include "../../include/ucfp_hip.h"
#include "../../include/ucfp_xxh3.h"
#include "idf_math.h"

extern "C" {

uint32_t ucfp_idf_log2_q16(uint64_t x) { return ucfp::idf_log2_q16(x); }

uint32_t ucfp_idf_weight_q16(uint64_t n_docs, uint64_t df) { return ucfp::idf_weight_q16(n_docs, df); }

uint64_t ucfp_text_token_key(const uint8_t* bytes, size_t len) {
    static const uint8_t none = 0;
    return ucfp_xxh3_64(len ? bytes : &none, len);
}

}  // extern "C"
