// idf_log2_check.cpp -- the host-only entries of the IDF block (ucfp_amd/csrc/idf_host.cpp) with their own main, built as
// plain C++ (no device, no HIP) so that sanitizers can watch them: ucfp_idf_log2_q16 against a 128-bit restatement of
// DESIGN.md T9.4, its monotony, ucfp_idf_weight_q16's floor of 1.0, and ucfp_text_token_key over every short length
// (reads stay inside the buffer: each length gets its own exact-size allocation).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/ucfp_hip.h"

static uint32_t log2_ref(uint64_t x) {
    int n = 63;
    while (!((x >> n) & 1)) n--;
    unsigned __int128 y = (unsigned __int128)x << (63 - n);
    uint32_t r = (uint32_t)n << 16;
    for (int i = 0; i < 16; i++) {
        y = (y * y) >> 63;
        if (y >> 64) {
            y >>= 1;
            r |= 1u << (15 - i);
        }
    }
    return r;
}

static int fail(const char* what, uint64_t a, uint64_t b) {
    std::printf("FAIL %s %llu %llu\n", what, (unsigned long long)a, (unsigned long long)b);
    return 1;
}

int main() {
    uint32_t prev = 0;
    for (uint64_t x = 1; x <= 300000; x++) {
        const uint32_t v = ucfp_idf_log2_q16(x);
        if (v != log2_ref(x)) return fail("log2", x, v);
        if (v < prev) return fail("monotone", x, v);
        prev = v;
    }
    for (int k = 1; k < 64; k++)
        for (int d = -1; d <= 1; d++) {
            const uint64_t x = ((uint64_t)1 << k) + (uint64_t)(int64_t)d;
            if (ucfp_idf_log2_q16(x) != log2_ref(x)) return fail("log2 edge", x, 0);
        }
    if (ucfp_idf_log2_q16(~0ull) != log2_ref(~0ull)) return fail("log2 max", ~0ull, 0);
    if (ucfp_idf_log2_q16(0) != 0) return fail("log2 zero", 0, 0);
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (int i = 0; i < 200000; i++) {
        s ^= s << 13, s ^= s >> 7, s ^= s << 17;
        if (ucfp_idf_log2_q16(s) != log2_ref(s)) return fail("log2 random", s, 0);
        const uint64_t n = s >> 20, df = n ? (s * 0x2545F4914F6CDD1Dull) % (n + 1) : 0;
        const uint32_t w = ucfp_idf_weight_q16(n, df);
        if (w < 0x10000u || w != 0x10000u + log2_ref(n + 1) - log2_ref(df + 1)) return fail("weight", n, df);
    }
    if (ucfp_idf_weight_q16(0, 0) != 0x10000u || ucfp_idf_weight_q16(10, 10) != 0x10000u) return fail("weight one", 0, 0);
    uint64_t acc = 0;
    for (size_t len = 0; len <= 600; len++) {
        std::vector<uint8_t> buf(len);
        for (size_t i = 0; i < len; i++) buf[i] = (uint8_t)(i * 131 + len);
        acc ^= ucfp_text_token_key(len ? buf.data() : nullptr, len);
    }
    if (ucfp_text_token_key(nullptr, 0) != 0x2D06800538D394C2ull) return fail("xxh3 of the empty string", 0, 0);
    std::printf("ok %016llx\n", (unsigned long long)acc);
    return 0;
}
