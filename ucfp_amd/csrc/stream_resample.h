// stream_resample.h -- the integer rule of a Wang / Panako stream set that takes its feed at a rate other than 8 kHz
// (DESIGN.md A21): which 8 kHz samples are final after n input samples, and which input samples a stream carries
// between pushes.  Plain host C++ with no HIP in it (tests/native/wang_stream_sr_check.cpp drives it on a CPU);
// wang_streams_core.h plans with it, audio.hip's assemble and save kernels read what it lays out.
#pragma once
#include <cstdint>

namespace ucfp {
namespace wstreams {

constexpr uint32_t kSr8k = 8000, kMinSr = 1000, kMaxSr = 384000;
inline bool sr_ok(uint32_t sr) { return sr >= kMinSr && sr <= kMaxSr; }

// S(n): the 8 kHz samples that are final after n input samples -- those whose right neighbour has arrived (they never
// see A1's n - 1 clamp), capped at the length of an offline clip that ends now; a final push releases that whole length.
inline uint64_t samples_of(uint64_t n, uint32_t sr, bool fin) {
    if (sr == kSr8k || n == 0) return n;
    if (n < ((uint64_t)1 << 50)) {                                       // n 8000 + sr < 2^64: every stream a set can hold
        const uint64_t len = n * kSr8k / sr, nb = ((n - 1) * kSr8k + sr - 1) / sr;
        return fin || len < nb ? len : nb;
    }
    const unsigned __int128 k = kSr8k;
    const uint64_t len = (uint64_t)(n * k / sr);                         // floor(n 8000 / sr)
    if (fin) return len;
    const uint64_t nb = (uint64_t)(((n - 1) * k + sr - 1) / sr);         // ceil((n - 1) 8000 / sr)
    return nb < len ? nb : len;
}

// the inputs a stream carries between pushes: those from floor(S sr / 8000) on, at most ceil(sr / 8000) + 1 of them
inline uint64_t carry_from(uint64_t s8k, uint32_t sr) {
    if (s8k < ((uint64_t)1 << 44)) return s8k * sr / kSr8k;              // s8k sr < 2^63: every stream a set can hold
    return (uint64_t)((unsigned __int128)s8k * sr / kSr8k);
}
inline uint32_t carry_cap_of(uint32_t sr) { return sr == kSr8k ? 0 : (sr + kSr8k - 1) / kSr8k + 1; }

// One stream's share of a push, in absolute positions since `open`: 8 kHz samples [s0, s1) become final; the state
// carries inputs [c_in, n0) into the push and [c_out, n1) out of it (nothing after a final push); the chunk is [n0, n1).
struct RsSpan {
    uint64_t s0, s1, n0, n1, c_in, c_out;
};
inline RsSpan rs_span(uint64_t n0, uint64_t m, uint32_t sr, bool fin) {
    RsSpan r;
    r.n0 = n0;
    r.n1 = n0 + m;
    if (sr == kSr8k) {                    // nothing is resampled, nothing carried: no division on the 8 kHz path
        r.s0 = r.c_in = r.n0;
        r.s1 = r.c_out = r.n1;
        return r;
    }
    r.s0 = samples_of(r.n0, sr, false);
    r.s1 = samples_of(r.n1, sr, fin);
    r.c_in = carry_from(r.s0, sr);
    r.c_out = fin ? r.n1 : carry_from(r.s1, sr);
    return r;
}

}  // namespace wstreams
}  // namespace ucfp
