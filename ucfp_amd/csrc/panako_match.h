// panako_match.h -- the integer arithmetic of the Panako scale/offset vote, shared by the kernels
// of panako_index.hip and by plain C++ checks on the CPU (tests/native/panako_match_check.cpp, panako_pitch_check.cpp):
// the probes of a query hash, the hypotheses a match supports, its offset under a hypothesis, the preference rank of a
// hypothesis, the packed keys the vote sorts and folds and, for A22, the bin map of a hypothesis and the hypotheses
// under which a posting's bin follows a query's.  No HIP types: it compiles with g++.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define UCFP_PKM __host__ __device__ __forceinline__
#else
#define UCFP_PKM inline
#endif

namespace ucfp {

constexpr uint32_t kPkMaxHyp = 64;           // hypotheses per query call
constexpr uint32_t kPkMaxD = 1023;           // d = t_c - t_a of a triple: 1 ... 1023
constexpr uint32_t kPkOrdBits = 23;          // ordinal bits of a posting entry: a' (31) | d' (10) | ordinal (23)
constexpr uint32_t kPkCountBits = 26;        // count bits of the packed best: count (26) | preference (6) | ~offset (32)
constexpr uint32_t kPkBias = 0x80000000u;    // an offset is stored as offset + 2^31 (monotone)
constexpr int32_t kPkMaxBin = 511;           // the three bins of a hash are 9 bits each: k_a << 23 | k_b << 14 | k_c << 5 | r
constexpr uint32_t kPkMaxFSlack = 3;

// a checked ucfp_panako_match_config; scales in units of 1/256
struct PkMatch {
    int32_t smin;     // hypothesis j is smin + j * step, j < nh
    int32_t step;     // clamped to 1024: a larger step leaves one hypothesis either way
    int32_t nh;       // 1 ... 64
    int32_t window;   // W
    int32_t slack;
    int32_t r_slack;
    int32_t bins;     // 0 = the bins are kept (A14), 1 = they follow the scale (A22)
    int32_t f_slack;  // 0 ... 3 bins, 0 when bins = 0
};

// false when a field is out of range or the hypotheses exceed kPkMaxHyp
UCFP_PKM bool pk_plan(uint32_t scale_min, uint32_t scale_max, uint32_t scale_step, uint32_t window, uint32_t slack,
                      uint32_t r_slack, PkMatch* m) {
    if (scale_min < 64 || scale_min > scale_max || scale_max > 1024 || scale_step < 1) return false;
    if (window < 1 || window > 256 || slack > 8 || r_slack > 1) return false;
    const uint32_t nh = (scale_max - scale_min) / scale_step + 1;
    if (nh > kPkMaxHyp) return false;
    m->smin = (int32_t)scale_min;
    m->step = (int32_t)(scale_step > 1024 ? 1024 : scale_step);
    m->nh = (int32_t)nh;
    m->window = (int32_t)window;
    m->slack = (int32_t)slack;
    m->r_slack = (int32_t)r_slack;
    m->bins = 0;
    m->f_slack = 0;
    return true;
}

// the same with the two parameters of A22: bins 0 or 1, f_slack 0 ... 3 and 0 when the bins are kept
UCFP_PKM bool pk_plan_ex(uint32_t scale_min, uint32_t scale_max, uint32_t scale_step, uint32_t window, uint32_t slack,
                         uint32_t r_slack, uint32_t bins, uint32_t f_slack, PkMatch* m) {
    if (bins > 1 || f_slack > kPkMaxFSlack || (bins == 0 && f_slack != 0)) return false;
    if (!pk_plan(scale_min, scale_max, scale_step, window, slack, r_slack, m)) return false;
    m->bins = (int32_t)bins;
    m->f_slack = (int32_t)f_slack;
    return true;
}

// the hashes a query hash probes: (h & ~31) | r' for r' = first_r ... first_r + n - 1
UCFP_PKM void pk_probes(uint32_t h, int32_t r_slack, uint32_t* first, uint32_t* n) {
    const int32_t r = (int32_t)(h & 31u);
    const int32_t lo = r - r_slack < 0 ? 0 : r - r_slack, hi = r + r_slack > 31 ? 31 : r + r_slack;
    *first = (h & ~31u) | (uint32_t)lo;
    *n = (uint32_t)(hi - lo + 1);
}

// The hypotheses j that a match of a query triple with d and a posting with d' supports: |256 d' - s d| <= 256 slack
// with s = smin + j step is  256 (d' - slack) - smin d <= j step d <= 256 (d' + slack) - smin d, one interval of j,
// its ends by two divisions.  Empty when *jlo > *jhi.  d, d' in 1 ... 1023: every product stays below 2^21.
UCFP_PKM void pk_interval(const PkMatch& m, int32_t d, int32_t dp, int32_t* jlo, int32_t* jhi) {
    const int32_t sd = m.step * d, base = m.smin * d;
    const int32_t lo = 256 * (dp - m.slack) - base, hi = 256 * (dp + m.slack) - base;
    *jlo = lo <= 0 ? 0 : (lo + sd - 1) / sd;
    const int32_t h = hi < 0 ? -1 : hi / sd;
    *jhi = h > m.nh - 1 ? m.nh - 1 : h;
}

// A22: the bin of the record that bin k of a query played at speed s / 256 came from: round(256 k / s), halves up.
// k <= 511 and 64 <= s <= 1024: non-increasing in s, at most 2048, and pk_bin(256, k) = k.
UCFP_PKM int32_t pk_bin(int32_t s, int32_t k) { return (512 * k + s) / (2 * s); }

// A22: the hypotheses j with |k' - pk_bin(s_j, k)| <= f.  Over 64 <= s <= 1024 they are the s of one interval,
//   k' - f <= (512 k + s) / (2 s)  <=>  s (2 (k' - f) - 1) <= 512 k       (no upper end when k' - f < 1)
//   (512 k + s) / (2 s) <= k' + f  <=>  s (2 (k' + f) + 1) >  512 k,
// so s_lo = 512 k / (2 k' + 2 f + 1) + 1 and s_hi = 512 k / (2 (k' - f) - 1); on the grid, clamped to [0, nh - 1].
// Empty when *jlo > *jhi.
UCFP_PKM void pk_bin_interval(const PkMatch& m, int32_t k, int32_t kp, int32_t f, int32_t* jlo, int32_t* jhi) {
    const int32_t s_lo = (512 * k) / (2 * kp + 2 * f + 1) + 1;
    *jlo = s_lo <= m.smin ? 0 : (s_lo - m.smin + m.step - 1) / m.step;
    int32_t h = m.nh - 1;
    if (kp - f >= 1) {
        const int32_t s_hi = (512 * k) / (2 * (kp - f) - 1);
        const int32_t t = s_hi < m.smin ? -1 : (s_hi - m.smin) / m.step;
        h = t < h ? t : h;
    }
    *jhi = h;
}

// A22: the hypotheses a (query triple, posting) pair supports in scaled mode -- the intersection of pk_interval's with
// the three bin intervals -- or none when the ratio bits differ by more than r_slack.  hq, hp = the two hashes.
UCFP_PKM void pk_interval_scaled(const PkMatch& m, uint32_t hq, int32_t d, uint32_t hp, int32_t dp, int32_t* jlo,
                                 int32_t* jhi) {
    const int32_t dr = (int32_t)(hp & 31u) - (int32_t)(hq & 31u);
    int32_t lo = 0, hi = -1;
    if (dr >= -m.r_slack && dr <= m.r_slack) {
        pk_interval(m, d, dp, &lo, &hi);
        for (uint32_t sh = 5; sh <= 23 && lo <= hi; sh += 9) {
            int32_t l, h;
            pk_bin_interval(m, (int32_t)((hq >> sh) & 511u), (int32_t)((hp >> sh) & 511u), m.f_slack, &l, &h);
            lo = l > lo ? l : lo;
            hi = h < hi ? h : hi;
        }
    }
    *jlo = lo;
    *jhi = hi;
}

// A22: the bins k' that bin k of a query can meet under the hypotheses jlo ... jhi, clamped to 0 ... 511 (a clamped bin
// never carries into the neighbouring field of the hash)
UCFP_PKM void pk_bin_range(const PkMatch& m, int32_t k, int32_t jlo, int32_t jhi, int32_t* klo, int32_t* khi) {
    const int32_t lo = pk_bin(m.smin + jhi * m.step, k) - m.f_slack, hi = pk_bin(m.smin + jlo * m.step, k) + m.f_slack;
    *klo = lo < 0 ? 0 : lo;
    *khi = hi > kPkMaxBin ? kPkMaxBin : hi;
}

// the offset of a match under scale s: a' - ((s a + 128) >> 8); a < 2^28, s <= 1024, a' < 2^31, so it fits an int32
UCFP_PKM int32_t pk_offset(int32_t s, uint32_t a, uint32_t ap) {
    return (int32_t)((int64_t)ap - (((int64_t)s * (int64_t)a + 128) >> 8));
}

// the rank of hypothesis j in the order (|s - 256|, s): 0 is the most preferred
UCFP_PKM uint32_t pk_pref_rank(const PkMatch& m, int32_t j) {
    const int32_t s = m.smin + j * m.step, ds = s < 256 ? 256 - s : s - 256;
    uint32_t rank = 0;
    for (int32_t i = 0; i < m.nh; i++) {
        const int32_t t = m.smin + i * m.step, dt = t < 256 ? 256 - t : t - 256;
        rank += (dt < ds || (dt == ds && t < s)) ? 1u : 0u;
    }
    return rank;
}

// a vote, sortable: (ordinal, j, offset) ascending
UCFP_PKM uint64_t pk_vote_key(uint32_t ord, uint32_t j, int32_t delta) {
    return ((uint64_t)ord << 38) | ((uint64_t)j << 32) | (uint32_t)((uint32_t)delta + kPkBias);
}
UCFP_PKM uint32_t pk_vote_ord(uint64_t key) { return (uint32_t)(key >> 38); }
UCFP_PKM uint32_t pk_vote_j(uint64_t key) { return (uint32_t)(key >> 32) & 63u; }
UCFP_PKM int32_t pk_vote_delta(uint64_t key) { return (int32_t)((uint32_t)key - kPkBias); }

// Is `key` past the window of W offsets that starts at the vote `at`: another (ordinal, j), or an offset >= its
// offset + W?  Monotone over sorted votes, so the first such position is found by bisection.
UCFP_PKM bool pk_past_window(uint64_t key, uint64_t at, uint32_t window) {
    const uint64_t ka = key >> 32, aa = at >> 32;
    return ka != aa ? ka > aa : (key & 0xffffffffull) >= (at & 0xffffffffull) + window;
}

// the best of a record under a 64-bit max: more votes, then the preferred hypothesis, then the smaller offset
UCFP_PKM uint64_t pk_best(uint32_t count, uint32_t rank, int32_t delta) {
    return ((uint64_t)count << 38) | ((uint64_t)(63u - rank) << 32) | (uint32_t)~((uint32_t)delta + kPkBias);
}
UCFP_PKM uint32_t pk_best_count(uint64_t b) { return (uint32_t)(b >> 38); }
UCFP_PKM uint32_t pk_best_rank(uint64_t b) { return 63u - ((uint32_t)(b >> 32) & 63u); }
UCFP_PKM int32_t pk_best_delta(uint64_t b) { return (int32_t)(~(uint32_t)b - kPkBias); }

// a posting entry: sorted by (a', d', ordinal)
UCFP_PKM uint64_t pk_entry(uint32_t ord, uint32_t ap, uint32_t dp) {
    return ((uint64_t)ap << 33) | ((uint64_t)dp << kPkOrdBits) | ord;
}
UCFP_PKM uint32_t pk_entry_ord(uint64_t e) { return (uint32_t)e & ((1u << kPkOrdBits) - 1u); }
UCFP_PKM uint32_t pk_entry_d(uint64_t e) { return (uint32_t)(e >> kPkOrdBits) & 1023u; }
UCFP_PKM uint32_t pk_entry_a(uint64_t e) { return (uint32_t)(e >> 33); }

}  // namespace ucfp
